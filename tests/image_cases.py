"""The test inputs of k_image_fill and k_layer_displacement_map at their coordinate edges, shared by
tests/test_image_cases_host.py (which checks on the CPU what the cases claim: routes, clearances, that the float64 restatement
stays inside the tolerance) and tests/test_gpu_image_seams.py / tests/test_gpu_displacement_seams.py (which run them through
the C ABI).

A FillCase is (name, shape, seed, inv_m, bbox, smooth, linear_rgb, route): an (h, w) image of seeded random bytes, the 3 x 3
pixel -> image map (u = m00 p0 + m01 p1 + m02 along the image's columns, p0 the device row), the output box (r0, c0, rows,
cols) and what the case is there for:
  seam        a box that ends on, one before or one behind the kernel's 32-column x 8-row tile
  stride      more than 32768 x 8 rows: the row-stride loop takes a second trip
  lod_int     the level of detail is an integer: one level, no blend
  lod_blend   a blend next to 0 or next to 1
  lod_top     the level of detail clamps to the last level: the whole fill is its one texel
  lod_last    between the last two levels
  degenerate  an image one to three texels wide or tall
  edge        a box far larger than the image
  exact       coordinates that are exact in every order of evaluation (dyadic, or saturated by a translation of 1e300):
              compared bit for bit with the float64 restatement
  nonfinite   NaN / inf / 1e308 in the map, through the C ABI only; expected from image_ref's non-finite rule, bit for bit
  nearest     nearest sampling under a rotation: needs `clearance` >= CLEARANCE
Smooth cases that are not exact / nonfinite are compared with image_ref.sample_wide at image_ref.fill_tolerance."""
import math
from collections import namedtuple

import numpy as np

from tests import image_ref as R

TILE_W, TILE_H, GRID_ROWS = 32, 8, 32768   # k_image_fill: a block's tile, and the cap of the grid's height in row tiles
CLEARANCE = 1e-9                           # of nearest sampling and of the displacement map from a pixel edge
EXACT_ROUTES = ("exact", "nonfinite", "lod_top")


class FillCase(namedtuple("FillCase", "name shape seed inv_m bbox smooth linear_rgb route")):
    def pixels(self):
        return R.random_rgba(self.shape, self.seed)

    def lam(self):
        """The level of detail the product computes for this map (paint.image_lod), 0 for nearest sampling."""
        from svgrasterize_amd import _abi, paint

        return paint.image_lod(self.inv_m, len(_abi.image_levels(*self.shape))) if self.smooth else 0.0

    def mask(self):
        return np.random.default_rng(self.seed + 1).uniform(0.05, 1.0, self.bbox[2:])


def inv_map(shape, bbox, per_pixel=1.0, theta=0.0, shift=(0.0, 0.0)):
    """A pixel -> image map that steps `per_pixel` texels per pixel, turned by theta, and takes the middle of the box to the
    middle of the image moved by `shift` texels."""
    h, w = shape
    r0, c0, rows, cols = bbox
    c, s = math.cos(theta), math.sin(theta)
    A = per_pixel * np.array([[-s, c], [c, s]])
    b = np.array([w / 2 + shift[0], h / 2 + shift[1]]) - A @ np.array([r0 + rows / 2, c0 + cols / 2])
    return np.array([[A[0, 0], A[0, 1], b[0]], [A[1, 0], A[1, 1], b[1]], [0.0, 0.0, 1.0]])


def _m(m00, m01, m02, m10, m11, m12):
    return np.array([[m00, m01, m02], [m10, m11, m12], [0.0, 0.0, 1.0]])


def _fill_cases():
    out = []

    def add(name, shape, bbox, inv, smooth=True, linear_rgb=False, route="seam"):
        out.append(FillCase(name, shape, len(out) + 11, np.asarray(inv, dtype=np.float64), tuple(bbox), smooth, linear_rgb, route))

    img = (37, 53)
    # ---- tile seams: 37 x 53 magnified 1.4 x under a rotation, origins that are no multiple of 8 or 32
    origins = [(-13, 5), (3, -37), (-7, -11), (9, 21)]
    n = 0
    for rows in (7, 8, 9, 17):
        for cols in (31, 32, 33, 65):
            box = origins[n % 4] + (rows, cols)
            add(f"seam_{rows}x{cols}", img, box, inv_map(img, box, 1 / 1.4, 0.5), linear_rgb=bool(n % 2))
            n += 1
    for rows, cols in ((1, 1), (1, 200), (200, 1)):
        box = (-5, 13, rows, cols)
        add(f"seam_{rows}x{cols}", img, box, inv_map(img, box, 0.23, 0.5))
    add("seam_nearest_9x33", img, (-13, 5, 9, 33), inv_map(img, (-13, 5, 9, 33), 1 / 1.4, 0.5), smooth=False, route="nearest")
    # ---- the row stride: 32768 x 8 + 9 rows of one column; the image lies in the first / in the last hundred rows, so the
    # first trip (head) and the second (tail: the last nine rows) gather from inside the image; elsewhere the clamped edge
    rows = GRID_ROWS * TILE_H + 9
    stride_inv = _m(0.13, 1.0, 10.3, 37 / 90, 0.0, 0.0)   # the image's rows lie on p0 in [0, 90], its columns 13.8 .. 25.5 there
    for name, first in (("head", 5), ("tail", rows - 91)):
        add(f"stride_{name}", img, (-first, 3, rows, 1), stride_inv, route="stride")   # (p0 = 0 at row `first`)
    add("stride_tail_nearest", img, (-(rows - 91), 3, rows, 1), stride_inv, smooth=False, route="stride")
    # ---- level of detail
    small = (0, 0, 23, 31)
    for k, per in enumerate((1.0, 2.0, 4.0)):
        box = (-3, 2, 41 >> k, 57 >> k)
        add(f"lod_{k}", img, box, inv_map(img, box, per, 0.0, (0.3, -0.2)), route="lod_int")
    add("lod_just_above_1", img, small, inv_map(img, small, 2.0 * (1 + 2.0 ** -30), 0.0, (0.3, -0.2)), route="lod_blend")
    add("lod_just_below_1", img, small, inv_map(img, small, 2.0 * (1 - 2.0 ** -30), 0.0, (0.3, -0.2)), route="lod_blend")
    tiny = (-2, 1, 9, 11)
    add("lod_top", img, tiny, inv_map(img, tiny, 1000.0, 0.4), route="lod_top")
    add("lod_last_two", img, tiny, inv_map(img, tiny, 2.0 ** 5.5, 0.4), route="lod_last")
    wide = (3, 257)   # levels 3 x 257, 2 x 129, 1 x 65, ... : one texel tall from level 2 on
    add("lod_wide_mid", wide, (-2, 1, 9, 21), inv_map(wide, (-2, 1, 9, 21), 2.0 ** 4.5, 0.1), route="lod_last")
    add("lod_wide_last_two", wide, tiny, inv_map(wide, tiny, 2.0 ** 8.5, 0.1), route="lod_last")
    add("lod_wide_top", wide, tiny, inv_map(wide, tiny, 3000.0, 0.1), route="lod_top")
    tall = (257, 3)
    add("lod_tall_3", tall, (-2, 1, 40, 9), inv_map(tall, (-2, 1, 40, 9), 8.0, 0.0, (0.1, 0.3)), route="lod_int")
    # ---- degenerate images, magnified and minified, smooth and nearest
    for shape in ((1, 1), (1, 64), (64, 1), (2, 2), (33, 1), (257, 3)):
        for name, per in (("mag", 1 / 3.3), ("min", 1 / 0.3)):
            h, w = shape
            box = (-4, 3, min(math.ceil(h / per) + 7, 150), min(math.ceil(w / per) + 7, 150))
            for smooth in (True, False):
                add(f"degenerate_{h}x{w}_{name}_{'smooth' if smooth else 'nearest'}", shape, box,
                    inv_map(shape, box, per, 0.3, (0.013, -0.017)), smooth=smooth, route="degenerate")
    # ---- edges: the box hangs over every side of the image by more than the image
    box = (-70, -90, 180, 230)
    add("edge_overhang", img, box, inv_map(img, box, 1.0, 0.2), route="edge")
    add("edge_overhang_nearest", img, box, inv_map(img, box, 1.0, 0.2, (0.013, -0.017)), smooth=False, route="edge")
    # translations of +-1e300 on both axes saturate both clamps (a corner texel); on one axis, the other is dyadic
    e = (-3, 2, 11, 35)
    add("far_plus_minus", img, e, _m(0.0, 0.75, 1e300, 0.75, 0.0, -1e300), route="exact")
    add("far_minus_plus", img, e, _m(0.0, 0.75, -1e300, 0.75, 0.0, 1e300), route="exact")
    add("far_u_only", img, e, _m(0.0, 1.0, 1e300, 1.0, 0.0, 3.25), route="exact")
    add("far_v_only", img, e, _m(0.0, 1.0, 3.25, 1.0, 0.0, -1e300), route="exact")
    add("far_nearest", img, e, _m(0.0, 1.0, 1e300, 1.0, 0.0, 3.25), smooth=False, route="exact")
    # ---- non-finite maps (C ABI only); the finite row is dyadic
    for smooth in (True, False):
        tag = "smooth" if smooth else "nearest"
        add(f"nonfinite_m02_nan_{tag}", img, e, _m(0.0, 1.0, math.nan, 1.0, 0.0, 3.25), smooth=smooth, route="nonfinite")
        add(f"nonfinite_m12_inf_{tag}", img, e, _m(0.0, 1.0, 3.25, 1.0, 0.0, math.inf), smooth=smooth, route="nonfinite")
        add(f"nonfinite_m02_neginf_{tag}", img, e, _m(0.0, 1.0, -math.inf, 1.0, 0.0, 3.25), smooth=smooth, route="nonfinite")
        add(f"nonfinite_m00_1e308_{tag}", img, e, _m(1e308, 1.0, 3.25, 1.0, 0.0, 3.25), smooth=smooth, route="nonfinite")
    # ---- nearest: rotations with clearance, and dyadic maps whose coordinates fall exactly on texel boundaries
    for k, theta in enumerate((math.radians(30), 0.7, 2.1)):
        box = (-6, 9, 45, 67)
        add(f"nearest_rot{k}", img, box, inv_map(img, box, 1 / 1.3, theta, (0.0137, -0.0171)), smooth=False, route="nearest")
    add("nearest_dyadic_half", img, (-4, -6, 90, 120), _m(0.0, 0.5, 0.25, 0.5, 0.0, -0.25), smooth=False, route="exact")
    add("nearest_dyadic_one", img, (-4, -6, 50, 70), _m(0.0, 1.0, 0.5, 1.0, 0.0, -1.5), smooth=False, route="exact")
    add("nearest_dyadic_two", img, (-4, -6, 30, 40), _m(0.0, 2.0, -1.0, 2.0, 0.0, 3.0), smooth=False, route="exact")
    add("smooth_dyadic_half", img, (-4, -6, 90, 120), _m(0.0, 0.5, 0.25, 0.5, 0.0, -0.25), route="exact")
    return out


FILL_CASES = _fill_cases()
MIP_SHAPES = [(1, 1), (1, 3), (3, 1), (2, 2), (17, 16), (16, 17), (255, 1), (257, 3), (37, 53)]


def fill_cases(*routes, smooth=None):
    return [c for c in FILL_CASES if c.route in routes and (smooth is None or c.smooth == smooth)]


# ------------------------------------------------------------------------------------------------------------------------
# feDisplacementMap
# ------------------------------------------------------------------------------------------------------------------------
# (name, src_shape, src_off, map_shape, map_off, lin, scale, special, route); `special`:
#   None      a seeded random straight-alpha map
#   "half"    every third map pixel is exactly 0.5 in all channels: no displacement there
#   "nan"     every fifth map pixel is NaN in the selected channels (C ABI only): transparent there
# route "off": the map box is disjoint from the source and no displacement reaches it (all transparent); "far": a scale of
# 1e300 or an inf in the linear part (all transparent); "on": the rest.
DmCase = namedtuple("DmCase", "name src_shape src_off map_shape map_off lin scale special route")
ROT = np.array([[0.9, -0.5], [0.4, 1.1]])


def _dm_cases():
    src, off = (9, 40), (-5, 8)
    out = [DmCase("dm_smallest", (5, 7), (-2, 3), (4, 6), (-1, 3), ROT, 3.5, None, "on")]
    for n in (255, 256, 257):
        out.append(DmCase(f"dm_flat_{n}", (9, n + 6), (-5, 8), (1, n), (-1, 11), ROT, 6.5, None, "on"))
    out.append(DmCase("dm_1x300", (9, 310), (-5, 8), (1, 300), (-1, 11), ROT, 6.5, None, "on"))
    out.append(DmCase("dm_300x1", (310, 9), (8, -5), (300, 1), (11, -1), ROT, 6.5, None, "on"))
    for name, moff in (("left", (-3, -60)), ("right", (-3, 70)), ("above", (-40, 12)), ("below", (30, 12))):
        out.append(DmCase(f"dm_off_{name}", src, off, (7, 33), moff, ROT, 9.5, None, "off"))
    out.append(DmCase("dm_src_1x1", (1, 1), (2, 13), (7, 33), (-1, 1), ROT, 2.0, "half", "on"))   # (map pixel [3, 12], exactly 0.5, lies on the source pixel)
    out.append(DmCase("dm_scale_0", src, off, (12, 45), (-7, 5), ROT, 0.0, None, "on"))
    out.append(DmCase("dm_half", src, off, (12, 45), (-7, 5), ROT, 9.5, "half", "on"))
    out.append(DmCase("dm_scale_1e300", src, off, (7, 33), (-4, 10), ROT, 1e300, None, "far"))
    out.append(DmCase("dm_lin_inf", src, off, (7, 33), (-4, 10), np.array([[math.inf, 0.0], [0.0, 1.0]]), 2.0, None, "far"))
    # (the source covers device pixel (0, 0): a NaN converted to an integer before the comparison -- 0 on the device -- would read
    #  it instead of failing the guard)
    out.append(DmCase("dm_nan", src, (-5, -8), (7, 33), (-4, -3), ROT, 4.5, "nan", "on"))
    return out


DM_CASES = _dm_cases()
DM_CHANNELS = (0, 1)   # (the channels every case selects; all sixteen pairs run on dm_smallest only)


def dm_inputs(case):
    """(premultiplied source, straight-alpha map) of a DmCase, both (rows, cols, 4) float64."""
    rng = np.random.default_rng(sum(case.name.encode()))
    src = rng.random(case.src_shape + (4,))
    src[..., :3] *= src[..., 3:]
    disp = rng.random(case.map_shape + (4,))
    flat = disp.reshape(-1, 4)
    if case.special == "half":
        flat[::3] = 0.5
    elif case.special == "nan":
        flat[::5, :2] = math.nan
    return src, disp


def dm_premultiplied_map(shape=(12, 45), seed=5):
    """A premultiplied map for Layer.displacement_map with pixels of alpha 0, 5e-5 (both kept as they are by the
    premultiplied -> straight conversion: alpha <= 1e-4) and 1e-3 (divided) among ordinary ones."""
    rng = np.random.default_rng(seed)
    img = rng.random(shape + (4,))
    flat = img.reshape(-1, 4)
    flat[1::7, 3] = 0.0
    flat[2::7, 3] = 5e-5
    flat[3::7, 3] = 1e-3
    flat[:, :3] *= flat[:, 3:]
    flat[1::7, :3] = rng.random((len(flat[1::7]), 3)) * 1e-5   # (colour under alpha 0: used as it is)
    return img
