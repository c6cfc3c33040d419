"""The gradient edge cases as data: what oracle/gen_golden.py --only gradedge records from the reference
(tests/golden/gradedge_kat.npz) and what tests/test_grad_cases_host.py and tests/test_gpu_gradient_edges.py build again.

Every finite input is chosen so that the gradient offset (S:1561-1562 / S:1606-1607 / S:1619-1644) is EXACT in binary64:
dyadic coordinates, `vec` = (1, 0) or (4, 0), radial points on the axes or on (3, 4, 5) triples with a power-of-two radius, and
two-circle forms whose `a` is a power of two.  A fused multiply-add or a reordered sum then cannot move an offset across one of
grad_interpolate's comparisons (S:1676-1680), and neighbouring stop colours differ by at least 0.1 in every channel: a pixel on
the wrong side of a comparison is wrong by 1e-1, not by an ulp.

POINT_CASES go through Grad*.fill on the caller's points, GRID_CASES through Path.fill on the pixel grid (and through the
batch).  `make_paint` / `make_transform` take the module to build with -- the reference or this package -- so that both sides
construct the same objects from the same numbers."""
import hashlib
import json
import math
from fractions import Fraction

import numpy as np

INF, NAN = float("inf"), float("nan")
SPREADS = ("pad", "repeat", "reflect")


# ------------------------------------------------------------------------------------------ stops
def colour(k):
    """Premultiplied linear RGBA of stop k: every channel of neighbouring stops differs by 0.15 or more, and no two of the first
    hundred stops share a colour (a slow ramp on top of a cycle of three)."""
    a = (1.0, 0.7, 0.85)[k % 3]
    ramp = 0.004 * (k // 3)
    return np.array([(0.1, 0.5, 0.3)[k % 3] + ramp, (0.6, 0.2, 0.4)[k % 3] + ramp, (0.3, 0.65, 0.05)[k % 3] + ramp, a])


def stops_at(offsets):
    return [(float(o), colour(k)) for k, o in enumerate(offsets)]


STOP_LISTS = {
    "inner": [0.25, 0.5, 0.5, 0.75],                    # first and last stop inside (0, 1), a hard step in the middle
    "hard_ends": [0.0, 0.0, 0.5, 1.0, 1.0],             # hard steps at the first and at the last position
    "hard_inner_ends": [0.125, 0.125, 0.5, 0.875, 0.875],
    "single": [0.5],
    "nonmono": [0.0, 0.8, 0.5],                         # the reference adds two contributions in (0.5, 0.8] (S:1679-1682)
    "two": [0.0, 1.0],
    "n32": [k / 32 for k in range(32)],                 # the last count carried inside the kernel argument
    "n33": [k / 32 for k in range(33)],                 # the first that travels in a device buffer
}
# the spread methods' own edges: signed zeros, odd and even integers on both sides, negative fractions, huge, non-finite
SPREAD_PROBES = [0.0, -0.0, 1.0, -1.0, 2.0, -2.0, 3.0, -3.0, -0.25, -1.5, 2.25, 1e300, INF, -INF, NAN]


def probes(offs):
    """Offsets to visit for a stop list: on every stop and one ulp to either side (for the long lists: the first two, two in
    the middle and the last three), an eighth below the first and above the last, between the stops, and SPREAD_PROBES."""
    on = sorted(set(offs))
    if len(on) > 8:
        on = on[:2] + on[15:17] + on[-3:]
    out = []
    for s in on:
        out += [float(np.nextafter(s, -INF)), s, float(np.nextafter(s, INF))]
    out += [min(offs) - 0.125, max(offs) + 0.125, 0.3125, 0.55, 0.6, 0.8125]
    return out + SPREAD_PROBES


# ------------------------------------------------------------------------------------------ points route
def _lin_pts(scale):
    def pts(os_):
        return [(scale * o, 3.0 if k % 2 else -2.0) for k, o in enumerate(os_)]
    return pts


RADIAL_FLOOR = 2.0 ** -537   # its square is the smallest subnormal, exactly


def _rad_pts(os_):
    """|o| along the four half-axes of a radius-4 circle.  1e300 would overflow when squared: 2**500 stands in for it; the
    neighbours of 0 would underflow to 0: RADIAL_FLOOR, the smallest offset whose square is a number, stands in for them."""
    out = []
    for k, o in enumerate(os_):
        d = 4.0 * (2.0 ** 500 if o == 1e300 else RADIAL_FLOOR if 0.0 < abs(o) < RADIAL_FLOOR else abs(o))
        out.append([(d, 0.0), (0.0, -d), (-d, 0.0), (0.0, d)][k % 4])
    # (3, 4, 5) triples: offsets 5/16, 5/8, 5/4, 5/2
    return out + [(0.75, 1.0), (-1.5, 2.0), (3.0, -4.0), (-8.0, -6.0)]


def _conc_pts(os_):
    """Concentric two-circle form, fr = 2, r = 6: a = -16, offset = (|pd| - 2) / 4.  Only the offsets whose point 4 o + 2 and
    whose determinant chain are exact (the ulp neighbours and the huge one are not) and the non-finite ones."""
    out = []
    for k, o in enumerate(os_):
        if math.isfinite(o):
            if o < -0.5 or abs(o) > 2.0 ** 20 or Fraction(o).denominator > 2 ** 12:
                continue
        d = 4.0 * o + 2.0
        out.append([(d, 0.0), (0.0, -d), (-d, 0.0), (0.0, d)][k % 4])
    return out + [(0.0, 0.0), (3.0, 4.0), (-6.0, 8.0)]   # the centre (-0.5), (3, 4, 5) triples: 0.75 and 2


# non-finite coordinates in the other places: inf * 0 in the linear dot product, inf - inf, NaN in either coordinate
_NONFINITE_PTS = [(0.5, INF), (INF, INF), (-INF, INF), (NAN, 0.0), (0.0, NAN), (INF, NAN)]

GEOMS = {
    "lin1": (dict(kind="linear", p0=(0.0, 0.0), p1=(1.0, 0.0)), _lin_pts(1.0)),
    "lin4": (dict(kind="linear", p0=(0.0, 0.0), p1=(4.0, 0.0)), _lin_pts(4.0)),
    "rad4": (dict(kind="radial", center=(0.0, 0.0), radius=4.0), _rad_pts),
    "conc": (dict(kind="radial", center=(0.0, 0.0), radius=6.0, fcenter=(0.0, 0.0), fradius=2.0), _conc_pts),
}

# The focal form the all-or-nothing mask is probed with: c = (0, 0), r = 3, f = (5, 0), fr = 0, so a = 16 and
# det = 9 pdx^2 - 16 pdy^2; exclusion threshold fr / (fr - r) = -0.  Every point below has a rational square root.
_FOCAL = dict(kind="radial", center=(0.0, 0.0), radius=3.0, fcenter=(5.0, 0.0), fradius=0.0)
_FOCAL_STOPS = [0.0, 0.5, 1.25, 2.0]
_FOCAL_SAFE = [(1.0, 3.0),      # det == 0 exactly, offset 1.25: on a stop
               (1.0, -3.0),     # det == 0 on the other side
               (0.0, 3.0),      # det = 81, offset 2.125
               (0.0, 0.0),      # the end circle's centre: 2.5
               (2.0, 0.0),      # 1.5
               (-3.0, 0.0),     # 4
               (9.0, 0.0),      # beyond the focus: offset -0.5, r(t) < 0: zero only when the mask exists
               (10.0, 3.0),     # offset -1, likewise
               (5.0, 0.0)]      # the focus itself: offset 0 = the threshold: `>` excludes it when the mask exists
_FOCAL_NEG = (1.0, 3.5)         # det = 144 - 196 < 0: its presence anywhere among the points switches the mask on
# fr == r (the exclusion is disabled, S:1642): c = (0, 0), f = (4, 0), fr = r = 3: a = 16, det = 16 (9 - pdy^2)
_FOCAL_EQ = dict(kind="radial", center=(0.0, 0.0), radius=3.0, fcenter=(4.0, 0.0), fradius=3.0)
_FOCAL_EQ_PTS = [(8.0, 0.0),    # offset -0.25: keeps its colour although the mask exists
                 (0.0, 0.0), (4.0, 3.0), (2.0, 3.0), (6.0, -3.0), (4.0, 0.0),
                 (4.0, 4.0)]    # det < 0


def _point_cases():
    cases = []
    for gname, (geom, to_pts) in GEOMS.items():
        for sname, offs in STOP_LISTS.items():
            for spread in SPREADS:
                pts = to_pts(probes(offs)) + _NONFINITE_PTS
                cases.append(dict(name=f"{gname}-{sname}-{spread}", geom=geom, stops=offs, spread=spread, pts=pts, exact=True))
    for spread in SPREADS:
        f = dict(geom=_FOCAL, stops=_FOCAL_STOPS, spread=spread, exact=True)
        cases.append(dict(name=f"focal-noneg-{spread}", pts=list(_FOCAL_SAFE), **f))
        cases.append(dict(name=f"focal-neglast-{spread}", pts=_FOCAL_SAFE + [_FOCAL_NEG], **f))
        cases.append(dict(name=f"focal-negfirst-{spread}", pts=[_FOCAL_NEG] + _FOCAL_SAFE, **f))
        # more than one block of 256 points, the negative determinant in the last place of the second
        cases.append(dict(name=f"focal-negblock2-{spread}", pts=(_FOCAL_SAFE * 34)[:299] + [_FOCAL_NEG], **f))
        cases.append(dict(name=f"focal-fr_eq_r-{spread}", geom=_FOCAL_EQ, stops=_FOCAL_STOPS, spread=spread, pts=list(_FOCAL_EQ_PTS),
                          exact=True))
    grid = [(float(x), float(y)) for x in (-6.0, -1.5, 0.0, 0.25, 3.0, 8.0) for y in (-4.0, 0.0, 0.5, 4.0)]
    # a == 0 (the focus on the end circle), r = 0 three ways: the reference divides by zero and answers with its zeros
    degenerate = {
        "focal-a0": dict(kind="radial", center=(0.0, 0.0), radius=5.0, fcenter=(3.0, 4.0), fradius=0.0),
        "focal-r0": dict(kind="radial", center=(0.0, 0.0), radius=0.0, fcenter=(5.0, 0.0), fradius=0.0),
        "focal-r0-same-centre": dict(kind="radial", center=(0.0, 0.0), radius=0.0, fcenter=None, fradius=0.0),
        "radial-r0": dict(kind="radial", center=(0.0, 0.0), radius=0.0),
    }
    for name, geom in degenerate.items():
        for spread in SPREADS:
            cases.append(dict(name=f"{name}-{spread}", geom=geom, stops=STOP_LISTS["inner"], spread=spread, pts=list(grid), exact=False))
    return cases


POINT_CASES = _point_cases()


# ------------------------------------------------------------------------------------------ pixel-grid routes
# transform spec: (scale, (tx, ty)): swap = matrix(0, 1, 0, 1, 0, 0), then .scale(s).translate(tx, ty) when not (1, (0, 0)):
# pixel (row, col) has its centre at user x = (col + 0.5) / s - tx, y = (row + 0.5) / s - ty
_SWAP = (1.0, (0.0, 0.0))


def _rect(x0, y0, x1, y1):
    return f"M{x0},{y0} H{x1} V{y1} H{x0} Z"


# The flag gradient: f = F, c = F + (D, 0), D = 32 + 2^-10, r = 32 - 2^-10, fr = 0: a = D^2 - r^2 = 1/8 exactly, and with
# q = p - F: det = r^2 qx^2 - qy^2 / 8.  The cone's edge has slope ~90.5, so a column a quarter pixel from F leaves the cone
# at |qy| > 22.6 and every other column (|qx| >= 0.75) only at |qy| > 67.  Pixels with qx < 0 and det >= 0 have r(t) < 0.
_FLAG_F = (439.25, 26.5)
_FLAG_D, _FLAG_R = 32.0 + 2.0 ** -10, 32.0 - 2.0 ** -10
_FLAG = dict(kind="radial", center=(_FLAG_F[0] + _FLAG_D, _FLAG_F[1]), radius=_FLAG_R, fcenter=_FLAG_F, fradius=0.0)
_FLAG_STOPS = [0.0, 64.0, 128.0]

# `solid`: a second leaf, painted SOLID_PAINT, that shares no pixel with the gradient's layer: a group of one leaf is drawn node by
# node, a group of two is a batch.  Its recorded fill is pasted next to the gradient's to make the expected layer of the group.
SOLID_PAINT = (0.2, 0.1, 0.4, 0.8)

GRID_CASES = [
    # p1 - p0 = 64 px along a row from the centre of column 10: offsets (col - 10) / 64
    dict(name="lin64", path=_rect(2.25, 1.5, 99.5, 8.75), solid=_rect(5, 13, 20, 14.5), tr=_SWAP, viewport=[0, 0, 16, 128], linear_rgb=False,
         geom=dict(kind="linear", p0=(10.5, 0.0), p1=(74.5, 0.0)), stops=STOP_LISTS["inner"], spread="pad"),
    # the same under the swap scaled by 2 with a dyadic translation: p1 - p0 = 32 user units = 64 px, from the centre of column 10
    dict(name="lin64-scaled", path=_rect(-1.125, 2.5, 47.5, 6.25), solid=_rect(2.25, 8.75, 12.25, 11.25), tr=(2.0, (2.75, -1.5)), viewport=[0, 0, 24, 128], linear_rgb=True,
         geom=dict(kind="linear", p0=(2.5, 0.0), p1=(34.5, 0.0)), stops=STOP_LISTS["inner"], spread="pad"),
    # p1 - p0 = 16 px from the centre of column 40: the pixel centres fall on every integer offset from -2 to 3
    dict(name="lin16-repeat", path=_rect(2.25, 1.5, 99.5, 8.75), solid=_rect(5, 13, 20, 14.5), tr=_SWAP, viewport=[0, 0, 16, 128], linear_rgb=True,
         geom=dict(kind="linear", p0=(40.5, 0.0), p1=(56.5, 0.0)), stops=STOP_LISTS["inner"], spread="repeat"),
    # ... under a viewport that cuts the layer above, left and right
    dict(name="lin16-reflect-cut", path=_rect(2.25, 1.5, 99.5, 8.75), solid=_rect(30, 11.25, 50, 13), tr=_SWAP, viewport=[3, 20, 9, 62], linear_rgb=False,
         geom=dict(kind="linear", p0=(40.5, 0.0), p1=(56.5, 0.0)), stops=STOP_LISTS["inner"], spread="reflect"),
    # radial, centred on the centre of pixel (10, 20), r = 4, stops at k / 4: the centre row and column and the (3, 4) pixels sit on stops
    dict(name="rad4", path=_rect(8.25, 2.5, 33.5, 18.25), solid=_rect(39.5, 3, 45, 9), tr=_SWAP, viewport=[0, 0, 24, 48], linear_rgb=False,
         geom=dict(kind="radial", center=(20.5, 10.5), radius=4.0), stops=[k / 4 for k in range(1, 7)], spread="pad"),
    dict(name="rad4-reflect-scaled", path=_rect(1.375, 2.75, 14.0, 10.625), solid=_rect(17, 3, 19.75, 6), tr=(2.0, (2.75, -1.5)), viewport=[0, 0, 24, 48], linear_rgb=True,
         geom=dict(kind="radial", center=(7.5, 6.75), radius=2.0), stops=[k / 4 for k in range(1, 5)], spread="reflect"),
    # 32 stops: a batch entry; 33: per node on both routes (the batch carries its stops inside the description)
    dict(name="n32", path=_rect(2.25, 1.5, 99.5, 8.75), solid=_rect(5, 13, 20, 14.5), tr=_SWAP, viewport=[0, 0, 16, 128], linear_rgb=False,
         geom=dict(kind="linear", p0=(10.5, 0.0), p1=(74.5, 0.0)), stops=STOP_LISTS["n32"], spread="pad"),
    dict(name="n33", path=_rect(2.25, 1.5, 99.5, 8.75), solid=_rect(5, 13, 20, 14.5), tr=_SWAP, viewport=[0, 0, 16, 128], linear_rgb=False,
         geom=dict(kind="linear", p0=(10.5, 0.0), p1=(74.5, 0.0)), stops=STOP_LISTS["n33"], spread="pad", batched=False),
    # The focal form's flag (S:1627), three layers of one gradient, each cut out of a larger rectangle by its viewport on the
    # sides that matter (so that the pixel that sets the flag and its neighbours are painted).  F sits a quarter pixel left of the centre of column 439, on the centre of row 26.
    #   flag-first: rows 3..10, columns 438..449 under a shift of half a pixel: only pixel (0, 0) of the layer is outside the cone
    dict(name="flag-first", path=_rect(430.5, 0, 460.5, 10), solid=_rect(440.5, 14, 445.5, 15.5), tr=(1.0, (-0.5, 0.0)), viewport=[3, 438, 14, 12], linear_rgb=False,
         geom=_FLAG, stops=_FLAG_STOPS, spread="pad", detneg=[0]),
    #   flag-last: rows 10..49, columns 20..439, 16 800 pixels: only the last one is outside
    dict(name="flag-last", path=_rect(10, 11, 450, 60), solid=_rect(30, 3, 60, 7), tr=_SWAP, viewport=[2, 20, 48, 420], linear_rgb=False,
         geom=_FLAG, stops=_FLAG_STOPS, spread="pad", detneg=[40 * 420 - 1]),
    #   flag-none: rows 22..30 around F, both sides of it: no mask, and the pixels with r(t) < 0 keep their colour
    dict(name="flag-none", path=_rect(420, 15, 460, 29), solid=_rect(433, 33, 440, 34.5), tr=_SWAP, viewport=[22, 430, 14, 16], linear_rgb=False,
         geom=_FLAG, stops=_FLAG_STOPS, spread="pad", detneg=[]),
]


# ------------------------------------------------------------------------------------------ builders
def make_paint(mod, geom, stops, spread):
    """The GradLinear / GradRadial of module `mod` (the reference, or this package)."""
    arr = lambda v: None if v is None else np.array(v, dtype=np.float64)
    if geom["kind"] == "linear":
        return mod.GradLinear(arr(geom["p0"]), arr(geom["p1"]), stops, None, spread, False, None)
    focal = "fradius" in geom
    return mod.GradRadial(arr(geom["center"]), geom["radius"], arr(geom.get("fcenter")) if focal else None,
                          geom["fradius"] if focal else None, stops, None, spread, False, None)


def make_transform(mod, spec):
    scale, (tx, ty) = spec
    tr = mod.Transform().matrix(0, 1, 0, 1, 0, 0)
    if spec != _SWAP:
        tr = tr.scale(scale).translate(tx, ty)
    return tr


def digest(case):
    """The inputs of a case in one line: what the fixture's `meta` records next to the reference's answer for them."""
    h = hashlib.sha256()
    h.update(json.dumps([case["name"], case["geom"], case["spread"], case.get("path"), case.get("solid"), case.get("tr"), case.get("viewport"),
                         case.get("linear_rgb")], sort_keys=True).encode())
    h.update(np.array(case["stops"], dtype=np.float64).tobytes())
    h.update(np.array([c for _, c in stops_at(case["stops"])]).tobytes())
    h.update(np.array(case.get("pts", []), dtype=np.float64).tobytes())
    return h.hexdigest()[:16]


def pixel_centres(spec, bbox):
    """User-space (x, y) of the pixel centres of the layer `bbox` = (row0, col0, rows, cols), exactly (dyadic arithmetic)."""
    scale, (tx, ty) = spec
    r0, c0, rows, cols = bbox
    ys = (np.arange(r0, r0 + rows) + 0.5) / scale - ty
    xs = (np.arange(c0, c0 + cols) + 0.5) / scale - tx
    return np.stack(np.broadcast_arrays(xs[None, :], ys[:, None]), axis=-1)


def geom_kwargs(geom):
    """`geom` as the keyword arguments of oracle.gradient_points / gradient_offsets."""
    kw = {k: (None if v is None else np.asarray(v, dtype=np.float64)) if k in ("p0", "p1", "center", "fcenter") else v
          for k, v in geom.items() if k != "kind"}
    if "fradius" in geom:
        kw.setdefault("fcenter", None)
    return kw


# ------------------------------------------------------------------------------------------ exact offsets
def _fsqrt(q):
    """The square root of a Fraction that is the square of one."""
    n, d = math.isqrt(q.numerator), math.isqrt(q.denominator)
    if n * n != q.numerator or d * d != q.denominator:
        raise ValueError(f"{q} has no rational square root")
    return Fraction(n, d)


def exact_offset(geom, x, y):
    """The offset at the finite point (x, y) in rational arithmetic, before the spread; None where det < 0."""
    F = Fraction
    x, y = F(x), F(y)
    if geom["kind"] == "linear":
        v = [F(b) - F(a) for a, b in zip(geom["p0"], geom["p1"])]
        return ((x - F(geom["p0"][0])) * v[0] + (y - F(geom["p0"][1])) * v[1]) / (v[0] * v[0] + v[1] * v[1])
    cx, cy, r = F(geom["center"][0]), F(geom["center"][1]), F(geom["radius"])
    if "fradius" not in geom:
        return _fsqrt(((x - cx) / r) ** 2 + ((y - cy) / r) ** 2)
    fx, fy = (cx, cy) if geom["fcenter"] is None else (F(geom["fcenter"][0]), F(geom["fcenter"][1]))
    fr = F(geom["fradius"])
    cdx, cdy, pdx, pdy, rd = cx - fx, cy - fy, x - fx, y - fy, r - fr
    a = cdx * cdx + cdy * cdy - rd * rd
    b = pdx * cdx + pdy * cdy + fr * rd
    c = pdx * pdx + pdy * pdy - fr * fr
    det = b * b - a * c
    if det < 0:
        return None
    t0 = _fsqrt(det)
    return max((b + t0) / a, (b - t0) / a)
