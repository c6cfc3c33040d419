"""Seeded cases of differentiable compositing, shared by tests/test_compose_host.py and the GPU tests: planes and paints, the
oracle's image of them, the host build of csrc/svgr_compose.h, and the central differences of the numpy restatement.

The arrays of a case are shared: leave them unchanged."""
import ctypes as C
import functools

import numpy as np

from oracle import oracle
from tests import compose_ref as R
from tests import cover_cases as K
from tests import cover_ref as CR

BG = (0.1, 0.2, 0.3, 0.5)   # premultiplied
H = 2.0 ** -10              # the composite is affine in every single input: any step is exact up to rounding


def _pre(rgb, a):
    return [rgb[0] * a, rgb[1] * a, rgb[2] * a, a]


def _scene(_rng):
    """Star over blob over polygon on cover_cases' viewport (24 x 21), planes from the coverage header."""
    planes = []
    for name, rule in (("polygon", 0), ("blob", 1), ("star", 0)):
        c = K.case(name, rule, "identity")
        planes.append(K.harness_forward(c["segs"], c["kinds"], c["off"], c["m6"], c["rules"], c["viewport"])[0][0])
    return np.stack(planes), np.array([_pre((0.9, 0.2, 0.1), 0.8), _pre((0.1, 0.7, 0.3), 0.55), _pre((0.2, 0.3, 0.95), 0.7)])


def _opaque_full(rng):
    """An opaque paint on fully covered pixels (u_p == 0 exactly) between two ordinary paths."""
    cover = rng.uniform(0.0, 1.0, (3, 5, 7))
    cover[1] = 0.0
    cover[1, 1:4, 2:6] = 1.0
    cover[1, 0, :3] = [0.25, 0.5, 1.0]
    return cover, np.array([_pre((0.3, 0.6, 0.9), 0.6), [0.2, 0.5, 0.3, 1.0], _pre((0.8, 0.1, 0.4), 0.5)])


def _alpha_zero(rng):
    cover = rng.uniform(0.0, 1.0, (3, 4, 6))
    return cover, np.array([_pre((0.3, 0.6, 0.9), 0.6), [0.3, 0.2, 0.1, 0.0], _pre((0.8, 0.1, 0.4), 0.5)])


def _zero_plane(rng):
    cover = rng.uniform(0.0, 1.0, (3, 4, 6))
    cover[1] = 0.0
    return cover, np.array([_pre((0.3, 0.6, 0.9), 0.6), _pre((0.5, 0.5, 0.2), 0.9), _pre((0.8, 0.1, 0.4), 0.5)])


def _single(rng):
    return random_planes(rng, 1, 3, 5), np.array([_pre((0.4, 0.7, 0.2), 0.75)])


# name -> (builder, seed)
CASES = {"scene": (_scene, 21), "opaque_full": (_opaque_full, 22), "alpha_zero": (_alpha_zero, 23), "zero_plane": (_zero_plane, 24),
         "single": (_single, 25)}
ALL = tuple((name, with_bg) for name in CASES for with_bg in (False, True))


def random_planes(rng, n_paths, rows, cols):
    """Planes in [0, 1] in which about a third of the entries are exactly 0 and about a tenth exactly 1."""
    cover = rng.uniform(0.0, 1.0, (n_paths, rows, cols))
    pick = rng.uniform(0.0, 1.0, cover.shape)
    cover[pick < 1.0 / 3.0] = 0.0
    cover[pick > 0.9] = 1.0
    return cover


def random_paints(rng, n_paths):
    """Premultiplied paints of alpha in [0.2, 1]; every fifth is opaque."""
    a = rng.uniform(0.2, 1.0, n_paths)
    a[::5] = 1.0
    return np.concatenate([rng.uniform(0.0, 1.0, (n_paths, 3)) * a[:, None], a[:, None]], axis=1)


def random_scene(seed, n_paths, rows, cols):
    """(cover, paints, g) for the launch seams."""
    rng = np.random.default_rng(seed)
    return random_planes(rng, n_paths, rows, cols), random_paints(rng, n_paths), rng.standard_normal((rows, cols, 4))


@functools.lru_cache(maxsize=None)
def case(name, with_bg):
    """dict(name, cover (n, rows, cols), paints (n, 4), bg (4 doubles or None), g (rows, cols, 4) standard normal)."""
    builder, seed = CASES[name]
    cover, paints = builder(np.random.default_rng(seed))
    g = np.random.default_rng(2000 + seed).standard_normal(cover.shape[1:] + (4,))
    return dict(name=name, cover=np.ascontiguousarray(cover), paints=np.ascontiguousarray(paints), bg=BG if with_bg else None, g=g)


def oracle_image(cover, paints, bg=None):
    """The oracle's solid fills composed OVER in paint order (under them a layer of bg, if any)."""
    rows, cols = cover.shape[1:]
    layers = [] if bg is None else [(np.tile(np.asarray(bg, dtype=np.float64), (rows, cols, 1)), (0, 0))]
    layers += [(oracle.fill_solid(cover[p], paints[p]), (0, 0)) for p in range(len(cover))]
    image, offset = oracle.compose_over(layers)
    assert offset == (0, 0)
    return image


def central_differences(c):
    """(fd_cover, fd_paints, tol): central differences at H of sum(g * image) from the numpy restatement, and their tolerance
    2^-50 * sum |g * C| / H.  The difference of the two images is taken before the sum, which is no less exact."""
    cover, paints, bg, g = c["cover"], c["paints"], c["bg"], c["g"]
    tol = 2.0 ** -50 * float(np.abs(g * R.forward(cover, paints, bg)).sum()) / H
    fd_cover, fd_paints = np.empty_like(cover), np.empty_like(paints)
    for p in range(len(cover)):
        hi, lo = cover.copy(), cover.copy()
        hi[p] += H   # every pixel of the plane at once: a pixel depends on its own coverage alone
        lo[p] -= H
        fd_cover[p] = (g * (R.forward(hi, paints, bg) - R.forward(lo, paints, bg))).sum(axis=-1) / (2 * H)
        for k in range(4):
            hi, lo = paints.copy(), paints.copy()
            hi[p, k] += H
            lo[p, k] -= H
            fd_paints[p, k] = (g * (R.forward(cover, hi, bg) - R.forward(cover, lo, bg))).sum() / (2 * H)
    return fd_cover, fd_paints, tol


# ------------------------------------------------------------------------------------------------ the host build of the header
def harness():
    from tests.util import host_build

    lib = host_build("compose_harness")
    lib.cmh_forward.restype = None
    lib.cmh_forward.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_longlong, C.c_void_p]
    lib.cmh_backward.restype = None
    lib.cmh_backward.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_longlong] + [C.c_void_p] * 2
    return lib


def _inputs(cover, paints, bg):
    cover = np.ascontiguousarray(cover, dtype=np.float64)   # (a float32 plane widens exactly)
    paints = np.ascontiguousarray(paints, dtype=np.float64)
    assert cover.ndim == 3 and paints.shape == (len(cover), 4)
    bg = None if bg is None else np.ascontiguousarray(bg, dtype=np.float64)
    return cover, paints, bg, (None if bg is None else bg.ctypes.data)


def harness_forward(cover, paints, bg=None):
    """image (rows, cols, 4) in double, as the header composes it on the host."""
    cover, paints, bg, bgp = _inputs(cover, paints, bg)
    n, rows, cols = cover.shape
    image = np.zeros((rows, cols, 4))
    harness().cmh_forward(cover.ctypes.data, paints.ctypes.data, bgp, n, rows * cols, image.ctypes.data)
    return image


def harness_backward(cover, paints, grad_image, bg=None):
    """(grad_cover (n, rows, cols), grad_paints (n, 4)) in double, as the header gives them on the host."""
    cover, paints, bg, bgp = _inputs(cover, paints, bg)
    n, rows, cols = cover.shape
    g = np.ascontiguousarray(grad_image, dtype=np.float64)
    assert g.shape == (rows, cols, 4)
    grad_cover, grad_paints = np.zeros_like(cover), np.zeros((n, 4))
    harness().cmh_backward(cover.ctypes.data, paints.ctypes.data, bgp, g.ctypes.data, n, rows * cols, grad_cover.ctypes.data, grad_paints.ctypes.data)
    return grad_cover, grad_paints


# ------------------------------------------------------------------------------------------------ geometry and colours together
RENDER_VIEWPORT = (8, 2, 12, 11)


def _about_centre(a, b, c, d, dr, dc):
    cr, cc = K.CENTRE
    return (a, b, cr - a * cr - b * cc + dr, c, d, cc - c * cr - d * cc + dc)


@functools.lru_cache(maxsize=None)
def render_case():
    """The star (even-odd, on top) over the blob (nonzero) on a 12 x 11 viewport, each under its own transform: dict(segs, kinds,
    off, m6, rules, viewport, paints, bg, groups).  No pixel an edge crosses sits on a kink of its fill rule."""
    blob, kb = K._blob(np.random.default_rng(31), 5, 4.6)
    star, ks = K._star(np.random.default_rng(32), 0.5)
    segs, kinds = np.concatenate([blob, star]), np.concatenate([kb, ks])
    off = np.array([0, len(blob), len(segs)], dtype=np.int32)
    m6 = np.array([_about_centre(1.04, 0.03, -0.02, 0.97, 0.3, -0.4), _about_centre(0.98, -0.05, 0.06, 1.02, -0.5, 0.6)])
    rules = np.array([0, 1], dtype=np.uint8)
    c = dict(segs=segs, kinds=kinds, off=off, m6=m6, rules=rules, viewport=RENDER_VIEWPORT, bg=BG,
             paints=np.array([_pre((0.9, 0.3, 0.1), 0.8), _pre((0.1, 0.4, 0.9), 0.6)]), groups=K.point_groups(segs, kinds))
    cover, _slope, A, _tol = CR.forward(segs, kinds, off, m6, rules, RENDER_VIEWPORT)
    assert all(0.05 < cover[p].mean() < 0.9 for p in range(2)) and (cover[0] * cover[1]).max() > 0.5   # both seen, overlapping
    for p in range(2):
        for _s, p0, p1, _t0, _t1 in CR.path_edges(segs, kinds, off, m6, p, RENDER_VIEWPORT):
            _ta, _tb, r, col = CR.edge_pieces(p0, p1, RENDER_VIEWPORT[2], RENDER_VIEWPORT[3])
            assert (CR.kink_distance(A[p][r, col], int(rules[p])) > 1e-6).all(), p
    return c


FIT_STEPS, FIT_RATE_PAINTS, FIT_RATE_SHIFT = 40, 0.015, 0.1  # fixed on the CPU with the harnesses (host_fit's losses, checked by its user)
FIT_SHIFT = (0.8, -0.6)                                        # the star's translation in the target
FIT_PAINTS = ((0.15, 0.45, 0.3, 0.75), (0.5, 0.1, 0.35, 0.9))  # the target's paints; the loop starts from render_case's


def fit_m6(m6, shift):
    """m6 with the star (path 1) moved by shift (numpy)."""
    out = np.array(m6, dtype=np.float64)
    out[1, 2] += shift[0]
    out[1, 5] += shift[1]
    return out


def host_render(c, m6, paints):
    """(image, planes, slope) of render_case's geometry by the two host harnesses."""
    planes, slope, _acc, st = K.harness_forward(c["segs"], c["kinds"], c["off"], m6, c["rules"], c["viewport"])
    assert st == 0
    return harness_forward(planes, paints, c["bg"]), planes, slope


def host_fit():
    """Plain gradient descent on the two paints and the star's translation with the host harnesses, towards the image of
    FIT_PAINTS and FIT_SHIFT: the losses of every step, the last one after the final update."""
    c = render_case()
    target = host_render(c, fit_m6(c["m6"], FIT_SHIFT), np.array(FIT_PAINTS))[0]
    paints, shift, losses = c["paints"].copy(), np.zeros(2), []
    for step in range(FIT_STEPS + 1):
        m6 = fit_m6(c["m6"], shift)
        image, planes, slope = host_render(c, m6, paints)
        r = image - target
        losses.append(0.5 * float((r * r).sum()))
        if step == FIT_STEPS:
            break
        grad_planes, grad_paints = harness_backward(planes, paints, r, c["bg"])
        _gs, gm, st = K.harness_backward(c["segs"], c["kinds"], c["off"], m6, c["viewport"], slope, grad_planes)
        assert st == 0
        paints = paints - FIT_RATE_PAINTS * grad_paints
        shift = shift - FIT_RATE_SHIFT * np.array([gm[1, 2], gm[1, 5]])
    return losses


def reference_render(segs, kinds, off, m6, rules, viewport, paints, bg):
    """The oracle's masks of the paths, composed by the numpy restatement: (rows, cols, 4)."""
    planes = np.stack([K.oracle_cover(segs[off[p]:off[p + 1]], kinds[off[p]:off[p + 1]], m6[p], int(rules[p]), viewport) for p in range(len(m6))])
    return R.forward(planes, paints, bg)
