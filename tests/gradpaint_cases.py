"""Seeded cases of gradient paints in differentiable compositing, shared by tests/test_gradpaint_host.py and the GPU tests:
planes, paints and gradient descriptions, the oracle's image of them, the host build of csrc/svgr_gradpaint.h, and the central
differences of the numpy restatement.

The builder asserts, for every case used with finite differences (``fd``): every pixel's offset after the spread is at least 1e-3
from every stop position (the clamps are the first and the last), every offset before the spread at least 1e-3 from every wrap and
fold point (the integers) and, for a radial gradient, from 0; and a step of 2e-6 in any transform or geometry component moves an
offset by less than 1e-4.  So no difference at h = 1e-6 or 2h crosses a kink.

"Dyadic" linear cases keep vec, vv and every offset exact in binary64: an identity transform, vec = (8, 8), p0 = (1.5, 0.75) make
the offsets of a 12 x 11 viewport odd multiples of 1/64, and the stops sit on multiples of 1/16.

The arrays of a case are shared: leave them unchanged."""
import ctypes as C
import functools

import numpy as np

from oracle import oracle
from tests import compose_cases as M
from tests import gradpaint_ref as R
from tests.gradpaint_ref import GP

BG = M.BG
H = 1e-6                      # the step of the central differences; 2 H is the second
ROWS, COLS = 12, 11
IDENT = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
SPREADS = ("pad", "repeat", "reflect")
KINDS = (None, "linear", "radial")
CLEAR = 1e-3


def _pre(rgb, a):
    return [rgb[0] * a, rgb[1] * a, rgb[2] * a, a]


def stop_colours(rng, n):
    a = rng.uniform(0.3, 1.0, n)
    return np.concatenate([rng.uniform(0.0, 1.0, (n, 3)) * a[:, None], a[:, None]], axis=1)


def make_gp(paths):
    """GP from a list of None (solid) or dict(kind=1|2, spread, m6, geom, pos, rgba)."""
    kind, spread, off, m6, geom, pos, rgba = [], [], [0], [], [], [], []
    for p in paths:
        if p is None:
            kind.append(0), spread.append(0), m6.append(IDENT), geom.append((0.0,) * 4), off.append(off[-1])
            continue
        kind.append(p["kind"]), spread.append(p["spread"]), m6.append(p.get("m6", IDENT))
        geom.append(tuple(p["geom"]) + (0.0,) * (4 - len(p["geom"])))
        pos += list(p["pos"])
        rgba += [list(c) for c in p["rgba"]]
        off.append(len(pos))
    return GP(np.array(kind, dtype=np.int32), np.array(spread, dtype=np.int32), np.array(off, dtype=np.int32), np.array(m6, dtype=np.float64).reshape(-1, 6),
              np.array(geom, dtype=np.float64).reshape(-1, 4), np.array(pos, dtype=np.float64), np.array(rgba, dtype=np.float64).reshape(-1, 4))


DYADIC_GEOM = (1.5, 0.75, 9.5, 8.75)   # vec = (8, 8): offsets (4 (i + j) - 5) / 64


def _linear(rng, spread, pos, m6=IDENT, geom=DYADIC_GEOM):
    return dict(kind=1, spread=spread, m6=m6, geom=geom, pos=pos, rgba=stop_colours(rng, len(pos)))


def _radial(rng, spread, pos, m6=IDENT, geom=(5.3, 4.9, 6.1)):
    return dict(kind=2, spread=spread, m6=m6, geom=geom, pos=pos, rgba=stop_colours(rng, len(pos)))


def _one(rng, path, opacity=None):
    cover = M.random_planes(rng, 1, ROWS, COLS)
    return cover, np.array([[1.0] * 4 if opacity is None else [opacity] * 4]), make_gp([path]), (0, 0)


def _mixed(rng):
    """A solid, a linear gradient over it, a radial one with an opacity, a solid on top: generic transforms, a non-zero origin."""
    cover = M.random_planes(rng, 4, ROWS, COLS)
    paints = np.array([_pre((0.9, 0.2, 0.1), 0.8), [1.0] * 4, [0.7] * 4, _pre((0.2, 0.3, 0.95), 0.6)])
    lin = _linear(rng, 2, (0.1, 0.35, 0.8), m6=(0.93, 0.11, -7.2, -0.07, 1.04, -1.3), geom=(1.2, 0.8, 9.45, 7.7))
    rad = _radial(rng, 1, (0.05, 0.4, 0.7, 0.95), m6=(1.02, -0.04, -8.4, 0.06, 0.97, -2.2), geom=(5.3, 4.9, 4.3))
    return cover, paints, make_gp([None, lin, rad, None]), (8, 2)


# name -> (builder, seed, dyadic, fd)
CASES = {
    "linear_pad4": (lambda r: _one(r, _linear(r, 0, (0.0, 0.25, 0.5, 1.0))), 51, True, True),
    "linear_repeat2": (lambda r: _one(r, _linear(r, 1, (0.125, 0.875))), 52, True, True),
    "linear_reflect4": (lambda r: _one(r, _linear(r, 2, (0.0625, 0.25, 0.75, 0.9375)), opacity=0.75), 53, True, True),
    "linear_step": (lambda r: _one(r, _linear(r, 0, (0.25, 0.5, 0.5, 0.75))), 54, True, False),
    "linear_one_stop": (lambda r: _one(r, _linear(r, 0, (0.5,))), 55, True, True),
    "radial_pad4": (lambda r: _one(r, _radial(r, 0, (0.1, 0.3, 0.6, 0.9))), 56, False, True),
    "radial_repeat2": (lambda r: _one(r, _radial(r, 1, (0.2, 0.8), geom=(5.3, 4.9, 3.7))), 57, False, True),
    "radial_reflect4": (lambda r: _one(r, _radial(r, 2, (0.0, 0.3, 0.6, 1.0), geom=(5.3, 4.9, 3.7))), 58, False, True),
    "mixed": (_mixed, 59, False, True),
}
ALL = tuple((name, with_bg) for name in CASES for with_bg in (False, True))
FD = tuple((name, with_bg) for name, with_bg in ALL if CASES[name][3])


def clear_stops(gp, rows, cols, origin, wanted):
    """`wanted` stop positions of the gradient paths moved up in steps of 1/512 until each is 2 CLEAR away from every pixel's
    offset: gp with those positions.  (The offsets depend on the transform and the geometry alone.)"""
    pos = np.array(wanted, dtype=np.float64)
    for p in range(len(gp.kind)):
        if gp.kind[p] == 0:
            continue
        u = R.offsets(gp, p, rows, cols, origin)[1].ravel()
        for s in range(int(gp.path_stop_off[p]), int(gp.path_stop_off[p + 1])):
            while np.abs(u - pos[s]).min() < 2 * CLEAR:
                pos[s] += 1.0 / 512
    return gp._replace(stop_pos=pos)


def check_clear(gp, rows, cols, origin):
    """The builder's conditions (the module's docstring) for a case used with finite differences."""
    for p in range(len(gp.kind)):
        if gp.kind[p] == 0:
            continue
        t, u = R.offsets(gp, p, rows, cols, origin)
        pos = gp.stop_pos[gp.path_stop_off[p]:gp.path_stop_off[p + 1]]
        assert (np.diff(pos) > 4 * H).all(), (p, pos)
        assert np.abs(u[..., None] - pos).min() >= CLEAR, (p, float(np.abs(u[..., None] - pos).min()))
        if gp.spread[p] != 0:
            assert np.abs(t - np.round(t)).min() >= CLEAR, (p, float(np.abs(t - np.round(t)).min()))
        if gp.kind[p] == 2:
            assert t.min() >= CLEAR
        for name, n in (("m6", 6), ("geom", 4 if gp.kind[p] == 1 else 3)):
            for k in range(n):
                arr = getattr(gp, name).copy()
                arr[p, k] += 2 * H
                moved = R.offsets(gp._replace(**{name: arr}), p, rows, cols, origin)[0]
                assert np.abs(moved - t).max() < 0.1 * CLEAR, (p, name, k)


@functools.lru_cache(maxsize=None)
def case(name, with_bg):
    """dict(name, cover (n, rows, cols), paints (n, 4), gp, origin, bg (4 doubles or None), g (rows, cols, 4) standard normal,
    dyadic, fd)."""
    builder, seed, dyadic, fd = CASES[name]
    cover, paints, gp, origin = builder(np.random.default_rng(seed))
    rows, cols = cover.shape[1:]
    if not dyadic:
        gp = clear_stops(gp, rows, cols, origin, gp.stop_pos)
    if fd:
        check_clear(gp, rows, cols, origin)
    g = np.random.default_rng(2000 + seed).standard_normal((rows, cols, 4))
    return dict(name=name, cover=np.ascontiguousarray(cover), paints=np.ascontiguousarray(paints), gp=gp, origin=origin, bg=BG if with_bg else None, g=g,
                dyadic=dyadic, fd=fd)


def _m33(m6):
    return np.array([[m6[0], m6[1], m6[2]], [m6[3], m6[4], m6[5]], [0.0, 0.0, 1.0]])


def oracle_image(cover, paints, gp, bg=None, origin=(0, 0)):
    """The oracle's layers composed OVER in paint order: fill_solid for a solid path, (gradient_image * cover) * paint for a
    gradient path (under them a layer of bg, if any)."""
    rows, cols = cover.shape[1:]
    layers = [] if bg is None else [(np.tile(np.asarray(bg, dtype=np.float64), (rows, cols, 1)), (0, 0))]
    for p in range(len(cover)):
        if gp.kind[p] == 0:
            layers.append((oracle.fill_solid(cover[p], paints[p]), (0, 0)))
            continue
        s0, s1 = gp.path_stop_off[p], gp.path_stop_off[p + 1]
        geo = dict(p0=gp.geom[p, :2], p1=gp.geom[p, 2:]) if gp.kind[p] == 1 else dict(center=gp.geom[p, :2], radius=float(gp.geom[p, 2]))
        grad = oracle.gradient_image(KINDS[gp.kind[p]], (origin[0], origin[1], rows, cols), _m33(gp.m6[p]), None, SPREADS[gp.spread[p]],
                                     gp.stop_pos[s0:s1], gp.stop_rgba[s0:s1], **geo)
        layers.append(((grad * cover[p][..., None]) * paints[p], (0, 0)))
    image, offset = oracle.compose_over(layers)
    assert offset == (0, 0)
    return image


# ------------------------------------------------------------------------------------------------ central differences
def _objective(c, g, **changed):
    cover, paints, gp = changed.pop("cover", c["cover"]), changed.pop("paints", c["paints"]), c["gp"]
    if changed:
        gp = gp._replace(**changed)
    return R.forward(cover, paints, gp, c["bg"], c["origin"], fused=False)


def central_differences(c):
    """(fd, tol): dicts over cover, paints, m6, geom, stop_pos, stop_rgba of the central differences at H of sum(g * image) from
    the numpy restatement, and their tolerance per component: twice the Richardson estimate |fd(2H) - fd(H)| / 3 of what the step
    leaves, plus the rounding term 2^-50 * sum |g * C| / H.  The difference of the two images is taken before the sum."""
    g, gp = c["g"], c["gp"]
    base = _objective(c, g)
    rounding = 2.0 ** -50 * float(np.abs(g * base).sum()) / H
    arrays = dict(cover=c["cover"], paints=c["paints"], m6=gp.m6, geom=gp.geom, stop_pos=gp.stop_pos, stop_rgba=gp.stop_rgba)
    fd, tol = {}, {}
    for name, arr in arrays.items():
        fd[name], tol[name] = np.zeros_like(arr), np.zeros_like(arr)
        if name == "cover":   # every pixel of a plane at once: a pixel depends on its own coverage alone
            for p in range(len(arr)):
                d = []
                for h in (H, 2 * H):
                    hi, lo = arr.copy(), arr.copy()
                    hi[p] += h
                    lo[p] -= h
                    d.append((g * (_objective(c, g, cover=hi) - _objective(c, g, cover=lo))).sum(axis=-1) / (2 * h))
                fd[name][p], tol[name][p] = d[0], 2.0 * np.abs(d[1] - d[0]) / 3.0 + rounding
            continue
        for idx in np.ndindex(arr.shape):
            d = []
            for h in (H, 2 * H):
                hi, lo = arr.copy(), arr.copy()
                hi[idx] += h
                lo[idx] -= h
                d.append(float((g * (_objective(c, g, **{name: hi}) - _objective(c, g, **{name: lo}))).sum()) / (2 * h))
            fd[name][idx], tol[name][idx] = d[0], 2.0 * abs(d[1] - d[0]) / 3.0 + rounding
    return fd, tol


# ------------------------------------------------------------------------------------------------ the host build of the header
def harness():
    from tests.util import host_build

    lib = host_build("gradpaint_harness")
    lib.gph_forward.restype = None
    lib.gph_forward.argtypes = [C.c_void_p] * 9 + [C.c_int, C.c_longlong, C.c_void_p]
    lib.gph_backward.restype = None
    lib.gph_backward.argtypes = [C.c_void_p] * 10 + [C.c_int, C.c_int, C.c_longlong] + [C.c_void_p] * 7
    return lib


def _inputs(cover, paints, gp, bg, origin):
    cover = np.ascontiguousarray(cover, dtype=np.float64)   # (a float32 plane widens exactly)
    paints = np.ascontiguousarray(paints, dtype=np.float64)
    n = len(cover)
    assert cover.ndim == 3 and paints.shape == (n, 4) and gp.m6.shape == (n, 6) and gp.geom.shape == (n, 4)
    desc = np.ascontiguousarray(np.stack([gp.kind, gp.spread, gp.path_stop_off[:-1], gp.path_stop_off[1:]], axis=1), dtype=np.int32)
    arrays = [cover, paints, desc] + [np.ascontiguousarray(a, dtype=np.float64) for a in (gp.m6, gp.geom, gp.stop_pos, gp.stop_rgba)]
    bg = None if bg is None else np.ascontiguousarray(bg, dtype=np.float64)
    view = np.array([origin[0], origin[1], cover.shape[2]], dtype=np.int64)
    return arrays, bg, view


def harness_forward(cover, paints, gp, bg=None, origin=(0, 0)):
    """image (rows, cols, 4) in double, as the header composes it on the host."""
    arrays, bg, view = _inputs(cover, paints, gp, bg, origin)
    n, rows, cols = arrays[0].shape
    image = np.zeros((rows, cols, 4))
    harness().gph_forward(*[a.ctypes.data for a in arrays], None if bg is None else bg.ctypes.data, view.ctypes.data, n, rows * cols, image.ctypes.data)
    return image


def harness_backward(cover, paints, gp, grad_image, bg=None, origin=(0, 0)):
    """(grad_cover (n, rows, cols), sums, used): sums is a dict over paints, m6, geom, stop_pos, stop_rgba in double, as the header
    gives them on the host in pixel order; used is (rows, cols, n, 2), the stops each pixel used of each path's own list."""
    arrays, bg, view = _inputs(cover, paints, gp, bg, origin)
    n, rows, cols = arrays[0].shape
    g = np.ascontiguousarray(grad_image, dtype=np.float64)
    assert g.shape == (rows, cols, 4)
    ns = len(gp.stop_pos)
    grad_cover = np.zeros_like(arrays[0])
    sums = dict(paints=np.zeros((n, 4)), m6=np.zeros((n, 6)), geom=np.zeros((n, 4)), stop_pos=np.zeros(ns), stop_rgba=np.zeros((ns, 4)))
    used = np.zeros((rows, cols, n, 2), dtype=np.int32)
    harness().gph_backward(*[a.ctypes.data for a in arrays], None if bg is None else bg.ctypes.data, view.ctypes.data, g.ctypes.data, n, ns, rows * cols,
                           grad_cover.ctypes.data, *[sums[k].ctypes.data for k in ("paints", "m6", "geom", "stop_pos", "stop_rgba")], used.ctypes.data)
    return grad_cover, sums, used


# ------------------------------------------------------------------------------------------------ the launch seams
def random_scene(seed, n_paths, rows, cols, stops=(2, 3, 4), first_gradient=0):
    """(cover, paints, gp, g): path p is solid, linear or radial in turn from `first_gradient` on (solid before it), with the
    spreads in turn and stops[q % len(stops)] stops on the q-th gradient path; generic transforms about the viewport."""
    rng = np.random.default_rng(seed)
    cover, paints = M.random_planes(rng, n_paths, rows, cols), M.random_paints(rng, n_paths)
    paths, q = [], 0
    for p in range(n_paths):
        kind = 0 if p < first_gradient else (p - first_gradient + 1) % 3
        if kind == 0:
            paths.append(None)
            continue
        n = stops[q % len(stops)]
        pos = np.sort(rng.uniform(0.0, 1.0, n))
        m6 = (1.0 + rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(-1.0, 1.0), rng.uniform(-0.1, 0.1), 1.0 + rng.uniform(-0.1, 0.1), rng.uniform(-1.0, 1.0))
        geom = (rng.uniform(0, 0.3) * rows, rng.uniform(0, 0.3) * cols, (0.6 + rng.uniform(0, 0.4)) * rows + 1.0, (0.6 + rng.uniform(0, 0.4)) * cols + 1.0) if kind == 1 \
            else (rng.uniform(0.3, 0.7) * rows, rng.uniform(0.3, 0.7) * cols, 0.3 * (rows + cols) + 1.0)
        paths.append(dict(kind=kind, spread=q % 3, m6=m6, geom=geom, pos=pos, rgba=stop_colours(rng, n)))
        paints[p] = 1.0 if q % 2 else rng.uniform(0.4, 1.0)
        q += 1
    return cover, paints, make_gp(paths), rng.standard_normal((rows, cols, 4))


# ------------------------------------------------------------------------------------------------ the torch tests' cases
@functools.lru_cache(maxsize=None)
def small_case():
    """(cover, paints, gp) at 6 x 5 for gradcheck: a solid, a linear gradient with reflect, a radial one with repeat; the
    builder's conditions hold."""
    rng = np.random.default_rng(61)
    cover, paints = M.random_planes(rng, 3, 6, 5), np.array([_pre((0.8, 0.3, 0.2), 0.7), [1.0] * 4, [0.8] * 4])
    lin = _linear(rng, 2, (0.1, 0.45, 0.9), m6=(0.95, 0.08, 0.3, -0.06, 1.03, 0.2), geom=(0.4, 0.3, 2.9, 2.3))
    rad = _radial(rng, 1, (0.15, 0.5, 0.85), m6=(1.02, -0.05, 0.1, 0.04, 0.98, -0.2), geom=(2.8, 2.3, 1.9))
    gp = clear_stops(make_gp([None, lin, rad]), 6, 5, (0, 0), make_gp([None, lin, rad]).stop_pos)
    check_clear(gp, 6, 5, (0, 0))
    return cover, paints, gp


RENDER_GEOM = (9.0, 3.0, 19.0, 12.0)


@functools.lru_cache(maxsize=None)
def render_case():
    """compose_cases.render_case() -- the star over the blob at 12 x 11 -- with the blob filled by a linear gradient:
    (c, paints, gp).  The builder's conditions hold on top of that case's own."""
    c = M.render_case()
    rng = np.random.default_rng(62)
    lin = _linear(rng, 0, (0.1, 0.5, 0.9), geom=RENDER_GEOM)
    origin = c["viewport"][:2]
    gp = clear_stops(make_gp([lin, None]), 12, 11, origin, make_gp([lin, None]).stop_pos)
    check_clear(gp, 12, 11, origin)
    paints = np.array([[1.0] * 4, c["paints"][1]])
    return c, paints, gp


def reference_render(c, segs, m6, paints, gp):
    """The oracle's masks of the paths, composed by the numpy restatement (without its exact fused multiply-adds)."""
    from tests import cover_cases as K

    off, vp = c["off"], c["viewport"]
    planes = np.stack([K.oracle_cover(segs[off[p]:off[p + 1]], c["kinds"][off[p]:off[p + 1]], m6[p], int(c["rules"][p]), vp) for p in range(len(m6))])
    return R.forward(planes, paints, gp, c["bg"], vp[:2], fused=False)


FIT_STEPS, FIT_RATE_COLOUR, FIT_RATE_GEOM = 40, 0.02, 0.6      # fixed on the CPU with the harnesses (host_fit's losses, checked by its user)
FIT_GEOM = (9.8, 2.4, 18.3, 12.9)                               # the target's end points; the loop starts from RENDER_GEOM
FIT_SOLID = (0.5, 0.1, 0.35, 0.9)                               # the target's solid paint; the loop starts from render_case's


def fit_target_rgba(rgba):
    """The target's stop colours: the case's, in the opposite order."""
    return np.ascontiguousarray(rgba[::-1])


def host_fit():
    """Plain gradient descent on the gradient's two end points, its stop colours and the star's solid paint with the host
    harnesses, towards the image of FIT_GEOM, fit_target_rgba and FIT_SOLID: the losses of every step, the last one after the
    final update.  The geometry of the paths stays: the planes are computed once."""
    from tests import cover_cases as K

    c, paints, gp = render_case()
    origin = c["viewport"][:2]
    planes, _slope, _acc, st = K.harness_forward(c["segs"], c["kinds"], c["off"], c["m6"], c["rules"], c["viewport"])
    assert st == 0
    t_paints, t_geom = paints.copy(), gp.geom.copy()
    t_paints[1], t_geom[0] = FIT_SOLID, FIT_GEOM
    target = harness_forward(planes, t_paints, gp._replace(geom=t_geom, stop_rgba=fit_target_rgba(gp.stop_rgba)), c["bg"], origin)
    paints, geom, rgba, losses = paints.copy(), gp.geom.copy(), gp.stop_rgba.copy(), []
    for step in range(FIT_STEPS + 1):
        now = gp._replace(geom=geom, stop_rgba=rgba)
        r = harness_forward(planes, paints, now, c["bg"], origin) - target
        losses.append(0.5 * float((r * r).sum()))
        if step == FIT_STEPS:
            break
        _gc, sums, _used = harness_backward(planes, paints, now, r, c["bg"], origin)
        paints = paints - FIT_RATE_COLOUR * np.array([[0.0], [1.0]]) * sums["paints"]
        rgba = rgba - FIT_RATE_COLOUR * sums["stop_rgba"]
        geom = geom - FIT_RATE_GEOM * sums["geom"]
    return losses
