"""Seeded cases of differentiable coverage, shared by tests/test_cover_host.py and the GPU tests, and the finite-difference
reference of their gradients, which comes from the oracle alone.

A case is drawn in presentation space over the viewport VIEWPORT; under a transform its user-space points are the inverse
images, so every case lands on the same pixels under the identity and under M6 (up to the rounding of the two maps: the
integer-aligned case is exactly aligned under the identity only).
"""
import functools
import math

import numpy as np

from oracle import oracle
from tests import cover_ref as R

VIEWPORT = (2, -3, 24, 21)   # row0, col0, rows, cols
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
M6 = (1.3 * math.sin(0.3), 1.3 * math.cos(0.3), 2.0, 1.1 * math.cos(0.3), -1.1 * math.sin(0.3), 14.0)
TRANSFORMS = {"identity": IDENTITY, "rotated": M6}
RULES = (0, 1)
H = 1e-6
CENTRE = np.array([VIEWPORT[0] + 12.3, VIEWPORT[1] + 10.1])


def _closed_lines(pts):
    pts = np.asarray(pts, dtype=np.float64)
    segs = np.zeros((len(pts), 4, 2))
    segs[:, 0], segs[:, 1] = pts, np.roll(pts, -1, axis=0)
    return segs, np.zeros(len(pts), dtype=np.uint8)


def _ring(rng, n, radius, jitter, centre=CENTRE, phase=None):
    ang = (rng.uniform(0, 2 * np.pi) if phase is None else phase) + 2 * np.pi * (np.arange(n) + rng.uniform(-jitter, jitter, n)) / n
    rad = radius * rng.uniform(0.75, 1.0, n)
    return centre + np.stack([rad * np.sin(ang), rad * np.cos(ang)], axis=1)


def _blob(rng, n, radius, centre=CENTRE):
    """n cubics through n anchors on a wobbly ring, neighbours sharing their end points."""
    a = _ring(rng, n, radius, 0.15, centre)
    d = np.roll(a, -1, axis=0) - np.roll(a, 1, axis=0)
    d = d * rng.uniform(0.12, 0.3, (n, 1)) + rng.normal(0, 0.4, (n, 2))
    segs = np.zeros((n, 4, 2))
    segs[:, 0], segs[:, 3] = a, np.roll(a, -1, axis=0)
    segs[:, 1], segs[:, 2] = a + d, np.roll(a - d, -1, axis=0)
    return segs, np.ones(n, dtype=np.uint8)


def _polygon(rng):
    return _closed_lines(_ring(rng, 6, 9.0, 0.2))


def _star(rng, scale=1.0):
    v = _ring(rng, 7, 9.5 * scale, 0.05)
    return _closed_lines(v[(3 * np.arange(7)) % 7])


def _two_blobs(rng):
    a, ka = _blob(rng, 5, 7.0, CENTRE + [-2.0, -2.5])
    b, kb = _blob(rng, 5, 6.0, CENTRE + [2.5, 3.0])
    return np.concatenate([a, b]), np.concatenate([ka, kb])


def _mixed(rng):
    segs, kinds = _blob(rng, 6, 8.5)
    kinds[::2] = 0   # every other cubic becomes the line between its end points
    segs[::2, 1] = segs[::2, 3]
    segs[::2, 2:] = 0.0
    order = np.argsort(kinds, kind="stable")   # packed(): lines first
    return segs[order], kinds[order]


def _far(rng):
    v = _ring(rng, 5, 8.0, 0.1)
    v[2] = CENTRE + [1.0e6, 0.7e6]
    return _closed_lines(v)


def _aligned(_rng):
    r0, c0 = VIEWPORT[0], VIEWPORT[1]
    return _closed_lines([[r0 + 5, c0 + 3], [r0 + 5, c0 + 12], [r0 + 15, c0 + 12], [r0 + 15, c0 + 3]])


def _one_pixel(_rng):
    o = np.array([VIEWPORT[0] + 10.0, VIEWPORT[1] + 6.0])
    return _closed_lines(o + [[0.2, 0.3], [0.7, 0.4], [0.4, 0.8]])


def _empty(_rng):
    return np.zeros((0, 4, 2)), np.zeros(0, dtype=np.uint8)


def _outside(rng):
    return _closed_lines(_ring(rng, 5, 6.0, 0.1, CENTRE + [40.0, 3.0]))


# name -> (builder, seed, checked against the differences)
CASES = {
    "polygon": (_polygon, 11, True),
    "star": (_star, 12, True),
    "blob": (lambda rng: _blob(rng, 5, 9.0), 13, True),
    "two_blobs": (_two_blobs, 14, True),
    "mixed": (_mixed, 15, True),
    "off_viewport": (lambda rng: _star(rng, 2.5), 16, True),
    "far_vertex": (_far, 17, True),
    "aligned": (_aligned, 0, False),
    "one_pixel": (_one_pixel, 0, True),
    "empty": (_empty, 0, True),
    "outside": (_outside, 18, True),
}
NAMES = tuple(CASES)
ALL = tuple((name, rule, tname) for name in NAMES for rule in RULES for tname in TRANSFORMS)


def _to_user(pts, m6):
    m = np.array([[m6[0], m6[1]], [m6[3], m6[4]]])
    b = np.array([m6[2], m6[5]])
    return np.linalg.solve(m, (pts - b).T).T


def lines_cubics(segs, kinds):
    return segs[kinds == 0][:, :2], segs[kinds != 0]


def oracle_cover(segs, kinds, m6, rule, viewport=VIEWPORT):
    """Path.mask of the oracle placed on the viewport's plane (zeros elsewhere)."""
    rows, cols = viewport[2], viewport[3]
    out = np.zeros((rows, cols))
    lines, cubics = lines_cubics(segs, kinds)
    res = oracle.path_mask(lines, cubics, R.m3(m6), ("nonzero", "evenodd")[rule], list(viewport)) if len(segs) else None
    if res is not None:
        mask, (r0, c0) = res[0], res[1]
        out[r0 - viewport[0]: r0 - viewport[0] + mask.shape[0], c0 - viewport[1]: c0 - viewport[1] + mask.shape[1]] = mask
    return out


def _objective(segs, kinds, m6, rule, g):
    if len(segs) == 0:
        return 0.0
    lines, cubics = lines_cubics(segs, kinds)
    edges = oracle.path_edges(lines, cubics, R.m3(m6))
    return float(np.sum(g * oracle.mask(edges, VIEWPORT, ("nonzero", "evenodd")[rule])))


def point_groups(segs, kinds):
    """The distinct control points of one path: [[(segment, point), ...] per distinct point], copies of a shared point together."""
    groups = {}
    for s in range(len(segs)):
        for k in range(4 if kinds[s] != 0 else 2):
            groups.setdefault((segs[s, k, 0], segs[s, k, 1]), []).append((s, k))
    return list(groups.values())


def _differences(segs, kinds, m6, rule, g, groups):
    """Central differences at H and 2H and their tolerance: (fd, tol) over the points' components, then the transform's six."""
    noise = 2.0 ** -50 * float(np.sum(np.abs(g) * oracle_cover(segs, kinds, m6, rule))) / H

    def moved(group, axis, d):
        out = segs.copy()
        for s, k in group:
            out[s, k, axis] += d
        return out, m6

    def moved_m(j, d):
        m = np.array(m6, dtype=np.float64)
        m[j] += d
        return segs, tuple(m)

    fd, tol = [], []
    for make in [functools.partial(moved, grp, ax) for grp in groups for ax in (0, 1)] + [functools.partial(moved_m, j) for j in range(6)]:
        d = []
        for h in (H, 2 * H):
            (sp, mp), (sm, mm) = make(h), make(-h)
            d.append((_objective(sp, kinds, mp, rule, g) - _objective(sm, kinds, mm, rule, g)) / (2 * h))
        fd.append(d[0])
        tol.append(4.0 * abs(d[0] - d[1]) + noise)
    return np.array(fd), np.array(tol)


@functools.lru_cache(maxsize=None)
def case(name, rule, tname):
    """One case: dict(segs, kinds, off, m6, rules, viewport, g, checked, groups, fd, fd_tol).  The arrays are shared: leave
    them unchanged."""
    builder, seed, checked = CASES[name]
    m6 = TRANSFORMS[tname]
    segs, kinds = builder(np.random.default_rng(seed))
    used = np.zeros((len(segs), 4), dtype=bool)
    used[:, :2] = True
    used[kinds != 0] = True
    user = np.zeros_like(segs)
    user[used] = segs[used] if tname == "identity" else _to_user(segs[used], m6)
    g = np.random.default_rng(1000 + seed).standard_normal((1, VIEWPORT[2], VIEWPORT[3]))
    off = np.array([0, len(user)], dtype=np.int32)
    c = dict(name=name, segs=user, kinds=kinds, off=off, m6=np.array([m6]), rules=np.array([rule], dtype=np.uint8), viewport=VIEWPORT,
             g=g, checked=checked and len(user) > 0, groups=point_groups(user, kinds))
    if c["checked"]:
        c["fd"], c["fd_tol"] = _differences(user, kinds, m6, rule, g[0], c["groups"])
        # the differences can be trusted: every tolerance is small against the gradient, and no pixel an edge crosses sits on a kink
        scale = float(np.abs(c["fd"]).max())
        assert (c["fd_tol"] <= 1e-5 * scale).all(), (name, rule, tname, float(c["fd_tol"].max()), scale)
        _cover, _slope, A, _tol = R.forward(user, kinds, off, c["m6"], c["rules"], VIEWPORT)
        for _s, p0, p1, _t0, _t1 in R.path_edges(user, kinds, off, c["m6"], 0, VIEWPORT):
            _ta, _tb, r, col = R.edge_pieces(p0, p1, VIEWPORT[2], VIEWPORT[3])
            assert (R.kink_distance(A[0][r, col], rule) > 1e-9).all(), (name, rule, tname)
    return c


def point_gradients(c, grad_segs):
    """grad_segs (n_segs, 4, 2) summed over the copies of every distinct point, in the order of the differences."""
    grad_segs = np.asarray(grad_segs).reshape(-1, 4, 2)
    return np.array([sum(grad_segs[s, k, ax] for s, k in grp) for grp in c["groups"] for ax in (0, 1)])


# ------------------------------------------------------------------------------------------------ the host build of the header
def harness():
    import ctypes as C

    from tests.util import host_build

    lib = host_build("cover_harness")
    lib.ch_slope.argtypes, lib.ch_slope.restype = [C.c_double, C.c_int], C.c_int
    lib.ch_fill.argtypes, lib.ch_fill.restype = [C.c_double, C.c_int], C.c_double
    lib.ch_edges.restype = C.c_longlong
    lib.ch_edges.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_longlong]
    lib.ch_forward.restype = C.c_int
    lib.ch_forward.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ch_backward.restype = C.c_int
    lib.ch_backward.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p, C.c_double] + [C.c_void_p] * 4
    return lib


def _arrays(segs, kinds, off, m6):
    segs = np.ascontiguousarray(segs, dtype=np.float64).reshape(-1, 4, 2)
    return (segs, np.ascontiguousarray(kinds, dtype=np.uint8), np.ascontiguousarray(off, dtype=np.int32),
            np.ascontiguousarray(m6, dtype=np.float64).reshape(-1, 6))


def _p(a):
    return a.ctypes.data


def harness_edges(segs, kinds, off, m6, viewport, flatness=R.FLATNESS):
    """(edges (n, 6): p0r, p0c, p1r, p1c, t0, t1; their segments (n,)) as the header makes them."""
    segs, kinds, off, m6 = _arrays(segs, kinds, off, m6)
    vp = np.array(viewport, dtype=np.int64)
    n = harness().ch_edges(_p(segs), _p(kinds), _p(off), _p(m6), len(segs), len(off) - 1, _p(vp), flatness, None, None, 0)
    edges, seg = np.zeros((n, 6)), np.zeros(n, dtype=np.int32)
    harness().ch_edges(_p(segs), _p(kinds), _p(off), _p(m6), len(segs), len(off) - 1, _p(vp), flatness, _p(edges), _p(seg), n)
    return edges, seg


def harness_forward(segs, kinds, off, m6, rules, viewport, flatness=R.FLATNESS):
    """(cover, slope, A-before-the-row-sums, status) of the header on the host."""
    segs, kinds, off, m6 = _arrays(segs, kinds, off, m6)
    rules = np.ascontiguousarray(rules, dtype=np.uint8)
    vp = np.array(viewport, dtype=np.int64)
    shape = (len(off) - 1, int(vp[2]), int(vp[3]))
    cover, slope, acc = np.zeros(shape), np.zeros(shape, dtype=np.int8), np.zeros(shape)
    st = harness().ch_forward(_p(segs), _p(kinds), _p(off), _p(m6), _p(rules), len(segs), shape[0], _p(vp), flatness, _p(cover), _p(slope), _p(acc))
    return cover, slope, acc, st


def harness_backward(segs, kinds, off, m6, viewport, slope, grad_out, flatness=R.FLATNESS):
    """(grad_segs (n_segs, 4, 2), grad_m6 (n_paths, 6), status) of the header on the host."""
    segs, kinds, off, m6 = _arrays(segs, kinds, off, m6)
    vp = np.array(viewport, dtype=np.int64)
    slope = np.ascontiguousarray(slope, dtype=np.int8)
    grad_out = np.ascontiguousarray(grad_out, dtype=np.float64)
    assert slope.shape == grad_out.shape == (len(off) - 1, int(vp[2]), int(vp[3]))
    gs, gm = np.zeros((len(segs), 4, 2)), np.zeros((len(off) - 1, 6))
    st = harness().ch_backward(_p(segs), _p(kinds), _p(off), _p(m6), len(segs), len(off) - 1, _p(vp), flatness, _p(slope), _p(grad_out), _p(gs), _p(gm))
    return gs, gm, st
