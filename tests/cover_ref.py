"""Differentiable coverage restated in numpy, independent of csrc/svgr_cover.h: the edges from the oracle's
transform, flatness and split; the accumulation plane from ``oracle.line_coverage``; the slope, the clipped edge walk, the
Bernstein weights and the two chain steps written out here.  Besides each result the functions give what bounds the rounding of
its sums: the number of terms and the sum of their magnitudes, as tests/layer_ref.py does for the layer formulas.
"""
import math

import numpy as np

from oracle import oracle

U = 2.0 ** -53   # unit round-off of a double
ZERO_CUT = 1e-6
FLATNESS = 0.1


def m3(m6):
    m6 = np.asarray(m6, dtype=np.float64)
    return np.array([[m6[0], m6[1], m6[2]], [m6[3], m6[4], m6[5]], [0.0, 0.0, 1.0]])


def seg_edges(pts, cubic, m6, origin, flatness=FLATNESS):
    """The edges of one segment in the viewport's coordinates, curve order: [(p0 (2,), p1 (2,), t0, t1)]."""
    o = np.asarray(origin, dtype=np.float64)
    c = oracle.transform_points(m3(m6), np.asarray(pts, dtype=np.float64).reshape(4, 2)[: 4 if cubic else 2])
    if not cubic:
        return [(c[0] - o, c[1] - o, 0.0, 1.0)]
    thr = (flatness * flatness) * 16.0
    out = []

    def walk(q, level, idx):
        if oracle.flatness(q)[0] < thr or level >= 40:
            out.append((q[0] - o, q[3] - o, idx / 2.0 ** level, (idx + 1) / 2.0 ** level))
            return
        halves = oracle.split(q)
        walk(halves[0], level + 1, 2 * idx)
        walk(halves[1], level + 1, 2 * idx + 1)

    walk(c, 0, 0)
    return out


def path_edges(segs, kinds, off, m6, p, viewport, flatness=FLATNESS):
    """[(segment, p0, p1, t0, t1)] of path p, in segment and curve order."""
    segs = np.asarray(segs, dtype=np.float64).reshape(-1, 4, 2)
    out = []
    for s in range(int(off[p]), int(off[p + 1])):
        out += [(s, *e) for e in seg_edges(segs[s], kinds[s] != 0, np.asarray(m6).reshape(-1, 6)[p], viewport[:2], flatness)]
    return out


def accumulate(edges, rows, cols):
    """A (rows, cols) of a path's edges, with the bound of its rounding: (A, tol)."""
    trace = np.zeros((rows, cols))
    mag = np.zeros((rows, cols))
    cnt = np.zeros((rows, cols))
    for _s, p0, p1, _t0, _t1 in edges:
        line = np.array([p0[0], p0[1], p1[0], p1[1]])
        oracle.line_coverage(trace, line)
        one = oracle.line_coverage(np.zeros((rows, cols)), line)
        mag += np.abs(one)
        # (a run of pieces folded into column 0 is one product in the header and many additions here: count them all)
        cnt += (one != 0.0) * (1.0 + (np.arange(cols) == 0) * max(0.0, -min(p0[1], p1[1])))
    A = np.cumsum(trace, axis=1)
    tol = (np.cumsum(cnt, axis=1) + np.arange(cols) + 8.0) * U * np.cumsum(mag, axis=1)
    return A, tol


def cover_of(A, rule):
    if rule == 0:
        m = np.minimum(np.abs(A), 1.0)
    else:
        m = np.abs(np.remainder(A + 1.0, 2.0) - 1.0)
    return np.where(m < ZERO_CUT, 0.0, m)


def slope_of(A, rule):
    if rule == 0:
        m = np.abs(A)
        return np.where((m < ZERO_CUT) | (m >= 1.0), 0, np.sign(A)).astype(np.int8)
    r = (A + 1.0) - 2.0 * np.floor((A + 1.0) / 2.0) - 1.0
    return np.where(np.abs(r) < ZERO_CUT, 0, np.sign(r)).astype(np.int8)


def kink_distance(A, rule):
    """How far A is from the nearest point where the rule's derivative jumps (the zero cut included)."""
    if rule == 0:
        m = np.abs(A)
        return np.minimum(np.minimum(np.abs(m - ZERO_CUT), np.abs(m - 1.0)), m)
    r = np.remainder(A + 1.0, 2.0) - 1.0   # in [-1, 1): kinks at 0 (and the cut around it) and at +-1
    return np.minimum(np.minimum(np.abs(np.abs(r) - ZERO_CUT), np.abs(r)), 1.0 - np.abs(r))


def forward(segs, kinds, off, m6, rules, viewport, flatness=FLATNESS):
    """(cover, slope, A, tol) of every path, (n_paths, rows, cols) each."""
    rows, cols = int(viewport[2]), int(viewport[3])
    n = len(off) - 1
    cover, slope = np.zeros((n, rows, cols)), np.zeros((n, rows, cols), dtype=np.int8)
    As, tols = np.zeros((n, rows, cols)), np.zeros((n, rows, cols))
    for p in range(n):
        As[p], tols[p] = accumulate(path_edges(segs, kinds, off, m6, p, viewport, flatness), rows, cols)
        cover[p], slope[p] = cover_of(As[p], int(rules[p]) & 1), slope_of(As[p], int(rules[p]) & 1)
    return cover, slope, As, tols


def clip_axis(p, e, limit, tlo, thi):
    if e == 0.0:
        return (tlo, thi) if 0.0 <= p <= limit else None
    ta, tb = (0.0 - p) / e, (limit - p) / e
    if ta > tb:
        ta, tb = tb, ta
    tlo, thi = max(tlo, ta), min(thi, tb)
    return (tlo, thi) if tlo < thi else None


def edge_pieces(p0, p1, rows, cols):
    """The pieces of the clipped walk of one edge: (ta, tb, row, col) arrays of those inside the plane."""
    e = p1 - p0
    span = (0.0, 1.0)
    for ax, limit in ((0, float(rows)), (1, float(cols))):
        span = clip_axis(p0[ax], e[ax], limit, *span)
        if span is None:
            return (np.zeros(0),) * 2 + (np.zeros(0, dtype=np.int64),) * 2
    tlo, thi = span
    cuts = [np.array([tlo, thi])]
    for ax in (0, 1):
        if e[ax] != 0.0:
            a, b = p0[ax] + e[ax] * tlo, p0[ax] + e[ax] * thi
            k = np.arange(math.floor(min(a, b)) - 1, math.ceil(max(a, b)) + 2, dtype=np.float64)
            t = (k - p0[ax]) / e[ax]
            cuts.append(t[(t > tlo) & (t < thi) & (t > 0.0) & (t < 1.0)])
    t = np.unique(np.concatenate(cuts))
    ta, tb = t[:-1], t[1:]
    tm = 0.5 * (ta + tb)
    r, c = np.floor(p0[0] + e[0] * tm), np.floor(p0[1] + e[1] * tm)
    keep = (r >= 0) & (r < rows) & (c >= 0) & (c < cols)
    return ta[keep], tb[keep], r[keep].astype(np.int64), c[keep].astype(np.int64)


def edge_walk(p0, p1, W):
    """(I0, I1, T0, T1, n): the two integrals of W along the edge, the sums of their terms' magnitudes and the term count."""
    ta, tb, r, c = edge_pieces(p0, p1, *W.shape)
    w = W[r, c]
    # (tb - ta) - (tb^2 - ta^2) / 2 and (tb^2 - ta^2) / 2 as the products (tb - ta) (1 - tm) and (tb - ta) tm: the differences of
    # squares cancel for an edge whose first point is far away
    tm = 0.5 * (ta + tb)
    a0, a1 = w * ((tb - ta) * (1.0 - tm)), w * ((tb - ta) * tm)
    return float(np.sum(a0)), float(np.sum(a1)), float(np.sum(np.abs(a0))), float(np.sum(np.abs(a1))), len(ta)


def bernstein(t):
    u = 1.0 - t
    return np.array([u * u * u, 3.0 * t * u * u, 3.0 * t * t * u, t * t * t])


def backward(segs, kinds, off, m6, viewport, slope, grad_out, flatness=FLATNESS):
    """(grad_segs (n_segs, 4, 2), grad_m6 (n_paths, 6), tol_segs, tol_m6): the gradients and the bounds of their rounding."""
    segs = np.asarray(segs, dtype=np.float64).reshape(-1, 4, 2)
    m6 = np.asarray(m6, dtype=np.float64).reshape(-1, 6)
    rows, cols = int(viewport[2]), int(viewport[3])
    n_paths = len(off) - 1
    gs, ts = np.zeros((len(segs), 4, 2)), np.zeros((len(segs), 4, 2))
    gm, tm = np.zeros((n_paths, 6)), np.zeros((n_paths, 6))
    for p in range(n_paths):
        W = grad_out[p].astype(np.float64) * slope[p]
        W = np.where(slope[p] == 0, 0.0, W)
        gp = np.zeros((len(segs), 4, 2))   # with respect to the transformed points, and the magnitudes of its terms
        tp = np.zeros((len(segs), 4, 2))
        terms = np.zeros(len(segs))
        for s, p0, p1, t0, t1 in path_edges(segs, kinds, off, m6, p, viewport, flatness):
            I0, I1, T0, T1, n = edge_walk(p0, p1, W)
            e = p1 - p0
            d = np.array([e[1], -e[0]])
            terms[s] += n + 8
            if kinds[s] == 0:
                gp[s, 0], gp[s, 1] = d * I0, d * I1
                tp[s, 0], tp[s, 1] = np.abs(d) * T0, np.abs(d) * T1
            else:
                B0, B1 = bernstein(t0), bernstein(t1)
                gp[s] += B0[:, None] * (d * I0)[None] + B1[:, None] * (d * I1)[None]
                tp[s] += B0[:, None] * (np.abs(d) * T0)[None] + B1[:, None] * (np.abs(d) * T1)[None]
        M = m6[p]
        for s in range(int(off[p]), int(off[p + 1])):
            g_r, g_c = gp[s, :, 0], gp[s, :, 1]
            t_r, t_c = tp[s, :, 0], tp[s, :, 1]
            gs[s, :, 0], gs[s, :, 1] = M[0] * g_r + M[3] * g_c, M[1] * g_r + M[4] * g_c
            bound = (terms[s] + 8.0) * U
            ts[s, :, 0] = bound * (abs(M[0]) * t_r + abs(M[3]) * t_c)
            ts[s, :, 1] = bound * (abs(M[1]) * t_r + abs(M[4]) * t_c)
            x, y = segs[s, :, 0], segs[s, :, 1]
            npts = 4 if kinds[s] != 0 else 2
            for k in range(npts):
                gm[p] += [g_r[k] * x[k], g_r[k] * y[k], g_r[k], g_c[k] * x[k], g_c[k] * y[k], g_c[k]]
                tm[p] += [t_r[k] * abs(x[k]), t_r[k] * abs(y[k]), t_r[k], t_c[k] * abs(x[k]), t_c[k] * abs(y[k]), t_c[k]]
        # (the transform's sums run over every point of the path: their additions on top of the longest walk's)
        tm[p] *= (terms.max(initial=0.0) + 4.0 * (off[p + 1] - off[p]) + 16.0) * U
    return gs, gm, ts, tm
