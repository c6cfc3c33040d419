"""Host reference of hit testing (csrc/svgr_hit.h), restated in numpy: nothing of the HIP code goes in.

An edge is (a0, b0) -> (a1, b1), `a` the first coordinate of an edge as svgr_batch_all_edges stores it and `b` the second; a point
is (pa, pb) in the same order.

    up   = b0 <= pb and b1 > pb           down = b1 <= pb and b0 > pb          (b0 == b1: neither)
    d    = (a1 - a0) * (pb - b0) - (pa - a0) * (b1 - b0)                       two rounded products, then the difference
    term = +1 if up and d > 0, -1 if down and d < 0, else 0
    a point with a NaN or infinite coordinate gets 0 from every edge

    winding(path) = sum of the terms of its edges;   inside = w != 0 (nonzero) or w & 1 (even-odd)

    pass(p) = inside(p) and for every clip group g of p: any(pass(s) for s in g)      p = 0 .. n - 1 in order, sources s < p
    top     = the largest p with pickable[p] and pass(p), or -1

numpy evaluates `x * y - z * w` on float64 arrays as two rounded products and a rounded difference: there is no fused form to
fall into.  `winding_exact` is the same in exact rational arithmetic, for inputs on which d is exact anyway.
"""
from fractions import Fraction

import numpy as np


def winding(edges, edge_path, n_paths, points, block=4096):
    """(n_points, n_paths) int32 winding numbers.  edges: (E, 2, 2) or (E, 4); edge_path: (E,) the path of every edge."""
    e = np.asarray(edges, dtype=np.float64).reshape(-1, 4)
    ep = np.asarray(edge_path, dtype=np.int64).reshape(-1)
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    out = np.zeros((len(pts), n_paths), dtype=np.int32)
    if len(e) == 0 or len(pts) == 0:
        return out
    order = np.argsort(ep, kind="stable")
    e, ep = e[order], ep[order]
    starts = np.searchsorted(ep, np.arange(n_paths + 1))
    a0, b0, a1, b1 = e[:, 0], e[:, 1], e[:, 2], e[:, 3]
    block = max(1, min(block, 2_000_000 // len(e)))   # (a few temporaries of block x E doubles)
    with np.errstate(invalid="ignore", over="ignore"):
        for i0 in range(0, len(pts), block):
            pa, pb = pts[i0:i0 + block, 0:1], pts[i0:i0 + block, 1:2]
            finite = np.isfinite(pa) & np.isfinite(pb)
            up = (b0 <= pb) & (b1 > pb)
            down = (b1 <= pb) & (b0 > pb)
            m0 = (a1 - a0) * (pb - b0)
            m1 = (pa - a0) * (b1 - b0)
            d = m0 - m1
            term = np.where(up & (d > 0), 1, 0) - np.where(down & (d < 0), 1, 0)
            term = np.where(finite, term, 0).astype(np.int32)
            csum = np.concatenate([np.zeros((term.shape[0], 1), dtype=np.int64), np.cumsum(term, axis=1, dtype=np.int64)], axis=1)
            out[i0:i0 + block] = (csum[:, starts[1:]] - csum[:, starts[:-1]]).astype(np.int32)
    return out


def winding_exact(edges, point):
    """The winding number of one list of edges at one finite point in exact rational arithmetic."""
    pa, pb = Fraction(float(point[0])), Fraction(float(point[1]))
    w = 0
    for a0, b0, a1, b1 in np.asarray(edges, dtype=np.float64).reshape(-1, 4).tolist():
        a0, b0, a1, b1 = Fraction(a0), Fraction(b0), Fraction(a1), Fraction(b1)
        d = (a1 - a0) * (pb - b0) - (pa - a0) * (b1 - b0)
        if b0 <= pb < b1 and d > 0:
            w += 1
        elif b1 <= pb < b0 and d < 0:
            w -= 1
    return w


def inside(w, rules):
    """(n_points, n_paths) bool from winding numbers and per-path rule bytes (bit 0: even-odd)."""
    w = np.asarray(w)
    evenodd = (np.asarray(rules, dtype=np.uint8) & 1).astype(bool)
    return np.where(evenodd[None, :], (w & 1) != 0, w != 0)


def pack_bits(flags):
    """(n_points, ceil(n_paths / 32)) uint32 words from (n_points, n_paths) bools: path p is bit p % 32 of word p // 32."""
    flags = np.asarray(flags, dtype=bool)
    n, m = flags.shape
    words = (m + 31) // 32
    padded = np.zeros((n, words * 32), dtype=np.uint64)
    padded[:, :m] = flags
    weights = (np.uint64(1) << np.arange(32, dtype=np.uint64))
    return (padded.reshape(n, words, 32) * weights).sum(axis=2).astype(np.uint32)


def unpack_bits(bits, n_paths):
    bits = np.asarray(bits, dtype=np.uint32)
    flags = (bits[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1
    return flags.reshape(len(bits), -1)[:, :n_paths].astype(bool)


def resolve(inside_flags, pickable, clips):
    """(pass (n_points, n_paths) bool, top (n_points,) int32).  clips: per path a sequence of groups, each a sequence of earlier
    path indices (None: nothing is clipped)."""
    ins = np.asarray(inside_flags, dtype=bool)
    n, m = ins.shape
    ok = np.zeros((n, m), dtype=bool)
    top = np.full(n, -1, dtype=np.int32)
    for p in range(m):
        cur = ins[:, p].copy()
        for group in (clips[p] if clips is not None else ()):
            if any(s >= p or s < 0 for s in group):
                raise ValueError(f"path {p}: a clip source must lie in front of its user")
            any_src = np.zeros(n, dtype=bool)
            for s in group:
                any_src |= ok[:, s]
            cur &= any_src
        ok[:, p] = cur
        if pickable[p]:
            top[cur] = p
    return ok, top
