"""Host reference of the marker vertex pass (svgr_path_markers, csrc/svgr_marker.h): the definitions of DESIGN.md "Markers"
restated subpath by subpath in plain Python over numpy long doubles -- no scan, no table, no slots.

Input: the stroker's array form (types, params (n, 8), sizes) and optional per-segment vertex flags.  A trailing UNCLOSED line
is not part of the outline; CLOSED is a line.  The vertices of a subpath are the start point of its first segment and the end
point of every flagged segment; kinds: 0 the path's first vertex, 2 its last, 1 every other.

Directions.  A line's is P1 - P0; a cubic's the first of P1 - P0, P2 - P0, P3 - P0 that is not (0, 0) at its start and the
first of P3 - P2, P3 - P1, P3 - P0 at its end.  A segment without one takes both from the end of the nearest earlier segment of
its subpath that has one, else from the start of the nearest later one, else (1, 0).  The first vertex of an open subpath
points along its outgoing direction, the last along its incoming one; every other vertex, and both end vertices of a closed
subpath (u_in: the closing segment's end, u_out: the first segment's start), along normalise(u_in + u_out) -- or along u_in
turned by +90 degrees when neither component of the sum exceeds CANCEL = 2^-40.

Tolerance (per vertex, on each component of the direction; U = 2^-53, first order).  The inputs are doubles, so the
reference's own error is that of long double arithmetic, ~2^-64 per operation, and is neglected.  The code under test
normalises d = P_b - P_a as x = d / max|d|, h = sqrt(x.x^2 + x.y^2), u = x / h.  Each difference rounds once (U, relative); the
larger component of x is exactly +-1, the smaller carries its own rounding, the divisor's and the division's: 3 U.  Of the two
squares one is exactly 1 and the other, at most 1, is within 2 x 3 U + U = 7 U; their sum, at most 2, rounds by at most 2 U: h^2
>= 1 is within 9 U, its root within 4.5 U + U = 5.5 U.  u = x / h: 3 U + 5.5 U + U = 9.5 U relative to a component of at most
1, taken as E = 12 U.  A bisected vertex adds two such vectors (2 E + U per component, sqrt(2) (2 E + U) in length) and
normalises the sum s: an error e of s turns s / |s| by at most |e| / |s|, and the normalisation adds its own E:
tol = E + sqrt(2) (2 E + U) / |s|.  A reversal copies u_in: E.

`detail["clearance"]`: the smallest |u_in + u_out| over the bisected vertices that are not reversals (inf without one); below
~1e-6 the two sides of the comparison may fall on different sides of CANCEL's neighbourhood and the tolerance grows past 1e-8.
"""
from __future__ import annotations

import math

import numpy as np

from tests.dash_ref import CLOSED, CUBIC, LINE, QUAD, UNCLOSED, concat, from_segments, polyline  # noqa: F401  (the case builders)

U = 2.0 ** -53
E_UNIT = 12 * U
CANCEL = 2.0 ** -40
START, MID, END = 0, 1, 2
LD = np.longdouble


def unit(dx, dy):
    """(dx, dy) / |(dx, dy)| in long double, scaled by the larger component first; None for exactly (0, 0)."""
    dx, dy = LD(dx), LD(dy)
    m = max(abs(dx), abs(dy))
    if not m > 0:
        return None
    x, y = dx / m, dy / m
    h = np.sqrt(x * x + y * y)
    return (x / h, y / h)


def seg_dirs(t, q):
    """(start, end) unit directions of a segment, or None for a degenerate one."""
    p = [(LD(q[2 * k]), LD(q[2 * k + 1])) for k in range(4)]
    if t != CUBIC:
        u = unit(p[1][0] - p[0][0], p[1][1] - p[0][1])
        return None if u is None else (u, u)
    start = next((u for u in (unit(p[k][0] - p[0][0], p[k][1] - p[0][1]) for k in (1, 2, 3)) if u is not None), None)
    if start is None:
        return None
    end = next(u for u in (unit(p[3][0] - p[k][0], p[3][1] - p[k][1]) for k in (2, 1, 0)) if u is not None)
    return start, end


def bisect(u_in, u_out):
    """(direction, |u_in + u_out| or None for a reversal)."""
    sx, sy = u_in[0] + u_out[0], u_in[1] + u_out[1]
    if max(abs(sx), abs(sy)) <= CANCEL:
        return (-u_in[1], u_in[0]), None
    return unit(sx, sy), float(np.sqrt(sx * sx + sy * sy))


def vertices(types, params, sizes, seg_vertex=None, detail=None):
    """(xy (n, 2) float64, direction (n, 2) long double, kind (n,) int32, tolerance (n,) float64)."""
    params = np.asarray(params, dtype=np.float64).reshape(-1, 8)
    xy, dirs, tol = [], [], []
    clearance = math.inf
    at = 0
    for size in sizes:
        size = int(size)
        idx = list(range(at, at + size))
        at += size
        if idx and types[idx[-1]] == UNCLOSED:
            idx = idx[:-1]
        if not idx:
            continue
        closed = types[idx[-1]] == CLOSED
        own = [seg_dirs(types[i], params[i]) for i in idx]
        # both directions of every segment, a degenerate one borrowing: backwards first, then forwards, then (1, 0)
        res = []
        for k, d in enumerate(own):
            if d is None:
                back = next((own[j][1] for j in range(k - 1, -1, -1) if own[j] is not None), None)
                fwd = next((own[j][0] for j in range(k + 1, len(own)) if own[j] is not None), None)
                v = back if back is not None else (fwd if fwd is not None else (LD(1), LD(0)))
                d = (v, v)
            res.append(d)

        def mid(u_in, u_out):
            nonlocal clearance
            u, s = bisect(u_in, u_out)
            if s is None:
                return u, E_UNIT
            clearance = min(clearance, s)
            return u, E_UNIT + math.sqrt(2) * (2 * E_UNIT + U) / s

        first = params[idx[0]]
        xy.append((first[0], first[1]))
        u, t = mid(res[-1][1], res[0][0]) if closed else (res[0][0], E_UNIT)
        dirs.append(u)
        tol.append(t)
        for k, i in enumerate(idx):
            if seg_vertex is not None and not seg_vertex[i]:
                continue
            q = params[i]
            xy.append((q[6], q[7]) if types[i] == CUBIC else (q[2], q[3]))
            if k == len(idx) - 1:
                u, t = mid(res[-1][1], res[0][0]) if closed else (res[-1][1], E_UNIT)
            else:
                u, t = mid(res[k][1], res[k + 1][0])
            dirs.append(u)
            tol.append(t)
    n = len(xy)
    kind = np.full(n, MID, dtype=np.int32)
    if n:
        kind[-1] = END
        kind[0] = START
    if detail is not None:
        detail["clearance"] = clearance
    return (np.array(xy, dtype=np.float64).reshape(n, 2), np.array(dirs, dtype=LD).reshape(n, 2), kind,
            np.array(tol, dtype=np.float64))


def check(got, want, what=""):
    """Positions and kinds exactly, directions within the per-vertex tolerance; returns the largest error / tolerance."""
    gxy, gdir, gkind = got
    wxy, wdir, wkind, tol = want
    assert gxy.shape == wxy.shape and gdir.shape == wdir.shape, (what, gxy.shape, wxy.shape)
    assert np.ascontiguousarray(gxy).tobytes() == np.ascontiguousarray(wxy).tobytes(), what   # (copies of the input, bit for bit)
    assert list(gkind) == list(wkind), what
    if not len(tol):
        return 0.0
    err = np.abs(np.asarray(gdir, dtype=LD) - wdir).max(axis=1).astype(np.float64)
    worst = float((err / tol).max())
    assert (err <= tol).all(), (what, int(np.argmax(err / tol)), float(err.max()), worst)
    return worst
