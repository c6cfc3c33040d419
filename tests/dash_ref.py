"""Host reference of the path dasher (stroke-dasharray / stroke-dashoffset), in the manner of ``layer_ref.py``.

Plain Python / numpy, no device, no project code: the arc-length metric, its inversion, the splitting and the output
structure exactly as DESIGN.md ("Dashed strokes") and include/svgr.h define them, in float64 (Python floats) or in long
double (``np.longdouble``), with the running arc length summed sequentially or pairwise.

Definitions
-----------
* A line is ``sqrt(dx^2 + dy^2)`` long.  A cubic's parameter range is cut into 32 equal sub-intervals; a sub-interval's
  length is the 4-point Gauss-Legendre quadrature of |B'(t)| over it; the cubic's length is their sum.
* A boundary at arc length s inside a cubic: the sub-interval from the cumulative values, then NEWTON = 8 safeguarded
  Newton steps inside it (bracket kept, bisection whenever a step leaves the bracket), derivative |B'(t)|.
* A piece [ta, tb] of a cubic is its restriction by de Casteljau twice (left part at tb, right part of that at ta / tb).
* Segments own half-open ranges [s0, s1) of their subpath's arc length; interval (k, j) of the pattern is
  [k P + pre[j], k P + pre[j + 1]) and is "on" for even j.  Only on-intervals of non-zero length produce pieces; pieces of
  one interval that follow one another form one output subpath, terminated by a PATH_UNCLOSED line from its end to its start.
* A closed subpath that begins and ends inside on-intervals: the same interval -> the subpath comes back whole (its segments
  of non-zero length, then the PATH_CLOSED line); two intervals -> the trailing dash's pieces, then the leading dash's, as
  the subpath's last output subpath.
* ``true_length(piece)`` is independent of the metric: a 64 x 8-point Gauss-Legendre quadrature.

Tolerance for output control points (``tolerance``)
---------------------------------------------------
With M = the largest |coordinate| of the input, L = the path's total length, n = its segment count and u = 2^-53:

* closed-form parts.  A line's piece end is ``p0 + d * (l / len)``: the subtraction for d, the division, the product and the
  sum are 4 roundings of values <= 2 M, and l itself (a boundary minus the segment's start: 3 roundings of values <= L + P)
  moves the point by its own error, <= (3 + 1) u (L + P) along the line.  (roundings + 1) u magnitudes, as layer_ref.py
  counts: 5 u 2 M + 4 u (L + P).  De Casteljau twice is 2 x 3 levels x 3 roundings = 18 roundings of values <= 2 M per
  coordinate: 19 u 2 M.  Together: (24 x 2 M + 4 (L + P)) u.
* the scan.  A segment's start arc length is a sum of up to n lengths whose association the launch geometry picks freely:
  n u L.  A boundary moves along the curve by that much, and |dB/ds| = 1: the term is n u L.
* the Newton part cannot be derived like this.  It is MEASURED: the largest distance between corresponding output control
  points of this reference run four ways -- long double and float64, each with sequential and with pairwise summation --
  over the inputs of the tests, relative to M.  ``NEWTON_SPREAD`` below records the largest value seen; the tolerance takes
  4 x that (the margin covers fma contraction and scan order).  It is never tuned against the kernel's output.

  NEWTON_SPREAD = 2.2e-15 x M (the largest seen: 2.104e-15, on mix1023), measured on the CPU over the inputs of tests/test_gpu_dash.py with curves: every fixed case
  that is not marked exact and the 200-path fuzz set, less the fuzz paths that the condition below drops
  (tests/test_dash_host.py::test_newton_spread_is_what_the_docstring_says measures the same set again and fails when it grows).

tolerance = (24 x 2 M + 4 (L + P) + n L) u + 4 x NEWTON_SPREAD x M.

Condition on inputs: the structure (subpath count, segments per subpath) is compared exactly, so a case must have no dash
boundary within 1e-6 L of a segment joint unless its arithmetic is exact (integer-length lines, integer dashes):
``dash(..., detail=d)`` reports the smallest distance as ``d['clearance']``.
"""
from __future__ import annotations

import math

import numpy as np

LINE, QUAD, CUBIC, ARC, CLOSED, UNCLOSED = 0, 1, 2, 3, 4, 5
SUB, MAX_ENTRIES, NEWTON = 32, 64, 8
NEWTON_SPREAD = 2.2e-15
METRIC_ACCURACY = 5.5e-5   # relative, near-cusp cubics; smooth cubics: 1e-14
U = 2.0 ** -53
_X0, _W0, _X1, _W1 = 0.3399810435848563, 0.6521451548625461, 0.8611363115940526, 0.3478548451374538


class _Num:
    """The number format of a run: Python floats (float64) or numpy long doubles."""

    def __init__(self, long_double: bool):
        self.ld = long_double
        self.F = np.longdouble if long_double else float
        self.sqrt = np.sqrt if long_double else math.sqrt
        self.floor = np.floor if long_double else math.floor


def is_solid(dashes) -> bool:
    d = [float(v) for v in (dashes if dashes is not None else [])]
    if not d or any(not math.isfinite(v) or v < 0 for v in d) or not sum(d) > 0:
        return True
    return not any(v > 0 for v in (d * 2 if len(d) & 1 else d)[1::2])


class Pattern:
    def __init__(self, num: _Num, dashes, offset, scale):
        F = num.F
        raw = [F(v) for v in dashes]
        n = len(raw)
        m = 2 * n if n & 1 else n
        assert m <= MAX_ENTRIES
        scale = F(scale)
        self.pre = [F(0)]
        for j in range(m):
            self.pre.append(self.pre[-1] + raw[j % n] * scale)
        self.m, self.P = m, self.pre[m]
        self.on = [j for j in range(0, m, 2) if self.pre[j + 1] > self.pre[j]]   # on-intervals of non-zero length
        off = F(offset) * scale
        ph = off - F(num.floor(off / self.P)) * self.P
        if not ph >= 0 or ph >= self.P:
            ph = F(0)
        self.phase = ph
        self.num = num

    def _split(self, u):
        kf = self.num.floor(u / self.P)
        r = u - self.num.F(kf) * self.P
        if r < 0:
            kf -= 1
            r += self.P
        if r >= self.P:
            kf += 1
            r -= self.P
        if not r >= 0:
            r = self.num.F(0)
        return int(kf), r

    def idx_ge(self, u):
        """(k, j, r): the interval that holds u; a boundary belongs to what follows it."""
        k, r = self._split(u)
        j = max(j for j in range(self.m) if self.pre[j] <= r)
        return k, j, r

    def idx_lt(self, u):
        k, r = self._split(u)
        cand = [j for j in range(self.m) if self.pre[j] < r]
        return (k, max(cand)) if cand else (k - 1, self.m - 1)

    def pieces_between(self, a, b):
        """The on-intervals of non-zero length from interval a to interval b (both (k, j)), in order."""
        out = []
        if b < a:
            return out
        for k in range(a[0], b[0] + 1):
            for j in self.on:
                if a <= (k, j) <= b:
                    out.append((k, j))
        return out

    def count_between(self, a, b):
        """len(pieces_between(a, b)) in closed form (a long line with a short period has thousands)."""
        below = lambda k, j: k * len(self.on) + sum(1 for x in self.on if x < j)  # noqa: E731
        return max(0, below(b[0], b[1] + 1) - below(*a))


# ---- the metric ---------------------------------------------------------------------------------------------------------
def speed(num, c, t):
    s = 1 - t
    a, b, d = s * s, 2 * (s * t), t * t
    x = 3 * ((a * (c[2] - c[0]) + b * (c[4] - c[2])) + d * (c[6] - c[4]))
    y = 3 * ((a * (c[3] - c[1]) + b * (c[5] - c[3])) + d * (c[7] - c[5]))
    return num.sqrt(x * x + y * y)


def gl4(num, c, ta, tb):
    F = num.F
    h, mid = (tb - ta) * F(0.5), (ta + tb) * F(0.5)
    s0 = speed(num, c, mid - h * F(_X0)) + speed(num, c, mid + h * F(_X0))
    s1 = speed(num, c, mid - h * F(_X1)) + speed(num, c, mid + h * F(_X1))
    return h * (F(_W0) * s0 + F(_W1) * s1)


def sub_lengths(num, c):
    F = num.F
    return [gl4(num, c, F(i) / SUB, F(i + 1) / SUB) for i in range(SUB)]


def _sum(values, pairwise, zero):
    if not pairwise or len(values) < 2:
        acc = zero
        for v in values:
            acc = acc + v
        return acc
    h = len(values) // 2
    return _sum(values[:h], True, zero) + _sum(values[h:], True, zero)


def _prefix(values):
    """Inclusive sums by halves: the left half's sums, then the right half's with the left half's total added (a tree, as a
    scan over lanes or workgroups associates them)."""
    if len(values) < 2:
        return list(values)
    h = len(values) // 2
    left, right = _prefix(values[:h]), _prefix(values[h:])
    return left + [left[-1] + v for v in right]


def cubic_table(num, c, pairwise=False):
    subs = sub_lengths(num, c)
    if not pairwise:
        tab, acc = [], num.F(0)
        for v in subs:
            acc = acc + v
            tab.append(acc)
        return tab
    return _prefix(subs)


def line_length(num, q):
    dx, dy = q[2] - q[0], q[3] - q[1]
    return num.sqrt(dx * dx + dy * dy)


def invert(num, c, tab, s):
    F = num.F
    i = sum(1 for v in tab[: SUB - 1] if v <= s)   # sub-intervals that end at or before s (the table is monotone)
    base = tab[i - 1] if i else F(0)
    rem, sub = s - base, tab[i] - base
    ta, tb = F(i) / SUB, F(i + 1) / SUB
    if not sub > 0 or not rem > 0:
        return ta
    lo, hi = ta, tb
    t = ta + (tb - ta) * (rem / sub)
    if not lo < t < hi:
        t = F(0.5) * (lo + hi)
    for _ in range(NEWTON):
        f = gl4(num, c, ta, t) - rem
        if f > 0:
            hi = t
        else:
            lo = t
        sp = speed(num, c, t)
        tn = t - f / sp if sp != 0 else F("nan")
        if not lo <= tn <= hi:   # (inclusive: a converged step, tn == t == lo or hi, stays)
            tn = F(0.5) * (lo + hi)
        t = tn
    return t


def split(num, c, ta, tb):
    p = list(c)
    if tb < 1:
        for a in range(2):
            p0, p1, p2, p3 = p[a], p[2 + a], p[4 + a], p[6 + a]
            q0, q1, q2 = p0 + (p1 - p0) * tb, p1 + (p2 - p1) * tb, p2 + (p3 - p2) * tb
            r0, r1 = q0 + (q1 - q0) * tb, q1 + (q2 - q1) * tb
            p[2 + a], p[4 + a], p[6 + a] = q0, r0, r0 + (r1 - r0) * tb
    if ta > 0:
        u = ta / tb if tb < 1 else ta
        for a in range(2):
            p0, p1, p2, p3 = p[a], p[2 + a], p[4 + a], p[6 + a]
            q0, q1, q2 = p0 + (p1 - p0) * u, p1 + (p2 - p1) * u, p2 + (p3 - p2) * u
            r0, r1 = q0 + (q1 - q0) * u, q1 + (q2 - q1) * u
            p[a], p[2 + a], p[4 + a] = r0 + (r1 - r0) * u, r1, q2
    return p


def true_length(piece_type, params, n_sub=64):
    """Length of a line or cubic piece by 64 x 8-point Gauss-Legendre quadrature in long double: independent of the metric."""
    q = [np.longdouble(v) for v in params]
    num = _Num(True)
    if piece_type != CUBIC:
        return float(line_length(num, q))
    x, w = np.polynomial.legendre.leggauss(8)
    total = np.longdouble(0)
    for i in range(n_sub):
        a, b = np.longdouble(i) / n_sub, np.longdouble(i + 1) / n_sub
        h, mid = (b - a) / 2, (a + b) / 2
        total += h * sum(np.longdouble(wi) * speed(num, q, mid + h * np.longdouble(xi)) for xi, wi in zip(x, w))
    return float(total)


# ---- the dasher ---------------------------------------------------------------------------------------------------------
def _subpaths(types, params, sizes):
    k = 0
    for n in sizes:
        n = int(n)
        if n > 0:
            yield list(range(k, k + n))
        k += n


def _measure(num, types, params, pairwise):
    F = num.F
    lens, tabs, coords = [], [], []
    for t, q in zip(types, params):
        c = [F(v) for v in q]
        coords.append(c)
        if t == CUBIC:
            tab = cubic_table(num, c, pairwise)
            tabs.append(tab)
            lens.append(tab[-1])
        else:
            tabs.append(None)
            lens.append(F(0) if t == UNCLOSED else line_length(num, c))
    return coords, lens, tabs


def _running(num, lens, idx, pairwise):
    """s1 of every segment of a subpath (inclusive sums)."""
    if not pairwise:
        out, acc = [], num.F(0)
        for i in idx:
            acc = acc + lens[i]
            out.append(acc)
        return out
    return _prefix([lens[i] for i in idx])


def dash(types, params, sizes, dashes, offset=0.0, path_length=0.0, long_double=False, pairwise=False, detail=None):
    """(types, params (n, 8) float64, sizes) of the dashed path.  `detail`, a dict, receives ``clearance`` (the smallest
    distance of a dash boundary from a segment joint, relative to the path's length; exact hits count as inf when
    ``exact`` arithmetic was asked for by the caller) and ``length``."""
    types = [int(t) for t in types]
    params = np.asarray(params, dtype=np.float64).reshape(-1, 8)
    sizes = [int(s) for s in sizes]
    if is_solid(dashes) or not types:
        return np.array(types, dtype=np.int32), params.copy(), np.array(sizes, dtype=np.int32)
    num = _Num(long_double)
    F = num.F
    coords, lens, tabs = _measure(num, types, params, pairwise)
    subs = list(_subpaths(types, params, sizes))
    s1s = {}
    for idx in subs:
        for i, v in zip(idx, _running(num, lens, idx, pairwise)):
            s1s[i] = v
    scale = F(1)
    total = _sum([s1s[idx[-1]] for idx in subs], False, F(0))
    if path_length and path_length > 0:
        scale = total / F(path_length)
        if not scale > 0 or not np.isfinite(float(scale)):
            scale = F(1)
    pat = Pattern(num, dashes, offset, scale)
    out_t, out_p, out_s = [], [], []
    clearance = math.inf

    def piece_of(i, kj, a, b, u0, ln):
        first, last = kj == a, kj == b
        kP = F(kj[0]) * pat.P
        la = F(0) if first else (kP + pat.pre[kj[1]]) - u0
        lb = ln if last else (kP + pat.pre[kj[1] + 1]) - u0
        if not la > 0:
            la = F(0)
        if not lb < ln:
            lb = ln
        c = coords[i]
        if types[i] == CUBIC:
            ta = invert(num, c, tabs[i], la) if la > 0 else F(0)
            tb = invert(num, c, tabs[i], lb) if lb < ln else F(1)
            return CUBIC, split(num, c, ta, tb)
        dx, dy = c[2] - c[0], c[3] - c[1]
        p = [c[0] + dx * (la / ln) if la > 0 else c[0], c[1] + dy * (la / ln) if la > 0 else c[1],
             c[0] + dx * (lb / ln) if lb < ln else c[2], c[1] + dy * (lb / ln) if lb < ln else c[3]]
        return LINE, p + [F(0)] * 4

    def end_point(t, p):
        return (p[6], p[7]) if t == CUBIC else (p[2], p[3])

    for idx in subs:
        L = s1s[idx[-1]]
        closed = types[idx[-1]] == CLOSED
        if not pat.on:
            continue
        mode = "normal"
        if closed and L > 0:
            k0, j0, _ = pat.idx_ge(pat.phase)
            k1, j1 = pat.idx_lt(L + pat.phase)
            if j0 in pat.on and j1 in pat.on:
                mode = "whole" if (k0, j0) == (k1, j1) else "merged"
        if mode == "whole":
            kept = [i for i in idx if lens[i] > 0 and types[i] not in (CLOSED, UNCLOSED)]
            if not kept:
                continue
            for i in kept:
                out_t.append(CUBIC if types[i] == CUBIC else LINE)
                out_p.append(list(coords[i]) if types[i] == CUBIC else list(coords[i][:4]) + [F(0)] * 4)
            ex, ey = end_point(out_t[-1], out_p[-1])
            sx, sy = out_p[-len(kept)][0], out_p[-len(kept)][1]
            out_t.append(CLOSED)
            out_p.append([ex, ey, sx, sy] + [F(0)] * 4)
            out_s.append(len(kept) + 1)
            continue
        dashes_out = []   # [interval, [(type, params), ...]]
        for n_i, i in enumerate(idx):
            ln = lens[i]
            if not ln > 0 or types[i] == UNCLOSED:
                continue
            s0 = s1s[idx[n_i - 1]] if n_i else F(0)
            u0, u1 = s0 + pat.phase, s1s[i] + pat.phase
            ka, ja, _ra = pat.idx_ge(u0)
            a, b = (ka, ja), pat.idx_lt(u1)
            # how close a boundary comes to this segment's joints
            # (every joint, and the subpath's end, is some segment's s1; the start, arc length 0, is exact)
            _k, r = pat._split(u1)
            for e in pat.pre:
                dist = abs(float(r - e))
                if dist != 0.0 or not detail or not detail.get("exact"):
                    clearance = min(clearance, dist)
            n_pieces = pat.count_between(a, b)
            own_len = tabs[i][-1] if types[i] == CUBIC else ln
            for kj in (pat.pieces_between(a, b) if n_pieces else []):
                piece = piece_of(i, kj, a, b, u0, own_len)
                if dashes_out and dashes_out[-1][0] == kj:
                    dashes_out[-1][1].append(piece)
                else:
                    dashes_out.append([kj, [piece]])
        if mode == "merged" and len(dashes_out) >= 2:
            lead = dashes_out.pop(0)
            dashes_out[-1][1].extend(lead[1])
        for _kj, pieces in dashes_out:
            for t, p in pieces:
                out_t.append(t)
                out_p.append(p)
            ex, ey = end_point(*pieces[-1])
            out_t.append(UNCLOSED)
            out_p.append([ex, ey, pieces[0][1][0], pieces[0][1][1]] + [F(0)] * 4)
            out_s.append(len(pieces) + 1)
    if detail is not None:
        detail["clearance"] = clearance / float(total) if float(total) > 0 else math.inf
        detail["length"] = float(total)
        detail["period"] = float(pat.P)
        detail["wide"] = [[v for v in p] for p in out_p]   # the control points in the run's own format
    return (np.array(out_t, dtype=np.int32), np.array([[float(v) for v in p] for p in out_p], dtype=np.float64).reshape(-1, 8),
            np.array(out_s, dtype=np.int32))


def tolerance(params, n_segments, length, period):
    """The bound on |control point difference| derived in the module docstring."""
    M = float(np.max(np.abs(params))) if len(params) else 0.0
    M = max(M, 1.0)
    return (24 * 2 * M + 4 * (length + period) + n_segments * length) * U + 4 * NEWTON_SPREAD * M


def spread(types, params, sizes, dashes, offset=0.0, path_length=0.0):
    """Largest distance between corresponding control points of the four runs of the reference (long double / float64 x
    sequential / pairwise), relative to the largest |coordinate|; None when their structures differ."""
    runs = []
    for ld in (True, False):
        for pw in (False, True):
            d = {}
            t, _p, s = dash(types, params, sizes, dashes, offset, path_length, long_double=ld, pairwise=pw, detail=d)
            runs.append((list(t), list(s), d.get("wide", [])))
    t0, s0, w0 = runs[0]
    worst = 0.0
    for t, s, w in runs[1:]:
        if t != t0 or s != s0:
            return None
        for a, b in zip(w0, w):
            worst = max(worst, max(abs(float(np.longdouble(x) - np.longdouble(y))) for x, y in zip(a, b)))
    M = max(1.0, float(np.max(np.abs(params)))) if len(params) else 1.0
    return worst / M


# ---- building inputs ------------------------------------------------------------------------------------------------------
def polyline(points, closed=False):
    """(types, params, sizes) of one subpath through `points`, terminated as pathdata.py does."""
    pts = [tuple(map(float, p)) for p in points]
    types, params = [], []
    for a, b in zip(pts, pts[1:]):
        types.append(LINE)
        params.append([a[0], a[1], b[0], b[1], 0, 0, 0, 0])
    types.append(CLOSED if closed else UNCLOSED)
    params.append([pts[-1][0], pts[-1][1], pts[0][0], pts[0][1], 0, 0, 0, 0])
    return types, params, [len(types)]


def from_segments(segments, closed=False):
    """One subpath from [(LINE, [x0, y0, x1, y1]) | (CUBIC, [8 numbers])]."""
    types, params = [], []
    for t, q in segments:
        types.append(t)
        params.append(list(map(float, q)) + [0.0] * (8 - len(q)))
    first, last = params[0], params[-1]
    end = (last[6], last[7]) if types[-1] == CUBIC else (last[2], last[3])
    types.append(CLOSED if closed else UNCLOSED)
    params.append([end[0], end[1], first[0], first[1], 0, 0, 0, 0])
    return types, params, [len(types)]


def concat(*paths):
    types, params, sizes = [], [], []
    for t, p, s in paths:
        types += list(t)
        params += [list(q) for q in p]
        sizes += list(s)
    return types, params, sizes
