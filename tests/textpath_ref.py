"""Host reference of text on a path (svgr_path_sample / svgr_path_place_glyphs, csrc/svgr_textpath.h): the definitions of
DESIGN.md "Text on a path" restated in plain Python over numpy long doubles -- no scan, no binary search, no slots.  The
metric and its inversion are dash_ref's (its `speed` / `gl4` / `sub_lengths` / `invert`, run in long double), the direction
rule for a vanishing derivative is marker_ref's (`seg_dirs`).

Input: the stroker's array form (types, params (n, 8), sizes).  A PATH_UNCLOSED line has length 0, PATH_CLOSED is a line, the
length runs over all subpaths in order.  cum[i]: the length in front of segment i (a sequential sum); L: the total.  The segment
of s is the last one of non-zero length with cum[i] <= s, for s = L the last one of non-zero length at its end; inside = 0 <= s
<= L, and s is clamped to that range for the point.  A line gives P0 + d r / len and unit(d); a cubic B(t) and unit(B'(t)) at
t = invert(r), or the segment's start (t < 0.5) or end direction where B'(t) is exactly (0, 0).  A path with L = 0 reports
inside = 0 everywhere.

An instance (glyph, s_mid, h, dy) maps an outline point (x, y) to P + u (x - h) + n (y + dy), n = (-uy, ux), with (P, u) the
frame at s_mid; it is hidden when s_mid is not inside.

Tolerance (U = 2^-53, first order; the reference's own error, ~2^-64 per operation, is neglected).  A placed point may differ
from the reference's by at most

    d_point + rho * d_dir + 10 U Mx

* d_point: the dasher's bound for a point at an arc length -- dash_ref.tolerance(params, n, L, 0), with its closed-form, scan
  (n U L: the scan's summation order is not replicated here) and Newton parts.
* d_dir: the direction is a normalised vector, which marker_ref bounds by E = 12 U per component, taken at a parameter that is
  off by at most d_point of arc length: the unit tangent turns by the curvature per unit of arc length, and the curvature is at
  most |B''| / |B'|^2 (the reference evaluates it at the sample; 0 on a line).  d_dir = E + d_point |B''| / |B'|^2.
* rho = hypot(x - h, y + dy), the glyph point's lever arm: an error of the direction moves the point by rho times it.
* the placement itself is x - h, y + dy and two fused multiply-adds per coordinate: 4 roundings of values of at most
  2 Mx, Mx = max|P| + rho; (roundings + 1) U magnitudes, as dash_ref counts: 10 U Mx.

For svgr_path_sample the point is within d_point + 10 U max|P| and each component of the direction within d_dir.

Clearance (`detail["clearance"]`): the smaller of (a) the smallest |B'(t)| over the located samples on cubics relative to the
segment's control-polygon length and (b) the smallest distance of a query from 0, L and any joint between segments relative
to L.  Below it the direction, the inside flag -- which glyphs are visible -- or the segment is a matter of rounding.
`detail["fragile"]` marks the queries within FRAGILE = 1e-6 L of 0, L or a joint.  `exact=True` says that the case is made of
axis-aligned lines of integer length and of queries that are multiples of 1/4: every sum and every comparison is then the same
under every association, nothing is decided by rounding, and (b) does not apply -- such cases may sit on joints and ends.
"""
from __future__ import annotations

import math

import numpy as np

from tests import dash_ref as D
from tests import marker_ref as M
from tests.dash_ref import CLOSED, CUBIC, LINE, QUAD, UNCLOSED, concat, from_segments, polyline  # noqa: F401  (the case builders)

U = 2.0 ** -53
LD = np.longdouble
FRAGILE = 1e-6
_NUM = D._Num(True)


class Measured:
    """A path measured once in long double: per-segment lengths, the cubics' tables, cum and L."""

    def __init__(self, types, params, sizes=None):
        self.types = np.asarray(types, dtype=np.int32)
        self.params = np.asarray(params, dtype=np.float64).reshape(-1, 8)
        n = len(self.types)
        q = self.params.astype(LD)
        self.lens = np.zeros(n, dtype=LD)
        line = (self.types == LINE) | (self.types == CLOSED)
        dx, dy = q[:, 2] - q[:, 0], q[:, 3] - q[:, 1]
        self.lens[line] = np.sqrt(dx * dx + dy * dy)[line]
        cub = np.flatnonzero(self.types == CUBIC)
        self.tabs = {}
        if len(cub):
            c = [q[cub, k] for k in range(8)]
            subs = D.sub_lengths(_NUM, c)            # 32 arrays, one value per cubic each (dash_ref's arithmetic, vectorised)
            acc, tab = np.zeros(len(cub), dtype=LD), []
            for v in subs:
                acc = acc + v
                tab.append(acc)
            tab = np.stack(tab, axis=1)
            for row, i in enumerate(cub):
                self.tabs[int(i)] = list(tab[row])
            self.lens[cub] = tab[:, -1]
        self.cum = np.zeros(n + 1, dtype=LD)
        for i in range(n):                           # (a sequential sum)
            self.cum[i + 1] = self.cum[i] + self.lens[i]
        self.L = self.cum[n] if n else LD(0)
        self.real = np.flatnonzero(self.lens > 0)    # the segments of non-zero length
        self.joints = np.unique(np.concatenate([self.cum[self.real], [self.L]]).astype(np.float64)) if len(self.real) else np.zeros(0)

    @property
    def n(self):
        return len(self.types)


def _frame(m: Measured, s):
    """(P (2,), u (2,), inside, kappa, speed relative to the control polygon (inf off a cubic)) at the arc length s."""
    s = LD(s)
    if not m.L > 0:
        p = m.params[0] if m.n else np.zeros(8)
        return (LD(p[0]), LD(p[1])), (LD(1), LD(0)), False, 0.0, math.inf
    inside = bool(0 <= s <= m.L)
    sc = min(max(s, LD(0)), m.L)
    if sc >= m.L:
        i = int(m.real[-1])
        r = m.lens[i]
    else:
        i = int(m.real[np.flatnonzero(m.cum[m.real] <= sc)[-1]])
        r = sc - m.cum[i]
    c = [LD(v) for v in m.params[i]]
    ln = m.lens[i]
    if m.types[i] != CUBIC:
        dx, dy = c[2] - c[0], c[3] - c[1]
        return (c[0] + dx * (r / ln), c[1] + dy * (r / ln)), M.unit(dx, dy), inside, 0.0, math.inf
    t = LD(0) if not r > 0 else (LD(1) if not r < ln else D.invert(_NUM, c, m.tabs[i], r))
    w = 1 - t
    pt = tuple(w * w * w * c[a] + 3 * w * w * t * c[2 + a] + 3 * w * t * t * c[4 + a] + t * t * t * c[6 + a] for a in range(2))
    d1 = tuple(3 * (w * w * (c[2 + a] - c[a]) + 2 * w * t * (c[4 + a] - c[2 + a]) + t * t * (c[6 + a] - c[4 + a])) for a in range(2))
    d2 = tuple(6 * (w * (c[4 + a] - 2 * c[2 + a] + c[a]) + t * (c[6 + a] - 2 * c[4 + a] + c[2 + a])) for a in range(2))
    u = M.unit(*d1)
    sp2 = d1[0] * d1[0] + d1[1] * d1[1]
    poly = sum(np.sqrt((c[2 * k + 2] - c[2 * k]) ** 2 + (c[2 * k + 3] - c[2 * k + 1]) ** 2) for k in range(3))
    if u is None:
        dirs = M.seg_dirs(CUBIC, m.params[i])
        u = dirs[0] if t < 0.5 else dirs[1]
        return pt, u, inside, math.inf, 0.0
    kappa = float(np.sqrt(d2[0] * d2[0] + d2[1] * d2[1]) / sp2)
    return pt, u, inside, kappa, float(np.sqrt(sp2) / poly)


def point_tolerance(m: Measured):
    """d_point of the module docstring."""
    return D.tolerance(m.params, m.n, float(m.L), 0.0)


def sample(types, params, sizes, s, exact=False, detail=None, measured=None):
    """(xy (n, 2) long double, direction (n, 2) long double, inside (n,) bool, tol_xy (n,), tol_dir (n,), L)."""
    m = Measured(types, params, sizes) if measured is None else measured
    s = np.asarray(s, dtype=np.float64).reshape(-1)
    n = len(s)
    xy, uv = np.zeros((n, 2), dtype=LD), np.zeros((n, 2), dtype=LD)
    inside, tol_xy, tol_dir = np.zeros(n, dtype=bool), np.zeros(n), np.zeros(n)
    fragile = np.zeros(n, dtype=bool)
    d_point = point_tolerance(m)
    clearance = math.inf
    L = float(m.L)
    for k in range(n):
        p, u, ins, kappa, rel_speed = _frame(m, s[k])
        xy[k], uv[k], inside[k] = p, u, ins
        tol_xy[k] = d_point + 10 * U * max(1.0, abs(float(p[0])), abs(float(p[1])))
        tol_dir[k] = M.E_UNIT + d_point * kappa
        if L > 0:
            gap = float(np.min(np.abs(m.joints - s[k]))) / L if len(m.joints) else math.inf
            fragile[k] = gap < FRAGILE
            if not exact:
                clearance = min(clearance, gap)
            clearance = min(clearance, rel_speed)
    if detail is not None:
        detail.update(clearance=clearance, fragile=fragile, length=L, d_point=d_point)
    return xy, uv, inside, tol_xy, tol_dir, m.L


def place(types, params, sizes, atlas_types, atlas_params, glyph_seg_off, inst_glyph, inst_s_mid, inst_half, inst_dy, exact=False,
          detail=None):
    """(params (n_out, 8) long double, tolerance (n_out,), visible (n_inst,) bool, row offsets (n_inst + 1,), L): every instance's
    atlas segments in instance order, placed; the rows of a hidden instance are 0."""
    atlas_types = np.asarray(atlas_types, dtype=np.int32)
    atlas_params = np.asarray(atlas_params, dtype=np.float64).reshape(-1, 8)
    off = np.asarray(glyph_seg_off, dtype=np.int64)
    inst_glyph = np.asarray(inst_glyph, dtype=np.int64)
    d = {}
    xy, uv, visible, _txy, tol_dir, L = sample(types, params, sizes, inst_s_mid, exact, d)
    rows = np.concatenate([[0], np.cumsum((off[1:] - off[:-1])[inst_glyph])]).astype(np.int64) if len(inst_glyph) else np.zeros(1, dtype=np.int64)
    out, tol = np.zeros((int(rows[-1]), 8), dtype=LD), np.zeros(int(rows[-1]))
    for k, g in enumerate(inst_glyph):
        if not visible[k]:
            continue
        h, dy = LD(inst_half[k]), LD(inst_dy[k])
        (px, py), (ux, uy) = xy[k], uv[k]
        for j, a in enumerate(range(int(off[g]), int(off[g + 1]))):
            np_ = 4 if atlas_types[a] == CUBIC else 2
            rho_max = 0.0
            for p in range(np_):
                x, y = LD(atlas_params[a, 2 * p]) - h, LD(atlas_params[a, 2 * p + 1]) + dy
                out[rows[k] + j, 2 * p] = px + ux * x - uy * y
                out[rows[k] + j, 2 * p + 1] = py + uy * x + ux * y
                rho_max = max(rho_max, float(np.hypot(x, y)))
            mx = max(abs(float(px)), abs(float(py))) + rho_max
            tol[rows[k] + j] = d["d_point"] + rho_max * tol_dir[k] + 10 * U * max(1.0, mx)   # (the segment's largest lever arm)
    if detail is not None:
        detail.update(d)
    return out, tol, visible, rows, L


def check_sample(got, want, fragile=None, exact=False, what=""):
    """Flags exactly, points and directions within tolerance; at a fragile query of a case that is not exact the flag is free and
    the direction is compared only when it passes.  Returns the largest error / tolerance."""
    gxy, guv, gin = got
    wxy, wuv, win, tol_xy, tol_dir, _L = want
    assert gxy.shape == wxy.shape and guv.shape == wuv.shape, (what, gxy.shape, wxy.shape)
    if not len(win):
        return 0.0
    free = np.zeros(len(win), dtype=bool) if fragile is None or exact else np.asarray(fragile)
    assert (np.asarray(gin)[~free] == win[~free]).all(), (what, "inside", np.flatnonzero(np.asarray(gin) != win)[:8])
    e_xy = np.abs(np.asarray(gxy, dtype=LD) - wxy).max(axis=1).astype(np.float64) / tol_xy
    e_uv = np.abs(np.asarray(guv, dtype=LD) - wuv).max(axis=1).astype(np.float64) / tol_dir
    e_uv[free] = 0.0   # (on a joint the two sides' directions are both right)
    share = np.maximum(e_xy, e_uv)
    share[~np.isfinite(share)] = 0.0   # (a vanishing derivative: the direction is a rule, its tolerance infinite)
    assert (share <= 1.0).all(), (what, int(np.argmax(share)), float(share.max()))
    return float(share.max())


def check_place(got, want, fragile=None, exact=False, what=""):
    """Visible flags exactly (but at fragile anchors of a case that is not exact), rows of instances both sides show within
    tolerance, rows of hidden instances 0.  Returns the largest error / tolerance."""
    gp, gvis = got
    wp, tol, wvis, rows, _L = want
    assert gp.shape == wp.shape and len(gvis) == len(wvis), (what, gp.shape, wp.shape)
    free = np.zeros(len(wvis), dtype=bool) if fragile is None or exact else np.asarray(fragile)
    assert (np.asarray(gvis)[~free] == wvis[~free]).all(), (what, "visible", np.flatnonzero(np.asarray(gvis) != wvis)[:8])
    worst = 0.0
    for k in range(len(wvis)):
        a, b = int(rows[k]), int(rows[k + 1])
        if a == b:
            continue
        if not gvis[k]:
            assert not np.asarray(gp[a:b]).any(), (what, "hidden rows", k)
        if gvis[k] and wvis[k] and not free[k]:
            err = np.abs(np.asarray(gp[a:b], dtype=LD) - wp[a:b]).max(axis=1).astype(np.float64) / tol[a:b]
            worst = max(worst, float(err.max()))
            assert (err <= 1.0).all(), (what, k, float(err.max()))
    return worst
