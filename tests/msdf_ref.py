"""Host reference of multi-channel distance fields (csrc/svgr_msdf.h), restated in numpy, one operation per line:
nothing of the HIP code goes in, and nothing is culled.  The A channel is tests/sdf_ref.py's signed distance of the group's edges.

    per edge      x, y, inv of sdf_ref;  rl = 1.0 / sqrt(len2) if len2 > 0 else 0.0;  an edge with rl == 0 is no candidate
    per pair      da = pa - a0;  db = pb - b0;  s = da*x + db*y;  t = s * inv
                  t <= 0:     d2c = da*da + db*db;                               se = s
                  t >= 1:     ea = pa - a1;  eb = pb - b1;  d2c = ea*ea + eb*eb;  se = ea*x + eb*y
                  otherwise:  d2c = sdf_ref's d2;                                 se = 0
                  o = (se*se) * inv;  perp = (x*db - da*y) * rl
    better        d2c < best_d2, or equal and o < best_o, or both equal and perp > best_perp
    channel c     over the edges whose path's colour has bit c; A where nothing was kept, where the point is not finite, or where
                  the spread is finite and best_d2 >= spread*spread; else clamp(-sigma * best_perp)
    repair        m = median(r, g, b);  r = g = b = A where (m < 0) != (A < 0)
    union         per channel the smaller value, from +spread

numpy evaluates every line as one rounded operation on float64 arrays, so this equals the header compiled with -ffp-contract=off bit
for bit on a CPU (tests/test_msdf_host.py asserts that).
"""
import numpy as np

from tests import sdf_ref as R


def prepare(edges):
    """(E, 8): a0, b0, x, y, inv, a1, b1, rl."""
    e = np.asarray(edges, dtype=np.float64).reshape(-1, 4)
    a0, b0, a1, b1 = e[:, 0], e[:, 1], e[:, 2], e[:, 3]
    x = a1 - a0
    y = b1 - b0
    xx = x * x
    yy = y * y
    len2 = xx + yy
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(len2 > 0.0, 1.0 / len2, 0.0)
        ln = np.sqrt(len2)
        rl = np.where(len2 > 0.0, 1.0 / ln, 0.0)
    return np.stack([a0, b0, x, y, inv, a1, b1, rl], axis=1)


def median(r, g, b):
    lo = np.where(r < g, r, g)
    hi = np.where(r < g, g, r)
    mid = np.where(hi < b, hi, b)
    return np.where(lo < mid, mid, lo)


def group(edges, masks, evenodd, sigma, spread, points):
    """One group: edges (E, 4) with a colour mask each.  Returns ((n, 4) R G B A, (n,) bool: the repair changed the point)."""
    e = np.asarray(edges, dtype=np.float64).reshape(-1, 4)
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    n = len(pts)
    finite = np.isfinite(pts).all(axis=1)
    pa = np.where(finite, pts[:, 0], np.nan)
    pb = np.where(finite, pts[:, 1], np.nan)
    zero = np.zeros(len(e), dtype=np.int64)
    a = R.finish(R.min_d2(e, zero, 1, pts), R.inside(e, zero, 1, pts, np.array([evenodd], dtype=np.uint8)), spread)[:, 0]
    bd2 = np.full((3, n), np.inf)
    bo = np.full((3, n), np.inf)
    bp = np.full((3, n), -np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        for (a0, b0, x, y, inv, a1, b1, rl), mask in zip(prepare(e).tolist(), masks):
            if not rl > 0.0:
                continue
            da = pa - a0
            db = pb - b0
            m0 = da * x
            m1 = db * y
            s = m0 + m1
            t = s * inv
            tc = np.where(t < 0.0, 0.0, np.where(t > 1.0, 1.0, t))
            tx = tc * x
            ty = tc * y
            qa = a0 + tx
            qb = b0 + ty
            fa = pa - qa
            fb = pb - qb
            fa2 = fa * fa
            fb2 = fb * fb
            d2mid = fa2 + fb2
            da2 = da * da
            db2 = db * db
            d2lo = da2 + db2
            ea = pa - a1
            eb = pb - b1
            ea2 = ea * ea
            eb2 = eb * eb
            d2hi = ea2 + eb2
            n0 = ea * x
            n1 = eb * y
            shi = n0 + n1
            d2c = np.where(t <= 0.0, d2lo, np.where(t >= 1.0, d2hi, d2mid))
            se = np.where(t <= 0.0, s, np.where(t >= 1.0, shi, 0.0))
            se2 = se * se
            o = se2 * inv
            c0 = x * db
            c1 = da * y
            cr = c0 - c1
            perp = cr * rl
            for c in range(3):
                if int(mask) >> c & 1:
                    better = (d2c < bd2[c]) | ((d2c == bd2[c]) & ((o < bo[c]) | ((o == bo[c]) & (perp > bp[c]))))
                    bd2[c] = np.where(better, d2c, bd2[c])
                    bo[c] = np.where(better, o, bo[c])
                    bp[c] = np.where(better, perp, bp[c])
    out = np.empty((n, 4))
    reach = spread * spread
    for c in range(3):
        own = finite & (bd2[c] < np.inf) & ~((spread < np.inf) & (bd2[c] >= reach))
        pseudo = -bp[c] if sigma > 0 else bp[c]
        out[:, c] = np.where(own, R.clamp(pseudo, spread), a)
    med = median(out[:, 0], out[:, 1], out[:, 2])
    repair = (med < 0.0) != (a < 0.0)
    changed = repair & ((out[:, 0] != a) | (out[:, 1] != a) | (out[:, 2] != a))
    for c in range(3):
        out[:, c] = np.where(repair, a, out[:, c])
    out[:, 3] = a
    return out, changed


def msdf(edges, edge_path, colour, rules, group_off, orient, points, spread):
    """(n, 4) R, G, B, A over the groups, and the number of (point, group) pairs the repair changed."""
    e = np.asarray(edges, dtype=np.float64).reshape(-1, 4)
    ep = np.asarray(edge_path, dtype=np.int64).reshape(-1)
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    best = np.full((len(pts), 4), float(spread))
    repairs = 0
    for g in range(len(orient)):
        p0, p1 = int(group_off[g]), int(group_off[g + 1])
        if p1 <= p0:
            continue
        sel = (ep >= p0) & (ep < p1)
        v, changed = group(e[sel], np.asarray(colour)[ep[sel]], int(rules[p0]) & 1, int(orient[g]), spread, pts)
        repairs += int(changed.sum())
        best = np.where(v < best, v, best)
    return best, repairs


def a_channel(edges, edge_path, rules, group_off, orient, points, spread):
    """sdf_ref's union over the groups taken as paths."""
    e = np.asarray(edges, dtype=np.float64).reshape(-1, 4)
    ep = np.asarray(edge_path, dtype=np.int64).reshape(-1)
    n_groups = len(orient)
    group_of = np.searchsorted(np.asarray(group_off)[1:], ep, side="right")
    keep = group_of < n_groups
    g_rules = np.array([int(rules[group_off[g]]) & 1 if group_off[g + 1] > group_off[g] else 0 for g in range(n_groups)], dtype=np.uint8)
    d = R.distance(e[keep], group_of[keep], n_groups, points, g_rules, spread)
    return R.union(d, spread)
