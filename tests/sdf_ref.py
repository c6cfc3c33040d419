"""Host reference of signed distance fields (csrc/svgr_sdf.h), restated in numpy, one operation per line: nothing of
the HIP code goes in, and nothing is culled (the kernels' cull is restated by itself: `out_of_reach`).

An edge is (a0, b0) -> (a1, b1) and a point (pa, pb), in the coordinate order of svgr_batch_all_edges (tests/hit_ref.py).

    per edge      x = a1 - a0;  y = b1 - b0;  len2 = x*x + y*y;  inv = 1.0 / len2 if len2 > 0 else 0.0
    per pair      da = pa - a0;  db = pb - b0
                  t  = clamp((da*x + db*y) * inv, 0, 1)
                  qa = a0 + t*x;  qb = b0 + t*y
                  d2 = (pa - qa)*(pa - qa) + (pb - qb)*(pb - qb)
    per path      d = sqrt(min d2); +inf for a path without edges and for a NaN / infinite point
                  signed: d = -d where hit_ref's inside holds (nonzero / even-odd of hit_ref's winding number)
                  d = min(max(d, -spread), spread)
    encodings     v = 0.5 - d / (2*spread);  F32: float32(v);  U8: rint(v * 255) saturated to [0, 255]
    union         min over the paths of d

numpy evaluates every line below as one rounded operation on float64 arrays; there is no fused form to fall into, so this equals
the header compiled with -ffp-contract=off bit for bit on a CPU (tests/test_sdf_host.py asserts that).

THE TOLERANCE against a device (`tolerance`, `unit_tolerance`).  Every operation above is an IEEE basic operation with one
correctly rounded result, except where a device's maths library could supply its own: the division `1.0 / len2` (per edge) and the
final `sqrt`.  Assume each of those within 1 ulp of the exact result instead of correctly rounded, i.e. a relative error of at most e = 2^-52 between device and host, and propagate (u = 2^-53 is the rounding
of one basic operation, 2u = e; M is the largest coordinate magnitude among the path's edges; primes are the device's values):

    inv           |inv' - inv| <= e |inv|
    t             before the clamp t = fl(s * inv) with the same s on both sides: |t' - t| <= e |s inv| + 2u |s inv| = 2e |t|.  The clamp
                  is monotone and 1-Lipschitz and |t| <= 1 + 2e wherever the two sides do not clamp to the same bound:
                  |t' - t| <= 3e
    t*x           |x| |t' - t| + 2u |x| <= 4e |x| <= 8e M                                (|x| <= 2M)
    qa            |qa' - qa| <= 8e M + 2u |qa| <= 9e M                                   (|qa| <= M(1 + 4u): between the ends)
    ea = pa - qa  |ea' - ea| <= 9e M + 2u |ea| = 9e M + e |ea|                           (and the same for eb)
    d2            |d2' - d2| <= 2 (|ea| + |eb|) 9e M + 2e (ea^2 + eb^2) + 2 (9e M + e d)^2 + 2e d2       (the last: the roundings
                  of the two squares and of the sum, both sides)
                             <= 26 e M d + 4e d^2 + 2 (9e M + e d)^2 =: D(d)             (|ea| + |eb| <= sqrt(2) d)
    min           each side's minimum is at most the other side's value on the same edge plus D there, so the minima differ by at
                  most D taken at the larger of the two distances; D is evaluated at d (1 + 2^-20), which covers that
    sqrt          |sqrt(a) - sqrt(b)| <= |a - b| / sqrt(a) and <= sqrt(|a - b|), whichever is smaller, plus e d for the device's
                  sqrt and its rounding:            tol(d) = min(D / d, sqrt(D)) + 2e d
    sign, clamp   the sign is the integer predicate of hit_ref, the same on both sides; the clamp is 1-Lipschitz: tol stays, and
                  where |d| - tol > spread both sides are the spread itself: 0
    v             the same correctly rounded operations on both sides, monotone in d: v' lies between v(d - tol) and v(d + tol),
                  which is v -+ tol / (2*spread) up to the roundings of the quotient and the difference (the factor 1 + 4e)
    F32 / U8      rounding is monotone: the result lies between the roundings of v - bound and v + bound (times 255 and its own
                  rounding, for U8) -- equal, so exact, unless a rounding boundary of the target lies within the bound of v; then
                  one float32 ulp / one code

On a device whose double division and square root are correctly rounded, as IEEE 754 asks, the difference is 0; DESIGN.md 7r
records what was seen.
"""
from fractions import Fraction

import numpy as np

from tests import hit_ref

E = 2.0 ** -52


def min_d2(edges, edge_path, n_paths, points, block=2048):
    """(n_points, n_paths) float64: the smallest d2 over every path's edges; +inf for a path without edges and for a point that is
    not finite.  edges: (E, 2, 2) or (E, 4); edge_path: (E,)."""
    e = np.asarray(edges, dtype=np.float64).reshape(-1, 4)
    ep = np.asarray(edge_path, dtype=np.int64).reshape(-1)
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    out = np.full((len(pts), n_paths), np.inf)
    if len(e) == 0 or len(pts) == 0:
        return out
    order = np.argsort(ep, kind="stable")
    e, ep = e[order], ep[order]
    starts = np.searchsorted(ep, np.arange(n_paths + 1))
    a0, b0, a1, b1 = e[:, 0], e[:, 1], e[:, 2], e[:, 3]
    x = a1 - a0
    y = b1 - b0
    xx = x * x
    yy = y * y
    len2 = xx + yy
    with np.errstate(divide="ignore"):
        inv = np.where(len2 > 0.0, 1.0 / len2, 0.0)
    block = max(1, min(block, 2_000_000 // len(e)))
    with np.errstate(invalid="ignore", over="ignore"):
        for i0 in range(0, len(pts), block):
            pa, pb = pts[i0:i0 + block, 0:1], pts[i0:i0 + block, 1:2]
            finite = np.isfinite(pa) & np.isfinite(pb)
            da = pa - a0
            db = pb - b0
            m0 = da * x
            m1 = db * y
            s = m0 + m1
            t = s * inv
            t = np.where(t < 0.0, 0.0, np.where(t > 1.0, 1.0, t))
            tx = t * x
            ty = t * y
            qa = a0 + tx
            qb = b0 + ty
            ea = pa - qa
            eb = pb - qb
            ea2 = ea * ea
            eb2 = eb * eb
            d2 = ea2 + eb2
            d2 = np.where(finite, d2, np.inf)
            for p in range(n_paths):
                if starts[p + 1] > starts[p]:
                    out[i0:i0 + block, p] = d2[:, starts[p]:starts[p + 1]].min(axis=1)
    return out


def clamp(d, spread):
    d = np.where(d < -spread, -spread, d)
    return np.where(d > spread, spread, d)


def inside(edges, edge_path, n_paths, points, rules):
    """(n_points, n_paths) bool: hit_ref's predicate."""
    return hit_ref.inside(hit_ref.winding(edges, edge_path, n_paths, points), rules)


def finish(d2, inside_flags, spread=np.inf, signed=True):
    """The clamped distances from the smallest d2 and the inside flags (both (n_points, n_paths))."""
    d = np.sqrt(d2)
    if signed:
        d = np.where(inside_flags, -d, d)
    return clamp(d, spread)


def distance(edges, edge_path, n_paths, points, rules=None, spread=np.inf, signed=True):
    """(n_points, n_paths) float64: the clamped distances, negative inside when `signed`."""
    rules = np.zeros(n_paths, dtype=np.uint8) if rules is None else np.asarray(rules, dtype=np.uint8)
    return finish(min_d2(edges, edge_path, n_paths, points), inside(edges, edge_path, n_paths, points, rules) if signed else None, spread, signed)


def union(d, spread):
    """(n_points,) from (n_points, n_paths) clamped distances: their minimum; +spread over no paths."""
    d = np.asarray(d, dtype=np.float64)
    return np.minimum(d.min(axis=1), spread) if d.shape[1] else np.full(len(d), float(spread))


def unit(d, spread):
    two = 2.0 * spread
    r = np.asarray(d, dtype=np.float64) / two
    return 0.5 - r


def encode_f32(d, spread):
    return unit(d, spread).astype(np.float32)


def encode_u8(d, spread):
    r = np.rint(unit(d, spread) * 255.0)       # (nearest-even)
    return np.where(r >= 0.0, np.where(r > 255.0, 255.0, r), 0.0).astype(np.uint8)


def encode(d, spread, out):
    return d if out == "f64" else encode_f32(d, spread) if out == "f32" else encode_u8(d, spread)


# ---- the kernels' cull (sdf_out_of_reach of csrc/svgr_sdf.h) ---------------------------------------------------------
def out_of_reach_clauses(ext, box, cull_spread):
    """(4, n) bool: the predicate's clauses one by one -- the extent beyond the box at larger b, at smaller b, at smaller a, and at
    larger a (the side the rays run through, with its 2^-400 condition) -- for ext (n, 4) = min a, min b, max a, max b, box (n, 5) =
    lo_a, hi_a, lo_b, hi_b, min |pb| and cull_spread (n,); all False where cull_spread is +inf."""
    ext, box = np.asarray(ext, dtype=np.float64).reshape(-1, 4), np.asarray(box, dtype=np.float64).reshape(-1, 5)
    s = np.broadcast_to(np.asarray(cull_spread, dtype=np.float64), (len(ext),))
    mna, mnb, mxa, mxb = ext.T
    lo_a, hi_a, lo_b, hi_b, min_absb = box.T
    with np.errstate(invalid="ignore", over="ignore"):
        big = np.maximum(np.maximum(np.abs(mna), np.abs(mxa)), np.maximum(np.abs(mnb), np.abs(mxb)))
        t0 = s * (1.0 + 2.0 ** -40)
        t1 = 2.0 ** -40 * big
        thr = t0 + t1
        clauses = np.array([mnb - hi_b > thr, lo_b - mxb > thr, lo_a - mxa > thr, (min_absb >= 2.0 ** -400) & (mna - hi_a > thr)])
    return clauses & (s < np.inf)


def out_of_reach(ext, box, cull_spread):
    """(n,) bool: the path may be left out for every point of the box."""
    return out_of_reach_clauses(ext, box, cull_spread).any(axis=0)


# ---- the tolerance (derived in the module's docstring) ---------------------------------------------------------------------------
def magnitude(edges, edge_path, n_paths):
    """(n_paths,) M: the largest coordinate magnitude among each path's edges (0 for a path without edges)."""
    e = np.abs(np.asarray(edges, dtype=np.float64).reshape(-1, 4)).max(axis=1, initial=0.0)
    m = np.zeros(n_paths)
    np.maximum.at(m, np.asarray(edge_path, dtype=np.int64).reshape(-1), e)
    return m


def tolerance(d, big, spread=np.inf):
    """tol(d) for UNCLAMPED distances `d` and magnitudes `big` that broadcast against them (``magnitude(...)[None, :]`` for
    (n_points, n_paths) distances; for a union the largest over the paths).  Infinite distances compare exactly: 0.  So do
    distances beyond the spread by more than their tolerance: both sides clamp to the spread itself."""
    a = np.abs(np.asarray(d, dtype=np.float64))
    big = np.asarray(big, dtype=np.float64)
    fin = np.isfinite(a)
    dd = np.where(fin, a, 0.0) * (1.0 + 2.0 ** -20)
    D = 26.0 * E * big * dd + 4.0 * E * dd * dd + 2.0 * (9.0 * E * big + E * dd) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        by_d = np.where(dd > 0.0, D / dd, np.inf)
    tol = np.where(fin, np.minimum(by_d, np.sqrt(D)) + 2.0 * E * dd, 0.0)
    return np.where(fin & (a - tol > spread), 0.0, tol)


def unit_tolerance(tol, spread):
    return np.asarray(tol) / (2.0 * spread) * (1.0 + 4.0 * E)


def f32_bounds(v, tol):
    """The float32 values a device may give for the reference's double `v` known to `tol`: rounding is monotone, so they lie
    between float32(v - tol) and float32(v + tol); where the two are equal no rounding boundary is within the tolerance and the
    result must be that value."""
    v = np.asarray(v, dtype=np.float64)
    return (v - tol).astype(np.float32), (v + tol).astype(np.float32)


def u8_bounds(v, tol):
    """The same for the uint8 codes: of v * 255, known to tol * 255 plus the product's own rounding."""
    s = np.asarray(v, dtype=np.float64) * 255.0
    slack = np.asarray(tol) * 255.0 + 255.0 * E

    def code(x):
        return np.clip(np.rint(x), 0.0, 255.0).astype(np.uint8)

    return code(s - slack), code(s + slack)


# ---- exact rational arithmetic ----------------------------------------------------------------------------------------------------
def d2_exact(edges, point):
    """The exact squared distance of one finite point to a list of edges, a Fraction."""
    pa, pb = Fraction(float(point[0])), Fraction(float(point[1]))
    best = None
    for a0, b0, a1, b1 in np.asarray(edges, dtype=np.float64).reshape(-1, 4).tolist():
        a0, b0, a1, b1 = Fraction(a0), Fraction(b0), Fraction(a1), Fraction(b1)
        x, y = a1 - a0, b1 - b0
        len2 = x * x + y * y
        t = ((pa - a0) * x + (pb - b0) * y) / len2 if len2 else Fraction(0)
        t = min(max(t, Fraction(0)), Fraction(1))
        qa, qb = a0 + t * x, b0 + t * y
        d2 = (pa - qa) ** 2 + (pb - qb) ** 2
        best = d2 if best is None or d2 < best else best
    return best
