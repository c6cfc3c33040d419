"""Shapes, points and worked values shared by the distance-field tests (tests/test_sdf_host.py on the CPU, tests/test_gpu_sdf.py on
the device).  Coordinates are (a, b) in the order of the renderer's edges, as in tests/hit_cases.py."""
import math

import numpy as np

from tests import hit_cases

NAN, INF = float("nan"), float("inf")

# an axis-aligned rectangle a in [2, 10], b in [2, 8] (hit_cases.SQUARE) and its closed-form signed distance
RECT = (2.0, 2.0, 10.0, 8.0)


def rect_distance(rect, points):
    """The signed distance to an axis-aligned box in the max / hypot formulation: with q = |p - centre| - half size,
    hypot(max(q, 0)) + min(max(qa, qb), 0).  Independent of the projection-onto-edges arithmetic."""
    a0, b0, a1, b1 = rect
    p = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    qa = np.abs(p[:, 0] - (a0 + a1) / 2.0) - (a1 - a0) / 2.0
    qb = np.abs(p[:, 1] - (b0 + b1) / 2.0) - (b1 - b0) / 2.0
    return np.hypot(np.maximum(qa, 0.0), np.maximum(qb, 0.0)) + np.minimum(np.maximum(qa, qb), 0.0)


# 3-4-5: (point, distance to hit_cases.SQUARE) with the nearest feature a corner, exactly 5 away, or an edge, exactly 3 / 4 away
PYTHAGOREAN = [((-1.0, -2.0), 5.0), ((14.0, 11.0), 5.0), ((13.0, 12.0), 5.0), ((-2.0, 11.0), 5.0), ((6.0, -1.0), 3.0), ((14.0, 5.0), 4.0),
               ((6.0, 5.0), -3.0), ((5.0, 4.0), -2.0)]


def u8_tie_distances(spread):
    """Distances whose value v = 0.5 - d / (2*spread) lands on or next to (k + 1/2) / 255 for every code k: the uint8 rounding's
    boundaries.  Some products v * 255 are k + 1/2 exactly (always the one of d = 0: 127.5) and must go to the even code."""
    k = np.arange(255, dtype=np.float64)
    d = (0.5 - (k + 0.5) / 255.0) * (2.0 * spread)
    return np.concatenate([d, np.nextafter(d, INF), np.nextafter(d, -INF), [0.0, -0.0]])


def integer_points(seed, n, extent=40):
    """Integer and half-integer points over and around the integer polygons of hit_cases.random_polygons."""
    rng = np.random.default_rng(seed)
    return rng.integers(-6, 2 * extent + 6, size=(n, 2)).astype(np.float64) / 2.0


def tiny_triangles(n, size=64.0, seed=5):
    """n small triangles scattered over [0, size)^2: (list of (3, 2) arrays)."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(1.0, size - 1.0, size=(n, 2))
    t = rng.uniform(0.0, 2.0 * math.pi, size=n)
    r = rng.uniform(0.4, 1.2, size=n)
    k = np.arange(3) * 2.0 * math.pi / 3.0
    return [np.stack([c[i, 0] + r[i] * np.cos(t[i] + k), c[i, 1] + r[i] * np.sin(t[i] + k)], axis=1) for i in range(n)]


def overlapping_squares():
    """Two squares, a in [0, 10] x b in [0, 10] and a in [6, 16] x b in [0, 10]: their overlap is a in [6, 10]."""
    return [np.array([(0.0, 0.0), (10.0, 0.0), (10.0, 10.0), (0.0, 10.0)]), np.array([(6.0, 0.0), (16.0, 0.0), (16.0, 10.0), (6.0, 10.0)])]


# ---- cases for the kernels' cull (sdf_out_of_reach of csrc/svgr_sdf.h): a closed polygon, a spread and the points of a box beside it
REACH_SIDES = 4      # the box lies at smaller b than the polygon, at larger b, at larger a, at smaller a (its rays run through the polygon)
REACH_MODES = ("below", "above", "far", "near", "overlap", "tiny")


def reach_threshold(ext, spread):
    """The predicate's thr for one extent (min a, min b, max a, max b), in its own operations."""
    return spread * (1.0 + 2.0 ** -40) + 2.0 ** -40 * float(np.abs(np.asarray(ext)).max())


def extent_of(polygons):
    """min a, min b, max a, max b over the corners of one polygon or of a list of them."""
    v = np.concatenate([np.asarray(p, dtype=np.float64).reshape(-1, 2) for p in (polygons if isinstance(polygons, list) else [polygons])])
    return np.array([v[:, 0].min(), v[:, 1].min(), v[:, 0].max(), v[:, 1].max()])


def box_of(points):
    """lo_a, hi_a, lo_b, hi_b, min |pb| of finite points: what a workgroup reduces."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    return np.array([p[:, 0].min(), p[:, 0].max(), p[:, 1].min(), p[:, 1].max(), np.abs(p[:, 1]).min()])


def reach_case(rng, side, mode):
    """(polygon (k, 2), spread, points (9, 2)): a box whose gap to the polygon's extent on `side` is thr * (1 - 2^-30) ("below"),
    thr * (1 + 2^-30) ("above"), many thr ("far"), a fraction of thr ("near") or negative ("overlap"); "tiny" is "far" with a corner
    at |pb| = 2^-450.  The points are the box's corners and its points nearest the extent's corners and centre.  Spreads run over
    2^-100 .. 2^40 and coordinates up to 2^50; near the threshold the coordinates stay within 2^12 spreads, so that the gap can be
    set to 2^-30 of thr."""
    k = rng.choice([-100.0, 40.0]) if rng.random() < 0.1 else rng.uniform(-100.0, 40.0)
    spread = 2.0 ** k if k in (-100.0, 40.0) else 2.0 ** k * rng.uniform(1.0, 2.0)
    spread = min(spread, 2.0 ** 40)
    c = 2.0 ** min(k + rng.uniform(0.0, 12.0), 49.0) if mode in ("below", "above") else 2.0 ** rng.uniform(max(k - 3.0, -100.0), 49.0)
    r = c * rng.uniform(0.05, 0.5)
    centre = c * rng.uniform(-1.0, 1.0, size=2)
    if mode == "tiny":
        centre[1] = r * rng.uniform(-0.5, 0.5)       # the polygon's b range reaches across 0, where the box's corner will be
    poly = centre + r * rng.uniform(-1.0, 1.0, size=(int(rng.integers(3, 8)), 2))
    ext = extent_of(poly)
    thr = reach_threshold(ext, spread)
    gap = {"below": thr * (1.0 - 2.0 ** -30), "above": thr * (1.0 + 2.0 ** -30), "far": thr * 2.0 ** rng.uniform(0.01, 8.0),
           "tiny": thr * 2.0 ** rng.uniform(0.01, 8.0), "near": thr * rng.uniform(0.0, 0.95), "overlap": -r * rng.uniform(0.0, 1.0)}[mode]
    width = r * rng.uniform(0.0, 1.0, size=2) * (rng.random(2) < 0.8)      # (a box may be a segment or one point)
    axis = 1 if side < 2 else 0                                           # the axis the gap is on
    other = 1 - axis
    lo, hi = np.zeros(2), np.zeros(2)
    if side in (0, 3):                                                    # the box at smaller b / smaller a than the polygon
        hi[axis] = ext[axis] - gap
        lo[axis] = hi[axis] - width[axis]
    else:
        lo[axis] = ext[2 + axis] + gap
        hi[axis] = lo[axis] + width[axis]
    if rng.random() < 0.7 or mode == "tiny":                              # beside the polygon: no other clause can hold
        lo[other] = rng.uniform(ext[other], ext[2 + other])
    else:                                                                 # off its corner
        lo[other] = ext[2 + other] + thr * rng.uniform(0.0, 10.0)
    hi[other] = lo[other] + width[other]
    if mode == "tiny":
        lo[1], hi[1] = 2.0 ** -450 * rng.choice([-1.0, 0.0, 1.0]), max(hi[1], 2.0 ** -450)
    corners = [(lo[0], lo[1]), (lo[0], hi[1]), (hi[0], lo[1]), (hi[0], hi[1])]
    targets = [(ext[0], ext[1]), (ext[0], ext[3]), (ext[2], ext[1]), (ext[2], ext[3]), ((ext[0] + ext[2]) / 2.0, (ext[1] + ext[3]) / 2.0)]
    nearest = [(min(max(a, lo[0]), hi[0]), min(max(b, lo[1]), hi[1])) for a, b in targets]
    return poly, spread, np.array(corners + nearest)


def reach_cases(seed, n):
    """n cases, the sides and the modes taking turns: (side, mode, polygon, spread, points).  |pb| only matters beside the polygon
    in a, so "tiny" takes those two sides."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        side, mode = i % REACH_SIDES, REACH_MODES[i // REACH_SIDES % len(REACH_MODES)]
        side = 2 + (side & 1) if mode == "tiny" else side
        out.append((side, mode) + reach_case(rng, side, mode))
    return out


polygon_edges, edge_table, random_polygons, regular_polygon, pentagram = (hit_cases.polygon_edges, hit_cases.edge_table, hit_cases.random_polygons,
                                                                          hit_cases.regular_polygon, hit_cases.pentagram)
SQUARE, TRIANGLE = hit_cases.SQUARE, hit_cases.TRIANGLE
