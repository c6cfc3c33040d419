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


polygon_edges, edge_table, random_polygons, regular_polygon, pentagram = (hit_cases.polygon_edges, hit_cases.edge_table, hit_cases.random_polygons,
                                                                          hit_cases.regular_polygon, hit_cases.pentagram)
SQUARE, TRIANGLE = hit_cases.SQUARE, hit_cases.TRIANGLE
