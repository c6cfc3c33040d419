"""Shapes and points shared by the hit-testing tests (tests/test_hit_host.py on the CPU, tests/test_gpu_hit.py on the device).
Coordinates are (a, b) in the order of the renderer's edges: a polygon given here is drawn as it stands under the identity."""
import math

import numpy as np

# a rectangle a in [2, 10], b in [2, 8]: two of its edges run along a (b0 == b1: they never count), one is `up`, one is `down`
SQUARE = [(2.0, 2.0), (10.0, 2.0), (10.0, 8.0), (2.0, 8.0)]
# a triangle whose apex (6, 9) is a local extremum in b, and whose base runs along a
TRIANGLE = [(1.0, 3.0), (11.0, 3.0), (6.0, 9.0)]

NAN, INF = float("nan"), float("inf")
# (point, winding of SQUARE, winding of TRIANGLE) worked out by hand from the predicate
SEAM_POINTS = [
    ((2.0, 2.0), 1, 0),      # a vertex: it belongs to the edge that starts there in b, and a == 2 is not left of the `down` edge
    ((10.0, 2.0), 0, 0),     # the vertex across: d == 0 on the `up` edge
    ((2.0, 8.0), 0, 0),      # b == 8 is the open end of both vertical edges
    ((5.0, 2.0), 1, 0),      # on an edge that runs along a (b0 == b1): that edge never counts, the others do
    ((6.0, 8.0), 0, 1),      # on the far edge along a: outside the square, inside the triangle
    ((5.0, 9.0), 0, 0),      # level with the triangle's apex, a local extremum: neither edge at the apex counts
    ((6.0, 9.0), 0, 0),      # the apex itself
    ((6.0, 3.0), 1, 1),      # on the triangle's base
    ((0.0, 3.0), 0, 0),      # level with the base, in front of it
    ((NAN, 5.0), 0, 0), ((5.0, NAN), 0, 0), ((INF, 5.0), 0, 0), ((-INF, 5.0), 0, 0), ((5.0, INF), 0, 0), ((5.0, -INF), 0, 0),
]


def polygon_edges(pts):
    """(n, 4) closed polygon edges (a0, b0, a1, b1)."""
    p = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    return np.concatenate([p, np.roll(p, -1, axis=0)], axis=1)


def regular_polygon(n, radius=20.0, centre=(32.25, 31.5), phase=0.1):
    """n corners: a path that flattens into exactly n edges."""
    t = phase + 2.0 * math.pi * np.arange(n) / n
    return np.stack([centre[0] + radius * np.cos(t), centre[1] + radius * np.sin(t)], axis=1)


def pentagram(radius=28.0, centre=(32.0, 32.0)):
    t = -math.pi / 2 + 2.0 * math.pi * (2 * np.arange(5) % 5) / 5
    return np.stack([centre[0] + radius * np.cos(t), centre[1] + radius * np.sin(t)], axis=1)


def random_polygons(seed, n_paths, lo=3, hi=9, extent=40):
    """Integer-coordinate polygons (d is exact on integer points): a list of (k, 2) arrays."""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, extent, size=(int(rng.integers(lo, hi)), 2)).astype(np.float64) for _ in range(n_paths)]


def edge_table(polys):
    """(edges (E, 4), edge_path (E,), off (n + 1,)) of a list of polygons; an empty polygon (0 corners) has no edges."""
    edges = [polygon_edges(p) if len(p) else np.zeros((0, 4)) for p in polys]
    off = np.concatenate([[0], np.cumsum([len(e) for e in edges])]).astype(np.int32)
    ep = np.concatenate([np.full(len(e), i, dtype=np.int32) for i, e in enumerate(edges)]) if edges else np.zeros(0, dtype=np.int32)
    return (np.concatenate(edges) if edges else np.zeros((0, 4))), ep, off
