"""Fixtures and the host harness shared by the multi-channel distance-field tests (tests/test_msdf_host.py on the CPU,
tests/test_gpu_msdf.py on the device).  Coordinates are (a, b) in the order of the renderer's edges, as in tests/hit_cases.py."""
import ctypes

import numpy as np

from tests import hit_cases
from tests.util import host_build

P = ctypes.c_void_p
NAN, INF = float("nan"), float("inf")

# a square of side 8 (1 / 8 is a double: every perpendicular distance to a dyadic point is exact), counter-clockwise in (a, b), an
# edge a path, coloured as colour_edges colours a subpath of four corners
SQUARE = [(2.0, 2.0), (10.0, 2.0), (10.0, 10.0), (2.0, 10.0)]
SQUARE_COLOURS = [6, 5, 3, 5]
# an L whose sides are 16 and 8, counter-clockwise; the reflex corner is (8, 8), between the edges 2 (b == 8) and 3 (a == 8)
L_SHAPE = [(0.0, 0.0), (16.0, 0.0), (16.0, 8.0), (8.0, 8.0), (8.0, 16.0), (0.0, 16.0)]
L_COLOURS = [6, 5, 3, 6, 5, 3]
# legs of Pythagorean triangles in dyadic numbers: (dx, dy, hypotenuse)
LEGS = [(1.5, 2.0, 2.5), (2.0, 1.5, 2.5), (0.75, 1.0, 1.25), (3.0, 4.0, 5.0), (2.5, 6.0, 6.5)]


def lib():
    h = host_build("msdf_harness")
    h.mh_median.restype = ctypes.c_double
    h.mh_median.argtypes = [ctypes.c_double] * 3
    return h


def ptr(a):
    return a.ctypes.data_as(P)


class Shape:
    """Groups of paths as svgr_batch_msdf takes them: `groups` is a list of (sigma, [(mask, edges (k, 4) or a polygon (k, 2))]);
    `rules` one per group.  A path may have no edges and a group no paths."""

    def __init__(self, groups, rules=None):
        edges, off, colour, group_off, orient, path_rule = [], [0], [], [0], [], []
        rules = [0] * len(groups) if rules is None else rules
        for (sigma, paths), rule in zip(groups, rules):
            for mask, e in paths:
                e = np.asarray(e, dtype=np.float64)
                e = hit_cases.polygon_edges(e) if e.ndim == 2 and e.shape[1] == 2 and len(e) else e.reshape(-1, 4)
                edges.append(e)
                off.append(off[-1] + len(e))
                colour.append(mask)
                path_rule.append(rule)
            group_off.append(len(colour))
            orient.append(sigma)
        self.edges = np.ascontiguousarray(np.concatenate(edges) if edges else np.zeros((0, 4)))
        self.off = np.array(off, dtype=np.int32)
        self.colour = np.array(colour, dtype=np.uint8)
        self.rules = np.array(path_rule, dtype=np.uint8)
        self.group_off = np.array(group_off, dtype=np.int32)
        self.orient = np.array(orient, dtype=np.int8)
        self.edge_path = np.repeat(np.arange(len(colour), dtype=np.int32), np.diff(self.off))

    def only(self, g):
        """Group g alone."""
        p0, p1 = int(self.group_off[g]), int(self.group_off[g + 1])
        paths = [(int(self.colour[p]), self.edges[self.off[p]:self.off[p + 1]]) for p in range(p0, p1)]
        return Shape([(int(self.orient[g]), paths)], [int(self.rules[p0]) if p1 > p0 else 0])


def harness(shape, points, spread=INF):
    """(n, 4) float64 R, G, B, A from the header compiled for the host."""
    pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2)
    out = np.full((len(pts), 4), 99.0)
    lib().mh_msdf(ptr(shape.edges), ptr(shape.off), ptr(shape.rules), ptr(shape.colour), ptr(shape.group_off), ptr(shape.orient),
                  ctypes.c_longlong(len(shape.orient)), ptr(pts), ctypes.c_longlong(len(pts)), ctypes.c_double(spread), ptr(out))
    return out


def harness_edges(edges, edge_path, n_paths, rules, colour, group_off, orient, points, spread=INF):
    """The same on a batch's own flattened edges (``batch.all_edges()``), grouped by path for the harness."""
    e = np.asarray(edges, dtype=np.float64).reshape(-1, 4)
    ep = np.asarray(edge_path, dtype=np.int64)
    order = np.argsort(ep, kind="stable")
    shape = Shape([])
    shape.edges = np.ascontiguousarray(e[order])
    shape.off = np.searchsorted(ep[order], np.arange(n_paths + 1)).astype(np.int32)
    shape.colour, shape.rules = np.ascontiguousarray(colour, dtype=np.uint8), np.ascontiguousarray(rules, dtype=np.uint8)
    shape.group_off, shape.orient = np.ascontiguousarray(group_off, dtype=np.int32), np.ascontiguousarray(orient, dtype=np.int8)
    return harness(shape, points, spread)


def harness_encode(d, spread):
    d = np.ascontiguousarray(d, dtype=np.float64)
    f32, u8 = np.zeros(d.shape, dtype=np.float32), np.zeros(d.shape, dtype=np.uint8)
    lib().mh_encode(ptr(d), ctypes.c_longlong(d.size), ctypes.c_double(spread), ptr(f32), ptr(u8))
    return f32, u8


def one_edge_a_path(polygon, colours, sigma=1):
    """A polygon as one group, every edge a path of its own with the colour given."""
    e = hit_cases.polygon_edges(polygon)
    return (sigma, [(c, e[k:k + 1]) for k, c in enumerate(colours)])


def square_wedge_points():
    """(points outside SQUARE in the wedge of each vertex, their (dx, dy, hypot) beyond the vertex)."""
    pts, legs = [], []
    for (va, vb), (sa, sb) in zip(SQUARE, [(-1, -1), (1, -1), (1, 1), (-1, 1)]):
        for dx, dy, h in LEGS:
            pts.append((va + sa * dx, vb + sb * dy))
            legs.append((dx, dy, h))
    return np.array(pts), np.array(legs)


def random_shape(seed, n_groups=5):
    """Random integer polygons dealt into groups of 0 .. 3 paths with random masks, sigma and rules; with an empty path inside a
    group, an empty group, zero-length edges and an edge twice in opposite directions."""
    rng = np.random.default_rng(seed)
    groups, rules = [], []
    for g in range(n_groups):
        paths = []
        for poly in hit_cases.random_polygons(seed * 100 + g, int(rng.integers(1, 4))):
            e = hit_cases.polygon_edges(poly)
            k = int(rng.integers(0, len(e)))
            extra = [e[k, [2, 3, 0, 1]], e[k], [e[k, 0], e[k, 1], e[k, 0], e[k, 1]]]     # back and forth again: still closed; a point
            paths.append((int(rng.integers(1, 8)), np.concatenate([e, extra])))
        if g == 1:
            paths.insert(1, (7, np.zeros((0, 4))))
        if g == 3:
            paths = []
        groups.append((int(rng.choice([-1, 1])), paths))
        rules.append(int(rng.integers(0, 2)))
    return Shape(groups, rules)


def random_points(seed, shape, n=200):
    rng = np.random.default_rng(seed)
    corners = shape.edges[:, :2]
    mids = (shape.edges[:, :2] + shape.edges[:, 2:]) / 2.0
    half = rng.integers(-6, 86, size=(n, 2)).astype(np.float64) / 2.0
    return np.concatenate([rng.uniform(-5.0, 45.0, size=(n, 2)), half, corners, mids, [(NAN, 5.0), (5.0, INF), (-INF, NAN), (1e9, -1e9)]])
