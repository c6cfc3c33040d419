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


def scattered_points(seed, n, extent=40.0):
    """Scattered points, a few on integer positions (vertices and edges of the integer polygons), a few far away, one NaN."""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-3.0, extent + 3.0, size=(n, 2))
    k = n // 4
    pts[:k] = rng.integers(0, int(extent), size=(k, 2))
    if n > 8:
        pts[-1] = (np.nan, 5.0)
        pts[-2] = (1e9, -1e9)
        pts[-3] = (-np.inf, 5.0)
    return pts


# ---- the rounds of the path table: k_hit_winding takes the paths 256 at a time ---------------------------------------------------
TABLE_ROUND_COUNTS = (255, 256, 257, 513)
TABLE_ROUND_EMPTY = (0, 255, 256)                                  # (and the last path): the end of round one, the start of round two
TABLE_ROUND_LISTED = (1, 31, 32, 33, 254, 257, 258, 511, 512)      # the paths on both sides of a word seam and of a round seam


class TableRoundCase:
    """`polys` (an emptied path has no corners), `rules`, `pickable`, `points`; `empty` and `listed`: the indices the condition
    names."""

    def __init__(self, n_paths):
        from tests import sdf_cases  # noqa: PLC0415  (sdf_cases imports this module)

        tris = sdf_cases.tiny_triangles(n_paths, size=40.0, seed=n_paths)
        self.empty = sorted({i for i in TABLE_ROUND_EMPTY + (n_paths - 1,) if 0 <= i < n_paths})
        self.polys = [np.zeros((0, 2)) if i in self.empty else t for i, t in enumerate(tris)]
        self.listed = [i for i in TABLE_ROUND_LISTED if i < n_paths and i not in self.empty]
        self.rules = (np.arange(n_paths) % 3 == 1).astype(np.uint8)
        self.pickable = np.arange(n_paths) % 5 != 0
        centroids = [tris[i].mean(axis=0) for i in self.listed]
        corners = np.concatenate([tris[i] for i in (self.listed[0], self.listed[-1], n_paths // 2)])   # (nine of the triangles' own)
        self.points = np.concatenate([scattered_points(n_paths, 120 - len(centroids) - len(corners)), centroids, corners])
        self.n_paths = n_paths

    def check(self, winding):
        """The case's condition on the reference's (n_points, n_paths) winding numbers."""
        assert winding.shape == (len(self.points), self.n_paths)
        for i in self.listed:
            assert (winding[:, i] != 0).any(), f"path {i} holds no query point"
        for i in self.empty:
            assert (winding[:, i] == 0).all(), f"the emptied path {i} has a winding number"


def table_round_case(n_paths):
    return TableRoundCase(n_paths)


# ---- clip tables across the words of a row and the rounds of the table -----------------------------------------------------------
CLIP_TABLE_SEED = 25   # (searched: the first seed under which every clip below bites and lets pass)


class ClipTableCase:
    def __init__(self, seed=CLIP_TABLE_SEED):
        n = self.n_paths = 300
        self.polys = random_polygons(seed, n)
        self.points = scattered_points(seed + 1, 600)
        clips = [() for _ in range(n)]
        for p in (31, 32, 33, 255, 256):        # the chains 30 <- 31 <- 32 <- 33 and 254 <- 255 <- 256 <- 257
            clips[p] = ((p - 1,),)
        clips[64] = ((0,),)
        clips[257] = ((256,), (256,))           # the chain's group, and a second one: bit 0 of word 8
        clips[288] = ((287,),)                  # a source in the user's own word
        clips[299] = ((3, 255), (256, 290))     # earlier words and the user's own word inside one group
        clips[100] = ((),)                      # a group without sources: never passes
        self.clips = clips
        self.clipped = [p for p in range(n) if clips[p] and p != 100]
        self.pickable = np.arange(n) % 7 != 3
        self.rules = np.zeros(n, dtype=np.uint8)

    def check(self, inside, ok):
        """The case's conditions on the reference's inside and pass flags, (n_points, 300) each: every clip bites and lets pass."""
        for p in self.clipped:
            assert (inside[:, p] & ~ok[:, p]).any() and ok[:, p].any(), f"path {p}: its clips do not bite, or let nothing pass"
        assert inside[:, 100].any() and not ok[:, 100].any()


def clip_table_case():
    return ClipTableCase()


# ---- the cull of k_hit_winding: points on a path's extent -------------------------------------------------------------------------
def cull_boundary_points(polygon):
    """For an integer polygon of extent [mna, mxa] x [mnb, mxb]: pa in {mna, mxa, a value strictly inside} crossed with pb in
    {mnb, mxb, a value strictly inside}, and the four points one unit outside each side: (13, 2)."""
    p = np.asarray(polygon, dtype=np.float64).reshape(-1, 2)
    (mna, mnb), (mxa, mxb) = p.min(axis=0), p.max(axis=0)
    assert mxa - mna >= 2 and mxb - mnb >= 2, "the extent has no integer strictly inside"
    ia, ib = mna + np.floor((mxa - mna) / 2), mnb + np.floor((mxb - mnb) / 2)
    pts = [(a, b) for a in (mna, mxa, ia) for b in (mnb, mxb, ib)]
    pts += [(mna - 1, ib), (mxa + 1, ib), (ia, mnb - 1), (ia, mxb + 1)]
    return np.array(pts, dtype=np.float64)


def cull_polygons():
    """SQUARE, TRIANGLE and two of the random polygons, as (k, 2) arrays."""
    return [np.array(SQUARE), np.array(TRIANGLE)] + random_polygons(21, 2, lo=5)


def edge_table(polys):
    """(edges (E, 4), edge_path (E,), off (n + 1,)) of a list of polygons; an empty polygon (0 corners) has no edges."""
    edges = [polygon_edges(p) if len(p) else np.zeros((0, 4)) for p in polys]
    off = np.concatenate([[0], np.cumsum([len(e) for e in edges])]).astype(np.int32)
    ep = np.concatenate([np.full(len(e), i, dtype=np.int32) for i, e in enumerate(edges)]) if edges else np.zeros(0, dtype=np.int32)
    return (np.concatenate(edges) if edges else np.zeros((0, 4))), ep, off
