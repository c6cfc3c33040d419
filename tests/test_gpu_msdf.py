"""Multi-channel distance fields on the GPU: svgr_batch_msdf through the C ABI against the per-lane header compiled for the host
(tests/msdf_harness.cpp, which has no cull) on the batch's own flattened edges (``batch.all_edges()``), bit for bit, at the seams of
the launch geometry -- 256 points per workgroup, 256 edges per LDS stage, 256 paths per round of the path table, a group across two
rounds --; the cull on every side; the scratch passes; the encodings; the errors; ``Font.msdf_atlas`` on the committed fonts against
``Font.sdf_atlas``; and ``Path.msdf`` against the mitres worked out by hand in tests/test_msdf_host.py."""
import os

import numpy as np
import pytest

from tests import msdf_cases as cases
from tests import sdf_cases
from tests.test_gpu_hit import query_points
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import svgrasterize_amd as S

    S.Context.get()
    return S


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32 if a.dtype == np.float32 else np.uint8)


class Built:
    """A tests/msdf_cases.Shape as a batch: every path a soup of lines under the identity, and the harness on what the batch kept."""

    def __init__(self, S, shape):
        from svgrasterize_amd import _abi

        self.shape = shape
        n = len(shape.colour)
        segs = np.zeros((len(shape.edges), 8))
        segs[:, :4] = shape.edges
        self.batch = _abi.Batch(S.Context.get(), segs, np.zeros(len(segs), dtype=np.uint8), shape.off.astype(np.int64), np.tile(S.Transform().m6(), (n, 1)),
                                shape.rules, np.zeros((n, 4)), viewport=None)
        self.kept = None

    def want(self, points, spread):
        if self.kept is None:
            self.kept = self.batch.all_edges()
        s = self.shape
        return cases.harness_edges(self.kept[0], self.kept[1], len(s.colour), s.rules, s.colour, s.group_off, s.orient, points, spread)

    def got(self, points=None, grid=None, spread=np.inf, out="f64", scratch_bytes=0):
        s = self.shape
        return self.batch.msdf(s.colour, s.group_off, s.orient, points, grid, spread, out, scratch_bytes)

    def check(self, points, spreads=(np.inf, 3.0), grid=None):
        """Every encoding of the query against the harness, bit for bit (but for the sign of a zero in float64)."""
        for spread in spreads:
            want = self.want(points, spread)
            got = self.got(None if grid else points, grid, spread)
            assert got.shape == want.shape and got.dtype == np.float64
            assert np.array_equal(got, want), f"spread {spread}: {int((got != want).sum())} of {got.size} values differ from the header's"
            if spread < np.inf:
                f32, u8 = cases.harness_encode(want, spread)
                assert np.array_equal(bits(self.got(None if grid else points, grid, spread, "f32")), bits(f32))
                assert np.array_equal(self.got(None if grid else points, grid, spread, "u8"), u8)
        return want


def grid_points(grid):
    rr, cc = np.meshgrid(np.arange(grid[2]), np.arange(grid[3]), indexing="ij")
    return np.stack([grid[0] + rr.ravel() + 0.5, grid[1] + cc.ravel() + 0.5], axis=1)


@pytest.fixture(scope="module")
def random_built(S):
    return Built(S, cases.random_shape(7))


# ---- the launch seams -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_point_counts_at_the_workgroup_seams(S, random_built, n):
    pts = query_points(n, n) if n > 8 else np.array([(11.5, 17.25)])          # (with a NaN, an infinite and a far point from 9 on)
    want = random_built.check(pts)
    assert want.shape == (n, 4)
    if n > 8:
        assert (want[-1] == 3.0).all() and (want[-3] == 3.0).all() and (want[:, 3] < 0).any() and (want[:, 0] != want[:, 3]).any()


def test_a_grid_at_a_negative_origin(S, random_built):
    grid = (-3, 5, 17, 33)             # not a multiple of the tile in either direction: two tiles by three
    want = random_built.check(grid_points(grid), grid=grid)
    assert (want[:, 3] < 0).any() and (want[:, :3] != want[:, 3:]).any()
    a, b = random_built.got(grid=grid, spread=2.5), random_built.got(grid_points(grid), spread=2.5)
    assert np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_edge_counts_at_the_chunk_seams(S, n):
    assert S.load_library().svgr_hit_chunk() == 256
    poly = sdf_cases.regular_polygon(n)
    built = Built(S, cases.Shape([(1, [(5, poly)])]))
    rng = np.random.default_rng(n)
    pts = np.concatenate([rng.uniform(5.0, 60.0, size=(250, 2)), poly[:16]])
    want = built.check(pts)
    assert len(built.kept[0]) == n and 0.2 < (want[:, 3] < 0).mean() < 0.9
    assert (want[:, 1] == want[:, 3]).all()                     # green has no edge: it is A


def test_a_group_across_two_rounds_of_the_path_table(S):
    assert S.load_library().svgr_hit_block() == 256
    tris = sdf_cases.tiny_triangles(86, size=40.0, seed=3)
    # 86 groups of 3 paths, an edge each: the group of the paths 255 .. 257 straddles the round
    by_three = cases.Shape([cases.one_edge_a_path(t, [6, 5, 3], sigma=1 if k % 2 else -1) for k, t in enumerate(tris)], rules=[k % 3 == 1 for k in range(86)])
    assert len(by_three.colour) == 258
    pts = np.concatenate([query_points(5, 120), np.concatenate(tris)[-9:], [t.mean(axis=0) for t in tris[-30:]]])
    want = Built(S, by_three).check(pts, spreads=(np.inf, 1.5))
    assert (want[-30:, 3] < 0).all()
    # 85 groups of 3, then a square of 4 paths on the paths 255 .. 258, then a triangle behind it
    square = np.array(cases.SQUARE) + 12.0
    mixed = cases.Shape([cases.one_edge_a_path(t, [6, 5, 3]) for t in tris[:85]] + [cases.one_edge_a_path(square, cases.SQUARE_COLOURS),
                                                                                  cases.one_edge_a_path(tris[85], [6, 5, 3])])
    assert mixed.group_off[85] == 255 and mixed.group_off[86] == 259
    wedge = cases.square_wedge_points()[0] + 12.0
    want = Built(S, mixed).check(np.concatenate([pts, wedge, [(18.0, 18.0)]]), spreads=(np.inf, 0.5))
    assert want[-1].tolist() == [-0.5] * 4


# ---- the cull ---------------------------------------------------------------------------------------------------------------------
def test_groups_out_of_reach_on_every_side(S):
    near = [(7, np.array([(-1.0, -1.0), (3.0, -1.5), (2.0, 3.0), (-2.0, 2.5)]))]
    far = [np.array(cases.SQUARE) + shift for shift in ((100.0, -6.0), (-120.0, -6.0), (-6.0, 100.0), (-6.0, -120.0), (80.0, 80.0), (-90.0, -90.0), (6.0, -6.0))]
    groups = [(1, near)] + [cases.one_edge_a_path(sq, cases.SQUARE_COLOURS, sigma=-1 if k % 2 else 1) for k, sq in enumerate(far)]
    built = Built(S, cases.Shape(groups, rules=[0, 1, 0, 1, 0, 1, 0, 0]))
    rng = np.random.default_rng(4)
    pts = np.concatenate([rng.uniform(-5.0, 5.0, size=(200, 2)), rng.uniform(-5.0, 5.0, size=(56, 2)) + (0.0, 1e-3)])
    assert (np.abs(pts[:, 1]) >= 2.0 ** -400).all()
    for spread in (2.0, 6.0, 20.0):
        want = built.check(pts, spreads=(spread,))              # every side is cut, the one the rays run through too
        assert (want[:, 3] < 0).any() and ((want == spread).all(axis=1).any() or spread > 2.0)
    # a point on the line b == 0 up to 2^-500: the side the rays run through is then kept
    tiny = pts.copy()
    tiny[17] = (1.0, 2.0 ** -500)
    tiny[18] = (-4.5, -(2.0 ** -420))
    for spread in (2.0, 20.0):
        built.check(tiny, spreads=(spread,))
    # the same points in a grid's tiles and as scattered points fall into other workgroups: the same bits
    grid = (-40, -40, 80, 80)
    centres = grid_points(grid)
    order = rng.permutation(len(centres))
    for out in ("f64", "u8"):
        tiled, scattered = built.got(grid=grid, spread=6.0, out=out), built.got(centres[order], spread=6.0, out=out)
        assert np.array_equal(bits(tiled[order]), bits(scattered))
    assert np.array_equal(built.got(grid=grid, spread=6.0), built.want(centres, 6.0))


# ---- passes, errors ---------------------------------------------------------------------------------------------------------------
def test_scratch_passes(S, random_built):
    ctx = S.Context.get()
    pts = query_points(4, 1000)
    grid = (-3, 2, 37, 21)
    one = random_built.got(pts)             # (also flattens: not counted below)
    n0 = ctx.launches()
    again = random_built.got(pts)
    n1 = ctx.launches()
    small = random_built.got(pts, scratch_bytes=8 * 4 * 256)          # one workgroup's rows: four passes
    n2 = ctx.launches()
    assert n1 - n0 == 2 and n2 - n1 == 5, (n0, n1, n2)                # (the groups' extents, then a launch per pass)
    assert np.array_equal(bits(one), bits(again)) and np.array_equal(bits(one), bits(small))
    for out, spread in (("f64", np.inf), ("u8", 2.0), ("f32", 2.0)):
        whole = random_built.got(grid=grid, spread=spread, out=out)
        n3 = ctx.launches()
        passes = random_built.got(grid=grid, spread=spread, out=out, scratch_bytes=1)          # a row of tiles at a time: three
        assert ctx.launches() - n3 == 4 and np.array_equal(bits(whole), bits(passes))


def test_errors_and_empty_queries_launch_nothing(S):
    from svgrasterize_amd import _abi

    ctx = S.Context.get()
    lib = S.load_library()
    shape = cases.Shape([cases.one_edge_a_path(cases.SQUARE, cases.SQUARE_COLOURS), (1, [(7, np.array(sdf_cases.TRIANGLE))])], rules=[0, 1])
    built = Built(S, shape)
    built.got(np.zeros((1, 2)))   # (flattened now: what follows must not launch)
    n0 = ctx.launches()
    pts, out = np.zeros((3, 2)), np.zeros((3, 4))
    grid = _abi._i64x4((0, 0, 1, 3))
    good = dict(points=pts, grid=None, n=3, spread=2.0, flags=_abi.SDF_F64, colour=shape.colour, group_off=shape.group_off, orient=shape.orient)

    def call(**change):
        a = dict(good, **change)
        colour, group_off, orient = (np.ascontiguousarray(a["colour"], dtype=np.uint8), np.ascontiguousarray(a["group_off"], dtype=np.int32),
                                     np.ascontiguousarray(a["orient"], dtype=np.int8))
        _abi._check(lib.svgr_batch_msdf(built.batch.handle, _abi.ptr(a["points"]) if a["points"] is not None else None, a["grid"], a["n"], a["spread"], a["flags"],
                                        _abi.ptr(colour), _abi.ptr(group_off), _abi.ptr(orient), len(orient), 0, _abi.ptr(out)))

    for spread in (0.0, -2.0, float("nan"), -np.inf):
        with pytest.raises(ValueError, match="spread"):          # (SVGR_E_INVALID, with a message)
            call(spread=spread)
    for flags in (_abi.SDF_F32, _abi.SDF_U8):
        with pytest.raises(ValueError, match="finite spread"):
            call(spread=np.inf, flags=flags)
    with pytest.raises(ValueError, match="one of them"):
        call(grid=grid)
    with pytest.raises(ValueError, match="one of them"):
        call(points=None)
    for flags in (4, 8, 16, 3, 1 << 20, -1):
        with pytest.raises(ValueError, match="unknown"):
            call(flags=flags)
    with pytest.raises(ValueError, match="rows x cols"):
        call(points=None, grid=grid, n=4)
    for bad in (0, 8, 255):
        colour = shape.colour.copy()
        colour[4] = bad                  # (the triangle's path)
        with pytest.raises(ValueError, match="colour"):
            call(colour=colour)
    for group_off in ([1, 4, 5], [0, 5, 4], [0, 4, 6], [0, -1, 5]):
        with pytest.raises(ValueError, match="group_off"):
            call(group_off=group_off)
    for orient in ([1, 0], [2, 1], [1, -2]):
        with pytest.raises(ValueError, match="orient"):
            call(orient=orient)
    with pytest.raises(ValueError, match="fill rule"):
        call(group_off=[0, 5], orient=[1])
    assert ctx.launches() == n0 and not out.any()
    # n_points == 0 launches nothing and succeeds; groups that cover no path, and no groups, are +spread without a launch
    assert built.got(np.zeros((0, 2))).shape == (0, 4) and built.got(grid=(0, 0, 0, 7)).shape == (0, 4)
    assert (built.batch.msdf(shape.colour, [0], [], pts, spread=2.0) == 2.0).all() and (built.batch.msdf(shape.colour, [0, 0], [-1], pts, spread=2.0, out="u8") == 0).all()
    assert ctx.launches() == n0
    # a group may leave paths behind the last group out: they are ignored
    first = built.batch.msdf(shape.colour, [0, 4], [1], pts + 6.0)
    assert np.array_equal(first, cases.harness_edges(*built.batch.all_edges(), 5, shape.rules, shape.colour, [0, 4], [1], pts + 6.0))
    with pytest.raises(ValueError):
        built.batch.msdf(shape.colour[:3], shape.group_off, shape.orient, pts)
    with pytest.raises(ValueError):
        built.batch.msdf(shape.colour, shape.group_off, shape.orient[:1], pts)


# ---- the library layer ------------------------------------------------------------------------------------------------------------
def test_path_msdf_reproduces_the_mitres(S):
    from svgrasterize_amd import sdf
    from tests.test_gpu_hit import poly_path

    path = poly_path(S, cases.SQUARE)
    field = path.msdf(None, (0, 0, 16, 16), 8.0, np.float64)
    assert field.shape == (16, 16, 4) and field.dtype == np.float64
    med = sdf.median(field)
    assert np.array_equal(field[..., 3], path.sdf(None, (0, 0, 16, 16), 8.0, np.float64))
    c = np.arange(16) + 0.5
    # outside, in the wedge of the vertex (10, 10): the mitre; A is the Euclidean distance there
    dr, dc = np.meshgrid(c[10:] - 10.0, c[10:] - 10.0, indexing="ij")
    assert np.array_equal(med[10:, 10:], np.maximum(dr, dc)) and (field[10:, 10:, 3] > med[10:, 10:]).all()
    assert np.array_equal(med[:2, :2], np.maximum(*np.meshgrid(2.0 - c[:2], 2.0 - c[:2], indexing="ij")))
    # inside: minus the distance to the nearest side, in the median and in A
    rr, cc = np.meshgrid(c[2:10], c[2:10], indexing="ij")
    depth = np.minimum(np.minimum(rr - 2.0, 10.0 - rr), np.minimum(cc - 2.0, 10.0 - cc))
    assert np.array_equal(med[2:10, 2:10], -depth) and np.array_equal(field[2:10, 2:10, 3], -depth)
    # the other dtypes are the same field; a mirror keeps it (sigma flips with the determinant)
    f32, u8 = path.msdf(None, (0, 0, 16, 16)), path.msdf(None, (0, 0, 16, 16), 8.0, np.uint8)
    want32, want8 = cases.harness_encode(field, 8.0)
    assert f32.dtype == np.float32 and np.array_equal(bits(f32), bits(want32)) and np.array_equal(u8, want8)
    mirror = S.Transform().translate(12.0, 0.0).scale(-1.0, 1.0)                  # x -> 12 - x: the square onto itself
    assert np.array_equal(sdf.median(path.msdf(mirror, (0, 0, 16, 16), 8.0, np.float64)), med)
    # a curve: the circle has no corner, every channel is A
    from tests.test_gpu_hit import circle_path

    ring = circle_path(S, (8.0, 8.0), 5.0).msdf(None, (0, 0, 16, 16), 4.0, np.float64)
    assert (ring[..., :3] == ring[..., :1]).all() and ring.min() < -3.0                # white: one nearest edge for all three
    assert np.array_equal(ring[..., 0] < 0, ring[..., 3] < 0) and np.abs(ring[..., 0] - ring[..., 3]).max() < 0.25


@pytest.mark.parametrize("face", ["varsynth.ttf", "varsynth.ttf@wght", "cffsynth.otf"])
def test_msdf_atlas_on_the_committed_fonts(S, face):
    from svgrasterize_amd import sdf

    name, _, axis = face.partition("@")
    with open(os.path.join(GOLDEN, "fonts", name), "rb") as f:
        font = S.read_font(f.read())
    if axis:
        ax = font.axes[0]
        font = font.instance({ax.tag: (ax.default + ax.maximum) / 2.0 if ax.maximum > ax.default else (ax.default + ax.minimum) / 2.0})
    size, spread, text = 40.0, 3.5, "AVo #D VA"
    atlas, plain = font.msdf_atlas(text, size, spread, max_cols=100), font.sdf_atlas(text, size, spread, max_cols=100)
    assert isinstance(atlas, S.SdfAtlas) and atlas.image.dtype == np.uint8 and atlas.image.shape == plain.image.shape + (4,)
    assert atlas.cells == plain.cells and list(atlas.cells) == list(plain.cells) and atlas.size == size and atlas.spread == spread
    assert np.array_equal(atlas.image[..., 3], plain.image)                                        # byte for byte
    assert np.array_equal(sdf.median(atlas.image) >= 128, atlas.image[..., 3] >= 128)
    assert (atlas.image[..., :3] != atlas.image[..., 3:]).any()                                     # (the channels do differ: corners)
    f64 = font.msdf_atlas(text, size, spread, np.float64, max_cols=100)
    want32, want8 = cases.harness_encode(f64.image, spread)
    assert f64.cells == atlas.cells and np.array_equal(want8, atlas.image)
    assert np.array_equal(bits(font.msdf_atlas(text, size, spread, np.float32, max_cols=100).image), bits(want32))
    assert np.array_equal(sdf.median(f64.image) < 0, f64.image[..., 3] < 0)
