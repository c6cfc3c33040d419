"""Hit testing on the GPU: svgr_batch_winding and svgr_batch_pick through the C ABI against the numpy reference (tests/hit_ref.py)
evaluated on the batch's own flattened edges (``batch.all_edges()``), exactly, at the seams of the launch geometry -- B =
svgr_hit_block() points per workgroup, C = svgr_hit_chunk() edges per LDS stage, 32 paths per word of the bit matrix --; the
rounds of the path table (256 paths a round), with clip tables across its words and rounds; the cull's comparisons, which only a
query of one point lets decide; the scratch passes of the pick, for points and for grids; ``Path.contains`` against ``Path.mask`` as
an independent witness that also pins the coordinate order; ``Scene.pick`` / ``Scene.id_map`` / ``Path.stroke_contains``; and the
errors.  tests/test_hit_host.py checks on the CPU that the reference and the per-lane header are the same predicate;
tests/test_gpu_hit_witness.py holds ``Scene.pick`` against what the renderer draws."""
import numpy as np
import pytest

from tests import hit_cases as cases
from tests import hit_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import svgrasterize_amd as S

    S.Context.get()
    return S


@pytest.fixture(scope="module")
def seams(S):
    lib = S.load_library()
    return lib.svgr_hit_block(), lib.svgr_hit_chunk()


def poly_path(S, pts):
    from svgrasterize_amd.geometry import PATH_CLOSED, PATH_LINE

    pts = [tuple(map(float, p)) for p in pts]
    if not pts:
        return S.Path([])
    segs = [(PATH_LINE, [list(a), list(b)]) for a, b in zip(pts, pts[1:])] + [(PATH_CLOSED, [list(pts[-1]), list(pts[0])])]
    return S.Path([segs])


def circle_path(S, centre, radius):
    """Four cubics."""
    from svgrasterize_amd.geometry import PATH_CUBIC

    k = 0.5522847498307936 * radius
    cx, cy = centre
    r = radius
    quads = [[(cx + r, cy), (cx + r, cy + k), (cx + k, cy + r), (cx, cy + r)], [(cx, cy + r), (cx - k, cy + r), (cx - r, cy + k), (cx - r, cy)],
             [(cx - r, cy), (cx - r, cy - k), (cx - k, cy - r), (cx, cy - r)], [(cx, cy - r), (cx + k, cy - r), (cx + r, cy - k), (cx + r, cy)]]
    return S.Path([[(PATH_CUBIC, [list(p) for p in q]) for q in quads]])


def make_batch(S, paths, rules=None, transform=None):
    from svgrasterize_amd import _abi

    packs = [p.packed() for p in paths]
    offs = np.concatenate([[0], np.cumsum([len(pk[0]) for pk in packs])]).astype(np.int64)
    segs = np.concatenate([pk[0] for pk in packs]) if packs else np.zeros((0, 8))
    kinds = np.concatenate([pk[1] for pk in packs]) if packs else np.zeros(0, dtype=np.uint8)
    m6 = (transform if transform is not None else S.Transform()).m6()
    n = len(paths)
    return _abi.Batch(S.Context.get(), segs, kinds, offs, np.tile(m6, (n, 1)), rules if rules is not None else np.zeros(n, dtype=np.uint8),
                      np.zeros((n, 4)), viewport=None)


def query_points(seed, n, extent=40.0):
    return cases.scattered_points(seed, n, extent)


def check_against_reference(S, batch, pts, rules=None):
    n_paths = batch.n_paths
    got = batch.winding(pts)
    edges, edge_path = batch.all_edges()
    want = R.winding(edges, edge_path, n_paths, pts)
    assert got.shape == want.shape and got.dtype == np.int32
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {got.size} winding numbers differ"
    rules = np.zeros(n_paths, dtype=np.uint8) if rules is None else rules
    top, bits = batch.pick(pts, want_bits=True)
    inside = R.inside(want, rules)
    assert np.array_equal(bits, R.pack_bits(inside))
    assert np.array_equal(top, R.resolve(inside, np.ones(n_paths), None)[1])
    return want, edges, edge_path


def test_seams_are_what_the_suite_assumes(S, seams):
    block, chunk = seams
    assert block == 256 and chunk >= 8


@pytest.mark.parametrize("n_paths", [1, 31, 32, 33, 65])
def test_winding_and_bits_across_the_word_seams(S, seams, n_paths):
    block, _chunk = seams
    polys = cases.random_polygons(n_paths, n_paths)
    paths = [poly_path(S, p) for p in polys]
    paths[n_paths // 2] = circle_path(S, (20.0, 21.0), 9.5)   # curves: the renderer's own flattening
    rules = (np.arange(n_paths) % 3 == 1).astype(np.uint8)
    batch = make_batch(S, paths, rules)
    want, _e, _ep = check_against_reference(S, batch, query_points(n_paths, block + 1), rules)
    assert (want != 0).any() and (want == 0).any()


@pytest.mark.parametrize("which", ["1", "block-1", "block", "block+1", "4*block+1"])
def test_point_counts_at_the_workgroup_seams(S, seams, which):
    block, _chunk = seams
    n = {"1": 1, "block-1": block - 1, "block": block, "block+1": block + 1, "4*block+1": 4 * block + 1}[which]
    paths = [poly_path(S, p) for p in cases.random_polygons(77, 3)]
    want, _e, _ep = check_against_reference(S, make_batch(S, paths), query_points(n, n))
    assert want.shape == (n, 3)


@pytest.mark.parametrize("which", ["chunk-1", "chunk", "chunk+1", "2*chunk+1"])
def test_edge_counts_at_the_chunk_seams(S, seams, which):
    block, chunk = seams
    n = {"chunk-1": chunk - 1, "chunk": chunk, "chunk+1": chunk + 1, "2*chunk+1": 2 * chunk + 1}[which]
    batch = make_batch(S, [poly_path(S, cases.regular_polygon(n))])
    rng = np.random.default_rng(n)
    pts = np.concatenate([rng.uniform(5.0, 60.0, size=(block, 2)), cases.regular_polygon(n)[:16]])   # some corners themselves
    want, edges, _ep = check_against_reference(S, batch, pts)
    assert len(edges) == n   # a many-sided polygon: as many edges as corners
    assert 0.2 < (want != 0).mean() < 0.9


def test_an_empty_path_between_two_others(S, seams):
    paths = [poly_path(S, cases.SQUARE), S.Path([]), poly_path(S, cases.TRIANGLE)]
    batch = make_batch(S, paths)
    pts = np.array([p for p, _s, _t in cases.SEAM_POINTS])
    want, _e, edge_path = check_against_reference(S, batch, pts)
    assert 1 not in set(edge_path.tolist())
    # the host file's seam points, with the windings worked out by hand
    assert want[:, 0].tolist() == [s for _p, s, _t in cases.SEAM_POINTS]
    assert want[:, 2].tolist() == [t for _p, _s, t in cases.SEAM_POINTS]
    assert (want[:, 1] == 0).all()


def test_a_transform_with_a_mirror(S, seams):
    block, _chunk = seams
    mirror = S.Transform().translate(40.0, 3.0).scale(-1.0, 0.75)
    paths = [poly_path(S, p) for p in cases.random_polygons(5, 4)] + [circle_path(S, (20.0, 20.0), 12.0)]
    batch = make_batch(S, paths, transform=mirror)
    want, _e, _ep = check_against_reference(S, batch, query_points(9, block + 7))
    assert (want != 0).any() and (want == 0).any()
    # mirrored, the circle winds the other way round
    plain = make_batch(S, paths[-1:]).winding(np.array([[20.0, 20.0]]))[0, 0]
    flipped = make_batch(S, paths[-1:], transform=mirror).winding(np.array([mirror(np.array([[20.0, 20.0]]))[0]]))[0, 0]
    assert plain == -flipped and abs(plain) == 1


def test_grid_points_are_the_pixel_centres(S, seams):
    paths = [poly_path(S, p) for p in cases.random_polygons(11, 5)]
    batch = make_batch(S, paths)
    row0, col0, rows, cols = -3, 2, 37, 21     # not a multiple of the tile in either direction, three tiles by two
    rr, cc = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    centres = np.stack([row0 + rr.ravel() + 0.5, col0 + cc.ravel() + 0.5], axis=1)
    assert np.array_equal(batch.winding(grid=(row0, col0, rows, cols)), batch.winding(centres))
    top_g, bits_g = batch.pick(grid=(row0, col0, rows, cols), want_bits=True)
    top_p, bits_p = batch.pick(centres, want_bits=True)
    assert np.array_equal(top_g, top_p) and np.array_equal(bits_g, bits_p) and (top_p >= 0).any() and (top_p < 0).any()


def test_scratch_passes(S, seams):
    block, _chunk = seams
    n_paths = 33
    polys = cases.random_polygons(3, n_paths)
    batch = make_batch(S, [poly_path(S, p) for p in polys])
    pts = query_points(4, 1000)
    clips = [() for _ in range(n_paths)]
    clips[32] = ((0, 31),)
    clips[20] = ((3,), (4, 5))
    pickable = (np.arange(n_paths) % 5 != 0)
    ctx = S.Context.get()
    top1, bits1 = batch.pick(pts, pickable=pickable, clips=clips, want_bits=True)     # (also flattens: not counted below)
    n0 = ctx.launches()
    top1b, _ = batch.pick(pts, pickable=pickable, clips=clips, want_bits=True)
    n1 = ctx.launches()
    words = (n_paths + 31) // 32
    top3, bits3 = batch.pick(pts, pickable=pickable, clips=clips, scratch_bytes=4 * words * block, want_bits=True)   # one workgroup's rows
    n2 = ctx.launches()
    assert n1 - n0 == 2 and n2 - n1 >= 3 * 2, (n0, n1, n2)    # a winding and a resolve launch per pass: three passes at least
    assert np.array_equal(top1, top1b) and np.array_equal(top1, top3) and np.array_equal(bits1, bits3)
    edges, edge_path = batch.all_edges()
    inside = R.inside(R.winding(edges, edge_path, n_paths, pts), np.zeros(n_paths, dtype=np.uint8))
    ok, top = R.resolve(inside, pickable, clips)
    assert np.array_equal(bits1, R.pack_bits(ok)) and np.array_equal(top1, top)
    assert (top >= 0).any() and (top < 0).any() and (inside[:, 32] & ~ok[:, 32]).any() and ok[:, 32].any()   # (the clips bite)


# ---- the rounds of the path table, the cull's comparisons, grids in passes ---------------------------------------------------------
def check_pick(batch, rules, pickable, clips, want_w, points=None, grid=None, **kw):
    """winding and pick (top and bits) of a query against the reference evaluated on the reference's windings `want_w`."""
    n_paths = batch.n_paths
    got_w = batch.winding(points, grid)
    assert got_w.dtype == np.int32 and got_w.shape == want_w.shape
    assert np.array_equal(got_w, want_w), f"{int((got_w != want_w).sum())} of {got_w.size} winding numbers differ"
    ok, top = R.resolve(R.inside(want_w, rules), pickable, clips)
    got_top, got_bits = batch.pick(points, grid, pickable=pickable, clips=clips, want_bits=True, **kw)
    assert got_bits.shape == (len(want_w), (n_paths + 31) // 32)
    assert np.array_equal(got_bits, R.pack_bits(ok)), f"{int((R.unpack_bits(got_bits, n_paths) != ok).sum())} pass bits differ"
    assert np.array_equal(got_top, top), f"{int((got_top != top).sum())} of {len(top)} tops differ"
    return got_w, got_top, got_bits


def table_round_batch(S, n_paths):
    case = cases.table_round_case(n_paths)
    return case, make_batch(S, [poly_path(S, p) for p in case.polys], case.rules)


def reference_winding(batch, pts):
    edges, edge_path = batch.all_edges()
    return R.winding(edges, edge_path, batch.n_paths, pts)


def grid_centres(grid):
    row0, col0, rows, cols = grid
    rr, cc = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    return np.stack([row0 + rr.ravel() + 0.5, col0 + cc.ravel() + 0.5], axis=1)


@pytest.mark.parametrize("n_paths", cases.TABLE_ROUND_COUNTS)
def test_path_counts_at_the_table_rounds(S, seams, n_paths):
    block, _chunk = seams
    assert block == 256     # the rounds the case is built around
    case, batch = table_round_batch(S, n_paths)
    want = reference_winding(batch, case.points)
    case.check(want)        # paths on both sides of every seam hold a point; the emptied ones -- 0, 255, 256, the last -- hold none
    assert set(batch.all_edges()[1].tolist()) == set(range(n_paths)) - set(case.empty)
    _w, top, _bits = check_pick(batch, case.rules, case.pickable, None, want, case.points)
    assert (top >= 0).any() and (top < 0).any() and not (top % 5 == 0).any()


def test_clip_tables_across_words_and_rounds(S, seams):
    block, _chunk = seams
    case = cases.clip_table_case()
    batch = make_batch(S, [poly_path(S, p) for p in case.polys], case.rules)
    want = reference_winding(batch, case.points)
    inside = R.inside(want, case.rules)
    case.check(inside, R.resolve(inside, case.pickable, case.clips)[0])     # every clip bites and lets pass; path 100 never passes
    _w, top1, bits1 = check_pick(batch, case.rules, case.pickable, case.clips, want, case.points)
    words = (case.n_paths + 31) // 32
    ctx = S.Context.get()
    n0 = ctx.launches()
    top3, bits3 = batch.pick(case.points, pickable=case.pickable, clips=case.clips, scratch_bytes=4 * words * block, want_bits=True)
    assert ctx.launches() - n0 == 2 * 3       # 600 points: three workgroups, one to a pass
    assert np.array_equal(top1, top3) and np.array_equal(bits1, bits3)


def cull_batch(S, shift=0.0):
    polys = [p + shift for p in cases.cull_polygons()]
    pts = np.concatenate([cases.cull_boundary_points(p) for p in cases.cull_polygons()])
    return make_batch(S, [poly_path(S, p) for p in polys]), pts


def test_one_point_queries_on_the_extent(S, seams):
    # a query of one point: the workgroup's extent is that point, and the cull's comparisons with a path's extent decide alone
    batch, pts = cull_batch(S)
    n_paths = batch.n_paths
    rules, pickable = np.zeros(n_paths, dtype=np.uint8), np.array([1, 1, 0, 1], dtype=np.uint8)
    want = reference_winding(batch, pts)
    assert len(pts) == 52 and (want[[6, 13 + 6], [0, 1]] != 0).all()       # (6, 2) on the square's, (6, 3) on the triangle's b == mnb
    rows = [check_pick(batch, rules, pickable, None, want[i:i + 1], pts[i:i + 1]) for i in range(len(pts))]
    together = check_pick(batch, rules, pickable, None, want, pts)
    for k in range(3):
        assert np.array_equal(np.concatenate([r[k] for r in rows]), together[k])
    assert (together[1] == 2).sum() == 0 and (together[1] >= 0).any() and (together[1] < 0).any()


def test_one_pixel_grids_on_the_extent(S, seams):
    # the same for the grid form of the query: polygons with half-integer corners, 1 x 1 grids whose pixel centre lies on an extent
    batch, corners = cull_batch(S, shift=0.5)
    n_paths = batch.n_paths
    rules, pickable = np.zeros(n_paths, dtype=np.uint8), np.ones(n_paths, dtype=np.uint8)
    want = reference_winding(batch, corners + 0.5)
    assert (want[[6, 13 + 6], [0, 1]] != 0).all() and (want == 0).any()
    for i, (r, c) in enumerate(corners.astype(np.int64).tolist()):
        check_pick(batch, rules, pickable, None, want[i:i + 1], grid=(r, c, 1, 1))


def test_grid_queries_in_scratch_passes(S, seams):
    block, _chunk = seams
    n_paths = 40
    batch = make_batch(S, [poly_path(S, p) for p in cases.random_polygons(20, n_paths)])
    rules = np.zeros(n_paths, dtype=np.uint8)
    clips = [() for _ in range(n_paths)]
    clips[33] = ((2, 31),)
    clips[39] = ((33,), (32, 38))
    clips[20] = ((3,), (4, 5))
    pickable = np.arange(n_paths) % 5 != 0
    words = (n_paths + 31) // 32
    assert words == 2
    ctx = S.Context.get()
    batch.winding(np.zeros((1, 2)))   # (flattened now: what follows launches the two kernels of a pass and nothing else)
    for grid in [(-3, 2, 37, 21), (0, 0, 16, 16), (5, -4, 1, 40), (5, -4, 40, 1), (0, 0, 17, 32)]:
        centres = grid_centres(grid)
        want = reference_winding(batch, centres)
        n_groups = -(-grid[2] // 16) * -(-grid[3] // 16)
        runs = []
        for tiles in (None, 1, 3):    # one pass; a tile to a pass; three tiles: a pass ends in the middle of a row of tiles
            n0 = ctx.launches()
            top, bits = batch.pick(grid=grid, pickable=pickable, clips=clips, want_bits=True,
                                   scratch_bytes=0 if tiles is None else 4 * words * block * tiles)
            passes = 1 if tiles is None else -(-n_groups // tiles)
            assert ctx.launches() - n0 == 2 * passes, (grid, tiles)
            runs.append((top, bits))
        for top, bits in runs[1:]:
            assert np.array_equal(top, runs[0][0]) and np.array_equal(bits, runs[0][1]), grid
        _w, top_p, bits_p = check_pick(batch, rules, pickable, clips, want, centres)
        assert np.array_equal(runs[0][0], top_p) and np.array_equal(runs[0][1], bits_p), grid
        if grid[2] * grid[3] > 100:
            inside = R.inside(want, rules)
            assert (top_p >= 0).any() and (inside[:, 39] & ~R.unpack_bits(bits_p, n_paths)[:, 39]).any()    # (the clips bite)


def test_winding_of_a_grid_beyond_one_round(S, seams):
    case, batch = table_round_batch(S, 257)
    grid = (-2, -2, 20, 35)
    centres = grid_centres(grid)
    want = reference_winding(batch, centres)
    got = batch.winding(grid=grid)
    assert np.array_equal(got, batch.winding(centres)) and np.array_equal(got, want)
    assert (want != 0).any(axis=0).sum() > 50           # (tiny triangles: most hold no pixel centre, many do)
    check_pick(batch, case.rules, case.pickable, None, want, grid=grid)


def test_a_fresh_batch_gives_the_same_rows(S, seams):
    # k_hit_place orders a path's edges by atomics: the rows must not depend on that order
    results = []
    for _ in range(2):
        case, batch = table_round_batch(S, 257)
        top, bits = batch.pick(case.points, pickable=case.pickable, want_bits=True)
        results.append((batch.winding(case.points).tobytes(), top.tobytes(), bits.tobytes()))
        batch.destroy()
    assert results[0] == results[1]


# ---- an independent witness: the renderer -----------------------------------------------------------------------------------------
L_SHAPE = [(6.0, 10.0), (50.0, 10.0), (50.0, 22.0), (20.0, 22.0), (20.0, 58.0), (6.0, 58.0)]   # not symmetric under transposition


def witness_shapes(S):
    return [("L", poly_path(S, L_SHAPE), None), ("circle", circle_path(S, (32.3, 31.7), 24.0), None),
            ("pentagram-nonzero", poly_path(S, cases.pentagram()), "nonzero"), ("pentagram-evenodd", poly_path(S, cases.pentagram()), "evenodd")]


@pytest.mark.parametrize("which", range(4), ids=["L", "circle", "pentagram-nonzero", "pentagram-evenodd"])
def test_contains_agrees_with_the_mask(S, which):
    name, path, rule = witness_shapes(S)[which]
    size = 64
    layer, _hull = path.mask(S.Transform(), rule, viewport=(0, 0, size, size))
    cov = np.zeros((size, size))
    x, y = layer.offset
    cov[x:x + layer.height, y:y + layer.width] = layer.image[..., 0]
    rr, cc = np.meshgrid(np.arange(size), np.arange(size), indexing="ij")
    centres = np.stack([rr.ravel() + 0.5, cc.ravel() + 0.5], axis=1)
    inside = path.contains(centres, S.Transform(), rule).reshape(size, size)
    full, empty = cov >= 1 - 1e-9, cov <= 1e-9
    skipped = 1.0 - (full | empty).mean()
    print(f"{name}: {int(full.sum())} full, {int(empty.sum())} empty, skipped share {skipped:.4f}")
    assert inside[full].all(), f"{int((~inside[full]).sum())} fully covered pixels are outside at their centre"
    assert not inside[empty].any(), f"{int(inside[empty].sum())} uncovered pixels are inside at their centre"
    assert skipped <= 0.12 and full.sum() > 100
    if name.startswith("pentagram"):
        centre = path.contains((32.0, 32.0), S.Transform(), rule)
        assert centre.shape == (1,) and bool(centre[0]) == (rule == "nonzero")
        assert abs(int(path.winding((32.0, 32.0))[0])) == 2


# ---- the scene layer --------------------------------------------------------------------------------------------------------------
def test_pick_id_map_and_stroke_contains(S):
    red = np.array([1.0, 0.0, 0.0, 1.0])
    a, b = poly_path(S, [(4, 4), (40, 4), (40, 40), (4, 40)]), poly_path(S, [(20, 20), (60, 20), (60, 60), (20, 60)])
    ring = circle_path(S, (32.0, 32.0), 20.0)
    hidden = poly_path(S, [(44, 2), (62, 2), (62, 16), (44, 16)])
    clip_a, clip_b = poly_path(S, [(0, 0), (30, 0), (30, 30), (0, 30)]), circle_path(S, (48.0, 48.0), 10.0)
    inner = poly_path(S, [(0, 0), (64, 0), (64, 52), (0, 52)])
    clipped = poly_path(S, [(2, 2), (62, 2), (62, 62), (2, 62)])
    clip_scene = S.Scene.group([S.Scene.fill(clip_a, red), S.Scene.fill(clip_b, red).clip(S.Scene.fill(inner, red))])
    scene = S.Scene.group([
        S.Scene.fill(a, red), S.Scene.fill(b, red, S.PATH_FILL_EVENODD),
        S.Scene.stroke(ring, red, 6.0),
        S.Scene.group([S.Scene.fill(hidden, red), S.Scene.fill(hidden, red).transform(S.Transform().translate(0.0, 20.0))]).opacity(0.0),
        S.Scene.fill(clipped, red).clip(clip_scene).transform(S.Transform().translate(1.0, 0.5)),
    ])
    tr = S.Transform().scale(1.0, 0.9)
    rng = np.random.default_rng(12)
    pts = rng.uniform(-2.0, 66.0, size=(700, 2))
    index, leaves = scene.pick(tr, pts)
    assert [l.kind for l in leaves] == ["fill", "fill", "stroke", "fill", "fill", "clip", "clip", "clip", "fill"]
    assert leaves[8].clips == ((5, 7),) and leaves[7].clips == ((6,),)
    # against the reference's resolve of the device's own bits
    rules = np.array([l.rule for l in leaves], dtype=np.uint8)
    batch = make_batch(S, [l.path for l in leaves], rules)
    from svgrasterize_amd import _abi

    m6s = np.ascontiguousarray([l.m6 for l in leaves], dtype=np.float64)
    _abi._check(S.load_library().svgr_batch_set_transforms(batch.handle, m6s.ctypes.data_as(_abi._P)))
    inside = R.inside(batch.winding(pts), rules)
    ok, top = R.resolve(inside, [l.pickable for l in leaves], [l.clips for l in leaves])
    assert np.array_equal(index, top)
    assert {0, 1, 2, 3, 4, 8, -1} <= set(index.tolist()) and not {5, 6, 7} & set(index.tolist())   # opacity 0 is hit; sources never
    assert (inside[:, 8] & ~ok[:, 8]).any()
    # the id map is the pick of the pixel centres
    vp = (-2, 3, 41, 50)
    id_map, leaves2 = scene.id_map(tr, vp)
    rr, cc = np.meshgrid(np.arange(vp[2]), np.arange(vp[3]), indexing="ij")
    centres = np.stack([vp[0] + rr.ravel() + 0.5, vp[1] + cc.ravel() + 0.5], axis=1)
    assert id_map.shape == (41, 50) and id_map.dtype == np.int32 and len(leaves2) == len(leaves)
    assert np.array_equal(id_map.ravel(), scene.pick(tr, centres)[0])
    # a wide stroke: its centre line is inside, the loop it encloses is not
    t = np.linspace(0.0, 2.0 * np.pi, 41)[:-1] + 0.05
    on_line = np.stack([32.0 + 20.0 * np.cos(t), 32.0 + 20.0 * np.sin(t)], axis=1)
    assert ring.stroke_contains(on_line, 6.0).all()
    assert not ring.stroke_contains([(32.0, 32.0), (32.0, 45.0), (20.0, 30.0)], 6.0).any()
    assert ring.contains([(32.0, 32.0)]).all()
    # elements_at on a document: innermost first
    doc = ('<svg xmlns="http://www.w3.org/2000/svg" width="40" height="40"><g id="g"><rect id="r" x="5" y="5" width="20" height="10"/>'
           '<rect id="s" x="10" y="8" width="4" height="4" opacity="0"/></g></svg>')
    dscene, ids, _size = S.svg_scene_from_str(doc)
    assert S.elements_at(dscene, ids, S.Transform(), [(6.0, 6.0), (11.0, 9.0), (30.0, 30.0)]) == [("r", "g"), ("s", "g"), ()]


# ---- errors and empty queries -----------------------------------------------------------------------------------------------------
def test_errors_and_empty_queries_launch_nothing(S, seams):
    from svgrasterize_amd import _abi

    ctx = S.Context.get()
    batch = make_batch(S, [poly_path(S, cases.SQUARE), poly_path(S, cases.TRIANGLE)])
    batch.winding(np.zeros((1, 2)))   # (flattened now: what follows must not launch)
    n0 = ctx.launches()
    for clips in ([(), ((1,),)], [((0,),), ()], [(), ((5,),)]):
        with pytest.raises(ValueError, match="clip source"):     # (SVGR_E_INVALID)
            batch.pick(np.zeros((3, 2)), clips=clips)
    for bad in (np.zeros((4, 3)), [1.0, 2.0, 3.0], np.zeros((2, 2, 2))):
        with pytest.raises(ValueError):
            poly_path(S, cases.SQUARE).contains(bad)
        with pytest.raises(ValueError):
            batch.winding(bad)
        with pytest.raises(ValueError):
            S.Scene.fill(poly_path(S, cases.SQUARE), np.ones(4)).pick(S.Transform(), bad)
    with pytest.raises(ValueError):
        batch.winding()
    assert batch.winding(np.zeros((0, 2))).shape == (0, 2)
    top, bits = batch.pick(np.zeros((0, 2)), want_bits=True)
    assert top.shape == (0,) and bits.shape == (0, 1)
    assert S.Path([]).contains([(1.0, 2.0)]).tolist() == [False] and S.Path([]).winding(np.zeros((3, 2))).tolist() == [0, 0, 0]
    assert ctx.launches() == n0
    # 31 bits
    with pytest.raises(_abi.SvgrError, match="status -5"):     # (SVGR_E_OVERFLOW)
        _abi._check(S.load_library().svgr_batch_winding(batch.handle, None, _abi._i64x4((0, 0, 1 << 15, 1 << 15)), 1 << 30, None))
    assert ctx.launches() == n0
    # (svgr_batch_create refuses a batch without paths; one whose only path has no segments is outside everywhere)
    hollow = make_batch(S, [S.Path([])])
    assert hollow.winding(np.zeros((5, 2))).tolist() == [[0]] * 5 and hollow.pick(np.zeros((5, 2)))[0].tolist() == [-1] * 5
