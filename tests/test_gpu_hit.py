"""Hit testing on the GPU: svgr_batch_winding and svgr_batch_pick through the C ABI against the numpy reference (tests/hit_ref.py)
evaluated on the batch's own flattened edges (``batch.all_edges()``), exactly, at the seams of the launch geometry -- B =
svgr_hit_block() points per workgroup, C = svgr_hit_chunk() edges per LDS stage, 32 paths per word of the bit matrix --; the
scratch passes of the pick; ``Path.contains`` against ``Path.mask`` as an independent witness that also pins the coordinate order;
``Scene.pick`` / ``Scene.id_map`` / ``Path.stroke_contains``; and the errors.  tests/test_hit_host.py checks on the CPU that the
reference and the per-lane header are the same predicate."""
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
