"""Hit testing on the CPU: the per-lane header (csrc/svgr_hit.h, through tests/hit_harness.cpp) against the numpy reference
(tests/hit_ref.py) and both against exact rational arithmetic; the seam cases by hand; the resolve of clips and paint order; the
conditions of the cases of tests/hit_cases.py that the device tests run (table rounds, clip tables, points on a path's extent);
and the library layer without a device: ``Scene.hit_leaves`` on a hand-built scene and the ownership rule of ``elements_at`` on
a loaded document."""
import ctypes

import numpy as np
import pytest

import svgrasterize_amd as S
from svgrasterize_amd import _abi, hit
from svgrasterize_amd.geometry import PATH_CLOSED, PATH_LINE
from tests import hit_cases as cases
from tests import hit_ref as R
from tests.util import host_build

P = ctypes.c_void_p


def lib():
    h = host_build("hit_harness")
    h.hh_check_tables.restype = ctypes.c_longlong
    return h


def ptr(a):
    return a.ctypes.data_as(P)


def harness_winding(edges, off, points):
    edges = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1, 4)
    off = np.ascontiguousarray(off, dtype=np.int32)
    pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2)
    out = np.full((len(pts), len(off) - 1), 99, dtype=np.int32)
    lib().hh_winding(ptr(edges), ptr(off), ctypes.c_longlong(len(off) - 1), ptr(pts), ctypes.c_longlong(len(pts)), ptr(out))
    return out


def harness_resolve(inside, pickable, clips):
    inside = np.asarray(inside, dtype=bool)
    n, m = inside.shape
    bits = np.ascontiguousarray(R.pack_bits(inside))
    pk = np.ascontiguousarray(pickable, dtype=np.uint8)
    co, cg, go, gs = _abi.clip_tables(clips, m)
    bad = lib().hh_check_tables(ctypes.c_longlong(m), ptr(co), ptr(cg), ptr(go), ptr(gs), ctypes.c_longlong(len(go) - 1))
    if bad:
        return int(bad), None, None
    top = np.full(n, 99, dtype=np.int32)
    lib().hh_resolve(ptr(bits), ctypes.c_longlong(n), m, ptr(pk), ptr(co), ptr(cg), ptr(go), ptr(gs), ptr(top))
    return 0, R.unpack_bits(bits, m), top


# ---- the predicate --------------------------------------------------------------------------------------------------------------
def test_exported_constants():
    assert lib().hh_block() == 256 and lib().hh_chunk() >= 2


def test_seam_points_by_hand():
    edges, ep, off = cases.edge_table([np.array(cases.SQUARE), np.array(cases.TRIANGLE)])
    pts = np.array([p for p, _s, _t in cases.SEAM_POINTS])
    want = np.array([[s, t] for _p, s, t in cases.SEAM_POINTS], dtype=np.int32)
    assert np.array_equal(R.winding(edges, ep, 2, pts), want)
    assert np.array_equal(harness_winding(edges, off, pts), want)


def test_a_vertex_belongs_to_exactly_one_of_its_edges():
    # a ray through a vertex where the outline passes from one side to the other crosses once; through a local extremum, never
    diamond = [(5.0, 0.0), (10.0, 5.0), (5.0, 10.0), (0.0, 5.0)]
    edges, ep, off = cases.edge_table([np.array(diamond)])
    pts = np.array([(-1.0, 5.0), (-1.0, 0.0), (-1.0, 10.0), (0.0, 5.0), (10.0, 5.0), (5.0, 5.0)])
    want = np.array([[0], [0], [0], [1], [0], [1]], dtype=np.int32)   # (in front of the shape both crossings cancel)
    assert np.array_equal(R.winding(edges, ep, 1, pts), want)
    assert np.array_equal(harness_winding(edges, off, pts), want)


def test_zero_length_and_repeated_edges():
    sq = cases.polygon_edges(cases.SQUARE)
    edges = np.concatenate([sq[:2], [[10.0, 8.0, 10.0, 8.0]], sq[2:], sq])   # a zero-length edge; the outline twice
    off = np.array([0, len(edges)], dtype=np.int32)
    pts = np.array([(5.0, 5.0), (10.0, 8.0), (2.0, 2.0), (11.0, 5.0)])
    want = np.array([[2], [0], [2], [0]], dtype=np.int32)
    assert np.array_equal(harness_winding(edges, off, pts), want)
    assert np.array_equal(R.winding(edges, np.zeros(len(edges), dtype=np.int32), 1, pts), want)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_header_reference_and_exact_arithmetic_agree_on_integer_polygons(seed):
    polys = cases.random_polygons(seed, 7)
    polys.insert(3, np.zeros((0, 2)))   # an empty path between others
    edges, ep, off = cases.edge_table(polys)
    rng = np.random.default_rng(100 + seed)
    grid = rng.integers(-2, 43, size=(150, 2)).astype(np.float64)   # integer points: many on vertices and edges
    half = grid[:50] + 0.5
    corners = np.concatenate([p for p in polys if len(p)])[:40]
    pts = np.concatenate([grid, half, corners])
    got_h = harness_winding(edges, off, pts)
    got_r = R.winding(edges, ep, len(polys), pts)
    exact = np.array([[R.winding_exact(edges[off[p]:off[p + 1]], pt) for p in range(len(polys))] for pt in pts], dtype=np.int32)
    assert np.array_equal(got_h, exact)
    assert np.array_equal(got_r, exact)
    assert (exact[:, 3] == 0).all() and (exact != 0).any()


def test_header_and_reference_agree_off_the_integers():
    # d is rounded here: the two are the same arithmetic (two rounded products, one difference), so they still agree exactly
    rng = np.random.default_rng(7)
    polys = [rng.uniform(0, 50, size=(int(rng.integers(3, 12)), 2)) for _ in range(9)]
    edges, ep, off = cases.edge_table(polys)
    mid = (edges[:, :2] + edges[:, 2:]) / 2      # points within rounding distance of an edge
    pts = np.concatenate([rng.uniform(-5, 55, size=(300, 2)), mid, edges[:, :2]])
    assert np.array_equal(harness_winding(edges, off, pts), R.winding(edges, ep, len(polys), pts))


def test_points_on_a_paths_extent():
    # what the device's cull must not change (tests/test_gpu_hit.py sends every one of these as a query of its own): the header,
    # the reference and exact arithmetic give the same numbers, and the closed sides of the extent do hold points
    polys = cases.cull_polygons()
    edges, ep, off = cases.edge_table(polys)
    on_min_b = 0
    for which, poly in enumerate(polys):
        pts = cases.cull_boundary_points(poly)
        assert pts.shape == (13, 2) and (pts == np.round(pts)).all()
        (mna, mnb), (mxa, mxb) = poly.min(axis=0), poly.max(axis=0)
        assert {(a, b) for a in (mna, mxa) for b in (mnb, mxb)} <= {tuple(p) for p in pts.tolist()}
        assert ((pts[:, 0] > mna) & (pts[:, 0] < mxa) & (pts[:, 1] > mnb) & (pts[:, 1] < mxb)).sum() == 1
        assert ((pts[:, 0] < mna) | (pts[:, 0] > mxa) | (pts[:, 1] < mnb) | (pts[:, 1] > mxb)).sum() == 4
        exact = np.array([[R.winding_exact(edges[off[p]:off[p + 1]], pt) for p in range(len(polys))] for pt in pts], dtype=np.int32)
        assert np.array_equal(harness_winding(edges, off, pts), exact)
        assert np.array_equal(R.winding(edges, ep, len(polys), pts), exact)
        outside = (pts[:, 0] < mna) | (pts[:, 0] > mxa) | (pts[:, 1] < mnb) | (pts[:, 1] > mxb) | (pts[:, 1] == mxb) | (pts[:, 0] == mxa)
        assert (exact[outside, which] == 0).all()          # b == mxb is the open end of every edge, a == mxa is left of none
        on_min_b += int((exact[pts[:, 1] == mnb, which] != 0).sum())
    assert on_min_b >= 2    # b == mnb is closed: SQUARE holds (2, 2) and (6, 2), TRIANGLE (6, 3)


@pytest.mark.parametrize("n_paths", cases.TABLE_ROUND_COUNTS)
def test_the_table_round_cases_meet_their_condition(n_paths):
    case = cases.table_round_case(n_paths)
    edges, ep, off = cases.edge_table(case.polys)
    want = R.winding(edges, ep, n_paths, case.points)
    case.check(want)
    assert 100 <= len(case.points) <= 130 and not np.isfinite(case.points).all()
    assert {0, n_paths - 1} <= set(case.empty) and set(case.empty) <= {0, 255, 256, n_paths - 1}
    assert np.array_equal(harness_winding(edges, off, case.points), want)


def test_inside_rules_and_bit_packing():
    w = np.array([[0, 1, 2, -1, -2, 3] * 6], dtype=np.int32)[:, :33]
    rules = np.array([0, 1] * 17, dtype=np.uint8)[:33]
    want = R.inside(w, rules)
    bits = np.zeros((1, 2), dtype=np.uint32)
    lib().hh_inside_bits(ptr(np.ascontiguousarray(w)), ptr(rules), ctypes.c_longlong(33), ctypes.c_longlong(1), ptr(bits))
    assert np.array_equal(bits, R.pack_bits(want)) and np.array_equal(R.unpack_bits(bits, 33), want)
    assert want[0, :6].tolist() == [False, True, True, True, True, True] and want[0, 2] and not R.inside(w, np.ones(33, dtype=np.uint8))[0, 2]


# ---- the resolve ----------------------------------------------------------------------------------------------------------------
def both_resolves(inside, pickable, clips):
    bad, ok_h, top_h = harness_resolve(inside, pickable, clips)
    assert bad == 0
    ok_r, top_r = R.resolve(inside, pickable, clips)
    assert np.array_equal(ok_h, ok_r) and np.array_equal(top_h, top_r)
    return ok_r, top_r


def test_resolve_topmost_and_pickable():
    inside = np.array([[1, 1, 0], [1, 1, 1], [0, 0, 0], [1, 0, 0]], dtype=bool)
    _ok, top = both_resolves(inside, [1, 1, 1], None)
    assert top.tolist() == [1, 2, -1, 0]
    _ok, top = both_resolves(inside, [1, 0, 1], None)
    assert top.tolist() == [0, 2, -1, 0]
    _ok, top = both_resolves(inside, [0, 0, 0], None)
    assert top.tolist() == [-1, -1, -1, -1]


def test_resolve_one_group_is_an_or_two_groups_are_an_and():
    # paths 0, 1: clip sources; path 2 clipped by the group (0, 1); path 3 by the groups (0,) and (1,)
    rows = [[a, b, 1, 1] for a in (0, 1) for b in (0, 1)]
    ok, top = both_resolves(np.array(rows, dtype=bool), [0, 0, 1, 1], [(), (), ((0, 1),), ((0,), (1,))])
    assert ok[:, 2].tolist() == [False, True, True, True]
    assert ok[:, 3].tolist() == [False, False, False, True]
    assert top.tolist() == [-1, 2, 2, 3]


def test_resolve_a_source_that_is_itself_clipped_and_an_empty_group():
    # 0 clips 1 (a source), 1 clips 2; 3 is clipped by a group without sources: never passes
    rows = [[a, 1, 1, 1] for a in (0, 1)]
    ok, top = both_resolves(np.array(rows, dtype=bool), [0, 0, 1, 1], [(), ((0,),), ((1,),), ((),)])
    assert ok.tolist() == [[False, False, False, False], [True, True, True, False]]
    assert top.tolist() == [-1, 2]


def test_resolve_across_the_word_seam():
    rng = np.random.default_rng(5)
    m = 70
    inside = rng.random((64, m)) < 0.5
    clips = [() for _ in range(m)]
    clips[33] = ((2, 31),)
    clips[40] = ((33,), (32, 39))
    clips[69] = ((40, 0), (64,))
    pickable = rng.random(m) < 0.7
    ok, top = both_resolves(inside, pickable, clips)
    assert np.array_equal(ok[:, 40], inside[:, 40] & ok[:, 33] & (inside[:, 32] | inside[:, 39]))
    assert (top >= 0).any()


def test_resolve_clip_tables_across_words_and_rounds():
    # chains over the 31 / 32 / 33 and the 255 / 256 / 257 seams, a source at bit 0 of a later word, sources in the user's own
    # word and in earlier ones within one group (tests/test_gpu_hit.py runs the same tables on the device)
    case = cases.clip_table_case()
    assert case.n_paths == 300 and len(case.points) == 600
    assert case.clips[33] == ((32,),) and case.clips[257] == ((256,), (256,)) and case.clips[299] == ((3, 255), (256, 290))
    edges, ep, _off = cases.edge_table(case.polys)
    inside = R.inside(R.winding(edges, ep, case.n_paths, case.points), case.rules)
    ok, top = both_resolves(inside, case.pickable, case.clips)
    case.check(inside, ok)
    assert not (top % 7 == 3).any() and (top >= 0).any()
    rng = np.random.default_rng(31)
    for density in (0.5, 0.8, 0.95):
        flags = rng.random((200, case.n_paths)) < density
        ok, _top = both_resolves(flags, case.pickable, case.clips)
        assert np.array_equal(ok[:, 33], flags[:, 30] & flags[:, 31] & flags[:, 32] & flags[:, 33])
        assert np.array_equal(ok[:, 299], flags[:, 299] & (flags[:, 3] | ok[:, 255]) & (ok[:, 256] | flags[:, 290]))
        assert not ok[:, 100].any()


@pytest.mark.parametrize("clips", [[(), ((1,),)], [(), ((2,),), ()], [((0,),)], [(), ((-1,),)]])
def test_a_clip_source_must_lie_in_front_of_its_user(clips):
    bad, _ok, _top = harness_resolve(np.ones((1, len(clips)), dtype=bool), [1] * len(clips), clips)
    assert bad != 0
    with pytest.raises(ValueError):
        R.resolve(np.ones((1, len(clips)), dtype=bool), [1] * len(clips), clips)


def test_points_are_pairs():
    assert _abi.hit_points((1, 2)).shape == (1, 2) and _abi.hit_points(np.zeros((0, 2))).shape == (0, 2)
    for bad in ([1, 2, 3], np.zeros((4, 3)), np.zeros((2, 2, 2)), 5.0):
        with pytest.raises(ValueError):
            _abi.hit_points(bad)


# ---- the library layer, without a device ----------------------------------------------------------------------------------------
def rect(x0, y0, x1, y1):
    return S.Path([[(PATH_LINE, [[x0, y0], [x1, y0]]), (PATH_LINE, [[x1, y0], [x1, y1]]), (PATH_LINE, [[x1, y1], [x0, y1]]),
                    (PATH_CLOSED, [[x0, y1], [x0, y0]])]])


RED = np.array([1.0, 0.0, 0.0, 1.0])


def test_hit_leaves_of_a_hand_built_scene():
    a, b, c, d, line = rect(0, 0, 10, 10), rect(5, 5, 15, 15), rect(0, 0, 4, 4), rect(1, 1, 3, 3), rect(0, 0, 20, 0)
    clip_a, clip_b, inner_clip = rect(0, 0, 6, 6), rect(8, 8, 12, 12), rect(0, 0, 100, 5)
    shift = S.Transform().translate(3, 4)
    stroke_node = S.Scene.stroke(line, RED, 2.0)
    clip_scene = S.Scene.group([S.Scene.fill(clip_a, RED), S.Scene.fill(clip_b, RED, S.PATH_FILL_EVENODD).clip(S.Scene.fill(inner_clip, RED))])
    scene = S.Scene.group([
        S.Scene.fill(a, RED),
        S.Scene.group([S.Scene.fill(b, RED, S.PATH_FILL_EVENODD), stroke_node]).transform(shift).opacity(0.0),
        S.Scene.group([S.Scene.fill(c, RED), S.Scene.fill(d, RED).transform(shift)]).clip(clip_scene),
    ])
    base = S.Transform().scale(2)
    leaves = scene.hit_leaves(base)
    assert [l.kind for l in leaves] == ["fill", "fill", "stroke", "clip", "clip", "clip", "fill", "fill"]
    assert [l.pickable for l in leaves] == [True, True, True, False, False, False, True, True]
    assert [l.rule for l in leaves] == [0, 1, 0, 0, 0, 1, 0, 0]
    # the order of paint; the clip scene's leaves in front of the target's, a nested clip's source in front of its own target
    assert [l.source for l in leaves] == [a, b, line, clip_a, inner_clip, clip_b, c, d]
    assert leaves[0].path is a and leaves[5].path is clip_b and leaves[2].path is not line and bool(leaves[2].path)
    assert [l.clips for l in leaves] == [(), (), (), (), (), ((4,),), ((3, 5),), ((3, 5),)]
    moved = (base @ shift).m6()
    assert np.array_equal(leaves[0].m6, base.m6()) and np.array_equal(leaves[1].m6, moved) and np.array_equal(leaves[2].m6, moved)
    assert np.array_equal(leaves[6].m6, base.m6()) and np.array_equal(leaves[7].m6, moved) and np.array_equal(leaves[3].m6, base.m6())
    # what the C entry is given
    co, cg, go, gs = _abi.clip_tables([l.clips for l in leaves], len(leaves))
    assert co.tolist() == [0, 0, 0, 0, 0, 0, 1, 2, 3] and cg.tolist() == [0, 1, 1] and go.tolist() == [0, 1, 3] and gs.tolist() == [4, 3, 5]
    assert S.HitLeaf is type(leaves[0]) and "elements_at" in S.__all__


def test_hit_leaves_looks_through_filter_mask_and_blend():
    a, m = rect(0, 0, 10, 10), rect(0, 0, 5, 5)
    node = S.Scene.fill(a, RED).mask(S.Scene.fill(m, RED)).blend("multiply").opacity(0.5)
    leaves = S.Scene.group([node, S.Scene.fill(m, RED)]).hit_leaves(S.Transform())
    assert [l.source for l in leaves] == [a, m] and all(l.pickable and l.clips == () for l in leaves)


DOC = """<svg xmlns="http://www.w3.org/2000/svg" xmlns:xlink="http://www.w3.org/1999/xlink" width="100" height="100">
<defs><rect id="proto" x="0" y="0" width="10" height="10"/>
<linearGradient id="grad"><stop offset="0" stop-color="red"/><stop offset="1" stop-color="blue"/></linearGradient>
<clipPath id="cp"><rect x="0" y="0" width="50" height="50"/></clipPath></defs>
<g id="outer" transform="translate(5,5)"><g id="inner"><rect id="r1" x="1" y="1" width="20" height="20" transform="scale(2)" fill="url(#grad)"/>
<circle id="c1" cx="50" cy="50" r="5" stroke="blue" stroke-width="2"/></g>
<use id="u1" xlink:href="#proto" x="60" y="60"/>
<rect id="r2" x="30" y="0" width="5" height="5" clip-path="url(#cp)"/></g>
<rect id="lone" x="90" y="90" width="5" height="5"/>
</svg>"""


def test_ownership_on_a_loaded_document():
    scene, ids, _size = S.svg_scene_from_str(DOC)
    leaves = scene.hit_leaves(S.Transform())
    names = hit.leaf_owners(leaves, ids)
    picked = [(l.kind, n) for l, n in zip(leaves, names) if l.pickable]
    assert picked == [
        ("fill", ("r1", "inner", "outer")),         # under a <g transform> with a transform of its own: the node is wrapped, the Path shared
        ("fill", ("c1", "inner", "outer")),
        ("stroke", ("c1", "inner", "outer")),       # fill and stroke of one element: two leaves, one owner
        ("fill", ("proto", "u1", "outer")),         # a <use> and its target both own the shared leaf
        ("fill", ("r2", "outer")),
        ("fill", ("lone",)),
    ]
    # the clip path's rectangle is a source: not pickable, owned by nobody; ids that are no scenes own nothing
    assert [n for l, n in zip(leaves, names) if not l.pickable] == [()]
    assert {name for name, _sources in hit.owners(ids)} == {"proto", "r1", "c1", "inner", "u1", "r2", "outer", "lone"}
    assert "grad" in ids and "cp" in ids
    # smallest first; ties keep the order of `ids`
    assert [name for name, _s in hit.owners(ids)][:2] == ["proto", "r1"]
