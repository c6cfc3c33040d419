"""k_flatten in every launch form against the curve-order reference of tests/flatten_ref.py: the counting pass + placed pass of the
plans, the emit by segment offsets (remembered end points, second traversal), the one-traversal look-back scan of a re-plan,
the per-lane places of the replays, the sharded cursors behind svgr_batch_all_edges, and the multi-GPU segment list -- at 64
and at 32 lanes per segment, at the segment counts where the look-back, k_seg_scan and the workgroup's extent fold change
path.  Every comparison is equality of float64 bit patterns or of integers, in order; under a viewport that cuts the drawing
it is a sandwich that is exact on both sides (a subsequence of the reference that holds every piece whose rows meet the
viewport).  tests/test_flatten_ref_host.py shows on the CPU that the reference is the reference and that the cases cross the
seams they are named for."""
import numpy as np
import pytest

from tests import flatten_ref as F

pytestmark = pytest.mark.gpu

BIG = ("T", "T+1", "T+2", "C", "C+1", "C+8", "2C+1")     # flatten_ref.large_sizes of the device's compute units, in order
CASES = [(n, lay) for n in F.SMALL_SIZES for lay in F.LAYOUTS if not (lay == "mixed" and n < 3)] + [(b, lay) for b in BIG for lay in F.LAYOUTS]
CULL = [(521, "mixed"), ("T+2", "mixed"), ("C+1", "singles")]      # flatten_ref.cull_case_ids
_id = lambda c: f"{c[0]}-{c[1]}"   # noqa: E731


@pytest.fixture(scope="module")
def S():
    import svgrasterize_amd as S

    S.Context.get()
    return S


@pytest.fixture(scope="module")
def n_cu(S):
    """The compute units choose_fl_sub sizes the launch by.  svgr_init (svgr_hip.hip) sets `c->n_cu = prop.multiProcessorCount` and
    its snprintf of `c->name` ("%s (%s, %d CUs)") prints the same field of the same hipDeviceProp_t: the count is taken from the
    name, i.e. the way the context holds it.  (torch.cuda.get_device_properties reports that field too, but torch finds no device
    in a process whose HIP runtime the library has already initialised, so it is not asked.)"""
    import re

    m = re.search(r"(\d+) CUs\)", S.Context.get().name())
    assert m, S.Context.get().name()
    return int(m.group(1))


@pytest.fixture(scope="module")
def canvas(S):
    return S.Context.get().alloc(F.VIEWPORT[2] * F.VIEWPORT[3] * 16)


def _cid(case, n_cu):
    n, layout = case
    if isinstance(n, str):
        return (F.large_sizes(n_cu)[BIG.index(n)], layout, False)
    return (n, layout, True)


def _batch(S, sc, m6=None, viewport=None):
    from svgrasterize_amd import _abi

    return _abi.Batch(S.Context.get(), sc["segs"], sc["seg_kind"], sc["path_seg_off"], sc["path_m6"] if m6 is None else m6,
                      sc["path_rule"], sc["path_paint"], viewport=list(sc["viewport"] if viewport is None else viewport))


def _render(b, canvas):
    from svgrasterize_amd import _abi

    b.render(canvas, _abi.OUT_CANVAS_F32, _abi.RENDER_CLIP01)


def _draw(b, canvas):
    from svgrasterize_amd import _abi

    b.draw(canvas, _abi.OUT_CANVAS_F32, _abi.RENDER_CLIP01)


def _edges(b):
    """edges() sizes its buffers by the plan's own count (svgr_batch_get_edges refuses a smaller one)."""
    n = int(b.stats.n_edges)
    e, ep = b.edges()
    assert e.shape == (n, 2, 2) and ep.shape == (n,)
    return e, ep


def _assert_is_reference(b, ref, what):
    ref_e, ref_p, _ = ref
    e, ep = _edges(b)
    assert len(e) == len(ref_e), f"{what}: {len(e)} edges, the reference has {len(ref_e)}"
    if not np.array_equal(e, ref_e):
        bad = np.flatnonzero((e != ref_e).any(axis=(1, 2)))
        same_set = np.array_equal(F.sorted_rows(e, ep), F.sorted_rows(ref_e, ref_p))
        raise AssertionError(f"{what}: {len(bad)} edges differ from the reference in place, the first at {bad[0]} "
                             f"({'the same multiset in another order' if same_set else 'another set'})")
    assert np.array_equal(ep, ref_p), f"{what}: the edges' paths differ"
    return e, ep


def _assert_sandwich(b, ref, must, what):
    ref_e, ref_p, _ = ref
    e, ep = _edges(b)
    at = F.place_in_reference(ref_e, ref_p, e, ep)
    assert at is not None, f"{what}: not a subsequence of the reference (a piece that is not the reference's, or out of order)"
    kept = np.zeros(len(ref_e), bool)
    kept[at] = True
    assert not (must & ~kept).any(), f"{what}: {int((must & ~kept).sum())} pieces whose rows meet the kept rows are missing"
    return kept


def test_the_sizes_straddle_the_lane_switch(S, n_cu):
    """choose_fl_sub restated (flatten_ref.lane_switch_sub) on the device's compute units: the small group, T and T + 1 run at 64
    lanes per segment -- the switch counts whole waves of two 32-lane segments, so the odd T + 1 is still below it --, T + 2 and
    everything above at 32.  The other tests know from this which instantiation a case ran."""
    big = F.large_sizes(n_cu)
    assert all(F.lane_switch_sub(n, n_cu) == 6 for n in F.SMALL_SIZES + big[:2])
    assert all(F.lane_switch_sub(n, n_cu) == 5 for n in big[2:])
    assert big[0] == 24 * n_cu and F.SMALL_SIZES[-1] < big[0]
    assert big[3] % F.SCAN_CHUNK == 0 and big[3] > big[2]


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_plans_give_the_reference_in_order(S, n_cu, canvas, monkeypatch, case):
    """Nothing can be culled (every point is inside the viewport's rows with 8 to spare).  svgr_batch_plan as shipped, without the
    two-pass plan, without the speculative plan, and under SVGR_SAFE_PATH: the edge array is the reference's, array for array.
    (SVGR_SAFE_PATH is read at the END of a plan: the plan's own passes still store at the per-lane places, and the first render
    takes that geometry as it is; the second render is the emit by segment offsets, with the remembered end points and the second
    traversal -- so the edges are compared again behind it.)"""
    cid = _cid(case, n_cu)
    sc, ref = F.make_case(*cid), F.reference(*cid)
    for switch in (None, "SVGR_NO_TWO_PASS_PLAN", "SVGR_NO_SPECULATIVE_PLAN", "SVGR_SAFE_PATH"):
        if switch:
            monkeypatch.setenv(switch, "1")
        b = _batch(S, sc)
        st = b.plan()
        assert st.n_edges == len(ref[0]), (switch, st.n_edges, len(ref[0]))
        _assert_is_reference(b, ref, f"plan, {switch or 'as shipped'}")
        if switch == "SVGR_SAFE_PATH":
            for _ in range(2):      # (the first render takes the plan's own geometry as it is; the second flattens again)
                _render(b, canvas)
            _assert_is_reference(b, ref, "second render of a plan made under SVGR_SAFE_PATH")
        if switch:
            monkeypatch.delenv(switch)
        b.destroy()


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_draws_and_replays_give_the_reference_in_order(S, n_cu, canvas, case):
    """A cold svgr_batch_draw; then three times new transforms and a draw -- the one-traversal scan, which reuses and replaces the
    kept seg_cnt / seg_off / lane_off: each against the reference computed for those transforms --; then two replays (the
    per-lane places), after which the bytes are still the last draw's."""
    cid = _cid(case, n_cu)
    sc = F.make_case(*cid)
    b = _batch(S, sc)
    _draw(b, canvas)
    _assert_is_reference(b, F.reference(*cid), "cold draw")
    for which in range(3):
        b.set_transforms(F.moved(sc["path_m6"], which))
        _draw(b, canvas)
        e, ep = _assert_is_reference(b, F.reference(*cid, which), f"draw after set_transforms #{which}")
        assert b.stats.n_edges == len(e)
    for _ in range(2):
        _render(b, canvas)
    e2, ep2 = _edges(b)
    assert e2.tobytes() == e.tobytes() and ep2.tobytes() == ep.tobytes(), "the replays stored other bytes than the draw"
    b.destroy()


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_extents_bboxes_and_all_edges(S, n_cu, case):
    from oracle import oracle as orc

    cid = _cid(case, n_cu)
    sc = F.make_case(*cid)
    ref_e, ref_p, _ = F.reference(*cid)
    n_paths = len(sc["path_seg_off"]) - 1
    b = _batch(S, sc)
    b.plan()
    # the extents of every path's flattened points, bit for bit (read between the plan and the first render)
    ext = b.extents()
    want = F.path_extents(ref_e, ref_p, n_paths)
    assert ext.shape == want.shape and np.array_equal(ext.view(np.uint64), want.view(np.uint64))
    empty = np.diff(sc["path_seg_off"]) == 0
    assert np.array_equal(ext[empty], np.tile([np.inf, np.inf, -np.inf, -np.inf], (int(empty.sum()), 1)))
    # the clipped integer bboxes
    bb = b.bboxes()
    assert bb.shape == (n_paths, 4)
    first = np.searchsorted(ref_p, np.arange(n_paths + 1))
    for p in range(n_paths):
        w = orc.bbox(ref_e[first[p]:first[p + 1]], sc["viewport"])
        if w is None:
            assert bb[p, 2] <= 0, (p, bb[p])
        else:
            assert tuple(int(v) for v in bb[p]) == w, (p, bb[p], w)
    # every edge, through the sharded cursors: the reference as a multiset of (path, edge) rows
    ae, ap = b.all_edges()
    assert ae.shape == (len(ref_e), 2, 2) and ap.shape == (len(ref_e),)
    assert np.array_equal(F.sorted_rows(ae, ap), F.sorted_rows(ref_e, ref_p))
    b.destroy()


@pytest.mark.parametrize("view", list(F.CUT_VIEWPORTS))
@pytest.mark.parametrize("case", CULL, ids=_id)
def test_row_culling_keeps_order_and_every_piece_that_counts(S, n_cu, canvas, monkeypatch, case, view):
    """The same drawings under a viewport that cuts them.  Which pieces survive depends on the lanes' granularity, so: the result
    is a subsequence of the reference (in order, with the reference's paths), it holds every piece whose closed row range meets
    the viewport's rows, and the statistics count exactly it.  Through the plan as shipped, the emit by segment offsets
    (SVGR_SAFE_PATH: the plan, then its renders) and the one-traversal scan of a re-plan."""
    cid = _cid(case, n_cu)
    assert cid in F.cull_case_ids(n_cu)
    sc, ref = F.make_case(*cid), F.reference(*cid)
    vp = F.CUT_VIEWPORTS[view]
    must = F.meets_rows(ref[0], vp[0], vp[0] + vp[2])
    b = _batch(S, sc, viewport=vp)
    b.plan()
    kept = _assert_sandwich(b, ref, must, "plan as shipped")
    # the re-plan in one traversal, for other transforms
    ref_m = F.reference(*cid, 1)
    b.set_transforms(F.moved(sc["path_m6"], 1))
    _draw(b, canvas)
    _assert_sandwich(b, ref_m, F.meets_rows(ref_m[0], vp[0], vp[0] + vp[2]), "draw after set_transforms")
    b.destroy()
    monkeypatch.setenv("SVGR_SAFE_PATH", "1")
    b = _batch(S, sc, viewport=vp)
    b.plan()
    kept_safe = _assert_sandwich(b, ref, must, "plan under SVGR_SAFE_PATH")
    for _ in range(2):      # (the first render takes the plan's own geometry as it is; the second flattens again)
        _render(b, canvas)
    kept_render = _assert_sandwich(b, ref, must, "second render of a plan made under SVGR_SAFE_PATH")
    monkeypatch.delenv("SVGR_SAFE_PATH")
    b.destroy()
    # (the same lanes decide in every route: the kept sets are one set)
    assert np.array_equal(kept, kept_safe) and np.array_equal(kept, kept_render)


def test_a_rank_keeps_what_reaches_its_bands_in_order(S):
    """svgr_batch_set_bands on one GPU, every rank of (world, strip) = (2, 1) and (3, 2) in turn, two plans per rank (as the code
    stands both go through the plan's segment list: svgr_batch_plan makes it before its first flatten, so k_flatten's own
    `prow` test is not reached from here).  Against the rank's owned bands -- bands of svgr_tile_rows() rows from the viewport's
    first, strips of `strip` bands dealt out in turn --: a subsequence of the reference that holds every piece whose rows meet an
    owned band; no edge of a path none of whose rows can reach one; and the ranks together hold all the unsharded render must."""
    from svgrasterize_amd import _abi

    band_rows = _abi.tile_rows()
    sc, ref = F.make_case(*F.SHARD_CASE), F.reference(*F.SHARD_CASE)
    ref_e, ref_p, info = ref
    vp = F.CUT_VIEWPORTS["middle"]
    n_bands = -(-vp[2] // band_rows)
    reach = F.path_row_reach(info, sc["seg_kind"], sc["path_seg_off"])
    whole = F.meets_rows(ref_e, vp[0], vp[0] + vp[2])
    b = _batch(S, sc, viewport=vp)
    for world, strip in F.SHARDINGS:
        union = np.zeros(len(ref_e), bool)
        for rank in range(world):
            bands = F.owned_bands(rank, world, strip, n_bands)
            must = F.meets_bands(ref_e, vp, band_rows, bands)
            foreign = np.isin(ref_p, np.flatnonzero(~F.reach_meets_bands(reach, vp, band_rows, bands)))
            b.set_bands(rank, world, strip)
            for rep in range(2):
                b.plan()
                kept = _assert_sandwich(b, ref, must, f"rank {rank} of {world}, strips of {strip}, plan {rep}")
                assert not (kept & foreign).any(), f"rank {rank} of {world}: edges of a path that cannot reach its bands"
                assert b.owned_rows() == len(bands) * band_rows
            union |= kept
        assert not (whole & ~union).any(), f"world {world}: the ranks together miss pieces the whole viewport needs"
    b.destroy()


def test_two_batches_store_the_same_bytes(S, n_cu, canvas):
    """The largest case from two new batches: the edge array is byte-identical through the plan and through the re-plan's scan."""
    cid = _cid(("2C+1", "mixed"), n_cu)
    sc = F.make_case(*cid)
    got = []
    for _ in range(2):
        b = _batch(S, sc)
        b.plan()
        e, ep = _edges(b)
        b.set_transforms(F.moved(sc["path_m6"], 2))
        _draw(b, canvas)
        e2, ep2 = _edges(b)
        got.append((e.tobytes(), ep.tobytes(), e2.tobytes(), ep2.tobytes()))
        b.destroy()
    assert got[0] == got[1]
    assert len(got[0][0]) == 32 * len(F.reference(*cid)[0]) and len(got[0][2]) == 32 * len(F.reference(*cid, 2)[0])
