"""CPU side of the flatten route tests: the curve-order reference of tests/flatten_ref.py is pinned against the recorded
fixtures, the oracle and the host build of the lanes' traversal; and every case the GPU comparison of k_flatten's launch forms
is to run is shown, from the reference's `info` alone, to cross the seams it is there for.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc
from tests import flatten_ref as F
from tests.util import host_build, load, sort_edges

KAT = ["rand_small", "rand_big", "tiny_curves", "degenerate", "tiger512"]
IDENT = np.array([[1.0, 0.0, 0.0, 0.0, 1.0, 0.0]])
CASES = F.case_ids(F.MI355X_CUS)


@pytest.fixture(scope="module")
def hh():
    L = host_build("host_harness")   # (the build and the library tests/test_core_host.py uses)
    L.hh_flatten.argtypes = [np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS"), C.c_double,
                             np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS"), C.c_long, C.c_int]
    L.hh_flatten.restype = C.c_long
    return L


def _one_path(cubics):
    cubics = np.ascontiguousarray(cubics, dtype=np.float64).reshape(-1, 8)
    return F.flatten_in_order(cubics, np.ones(len(cubics), np.uint8), [0, len(cubics)], IDENT)


# ------------------------------------------------------------------------------------------
# the reference is the reference
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", KAT)
def test_reference_gives_the_recorded_edge_sets(name):
    g = load("flatten_kat.npz")
    edges, edge_path, info = _one_path(g[name + "_in"])
    want = g[name + "_edges"]
    assert len(edges) == len(want)
    assert np.array_equal(sort_edges(edges), sort_edges(want))
    assert not edge_path.any()
    # ... and the order is the curve's: the segments in turn, every piece starting where the one before it ended
    assert (np.diff(info["seg"]) >= 0).all()
    same = info["seg"][1:] == info["seg"][:-1]
    assert np.array_equal(edges[1:, 0][same], edges[:-1, 1][same])
    first = np.concatenate([[True], ~same])
    assert np.array_equal(edges[first, 0], info["pts"][info["seg"][first], 0])


def test_reference_is_path_edges_on_one_path():
    """Lines and cubics of one path under a transform: the set `oracle.path_edges` gives (its order is the reference's own: the
    lines, then the cubics level by level)."""
    sc = F.make_case(261, "one", True)
    m = np.eye(3)
    m[:2] = sc["path_m6"][0].reshape(2, 3)
    line = sc["seg_kind"] == F.SEG_LINE
    pts = sc["segs"].reshape(-1, 4, 2)
    want = orc.path_edges(pts[line][:, :2], pts[~line], m)
    edges, _, _ = F.reference(261, "one", True)
    assert len(want) == len(edges) > 5000
    assert np.array_equal(sort_edges(edges), sort_edges(want))


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("name", KAT + ["deep"])
def test_host_traversals_emit_in_curve_order(hh, name, mode):
    """hh_flatten is the host build of what the lanes run (svgr_core.h).  Every mode emits in CURVE order, so each is held to
    the reference's pieces in the reference's order: mode 0 (flatten_cubic) is depth-first with an explicit stack, left half
    first -- not level by level as the reference's own batch is --, mode 1 the stack-free walk, modes 2 and 3 the 32- and
    64-lane cut with the lanes taken in turn."""
    if name == "deep":
        sc = F.make_case(521, "one", True)
        pts = F.reference(521, "one", True)[2]["pts"]           # (presentation space: the harness takes no transform)
        cubics = pts[sc["seg_kind"] != F.SEG_LINE].reshape(-1, 8)
    else:
        cubics = load("flatten_kat.npz")[name + "_in"].reshape(-1, 8)
    want, _, info = _one_path(cubics)
    if name == "deep":
        assert info["depth"].max() >= 10 and np.bincount(info["seg"]).max() > 512
    buf = np.empty(4 * 8192)
    got = []
    for c in cubics:
        n = hh.hh_flatten(np.ascontiguousarray(c), 0.1, buf, 8192, mode)
        assert 0 < n <= 8192
        got.append(buf[: 4 * n].copy())
    got = np.concatenate(got).reshape(-1, 2, 2)
    assert got.shape == want.shape
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------
# the cases cross what they are there to cross
# ------------------------------------------------------------------------------------------
def test_sizes_sit_on_the_seams():
    small, big = F.SMALL_SIZES, F.large_sizes(F.MI355X_CUS)
    t = 24 * F.MI355X_CUS
    assert all(F.lane_switch_sub(n, F.MI355X_CUS) == 6 for n in small + big[:2])
    assert all(F.lane_switch_sub(n, F.MI355X_CUS) == 5 for n in big[2:])
    assert big[:3] == (t, t + 1, t + 2)
    # the look-back of the last workgroup: 63 predecessors (one window, its last lane in front of workgroup 0), 64 (one window
    # exactly), 65 (the first that can need a second), and more than two full windows
    wgs = {sub: sorted(-(-n // (F.FL_BLOCK >> sub)) for n in sizes) for sub, sizes in ((6, small), (5, big[2:]))}
    assert {F.SCAN_WINDOW, F.SCAN_WINDOW + 1, F.SCAN_WINDOW + 2} <= set(wgs[6])
    assert wgs[6][-1] - 1 > 2 * F.SCAN_WINDOW and wgs[5][0] - 1 > 2 * F.SCAN_WINDOW
    for sub, sizes in ((6, small), (5, big[2:])):     # a last workgroup that is full, and one that is not
        assert any(n % (F.FL_BLOCK >> sub) for n in sizes) and any(n % (F.FL_BLOCK >> sub) == 0 for n in sizes)
    # k_seg_scan: a chunk exactly, a tail of one (scalar), a tail of eight (one vector step), three steps with a scalar tail
    base = big[3]
    assert base % F.SCAN_CHUNK == 0 and big[4:] == (base + 1, base + 8, 2 * base + 1)
    # the layouts: a boundary inside a workgroup and on one, a path with no segments between two others, one path over at
    # least three workgroups with others on both sides
    off = F.make_case(521, "mixed", True)["path_seg_off"]
    assert 2 in off and 8 in off and (np.diff(off) == 0).any() and off[0] == 0
    long_ = np.flatnonzero(np.diff(off) >= 3 * 8 + 2)
    assert len(long_) and 0 < long_[0] < len(off) - 2
    assert all(F.make_case(n, "mixed", True)["path_seg_off"].tolist() == [0, 1, 1, n] for n in (3, 4, 5))


@pytest.mark.parametrize("cid", CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_case_conditions(cid):
    n, layout, rich = cid
    sc = F.make_case(*cid)
    edges, edge_path, info = F.reference(*cid)
    assert np.isfinite(sc["segs"]).all() and np.isfinite(edges).all()
    assert 0 < len(edges) <= F.EDGE_BUDGET
    assert info["depth"].max() <= 12 < F.MAX_LEVELS      # (nowhere near kMaxFlattenDepth)
    # all-kept: every point inside the viewport's rows with 8 rows to spare, under the case's transforms and the moved ones
    vp = sc["viewport"]
    for which in (-1, 0, 1, 2):
        r = F.reference(n, layout, rich, which)[0][:, :, 0]
        assert r.min() >= vp[0] + 8 and r.max() <= vp[0] + vp[2] - 8
    counts = [len(F.reference(n, layout, rich, which)[0]) for which in (-1, 0, 1, 2)]
    if n >= 256:
        assert len(set(counts)) > 1, "the moved transforms leave every count as it was"
    cubic = info["is_cubic"]
    assert cubic.any()
    if n < 256:
        # (a handful of segments cannot hold every depth: these sizes are launch shapes -- their one large cubic still runs the
        #  lanes' second traversal at both widths)
        assert all((F.lane_counts(info, sub) > F.FL_ENDS).any() for sub in F.SUBS)
        return
    assert (~cubic).any() and (cubic & (info["depth"] == 0)).any()      # lines, and cubics flat at the root
    depths = set(info["depth"][cubic].tolist())
    for sub in F.SUBS:
        assert depths >= set(range(0, sub + 4)), (sub, sorted(depths))            # every stopping depth 0 .. SUB + 3
        lc = F.lane_counts(info, sub)
        for want in (1, F.FL_ENDS, F.FL_ENDS + 1):
            assert (lc == want).any(), (sub, want)
        assert (lc >= 16).any(), sub
        # a cubic that goes flat at each level above the lane level: its piece belongs to the lane whose remaining bits are 0
        above = cubic & (info["depth"] < sub)
        assert set(info["depth"][above].tolist()) == set(range(sub))
        assert not (info["lane"][sub][above] & ((1 << (sub - info["depth"][above])) - 1)).any()


@pytest.mark.parametrize("cid", F.cull_case_ids(F.MI355X_CUS), ids=lambda c: f"{c[0]}-{c[1]}")
def test_culling_sandwich_is_not_trivial(cid):
    edges, edge_path, _ = F.reference(*cid)
    assert F.place_in_reference(edges, edge_path, edges, edge_path) is not None      # (no piece twice: a subsequence has one place)
    vp = F.CUT_VIEWPORTS["middle"]
    must = F.meets_rows(edges, vp[0], vp[0] + vp[2])
    assert 0 < must.sum() < len(edges)
    assert len(np.unique(edge_path[must])) > 1 and len(np.unique(edge_path[~must])) > 1
    for name in ("below", "above"):     # nothing has to stay; whatever stays is held to the reference's order all the same
        vp = F.CUT_VIEWPORTS[name]
        assert not F.meets_rows(edges, vp[0], vp[0] + vp[2]).any()


def test_sharding_sandwich_is_not_trivial():
    sc = F.make_case(*F.SHARD_CASE)
    edges, edge_path, info = F.reference(*F.SHARD_CASE)
    from svgrasterize_amd import _abi

    BAND_ROWS = _abi.tile_rows()      # (the built library's band height, as tests/test_core_host.py reads it: no device needed)
    vp = F.CUT_VIEWPORTS["middle"]
    assert vp[2] % BAND_ROWS == 0 and vp[0] % BAND_ROWS != 0
    n_bands = vp[2] // BAND_ROWS
    reach = F.path_row_reach(info, sc["seg_kind"], sc["path_seg_off"])
    whole = F.meets_rows(edges, vp[0], vp[0] + vp[2])
    for world, strip in F.SHARDINGS:
        union = np.zeros(len(edges), bool)
        seen = []
        for rank in range(world):
            bands = F.owned_bands(rank, world, strip, n_bands)
            assert len(bands)
            must = F.meets_bands(edges, vp, BAND_ROWS, bands)
            assert 0 < must.sum() < whole.sum()
            assert all((must != m).any() for m in seen)
            seen.append(must)
            union |= must
            out_of_reach = ~F.reach_meets_bands(reach, vp, BAND_ROWS, bands)
            assert np.isin(edge_path, np.flatnonzero(out_of_reach)).any()           # paths with edges that this rank must not keep
            assert not np.isin(edge_path[must], np.flatnonzero(out_of_reach)).any()
        assert np.array_equal(union, whole)
    assert sorted(b for r in range(3) for b in F.owned_bands(r, 3, 2, 13)) == list(range(13))
    assert F.owned_bands(1, 3, 2, 13).tolist() == [2, 3, 8, 9]
