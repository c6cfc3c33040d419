"""The lean placed flatten (k_flatten<true, true, SUB, false, LEAN>): a replay that keeps its slab table stores the edges at the
lanes' places and nothing else -- no min / max keys, no row reach, no counting atomic, no comparison of the counts with the plan's.
Here: after such replays the edge array is still the curve-order reference of tests/flatten_ref.py, bit for bit and in order, at
64 and at 32 lanes per segment; under a viewport that cuts the drawing no lane has written outside its place; everything that
leaves the lean path (new transforms, a new plan, other bands) finds real keys behind it -- every picture against a FRESH batch
of the same inputs, the bboxes against the oracle's --; and, in a fresh interpreter under SVGR_DBG_PLAN, the lean form is what
ran exactly in the passes that kept their slab table.  tests/test_flatten_lean_host.py shows on the CPU that the cases reach both
lane widths and hold lanes with several pieces and lanes with none.

The batches are planned with SVGR_NO_SPECULATIVE_PLAN: the two-pass plan orders the slabs of a batch of any size, and only a
batch with a slab order replays under the plan's places (as shipped: more than 4096 segments)."""
import contextlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import flatten_ref as F
from tests.util import ROOT

pytestmark = pytest.mark.gpu

# 64 lanes per segment (four segments per workgroup): one segment, a size that is no multiple of four, more than one workgroup;
# "T+2": the first size that launches at 32 lanes per segment (flatten_ref.large_sizes), the production form
CASES = [(1, "singles"), (5, "mixed"), (5, "singles"), (261, "mixed"), (261, "singles"), ("T+2", "mixed"), ("T+2", "singles")]
CULL = [(521, "mixed"), ("T+2", "mixed"), ("C+1", "singles")]      # flatten_ref.cull_case_ids
CULL_VIEWS = ("middle", "below")
ROUND_TRIP = [(261, "mixed"), ("T+2", "mixed")]
BIG = ("T", "T+1", "T+2", "C", "C+1", "C+8", "2C+1")     # flatten_ref.large_sizes, in order
CHILD = "SVGR_FLEAN_CHILD"   # set in the child interpreter: the scenarios announce themselves on stderr
_id = lambda c: f"{c[0]}-{c[1]}"   # noqa: E731


def case_id(case, n_cu):
    n, layout = case
    if isinstance(n, str):
        return (F.large_sizes(n_cu)[BIG.index(n)], layout, False)
    return (n, layout, True)


@pytest.fixture(scope="module")
def S():
    import svgrasterize_amd as S

    S.Context.get()
    return S


def _n_cu(S):
    """the compute units choose_fl_sub sizes the launch by, as the context holds them (tests/test_gpu_flatten_routes.py)"""
    m = re.search(r"(\d+) CUs\)", S.Context.get().name())
    assert m, S.Context.get().name()
    return int(m.group(1))


@pytest.fixture(scope="module")
def n_cu(S):
    return _n_cu(S)


@contextlib.contextmanager
def _no_spec():
    before = os.environ.get("SVGR_NO_SPECULATIVE_PLAN")
    os.environ["SVGR_NO_SPECULATIVE_PLAN"] = "1"
    try:
        yield
    finally:
        os.environ.pop("SVGR_NO_SPECULATIVE_PLAN", None)
        if before is not None:
            os.environ["SVGR_NO_SPECULATIVE_PLAN"] = before


def _mark(name):
    if os.environ.get(CHILD):
        print(f"[case] {name}", file=sys.stderr, flush=True)


class _Run:
    """a case's batch with a float32 canvas of its viewport"""

    def __init__(self, S, sc, viewport=None, m6=None):
        from svgrasterize_amd import _abi

        self.abi, self.ctx = _abi, S.Context.get()
        self.vp = tuple(sc["viewport"] if viewport is None else viewport)
        self.b = _abi.Batch(self.ctx, sc["segs"], sc["seg_kind"], sc["path_seg_off"], sc["path_m6"] if m6 is None else m6, sc["path_rule"],
                            sc["path_paint"], viewport=list(self.vp))
        self.out = self.ctx.alloc(self.vp[2] * self.vp[3] * 16)

    def plan(self):
        with _no_spec():
            self.b.plan()

    def _det(self):
        return self.abi.RENDER_CLIP01 | self.abi.RENDER_DETERMINISTIC

    def draw(self):
        with _no_spec():
            self.b.draw(self.out, self.abi.OUT_CANVAS_F32, self._det())
        return self.out.download((self.vp[2], self.vp[3], 4), np.float32)

    def render(self, det=True):
        self.b.render(self.out, self.abi.OUT_CANVAS_F32, self._det() if det else self.abi.RENDER_CLIP01)
        return self.out.download((self.vp[2], self.vp[3], 4), np.float32) if det else None

    def edges(self):
        n = int(self.b.stats.n_edges)
        e, ep = self.b.edges()
        assert e.shape == (n, 2, 2) and ep.shape == (n,)
        return e, ep

    def close(self):
        self.b.timings()    # (waits for the stream and raises on the device's sticky error word)
        self.b.destroy()
        self.out.free()


def _fresh(S, sc, m6=None):
    """the picture of a new batch of the same inputs: plan + one deterministic render (a full flatten by construction)"""
    r = _Run(S, sc, m6=m6)
    r.plan()
    want = r.render()
    r.close()
    assert want.any()
    return want


def _assert_is_reference(r, ref, what):
    """tests/test_gpu_flatten_routes.py's comparison: the reference's array, bit for bit and in order, and every edge's path"""
    ref_e, ref_p, _ = ref
    e, ep = r.edges()
    assert len(e) == len(ref_e), f"{what}: {len(e)} edges, the reference has {len(ref_e)}"
    if not np.array_equal(e, ref_e):
        bad = np.flatnonzero((e != ref_e).any(axis=(1, 2)))
        same_set = np.array_equal(F.sorted_rows(e, ep), F.sorted_rows(ref_e, ref_p))
        raise AssertionError(f"{what}: {len(bad)} edges differ from the reference in place, the first at {bad[0]} "
                             f"({'the same multiset in another order' if same_set else 'another set'})")
    assert np.array_equal(ep, ref_p), f"{what}: the edges' paths differ"


def _assert_bboxes(r, sc, ref, what):
    """the clipped integer bboxes against oracle.bbox of the reference's edges, path by path: the pass wrote real keys"""
    from oracle import oracle as orc

    ref_e, ref_p, _ = ref
    n_paths = len(sc["path_seg_off"]) - 1
    bb = r.b.bboxes()
    assert bb.shape == (n_paths, 4)
    first = np.searchsorted(ref_p, np.arange(n_paths + 1))
    for p in range(n_paths):
        w = orc.bbox(ref_e[first[p]:first[p + 1]], r.vp)
        if w is None:
            assert bb[p, 2] <= 0, (what, p, bb[p])
        else:
            assert tuple(int(v) for v in bb[p]) == w, (what, p, bb[p], w)


# ------------------------------------------------------------------------------------------------------------------- scenarios
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_edges_after_lean_replays_are_the_reference_in_order(S, n_cu, case):
    """Plan, six renders (the first takes the plan's own pass, the second is the full placed flatten that writes the slab table,
    the other four are lean): the edge array is the reference's, the bboxes are the plan's."""
    cid = case_id(case, n_cu)
    sc, ref = F.make_case(*cid), F.reference(*cid)
    _mark(f"edges {_id(case)}")
    r = _Run(S, sc)
    r.plan()
    _assert_is_reference(r, ref, "plan")
    bb0 = r.b.bboxes()
    for _ in range(6):
        r.render(det=False)
    _assert_is_reference(r, ref, "after six renders")
    assert np.array_equal(r.b.bboxes(), bb0)
    r.close()


@pytest.mark.parametrize("view", CULL_VIEWS)
@pytest.mark.parametrize("case", CULL, ids=_id)
def test_culled_lanes_store_nothing(S, n_cu, case, view):
    """A viewport that cuts the drawing (or misses it): the lanes the counting pass culled have an empty place.  The second render
    is the last full placed pass; after four more the edge bytes, and the paths beside them, are still its bytes."""
    cid = case_id(case, n_cu)
    assert cid in F.cull_case_ids(n_cu)
    sc = F.make_case(*cid)
    _mark(f"cull {_id(case)} {view}")
    r = _Run(S, sc, viewport=F.CUT_VIEWPORTS[view])
    r.plan()
    bb0 = r.b.bboxes()
    for _ in range(2):
        r.render(det=False)
    e2, p2 = r.edges()
    for _ in range(4):
        r.render(det=False)
    e6, p6 = r.edges()
    assert e6.tobytes() == e2.tobytes() and p6.tobytes() == p2.tobytes(), "a lean replay stored other bytes than the full placed pass"
    assert np.array_equal(r.b.bboxes(), bb0)
    r.close()


@pytest.mark.parametrize("case", ROUND_TRIP, ids=_id)
def test_leaving_and_reentering_the_lean_path(S, n_cu, case):
    """Six renders, then in turn: set_transforms + draw + three renders; set_transforms + plan + four renders; a window render
    between two replays; set_bands(0, 1, 3) + plan + four renders.  Every picture is a fresh batch's deterministic render, bit for
    bit; after each draw or plan the bboxes are the oracle's for the reference's edges."""
    cid = case_id(case, n_cu)
    sc = F.make_case(*cid)
    m1, m2 = F.moved(sc["path_m6"], 0), F.moved(sc["path_m6"], 2)
    want0, want1, want2 = _fresh(S, sc), _fresh(S, sc, m6=m1), _fresh(S, sc, m6=m2)
    assert not np.array_equal(want0, want1) and not np.array_equal(want1, want2)
    _mark(f"round trip {_id(case)}")
    r = _Run(S, sc)
    r.plan()
    _assert_bboxes(r, sc, F.reference(*cid), "plan")
    for k in range(6):
        assert np.array_equal(r.render(), want0), f"replay {k}"
    r.b.set_transforms(m1)
    assert np.array_equal(r.draw(), want1), "draw after set_transforms"
    _assert_bboxes(r, sc, F.reference(*cid, 0), "draw after set_transforms")
    for k in range(3):
        assert np.array_equal(r.render(), want1), f"replay {k} after set_transforms + draw"
    _assert_is_reference(r, F.reference(*cid, 0), "replays after set_transforms + draw")
    r.b.set_transforms(m2)
    r.plan()
    _assert_bboxes(r, sc, F.reference(*cid, 2), "plan after set_transforms")
    for k in range(4):
        assert np.array_equal(r.render(), want2), f"replay {k} after set_transforms + plan"
    tr, tc = r.abi.tile_rows(), r.abi.tile_cols()
    win = (5 * tr, 2 * tc, 30 * tr, 9 * tc)
    wout = r.ctx.alloc(win[2] * win[3] * 16)
    r.b.render(wout, r.abi.OUT_CANVAS_F32, r._det(), window=win)
    part = wout.download((win[2], win[3], 4), np.float32)
    wout.free()
    assert np.array_equal(part, want2[win[0]:win[0] + win[2], win[1]:win[1] + win[3]]), "the window"
    assert np.array_equal(r.render(), want2), "replay after the window"
    r.b.set_bands(0, 1, 3)
    r.plan()
    _assert_bboxes(r, sc, F.reference(*cid, 2), "plan after set_bands")
    for k in range(4):
        assert np.array_equal(r.render(), want2), f"replay {k} after set_bands + plan"
    _assert_is_reference(r, F.reference(*cid, 2), "replays after set_bands + plan")
    r.close()


# ----------------------------------------------------------------------------------------------------------------- who ran
def _child():
    """(in the child interpreter) the scenarios once: every case of the first and the last, one culled case"""
    import svgrasterize_amd as S

    S.Context.get()
    n_cu = _n_cu(S)
    for case in CASES:
        test_edges_after_lean_replays_are_the_reference_in_order(S, n_cu, case)
    test_culled_lanes_store_nothing(S, n_cu, CULL[0], "middle")
    for case in ROUND_TRIP:
        print("[case] -", file=sys.stderr, flush=True)   # (the scenario's fresh batches, in front of its own mark)
        test_leaving_and_reentering_the_lean_path(S, n_cu, case)
    print("[case] end", file=sys.stderr, flush=True)


def test_the_lean_form_runs_exactly_where_the_slab_table_is_kept():
    """SVGR_DBG_PLAN in a fresh child (one child, under a time limit): pictures and edges alone would pass a shortcut that never
    ran.  Pass by pass, the flatten's line says `lean` exactly when the k_path_build line behind it ends in `kept`; both lane
    widths ran lean; every scenario had lean passes, and as many as its renders say."""
    env = dict(os.environ, SVGR_DBG_PLAN="1")
    env[CHILD] = "1"
    for k in ("SVGR_NO_SPECULATIVE_PLAN", "SVGR_NO_TWO_PASS_PLAN", "SVGR_SAFE_PATH", "SVGR_NO_SPARE", "SVGR_DBG_STALE_BAND"):
        env.pop(k, None)
    code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests import test_gpu_flatten_lean as T; T._child()"
    res = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert res.returncode == 0, res.stderr[-3000:]
    got, key, fl = {}, None, None
    lean_subs = set()
    for line in res.stderr.splitlines():
        if line.startswith("[case] "):
            key, fl = line[7:].strip(), None
            got.setdefault(key, "")
        elif line.startswith("[geometry] k_flatten<"):
            m = re.fullmatch(r"\[geometry\] k_flatten<(count|scan|offsets|placed), ([56])> (lean|full)", line)
            assert m, line
            fl = m.groups()
            assert fl[2] == "full" or fl[0] == "placed", line
        elif line.startswith("[geometry] k_path_build<"):
            assert fl is not None, f"no flatten line in front of: {line}"
            kept = line.endswith("slab table kept")
            assert kept or line.endswith("slab table written"), line
            assert (fl[2] == "lean") == kept, (fl, line)
            if kept:
                assert line.startswith("[geometry] k_path_build<1>"), line
                lean_subs.add(int(fl[1]))
            if key is not None:
                got[key] += "L" if kept else "f"
            fl = None
    assert got.pop("end", None) == "" and set(got.pop("-", "")) <= {"f"}   # (a fresh batch with one render never runs lean)
    for k, v in got.items():
        print(f"{k:28s} {v}")
    assert lean_subs == {5, 6}, lean_subs
    # The runs of lean passes, per scenario.  A render without the deterministic flag right behind a plan takes the plan's own pass,
    # the next one is the full placed pass that writes the table: four of six are lean.  A deterministic render runs its own pass:
    # the first behind a plan or a draw's plan is full, every further one lean, the window's among them.
    runs = lambda s: [len(m) for m in re.findall("L+", s)]   # noqa: E731
    for case in CASES:
        assert runs(got[f"edges {_id(case)}"]) == [4] and got[f"edges {_id(case)}"].endswith("fLLLL"), (case, got[f"edges {_id(case)}"])
    assert runs(got[f"cull {_id(CULL[0])} middle"]) == [4]
    for case in ROUND_TRIP:
        assert runs(got[f"round trip {_id(case)}"]) == [5, 3, 3 + 1 + 1, 3], (case, got[f"round trip {_id(case)}"])
