"""CPU side of tests/test_gpu_flatten_lean.py: from the reference's `info` alone, the cases it runs reach both lane widths of the
flatten, and they hold lanes with more than one piece and lanes with none -- the stores of the lean form, which no longer compares
a lane's count with its place's size, are bounded by that size alone.  No GPU needed."""
import numpy as np
import pytest

from tests import flatten_ref as F
from tests import test_gpu_flatten_lean as L

ALL = sorted(set(L.CASES + L.CULL + L.ROUND_TRIP), key=str)


def test_the_sizes_reach_both_lane_widths():
    """choose_fl_sub restated (flatten_ref.lane_switch_sub) on an MI355X's compute units: every numbered size runs at 64 lanes per
    segment, every named one at or above T + 2 at 32; among the 64-lane sizes one segment, a size that is no multiple of the four
    segments of a workgroup, and more than one workgroup."""
    subs = {c: F.lane_switch_sub(L.case_id(c, F.MI355X_CUS)[0], F.MI355X_CUS) for c in ALL}
    assert all(s == (5 if isinstance(c[0], str) else 6) for c, s in subs.items()), subs
    for group in (L.CASES, L.ROUND_TRIP, L.CULL):
        assert {subs[c] for c in group} == {5, 6}, group
    small = {c[0] for c in L.CASES if not isinstance(c[0], str)}
    per_wg = F.FL_BLOCK >> 6
    assert 1 in small and any(n % per_wg for n in small if n > per_wg) and any(n > 2 * per_wg for n in small)
    assert set(small) <= set(F.SMALL_SIZES)
    # two layouts, one of them with paths that have no segment
    assert {c[1] for c in L.CASES} == {"mixed", "singles"}
    for c in L.CASES:
        off = F.make_case(*L.case_id(c, F.MI355X_CUS))["path_seg_off"]
        assert (c[1] == "mixed") == bool((np.diff(off) == 0).any()), c


@pytest.mark.parametrize("case", [c for c in ALL if c[0] != 1], ids=L._id)
def test_lanes_with_several_pieces_and_lanes_with_none(case):
    """At the case's own lane width: a lane that owns more than one piece (its traversal stores at `at` = 0, 1, ...: bounded by
    the place's size) and a lane of a cubic that owns none (an ancestor went flat: an empty place)."""
    cid = L.case_id(case, F.MI355X_CUS)
    _, _, info = F.reference(*cid)
    sub = F.lane_switch_sub(cid[0], F.MI355X_CUS)
    n = F.lane_counts(info, sub)
    assert n.max() > 1, "no lane with more than one piece"
    n_cubics = len(np.unique(info["seg"][info["is_cubic"]]))
    assert len(n) < (n_cubics << sub), "every lane of every cubic owns a piece"


def test_one_segment_is_one_deep_cubic():
    """The one-segment case is a cubic whose lanes all own pieces, several of them more than one."""
    _, _, info = F.reference(1, "singles", True)
    n = F.lane_counts(info, 6)
    assert info["is_cubic"].all() and n.max() > 1
