"""The directed cases of tests/pathbuild_cases.py on the host: from the reference (tests/canvas_ref.py, the committed oracle) and the
restated integer rules alone, every case crosses the seam it is named for -- its slab list, the live edges and task totals of its
batches, the classes of the cells it names --, is non-trivial in every tile under test, keeps every coverage 1e-9 away from the
`mask < 1e-6` cut, and, where the viewport is wide, has a float64 reference that a long-double row sum confirms to 1e-11 (the
project's 1e-10 then leaves the device's order of summation a tenfold margin).  A case that is missing from the lists is a failure
of this file, not a skip.  No GPU needed."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import canvas_cases as cc
from tests import canvas_ref as cr
from tests import pathbuild_cases as pc

TR, TC = cc.TR, cc.TC


def _entry(pb, path):
    return pb.case.entries[path]


# ---------------------------------------------------------------------------------------------------------------- the restatements
def test_slab_shape_is_the_table_of_the_cases():
    """bands per slab at every width the cases use, and on either side of every step of min(80 / nct, 16)"""
    for nct, _nb, per in pc.SLAB_SHAPES:
        assert pc.slab_shape(_nb, nct)[0] == per
    assert [pc.slab_shape(20, n) for n in (1, 5, 6, 26, 27, 40, 41, 80, 81, 160, 161)] == \
        [(16, 1), (16, 1), (13, 1), (3, 1), (2, 1), (2, 1), (1, 1), (1, 1), (1, 2), (1, 2), (1, 3)]
    assert pc.path_ctiles(83 + 63, 2, 83) == (0, 2) and pc.path_ctiles(83 + 64, 64, 83) == (1, 1)
    assert pc.band_groups(1024) == (1, 64) and pc.band_groups(1025) == (2, 128) and pc.band_groups(8193) == (9, 576)


def test_the_case_list_is_what_it_says():
    names = set(pc.IDS)
    assert len(names) == len(pc.IDS)
    for origin in cc.ORIGINS:
        tag = "o%d_%d" % origin
        for nct, nb, _per in pc.SLAB_SHAPES:
            for rule in ("nonzero", "evenodd"):
                assert f"slab_{nct}x{nb}_{rule}-{tag}" in names
        for right in ("border", "cut"):
            assert sum(n.startswith(f"slab_81x2_{right}_") and n.endswith(tag) for n in names) == 1
            assert sum(n.startswith(f"slab_27x3_{right}_") and n.endswith(tag) for n in names) == 1
        for n in pc.BATCH_EDGES:
            assert f"batch_{n}_edges-{tag}" in names
        for total in (1, *pc.TASKS_256):
            assert f"tasks_{total}_of_256_lanes-{tag}" in names
        for total in pc.TASKS_64:
            assert f"tasks_{total}_of_64_lanes-{tag}" in names
        for other in ("batch_tall_two_slabs", "tasks_single_long_edge", "tasks_one_row_edges", *("twopass_" + n for n in pc.TWO_PASS)):
            assert f"{other}-{tag}" in names
        for base in pc.MULTI_BAND:
            assert f"{base}_nonzero-{tag}" in names and f"{base}_evenodd-{tag}" in names
    lists = pc.list_cases()
    assert set(lists) == set(pc.BAND_IDS) | set(pc.WEIGHT_IDS) | set(pc.WIDE_IDS)
    assert len(pc.BAND_IDS) == 14 and len(pc.WEIGHT_IDS) == 2 and len(pc.WIDE_IDS) == 6
    for n in (23, 24, 25, 26):   # the page boundary of k_tile_lists: PAGE_ITEMS = 24
        assert n in cc.DEEP_COUNTS
    assert pc.PAGE_ITEMS == 24


# ---------------------------------------------------------------------------------------------------------------- k_path_build
@pytest.mark.parametrize("pb", pc.CASES, ids=pc.IDS)
def test_slab_lists_live_edges_and_task_totals(pb):
    c = pb.case
    assert pb.slabs, pb.name
    for path, want in pb.slabs:
        got = tuple(pc.slabs_of(_entry(pb, path).d, c.viewport))
        assert got == want, f"{pb.name}: path {path} is cut into {got}"
        assert all(nb <= pc.PB_BANDS and nb * nk <= pc.PB_CELLS for _b, nb, _k0, nk in got)
    staged = {}
    for path, si, spec in pb.batches:
        got = pc.stage(_entry(pb, path).d, c.viewport, dict(pb.slabs)[path][si])
        staged[si] = got
        print(f"{pb.name}: slab {si}: (live edges, tasks) per batch {got}")
        if spec is not None:
            assert len(got) == len(spec), f"{pb.name}: {len(got)} batches"
            for (live, tasks), (w_live, w_tasks) in zip(got, spec):
                assert (w_live is None or live == w_live) and (w_tasks is None or tasks == w_tasks), f"{pb.name}: {got} is not {spec}"
    base = pc.base_name(pb)
    er = pc.edge_rows(_entry(pb, 0).d, c.viewport)
    rows = np.where(er[:, 2] != 0, er[:, 1] - er[:, 0], 0)
    if base.startswith("slab_") or base.startswith("twopass_"):
        r0, c0, n_rows, n_cols = pc.layer_of(_entry(pb, 0).d, c.viewport)
        # the shallow edge: ONE row, from the first column tile to the last; across the run border where there is one
        e = cr.edges_of(_entry(pb, 0).d)[0]
        assert rows[0] == 1 and abs(e[1, 1] - e[0, 1]) > n_cols - TC
        nct = pc.path_ctiles(c0, n_cols, c.viewport[1])[1]
        if nct > pc.PB_CELLS:
            x_border = c.viewport[1] + pc.PB_CELLS * TC
            assert min(e[0, 1], e[1, 1]) < x_border - TC and max(e[0, 1], e[1, 1]) > x_border + 8
        # a steep edge across every band border of every slab: the right one (wholly right of the layer in the cut variants), the left one
        steep = np.flatnonzero(rows == n_rows - (3 - (r0 - c.viewport[0])) if False else rows >= n_rows - 2)
        assert len(steep) >= 1, f"{pb.name}: no edge through every band"
        right_end = c0 + n_cols - c.viewport[1]
        if "_border_" in base:
            assert right_end % TC == 0 and right_end < c.viewport[3]      # no sentinels
        elif "_cut_" in base:
            assert right_end == c.viewport[3] and c0 == c.viewport[1]
            assert (er[:, 2] == 0).sum() >= 2                                  # edges wholly right of the layer
            assert cr.edges_of(_entry(pb, 0).d)[:, :, 1].min() < c.viewport[1]   # ... and one left of the viewport
        else:
            assert right_end % TC != 0 and right_end < c.viewport[3]
    if base.startswith("batch_") and base.endswith("_edges"):
        n = int(base.split("_")[1])
        assert len(er) == n and (rows > 0).all(), f"{pb.name}: {len(er)} edges, {int((rows > 0).sum())} with rows in the slab"
        assert [live for live, _t in staged[0]] == [min(pc.PB_BATCH, n - i) for i in range(0, n, pc.PB_BATCH)]
    if base == "batch_tall_two_slabs":
        assert 590 <= len(er) <= 610
        assert any(0 < live < min(pc.PB_BATCH, len(er) - i * pc.PB_BATCH) for i, (live, _t) in enumerate(staged[0]))   # compaction
        assert len(staged[1]) == 3 and staged[1][0] == (0, 0) and staged[1][1][0] > 0                              # a batch without a live edge
        assert all(t > 0 for _l, t in staged[0])
    if base.startswith("tasks_") and "_lanes" in base:
        total, lanes = int(base.split("_")[1]), int(base.split("_")[3])
        assert staged[0][-1][1] == total
        assert pc.tasks_per_lane(total, lanes) == (1 if total <= lanes else 2 if total <= 2 * lanes else 3)
    if base == "tasks_single_long_edge":
        assert staged[0] == [(1, 212)] and len(er) == 4 and (er[:, 2] != 0).sum() == 1   # lanes 1 .. 211 start inside the edge
    if base == "tasks_one_row_edges":
        assert (rows[:pc.PB_BATCH] == 1).sum() == 255 and (rows == 1).sum() > 300
        assert pc.tasks_per_lane(staged[0][0][1], pc.PB_THREADS) == 2 and pc.tasks_per_lane(staged[0][0][1], pc.DET_LANES) >= 4
    if pc.is_two_pass(pb):
        assert sum(len(cr.segments(e.d)[0]) for e in c.entries) > 4096
    else:
        assert sum(len(cr.segments(e.d)[0]) for e in c.entries) <= 4096   # (the single-pass plan is tried up to 4096 segments)
    # every vertex lies inside the viewport's rows or below them: the flatten keeps every edge, the batches are the reference's
    for e in c.entries:
        assert cr.edges_of(e.d)[:, :, 0].min() >= c.viewport[0]


@pytest.mark.parametrize("pb", pc.CASES, ids=pc.IDS)
def test_tiles_are_nontrivial_and_cells_have_their_class(pb):
    c = pb.case
    assert c.tiles
    pc.reference(c)   # (asserts every tile under test non-trivial)
    for band, ct in c.tiles:
        assert band * TR < c.viewport[2] and ct * TC < c.viewport[3]
    for kind, idx, band, ct, cls in c.layout:
        assert kind == "entry"
        e = c.entries[idx]
        assert cc.cell_class(e.d, e.rule, c.viewport, band, ct) == cls, f"{pb.name}: path {idx} in tile ({band}, {ct})"
    assert all(e.clip is None and e.group is None and e.opacity is None and not isinstance(e.paint, cr.Grad) for e in c.entries)


def _clear_of_the_cut(case):
    worst = np.inf
    for e in case.entries:
        raw = cr.raw_coverage(e.d, e.rule, case.viewport)
        if raw is None:
            continue
        worst = min(worst, float(np.abs(raw - cr.CUT).min()))
        assert (np.abs(raw - cr.CUT) > 1e-9).all(), f"{case.name}: coverage within 1e-9 of the cut: {e.d[:80]}"
        got, bb = cr.mask_layer(e.d, e.rule, case.viewport)
        r0, c0 = bb[0] - case.viewport[0], bb[1] - case.viewport[1]
        assert np.array_equal(got[r0:r0 + bb[2], c0:c0 + bb[3]], np.where(raw < cr.CUT, 0.0, raw))
    return worst


@pytest.mark.parametrize("pb", pc.CASES, ids=pc.IDS)
def test_no_coverage_near_the_cut(pb):
    print(f"{pb.name}: nearest coverage to the cut: {_clear_of_the_cut(pb.case):.3e}")


# ---------------------------------------------------------------------------------------------------------------- wide viewports
def _render_longdouble(case):
    """canvas_ref.render of solid fills with the row cumsum of every coverage taken in np.longdouble"""
    canvas = np.zeros((case.viewport[2], case.viewport[3], 4))
    for e in case.entries:
        edges = cr.edges_of(e.d)
        bb = orc.bbox(edges, tuple(case.viewport)) if len(edges) else None
        if bb is None:
            continue
        trace = np.zeros((bb[2], bb[3]))
        for edge in edges - np.array([bb[0], bb[1]], dtype=np.float64):
            orc.line_coverage(trace, edge)
        s = np.cumsum(trace.astype(np.longdouble), axis=1)
        cov = np.fabs(s).clip(0, 1) if e.rule is None else np.fabs(np.remainder(s + 1.0, 2.0) - 1.0)
        cov = cov.astype(np.float64)
        cov[cov < cr.CUT] = 0.0
        layer = np.zeros_like(canvas)
        r, cl = bb[0] - case.viewport[0], bb[1] - case.viewport[1]
        layer[r:r + bb[2], cl:cl + bb[3]] = cov[..., None] * np.asarray(e.paint, dtype=np.float64)
        canvas = cr.over(canvas, layer)
    return canvas


WIDE = [n for n in pc.IDS if "161x2" in n] + pc.WIDE_IDS


@pytest.mark.parametrize("name", WIDE)
def test_wide_references_hold_under_a_long_double_row_sum(name):
    assert np.finfo(np.longdouble).nmant > 60   # (x87 extended: 64 bits)
    case = pc.BY_NAME[name].case if name in pc.BY_NAME else pc.list_cases()[name][0]
    assert case.viewport[3] >= 10304
    err = float(np.abs(_render_longdouble(case) - pc.reference(case)).max())
    print(f"{name}: float64 against long-double row sums: {err:.3e}")
    assert err < 1e-11


def test_the_wide_list_reaches_both_widths():
    cols = {(pc.BY_NAME[n].case if n in pc.BY_NAME else pc.list_cases()[n][0]).viewport[3] for n in WIDE}
    assert min(cols) >= 10304 and 65600 in cols and len(WIDE) == 12


# ---------------------------------------------------------------------------------------------------------------- k_band_entries
@pytest.mark.parametrize("name", pc.BAND_IDS)
def test_band_list_cases(name):
    case, second = pc.list_cases()[name]
    n = len(case.entries)
    groups, chunk = pc.band_groups(n)
    assert n == int(name.split("_")[1].split("-")[0]) and case.viewport[2:] == (3 * TR, 3 * TC + 38)
    # the pairs sit where the list is put together: between two waves, and between the groups 3|4 and 7|8 of a wave
    assert sum(i % chunk == 0 for i in second) >= min(3, (n - 1) // chunk)
    if groups > 4:
        assert any(i % chunk == 4 * 64 for i in second)
    if groups > 8:
        assert any(i % chunk == 8 * 64 for i in second)
    assert groups in {1023: (1,), 1024: (1,), 1025: (2,), 4096: (4,), 4097: (5,), 5121: (6,), 8193: (9,)}[n]
    # every path lies in one or two bands; colours differ inside a pair
    r0 = case.viewport[0]
    ref = pc.reference(case)
    for i, e in enumerate(case.entries):
        _r, _c, rows, _cols = lay = pc.layer_of(e.d, case.viewport)
        assert pc.path_bands(lay[0], rows, r0)[1] in (1, 2), f"{name}: path {i}"
    worst = np.inf
    for i in second:
        a, b = case.entries[i - 1], case.entries[i]
        ab, ba = cr.render([a, b], (), case.viewport), cr.render([b, a], (), case.viewport)
        la = pc.layer_of(a.d, case.viewport)
        lb = pc.layer_of(b.d, case.viewport)
        lo_r, hi_r = min(la[0], lb[0]) - r0, max(la[0] + la[2], lb[0] + lb[2]) - r0
        lo_c, hi_c = min(la[1], lb[1]) - case.viewport[1], max(la[1] + la[3], lb[1] + lb[3]) - case.viewport[1]
        assert pc.PAIR_ROWS[0] <= lo_r and hi_r <= pc.PAIR_ROWS[1] + 1
        # nothing else reaches the pair: the whole reference is the pair's own there, so a swap changes the canvas by exactly this
        assert np.array_equal(ref[lo_r:hi_r, lo_c:hi_c], ab[lo_r:hi_r, lo_c:hi_c]), f"{name}: pair {i - 1}|{i} is not alone"
        diff = float(np.abs(ab - ba).max())
        worst = min(worst, diff)
        assert diff > 1e-6, f"{name}: swapping {i - 1} and {i} changes nothing"
    print(f"{name}: pairs {second}: a swap changes a pixel by at least {worst:.3e}")
    _clear_of_the_cut(case)


# ---------------------------------------------------------------------------------------------------------------- k_tile_lists
def _weights(case, band):
    n_ct = -(-case.viewport[3] // TC)
    w = [0] * n_ct
    for e in case.entries:
        for ct in range(n_ct):
            cls = cc.cell_class(e.d, e.rule, case.viewport, band, ct)
            w[ct] += {0: 0, 1: 1, 2: 2}[cls]
    return w


@pytest.mark.parametrize("name", pc.WEIGHT_IDS)
def test_weights_case(name):
    """weight_of = items + class-2 items, saturating at 63: tiles on either side of the last bin"""
    case, want = pc.list_cases()[name]
    got = _weights(case, 1)
    assert got == [want[t] for t in range(len(got))], got
    assert {62, 63, 64} <= set(got) and max(got) > 64 and pc.WEIGHT_MAX == 63
    pc.reference(case)
    for (band, ct), count in case.items:
        assert sum(cc.cell_class(e.d, e.rule, case.viewport, band, ct) != 0 for e in case.entries) == count
    _clear_of_the_cut(case)


@pytest.mark.parametrize("name", pc.WIDE_IDS)
def test_wide_cases(name):
    case, _ = pc.list_cases()[name]
    cols = case.viewport[3]
    n_ct = -(-cols // TC)
    assert case.viewport[2] == 20 and (n_ct > pc.TL_BLOCK) == (cols > 65536)
    wide = case.entries[0]
    slabs = pc.slabs_of(wide.d, case.viewport)
    assert len(slabs) == 2 * -(-n_ct // pc.PB_CELLS) and slabs[-1][2] == (n_ct - 1) // pc.PB_CELLS * pc.PB_CELLS   # 13 column runs per band
    assert -(-n_ct // pc.PB_CELLS) == 13
    pc.reference(case)
    for _kind, idx, band, ct, cls in case.layout:
        e = case.entries[idx]
        assert cc.cell_class(e.d, e.rule, case.viewport, band, ct) == cls
    for (band, ct), count in case.items:
        assert count == pc.WIDE_DEEP == pc.PAGE_ITEMS + 1
        assert sum(cc.cell_class(e.d, e.rule, case.viewport, band, ct) != 0 for e in case.entries) == count
    assert bool(case.items) == (n_ct > pc.TL_BLOCK and cols - pc.TL_BLOCK * TC >= 20)
    # small paths in tiles 0, 1022, 1023, 1024 and the last one
    for k, t in enumerate((0, 1022, 1023, 1024, n_ct - 1)):
        e = case.entries[1 + k]
        if t < n_ct and (t + 1) * TC <= cols + 40:
            assert cc.cell_class(e.d, e.rule, case.viewport, 0, t) == 2 or cols - t * TC < 20
    _clear_of_the_cut(case)
