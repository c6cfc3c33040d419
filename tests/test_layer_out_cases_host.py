"""The directed cases of tests/layer_out_cases.py on the host: from the reference (canvas_ref.mask_layer = oracle.path_mask, and
canvas_ref.raw_coverage) alone, every case crosses the seam it is named for -- where its layer starts and ends in the 16 x 64 tile
grid, the classes of the cells it names, the items of its deep tile, the paths without a layer --, is non-trivial in every tile it
is about (values strictly between 0 and 1, or exactly the value the case names), and keeps EVERY pixel's raw coverage 1e-9 away
from the `mask < 1e-6` cut, at both origins and under the translation of the set_transforms route: the GPU tests exclude nothing.
No GPU needed."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import canvas_cases as cc
from tests import canvas_ref as cr
from tests import layer_out_cases as lc
from tests.util import assert_close64

TR, TC = cc.TR, cc.TC
SHIFTS = ((0, 0), lc.SHIFT)


def _in_tile(case, path, band, ct, shift=(0, 0)):
    """The reference mask's pixels of `path` inside a tile (cut to the layer): a 2-d array, possibly empty."""
    m, _f, bb = lc.reference(case, shift)[path]
    g = lc.grid(case, shift)
    r0, c0, r1, c1 = cc.tile_box(g, band, ct)
    lo_r, hi_r = max(r0, bb[0]), min(r1, bb[0] + bb[2])
    lo_c, hi_c = max(c0, bb[1]), min(c1, bb[1] + bb[3])
    if lo_r >= hi_r or lo_c >= hi_c:
        return np.zeros((0, 0))
    return m[lo_r - bb[0]: hi_r - bb[0], lo_c - bb[1]: hi_c - bb[1]]


def _fractional(a):
    return bool(((a > 0) & (a < 1)).any())


# ------------------------------------------------------------------------------------------------------------------ the case list
def test_the_case_list_is_what_it_says():
    names = set(lc.IDS)
    assert len(names) == len(lc.IDS)
    singles = ["row_start_0", "row_start_7", "row_start_8", "row_start_15", "row_first_half", "row_second_half",
               "row_end_on_border", "row_end_before_border", "row_end_past_border", "one_row",
               *(f"col_start_{k}" for k in (0, 7, 8, 9, 63)), *(f"col_end_{k}" for k in (0, 7, 8, 63)), "one_col", "one_pixel",
               "class1_interior", "class1_cut_right", "untouched_tiles", "cut_top", "cut_bottom", "cut_left", "cut_right", "cut_all_sides",
               "outside", "slivers_at_the_cut", "no_viewport"]
    for origin in cc.ORIGINS:
        assert origin == (0, 0) or (origin[0] % TR and origin[1] % TC)
        tag = "o%d_%d" % origin
        for s in singles:
            for rule in ("nonzero", "evenodd"):
                assert f"{s}_{rule}-{tag}" in names
        for m in ("neighbours", "big_neighbours", *(f"deep_{n}" for n in lc.DEEP_COUNTS)):
            assert f"{m}-{tag}" in names
    assert len(lc.SINGLE) == 2 * 2 * len(singles) and len(lc.MULTI) == 2 * (2 + len(lc.DEEP_COUNTS))
    assert lc.PAGE_ITEMS == 24 and lc.DEEP_COUNTS == (23, 24, 25, 26) and all(n in cc.DEEP_COUNTS for n in lc.DEEP_COUNTS)
    for c in lc.CASES:
        assert all(len(p) == 3 for p in c.paths)
        assert (len(c.paths) == 1) == (c in lc.SINGLE)
        if c.viewport is not None:   # small viewports: a few bands by a few column tiles
            assert c.viewport[2] <= cc.VIEW[0] and c.viewport[3] <= cc.VIEW[1] and tuple(c.viewport[:2]) in cc.ORIGINS
        for _d, rule, paint in c.paths:
            assert rule in (None, "evenodd") and 0 < paint[3] < 1
    assert sum(c.viewport is None for c in lc.CASES) == 4
    for c in lc.BIG:
        assert lc.n_segments(c) > 4096
    for c in lc.SMALL_MULTI + lc.SINGLE:
        assert lc.n_segments(c) <= 4096


# ------------------------------------------------------------------------------------------------------------------ the seams
@pytest.mark.parametrize("case", lc.CASES, ids=lc.IDS)
def test_every_case_crosses_its_seam(case):
    refs = lc.reference(case)
    for p, (m, _f, bb) in enumerate(refs):
        assert (bb is None) == (p in case.empty), f"{case.name}: path {p} has the layer {bb}"
        if bb is not None:
            d = case.paths[p][0]
            assert bb == (lc.layer_of(d, case.viewport) if case.viewport is not None else orc.bbox(cr.edges_of(d)))
            assert m.shape == (bb[2], bb[3]) and bb[2] > 0 and bb[3] > 0
    if 0 in case.empty and len(case.paths) == 1:
        return
    g = lc.grid(case)
    w = case.want
    if w:
        _m, _f, (r0, c0, rows, cols) = refs[0]
        row0, col0 = (r0 - g[0]) % TR, (c0 - g[1]) % TC
        row_last, col_last = (r0 + rows - 1 - g[0]) % TR, (c0 + cols - 1 - g[1]) % TC
        for key, got in (("row0", row0), ("col0", col0), ("row_last", row_last), ("col_last", col_last), ("rows", rows), ("cols", cols)):
            assert key not in w or w[key] == got, f"{case.name}: {key} is {got}"
        b0, b1 = (r0 - g[0]) // TR, (r0 + rows - 1 - g[0]) // TR
        t0, t1 = (c0 - g[1]) // TC, (c0 + cols - 1 - g[1]) // TC
        if "half" in w:   # every row of the layer in one wave's half of ONE band
            assert b0 == b1 and row0 // lc.HALF == row_last // lc.HALF == w["half"], f"{case.name}: rows {row0} .. {row_last} of bands {b0} .. {b1}"
        assert "bands" not in w or b1 - b0 + 1 == w["bands"]
        assert "ctiles" not in w or t1 - t0 + 1 == w["ctiles"]
        if "cut" in w:   # the uncut bbox reaches beyond the viewport on exactly these sides, and the layer ends with the viewport there
            full = orc.bbox(cr.edges_of(case.paths[0][0]))
            over = {"t": full[0] < g[0], "l": full[1] < g[1], "b": full[0] + full[2] > g[0] + g[2], "r": full[1] + full[3] > g[1] + g[3]}
            assert {k for k, v in over.items() if v} == set(w["cut"]), f"{case.name}: cut on {over}"
            ends = {"t": r0 == g[0], "l": c0 == g[1], "b": r0 + rows == g[0] + g[2], "r": c0 + cols == g[1] + g[3]}
            assert all(ends[k] for k in w["cut"])
        else:    # ... else the viewport cuts nothing: the layer is the path's own bbox
            assert (r0, c0, rows, cols) == orc.bbox(cr.edges_of(case.paths[0][0]))
    for p, band, ct, cls in case.classes:
        assert cc.cell_class(case.paths[p][0], None, g, band, ct) == cls, f"{case.name}: path {p} in tile ({band}, {ct})"
    for (band, ct), count in case.items:
        n = sum(cc.cell_class(d, None, g, band, ct) != 0 for p, (d, _r, _pt) in enumerate(case.paths) if p not in case.empty)
        assert n == count, f"{case.name}: {n} items in tile ({band}, {ct})"
    for band, ct in case.tiles:
        assert band * TR < g[2] and ct * TC < g[3]


def test_the_class1_layer_is_partial_in_its_first_and_last_column_tile():
    for case in lc.SINGLE:
        if lc.base_name(case).startswith("class1_interior"):
            _m, _f, (r0, c0, rows, cols) = lc.reference(case)[0]
            g = case.viewport
            assert (c0 - g[1]) % TC != 0 and (c0 + cols - g[1]) % TC != 0 and c0 + cols < g[1] + g[3]
            assert (r0 - g[0]) % TR != 0 and r0 + rows < g[0] + g[2]
        if lc.base_name(case).startswith("class1_cut_right"):   # class 1 where the layer ends inside the tile (with the viewport)
            _m, _f, (r0, c0, rows, cols) = lc.reference(case)[0]
            g = case.viewport
            assert c0 + cols == g[1] + g[3] and (c0 + cols - g[1]) % TC != 0 and (c0 - g[1]) % TC != 0
            a = _in_tile(case, 0, 1, 3)
            assert (r0 - g[0]) % TR == 2 and a.shape == (TR - 2, g[3] - 3 * TC)   # (the layer's rows of that band: tile rows 2 .. 15)
            assert (a[0] == 0).all() and (a[2:] == 1).all() and (a[1] == a[1, 0]).all() and 0 < a[1, 0] < 1


# ------------------------------------------------------------------------------------------------------------------ the cut
@pytest.mark.parametrize("shift", SHIFTS, ids=["as_built", "translated"])
@pytest.mark.parametrize("case", lc.CASES, ids=lc.IDS)
def test_no_pixel_lies_near_the_cut_and_the_reference_is_the_raw_coverage_cut(case, shift):
    """Zero pixels within 1e-9 of the cut: a condition on the cases, not a tolerance of the comparison.  And the reference is the
    raw coverage with `raw < 1e-6 -> 0`, bit for bit."""
    for p, (d, rule, _paint) in enumerate(case.paths):
        raw = lc.raw_coverage(d, rule, case.viewport, shift)
        m, _f, bb = lc.reference(case, shift)[p]
        if raw is None:
            assert m is None
            continue
        assert int((np.abs(raw - cr.CUT) <= 1e-9).sum()) == 0, f"{case.name}: path {p} has coverage within 1e-9 of the cut"
        assert raw.shape == m.shape and np.array_equal(m, np.where(raw < cr.CUT, 0.0, raw)), f"{case.name}: path {p}"
        assert not np.signbit(m).any()


def test_the_slivers_lie_on_either_side_of_the_cut():
    (ra, rb), (ca, cb) = lc.SLIVER_ROWS, lc.SLIVER_COLS
    seen = 0
    for case in lc.SINGLE:
        if not lc.base_name(case).startswith("slivers_at_the_cut"):
            continue
        seen += 1
        for shift in SHIFTS:
            d, rule, _p = case.paths[0]
            raw = lc.raw_coverage(d, rule, case.viewport, shift)
            m, _f, bb = lc.reference(case, shift)[0]
            r = case.viewport[0] + shift[0] - bb[0]
            c = case.viewport[1] + shift[1] - bb[1]
            below, kept = raw[r + ra, c + ca: c + cb + 1], raw[r + rb, c + ca: c + cb + 1]
            assert len(below) == cb - ca + 1 > 64                           # a run of pixels, across a column-tile border
            assert (below > 0).all() and (below * 1.5 < cr.CUT).all() and np.allclose(below[1:-1], lc.SLIVER_BELOW, rtol=1e-6, atol=0)
            assert (kept > 1.5 * cr.CUT).all() and np.allclose(kept[1:-1], lc.SLIVER_KEPT, rtol=1e-6, atol=0)
            assert (m[r + ra] == 0.0).all() and np.array_equal(m[r + rb, c + ca: c + cb + 1], kept)
            assert not m[[k for k in range(m.shape[0]) if k != r + rb]].any()   # nothing else in the layer
    assert seen == 4


# ------------------------------------------------------------------------------------------------------------------ non-trivial
@pytest.mark.parametrize("case", lc.CASES, ids=lc.IDS)
def test_the_reference_is_not_trivial_in_the_tiles_under_test(case):
    exact = {(p, b, t): v for p, b, t, v in case.exact}
    for band, ct in case.tiles:
        if len(case.paths) == 1:
            a = _in_tile(case, 0, band, ct)
            assert a.size, f"{case.name}: the layer has no pixel in tile ({band}, {ct})"
            if (0, band, ct) in exact:
                assert (a == exact[0, band, ct]).all() and not np.signbit(a).any(), f"{case.name}: tile ({band}, {ct}) is not all {exact[0, band, ct]}"
            else:
                assert _fractional(a), f"{case.name}: the reference is trivial in tile ({band}, {ct})"
        else:    # several layers with partial coverage meet in the tile
            n = sum(_fractional(_in_tile(case, p, band, ct)) for p in case.named)
            assert n >= 2 or (band, ct) == (0, 3), f"{case.name}: {n} paths with partial coverage in tile ({band}, {ct})"
    for p in case.named:
        assert _fractional(lc.reference(case)[p][0]), f"{case.name}: path {p}"
    for (p, band, ct), _v in exact.items():
        assert (band, ct) in case.tiles


# ------------------------------------------------------------------------------------------------------------------ several paths
def test_the_neighbours_are_laid_out_as_described():
    for case in lc.MULTI:
        base = lc.base_name(case)
        if base not in ("neighbours", "big_neighbours"):
            continue
        n = len(case.paths)
        assert 5 <= len(case.named) <= 8 and 0 in case.empty and n - 1 in case.empty and any(0 < p < n - 1 for p in case.empty)
        if base == "neighbours":
            assert 5 <= n <= 8 and [p for p in range(n) if case.paths[p][1] == "evenodd"] == [p for p in range(n) if p % 3 == 2]
        refs = lc.reference(case)
        live = [p for p in range(n) if p not in case.empty]
        shapes = [refs[p][2][2:] for p in live]
        for a, b in zip(shapes, shapes[1:]):   # a store with the neighbour's `lcols` or `layer_off` lands somewhere else
            assert a[1] != b[1] and a[0] * a[1] != b[0] * b[1]
        for shift in SHIFTS[1:]:               # the same layers, moved
            for p in live:
                assert lc.reference(case, shift)[p][2][2:] == refs[p][2][2:]
        assert len({tuple(case.paths[p][2]) for p in live}) == len(live)   # every layer its own paint
    for case in lc.BIG:
        _m, _f, bb = lc.reference(case)[7]   # the filler: in the viewport's last column tile of its first band
        assert (bb[1] - case.viewport[1]) // TC == 3 and bb[0] + bb[2] - case.viewport[0] <= TR


# ------------------------------------------------------------------------------------------------------------------ the translation
def test_the_translation_moves_the_layers_and_their_tile_alignment():
    assert lc.SHIFT == (3, -5) and lc.SHIFT[0] % TR and lc.SHIFT[1] % TC
    moved = 0
    for case in lc.SINGLE:
        if case.viewport is None or "cut" in case.want or 0 in case.empty or "one_" in case.name or "class1_cut" in case.name:
            continue
        bb, sb = lc.reference(case)[0][2], lc.reference(case, lc.SHIFT)[0][2]
        assert sb == (bb[0] + 3, bb[1] - 5, bb[2], bb[3]), f"{case.name}: {bb} -> {sb}"
        moved += 1
    assert moved >= 40
    # the reference of the shifted points is the reference of the path data written at the shifted place
    for origin in cc.ORIGINS:
        vp = (*origin, *cc.VIEW)
        there = lc.lbox(cc.Geo((origin[0] + 3, origin[1] - 5)), 23, 70, 36, 150)
        here = lc.lbox(cc.Geo(origin), 23, 70, 36, 150)
        for rule in (None, "evenodd"):
            a, abb = lc.mask_ref(there, rule, vp)
            b, bbb = lc.mask_ref(here, rule, vp, lc.SHIFT)
            assert abb == bbb
            assert_close64(b, a, atol=1e-12, what="shifted reference")


def test_mask_ref_is_path_mask():
    for case in lc.SINGLE[:8] + lc.SINGLE[-2:]:
        d, rule, _p = case.paths[0]
        lines, cubics = cr.segments(d)
        m, (r0, c0), _e = orc.path_mask(lines, cubics, None, rule, case.viewport)
        got, bb = lc.mask_ref(d, rule, case.viewport)
        assert bb == (r0, c0, *m.shape) and np.array_equal(got, m)
        assert np.array_equal(lc.raw_coverage(d, rule, case.viewport), cr.raw_coverage(d, rule, case.viewport))
