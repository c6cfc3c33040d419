"""What tests/test_gpu_image_seams.py and tests/test_gpu_displacement_seams.py rely on, shown on the CPU: the host build of
svgr_core.h's image index rule (tests/image_harness.cpp) and of the displacement map's guard (tests/filter_harness.cpp) keep
every index inside its level / source for NaN, infinite, huge and boundary coordinates -- the evidence that the non-finite
GPU cases cannot read outside a buffer --; the cases of tests/image_cases.py take the routes they are named for, keep their
clearances, show more than blank pixels, and their float64 restatement stays within half of image_ref.fill_tolerance of the
long-double sample, so the reference alone never trips the bound.  No GPU needed."""
import ctypes as C
import functools
import itertools
import math

import numpy as np
import pytest

from tests import filter_ref as F
from tests import image_cases as IC
from tests import image_ref as R
from tests.util import host_build


@functools.lru_cache(maxsize=None)
def _harness():
    L = host_build("image_harness")
    f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
    i32p = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
    L.ih_corner.argtypes = [f64p, f64p, i32p, i32p, C.c_long, i32p, f64p]
    L.ih_nearest.argtypes = [f64p, f64p, i32p, i32p, C.c_long, i32p]
    return L


def _corner(x, y, w, h):
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    ws, hs = np.full(len(x), w, dtype=np.int32), np.full(len(x), h, dtype=np.int32)
    idx, frac = np.full((len(x), 4), -99, dtype=np.int32), np.full((len(x), 2), np.nan)
    _harness().ih_corner(x, y, ws, hs, len(x), idx, frac)
    return idx, frac


def _nearest(u, v, w, h):
    u, v = np.ascontiguousarray(u, dtype=np.float64), np.ascontiguousarray(v, dtype=np.float64)
    idx = np.full((len(u), 2), -99, dtype=np.int32)
    _harness().ih_nearest(u, v, np.full(len(u), w, dtype=np.int32), np.full(len(u), h, dtype=np.int32), len(u), idx)
    return idx


def _neighbours(v):
    return [np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf)]


def sweep(n):
    """The coordinates the index rule is swept over for an axis of n texels."""
    vals = [math.nan, math.inf, -math.inf, 1e300, -1e300, 2.0 ** 31, -2.0 ** 31, 2.0 ** 62, -2.0 ** 62, 0.0, -0.0]
    for v in (-1.0, 0.0, n - 1.0, float(n)):
        vals += _neighbours(v)
    vals += _neighbours(2.0 ** 31 - 1) + _neighbours(-2.0 ** 31 - 1) + [-1.5, -0.5, 0.5, n - 0.5, n + 0.5, 5e-324, -5e-324]
    return np.array(vals)


SIZES = (1, 2, 3, 37)


# ====================================================================================== 1. the index rule
@pytest.mark.parametrize("w, h", list(itertools.product(SIZES, SIZES)))
def test_corner_indices_stay_inside_the_level(w, h):
    xs, ys = sweep(w), sweep(h)
    x, y = (a.ravel() for a in np.meshgrid(xs, ys, indexing="ij"))
    idx, frac = _corner(x, y, w, h)
    assert ((idx[:, :2] >= 0) & (idx[:, :2] <= w - 1)).all(), x[((idx[:, :2] < 0) | (idx[:, :2] > w - 1)).any(axis=1)][:5]
    assert ((idx[:, 2:] >= 0) & (idx[:, 2:] <= h - 1)).all(), y[((idx[:, 2:] < 0) | (idx[:, 2:] > h - 1)).any(axis=1)][:5]
    assert ((frac >= 0.0) & (frac <= 1.0)).all()   # (false for a NaN)
    # the restatement's rule is the harness's, value for value
    for col, (i0, i1, f) in zip((x, y), (R.corner(x, w), R.corner(y, h))):
        k = 0 if col is x else 2
        assert np.array_equal(idx[:, k], i0) and np.array_equal(idx[:, k + 1], i1)
        assert np.array_equal(frac[:, k // 2], f)


@pytest.mark.parametrize("w", SIZES)
def test_corner_non_finite_rule(w):
    """NaN: texel 0, fraction 0; + inf and anything >= w: the last texel; - inf and anything below -1: the first."""
    x = np.array([math.nan, math.inf, float(w), 1e300, -math.inf, -1e300, np.nextafter(-1.0, -np.inf)])
    idx, frac = _corner(x, x, w, w)
    assert idx[0].tolist() == [0, 0, 0, 0] and frac[0].tolist() == [0.0, 0.0]
    assert (idx[1:4] == w - 1).all() and (idx[4:] == 0).all()
    # between the two, an in-range coordinate gives floor and floor + 1 with the fraction between them
    idx, frac = _corner(np.array([w - 1.0 - 0.25]), np.array([0.25]), w, 3)
    assert idx[0].tolist() == [max(w - 2, 0), w - 1, 0, 1] and frac[0].tolist() == [0.75, 0.25]


@pytest.mark.parametrize("w, h", list(itertools.product(SIZES, SIZES)))
def test_nearest_indices_stay_inside_the_level(w, h):
    xs, ys = sweep(w), sweep(h)
    u, v = (a.ravel() for a in np.meshgrid(xs, ys, indexing="ij"))
    idx = _nearest(u, v, w, h)
    assert ((idx[:, 0] >= 0) & (idx[:, 0] <= w - 1)).all() and ((idx[:, 1] >= 0) & (idx[:, 1] <= h - 1)).all()
    assert np.array_equal(idx[:, 0], R.nearest_index(u, w)) and np.array_equal(idx[:, 1], R.nearest_index(v, h))
    assert (idx[np.isnan(u), 0] == 0).all() and (idx[np.isnan(v), 1] == 0).all()


def test_indices_of_every_case_stay_inside_their_levels():
    """Every FillCase, the non-finite ones included, at every level it reads: the coordinates of the whole box through the
    host build."""
    for case in IC.FILL_CASES:
        u, v = R.coordinates(case.inv_m, *case.bbox)
        u, v = u.ravel(), v.ravel()
        sizes = [lv[1:] for lv in _levels(case.shape)]
        if not case.smooth:
            h, w = case.shape
            idx = _nearest(u, v, w, h)
            assert ((idx >= 0) & (idx <= [w - 1, h - 1])).all(), case.name
            continue
        for k in R.levels_read(len(sizes), case.lam(), True):
            h, w = sizes[k]
            s = 2.0 ** -k
            idx, frac = _corner(u * s - 0.5, v * s - 0.5, w, h)
            assert ((idx >= 0) & (idx <= [w - 1, w - 1, h - 1, h - 1])).all(), (case.name, k)
            assert ((frac >= 0.0) & (frac <= 1.0)).all(), (case.name, k)


def _levels(shape):
    from svgrasterize_amd import _abi

    return _abi.image_levels(*shape)


# ====================================================================================== 2. the displacement map's guard
@pytest.mark.parametrize("srows, scols", [(1, 1), (2, 3), (37, 3)])
@pytest.mark.parametrize("s0, s1", [(0, 0), (-5, 8)])
def test_displacement_guard_reads_inside_the_source(srows, scols, s0, s1):
    L = F.harness()
    p0 = np.concatenate([sweep(srows), sweep(srows) + s0])
    p1 = np.concatenate([sweep(scols), sweep(scols) + s1])
    a, b = (np.ascontiguousarray(g.ravel()) for g in np.meshgrid(p0, p1, indexing="ij"))
    out = np.full(len(a), -99, dtype=np.int64)
    L.fh_dm_index(a, b, len(a), s0, s1, srows, scols, out)
    assert ((out >= -1) & (out < srows * scols)).all()
    with np.errstate(invalid="ignore"):
        r, c = np.floor(a) - s0, np.floor(b) - s1
        inside = (r >= 0) & (r < srows) & (c >= 0) & (c < scols)
    want = np.where(inside, np.where(inside, r, 0).astype(np.int64) * scols + np.where(inside, c, 0).astype(np.int64), -1)
    assert np.array_equal(out, want) and inside.any() and not inside[~np.isfinite(a) | ~np.isfinite(b)].any()


def test_displacement_guard_negative_zero_reads_row_0():
    """floor(p) - s0 == -0.0 passes `>= 0.0` and casts to 0.  (The kernel's own sum cannot produce it: x + 0.5 + d is +0.0
    when it is zero; the guard is shown on the harness alone.)"""
    out = np.full(2, -99, dtype=np.int64)
    F.harness().fh_dm_index(np.array([-0.0, 1.0]), np.array([-0.0, -0.0]), 2, 0, 0, 2, 3, out)
    assert out.tolist() == [0, 3]


# ====================================================================================== 3. the fill cases
SMOOTH_WIDE = [c for c in IC.FILL_CASES if c.smooth and c.route not in IC.EXACT_ROUTES]


def test_case_names_are_unique():
    assert len({c.name for c in IC.FILL_CASES}) == len(IC.FILL_CASES)
    assert len({c.name for c in IC.DM_CASES}) == len(IC.DM_CASES)


@pytest.mark.parametrize("case", SMOOTH_WIDE, ids=lambda c: c.name)
def test_float64_restatement_stays_within_half_the_tolerance(case):
    levels = R.mip_chain(case.pixels(), case.linear_rgb)
    lam = case.lam()
    wide = R.sample_wide(levels, case.inv_m, True, lam, *case.bbox)
    plain = R.sample(levels, case.inv_m, True, *case.bbox, lam=lam)
    tol = R.fill_tolerance(case, levels)
    err = float(np.abs(plain - wide).max())
    assert 0.0 < tol < 1e-9 and err <= 0.5 * tol, (case.name, err, tol)


@pytest.mark.parametrize("case", [c for c in IC.FILL_CASES if c.smooth and c.route in IC.EXACT_ROUTES and c.route != "nonfinite"],
                         ids=lambda c: c.name)
def test_exact_smooth_cases_agree_in_both_precisions(case):
    """The cases compared bit for bit with the float64 restatement: the long-double sample, rounded, differs from it by no
    more than the lerps' own roundings -- the coordinates themselves carry no error."""
    levels = R.mip_chain(case.pixels(), case.linear_rgb)
    lam = case.lam()
    wide = R.sample_wide(levels, case.inv_m, True, lam, *case.bbox)
    plain = R.sample(levels, case.inv_m, True, *case.bbox, lam=lam)
    assert float(np.abs(plain - wide).max()) <= R.U * (R.FILL_ROUNDINGS + 1)


def test_nearest_cases_keep_their_clearance_or_are_dyadic():
    for case in IC.FILL_CASES:
        if case.smooth or case.route == "nonfinite":
            continue
        if case.route == "exact":
            # exact arithmetic: fused, unfused and long double give the same coordinates
            u, v = R.coordinates(case.inv_m, *case.bbox)
            uw, vw = R.coordinates(case.inv_m, *case.bbox, dtype=R.LD)
            assert np.array_equal(u.astype(R.LD), uw) and np.array_equal(v.astype(R.LD), vw), case.name
            if "dyadic" in case.name:
                assert (u == np.floor(u)).any() and (v == np.floor(v)).any(), case.name   # (on boundaries, on purpose)
        else:
            assert R.clearance(case) >= IC.CLEARANCE, (case.name, R.clearance(case))


def test_cases_take_their_routes():
    seen = set()
    for case in IC.FILL_CASES:
        seen.add(case.route)
        r0, c0, rows, cols = case.bbox
        n_levels = len(_levels(case.shape))
        lam = case.lam()
        if case.route == "seam":
            assert rows < 3 * IC.TILE_H or cols < 3 * IC.TILE_W
        elif case.route == "stride":
            assert rows > IC.GRID_ROWS * IC.TILE_H and rows % IC.TILE_H != 0
        elif case.route == "lod_int":
            assert lam == math.floor(lam) and lam == math.log2(abs(case.inv_m[0, 1])) and lam < n_levels - 1
        elif case.route == "lod_blend":
            f = lam - math.floor(lam)
            assert 0.0 < f < 1e-8 or 1 - 1e-8 < f < 1.0
        elif case.route == "lod_top":
            assert lam == n_levels - 1 and n_levels > 1
        elif case.route == "lod_last":
            assert lam != math.floor(lam)
            sizes = [lv[1:] for lv in _levels(case.shape)]
            assert min(sizes[math.floor(lam) + 1]) == 1   # (the upper level is one texel on an axis at least)
        elif case.route == "degenerate":
            assert min(case.shape) <= 3
        elif case.route == "edge":
            h, w = case.shape
            assert rows > 3 * h and cols > 3 * w
        elif case.route == "nonfinite":
            assert not np.isfinite(case.inv_m).all() or np.abs(case.inv_m).max() >= 1e308
    assert seen == {"seam", "stride", "lod_int", "lod_blend", "lod_top", "lod_last", "degenerate", "edge", "exact", "nonfinite", "nearest"}
    rows = {c.bbox[2] for c in IC.fill_cases("seam")}
    cols = {c.bbox[3] for c in IC.fill_cases("seam")}
    assert {7, 8, 9, 17, 1, 200} <= rows and {31, 32, 33, 65, 1, 200} <= cols
    assert any(c.bbox[0] % IC.TILE_H and c.bbox[0] < 0 for c in IC.fill_cases("seam"))
    assert any(c.bbox[1] % IC.TILE_W and c.bbox[1] < 0 for c in IC.fill_cases("seam"))


def test_stride_cases_gather_from_inside_the_image_on_both_trips():
    first_trip_rows = IC.GRID_ROWS * IC.TILE_H
    for case in IC.fill_cases("stride"):
        u, v = R.coordinates(case.inv_m, *case.bbox)
        h, w = case.shape
        inside = ((u > 0) & (u < w) & (v > 0) & (v < h))[:, 0]
        rows = np.flatnonzero(inside)
        assert 50 < len(rows) < 100
        if "tail" in case.name:
            assert rows.min() >= case.bbox[2] - 100 and (rows >= first_trip_rows).sum() >= 4
        else:
            assert rows.max() < 100


@pytest.mark.parametrize("case", IC.fill_cases("seam", "stride"), ids=lambda c: c.name)
def test_seam_cases_are_not_blank(case):
    levels = R.mip_chain(case.pixels(), case.linear_rgb)
    want = R.sample(levels, case.inv_m, case.smooth, *case.bbox, lam=case.lam()) * case.mask()[..., None]
    assert (want == 0.0).mean() < 0.05
    if case.bbox[2] * case.bbox[3] > 1:
        assert len(np.unique(want[..., 3])) > 1


def test_non_finite_rule_of_the_restatement():
    """NaN -> texel 0; + inf -> the last texel; - inf -> the first; 1e308 times a pixel coordinate -> the first / last column
    by the coordinate's sign."""
    by_name = {c.name: c for c in IC.fill_cases("nonfinite")}
    img = by_name["nonfinite_m02_nan_nearest"]
    levels = R.mip_chain(img.pixels(), False)
    L0 = levels[0].astype(np.float64)
    r0, c0, rows, cols = img.bbox
    v_rows = np.clip(np.floor(np.arange(rows) + r0 + 0.5 + 3.25), 0, 36).astype(int)   # (v = p0 + 3.25)
    u_cols = np.clip(np.floor(np.arange(cols) + c0 + 0.5 + 3.25), 0, 52).astype(int)   # (u = p1 + 3.25)
    for tag, smooth in (("nearest", False), ("smooth", True)):
        def run(name):
            c = by_name[f"nonfinite_{name}_{tag}"]
            return R.sample(levels, c.inv_m, smooth, *c.bbox, lam=c.lam())
        got = run("m02_nan")
        if not smooth:
            assert np.array_equal(got, np.broadcast_to(L0[v_rows, 0][:, None], got.shape))
            assert np.array_equal(run("m02_neginf"), got)
            assert np.array_equal(run("m12_inf"), np.broadcast_to(L0[36, u_cols][None], got.shape))
            edge = run("m00_1e308")
            p0 = np.arange(rows) + r0 + 0.5
            assert np.array_equal(edge[:, 0], np.where((p0 < 0)[:, None], L0[v_rows, 0], L0[v_rows, 52]))
        else:
            assert np.array_equal(got[:, 0], got[:, -1]) and np.array_equal(run("m02_neginf"), got)   # (column 0, whatever p1)
            y = np.arange(rows) + r0 + 0.5 + 3.25 - 0.5   # (level 0: exact)
            yf = np.floor(y)
            want = R._lerp(L0[np.clip(yf, 0, 36).astype(int), 0], L0[np.clip(yf + 1, 0, 36).astype(int), 0], (y - yf)[:, None])
            assert np.array_equal(got[:, 0], want)
            top = run("m00_1e308")
            assert np.array_equal(top, np.broadcast_to(levels[-1][0, 0].astype(np.float64), top.shape))
        assert np.isfinite(got).all()


# ====================================================================================== 4. the displacement cases
@pytest.mark.parametrize("case", IC.DM_CASES, ids=lambda c: c.name)
def test_displacement_cases(case):
    src, disp = IC.dm_inputs(case)
    xc, yc = IC.DM_CHANNELS
    args = (disp, case.map_off, case.lin, case.scale, xc, yc)
    wide = F.displacement_map_wide(src, case.src_off, *args)
    assert F.displacement_clearance(case.src_shape, case.src_off, *args) >= IC.CLEARANCE
    (s0, s1), (sr, sc) = case.src_off, case.src_shape
    (m0, m1), (mr, mc) = case.map_off, case.map_shape
    disjoint = m0 + mr <= s0 or s0 + sr <= m0 or m1 + mc <= s1 or s1 + sc <= m1
    assert disjoint == (case.route == "off")
    if case.route in ("off", "far"):
        assert not wide.any()   # (the stated exception: zero is the expected value)
        return
    hit = wide[..., 3] != 0
    assert hit.any()
    if case.special is None and all(np.isfinite(case.lin).ravel()):
        with np.errstate(invalid="ignore"):
            plain = F.displacement_map(src, case.src_off, *args)
        assert np.array_equal(plain, wide)
    if case.special == "nan":
        nan_px = np.isnan(disp[..., 0])
        assert nan_px.any() and not wide[nan_px].any() and hit[~nan_px].any()
        # a NaN cast to an integer before the comparison would be device pixel (0, 0) on the GPU: the source covers it
        assert s0 <= 0 < s0 + sr and s1 <= 0 < s1 + sc and src[-s0, -s1].any()
    if case.special == "half" or case.scale == 0.0:
        # no displacement: the pixel under the map pixel, transparent off the source
        still = np.ones(case.map_shape, bool) if case.scale == 0.0 else (disp[..., 0] == 0.5)
        R_, C_ = np.nonzero(still)
        r, c = R_ + m0 - s0, C_ + m1 - s1
        ok = (r >= 0) & (r < sr) & (c >= 0) & (c < sc)
        want = np.where(ok[:, None], src[np.where(ok, r, 0), np.where(ok, c, 0)], 0.0)
        assert ok.any() and np.array_equal(wide[R_, C_], want)


def test_premultiplied_map_has_the_alphas_of_the_convert_rule():
    from tests import layer_ref as LR

    img = IC.dm_premultiplied_map()
    a = img[..., 3]
    assert (a == 0.0).any() and (a == 5e-5).any() and (a == 1e-3).any() and (a > 0.01).any()
    straight, _tol = LR.convert(img, LR.PRE_TO_STRAIGHT)
    straight = straight.astype(np.float64)
    kept = a <= 1e-4
    assert np.array_equal(straight[kept], np.clip(img[kept], 0, 1)) and (straight[a == 1e-3][:, :3] > 0.01).any()
