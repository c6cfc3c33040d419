"""The tile kernel's CLIP, GROUPS and GRAD variants (and, for the same layouts without clips, the plain ones) against the plain
float64 reference of tests/canvas_ref.py, on the directed cases of tests/canvas_cases.py: clip sources, clipped paths, groups and
gradients placed relative to the 16 x 64 tile grid and the 8-row halves of the two waves, and tiles of 1 .. 130 items.  Every
launch form -- both canvas types, with and without SVGR_RENDER_CLIP01, a second render, deterministic renders, a window, the window
table, band sharding -- is compared with the reference's pixels, never with another render.

Tolerances are the project's existing ones (tests/test_gpu_fuzz.py): 1e-10 absolute on the float64 canvas, 1 ULP(float32) on the
float32 canvas.  The cases keep every coverage 1e-9 away from the `mask < 1e-6` cut (tests/test_canvas_ref_host.py), so neither
needs an allowance for it.  Each comparison prints its worst error before it asserts."""
import numpy as np
import pytest

from tests import canvas_cases as cc
from tests import canvas_ref as cr
from tests.util import assert_close64, assert_f32_1ulp, ulp_f32

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import svgrasterize_amd as S

    S.Context.get()
    return S


_REFS = {}


def _ref(case, clamp=False):
    """The reference canvas of a case, computed once and shared (read-only); non-trivial in every tile under test."""
    if case.name not in _REFS:
        ref = cr.render(case.entries, case.groups, case.viewport)
        for band, ct in case.tiles:
            assert cc.nontrivial(case, ref, band, ct), f"{case.name}: the reference is trivial in tile ({band}, {ct})"
        clamped = ref.clip(0, 1)
        ref.flags.writeable = clamped.flags.writeable = False
        _REFS[case.name] = (ref, clamped)
    return _REFS[case.name][1 if clamp else 0]


def _planned(S, case):
    ctx = S.Context.get()
    batch = cc.build_batch(S, case, ctx)
    batch.plan()
    return ctx, batch


def _kinds():
    from svgrasterize_amd import _abi

    return ((_abi.OUT_CANVAS_F64, np.float64, 32), (_abi.OUT_CANVAS_F32, np.float32, 16))


def _check(got, ref, what):
    """float64: within 1e-10 of the reference; float32: within 1 ULP of float32(reference).  The worst error is printed first."""
    if got.dtype == np.float64:
        print(f"{what}: f64 max abs err {np.abs(got - ref).max(initial=0.0):.3e}")
        assert_close64(got, ref, atol=1e-10, what=what)
    else:
        err = np.abs(got.astype(np.float64) - ref.astype(np.float32).astype(np.float64))
        print(f"{what}: f32 max abs err {err.max(initial=0.0):.3e}, {(err / np.maximum(ulp_f32(ref), 2.0 ** -24)).max(initial=0.0):.2f} ulp")
        assert_f32_1ulp(got, ref, what=what)


def _window(case):
    """An unaligned window that cuts through the first tile under test: it starts inside the tile's rows and, unless the tile is
    the first of its band, in the column tile to its left, and ends in the next band / the next column tile."""
    r0, c0, rows, cols = case.viewport
    band, ct = case.tiles[0]
    r_lo, c_lo = band * cc.TR + 3, ct * cc.TC + 5 if ct == 0 else ct * cc.TC - 9
    r_hi, c_hi = min(rows, r_lo + 21), min(cols, ct * cc.TC + 88)
    return (r0 + r_lo, c0 + c_lo, r_hi - r_lo, c_hi - c_lo)


def _cut(ref, case, win):
    r, c = win[0] - case.viewport[0], win[1] - case.viewport[1]
    return ref[r:r + win[2], c:c + win[3]]


@pytest.mark.parametrize("case", cc.CASES, ids=cc.IDS)
def test_canvas_equals_the_reference(S, case):
    """Both canvas types, with and without SVGR_RENDER_CLIP01, each rendered twice: the second render runs the geometry pass again
    instead of reusing the plan's."""
    from svgrasterize_amd import _abi

    ctx, batch = _planned(S, case)
    _r0, _c0, rows, cols = case.viewport
    for kind, dt, px in _kinds():
        out = ctx.alloc(rows * cols * px)
        for flags in (0, _abi.RENDER_CLIP01):
            for nth in (1, 2):
                batch.render(out, kind, flags)
                _check(out.download((rows, cols, 4), dt), _ref(case, bool(flags)), f"{case.name} flags {flags} render {nth}")
        out.free()
    batch.destroy()


@pytest.mark.parametrize("case", cc.CASES, ids=cc.IDS)
def test_deterministic_renders_are_identical_and_equal_the_reference(S, case):
    from svgrasterize_amd import _abi

    ctx, batch = _planned(S, case)
    _r0, _c0, rows, cols = case.viewport
    for kind, dt, px in _kinds():
        outs = [ctx.alloc(rows * cols * px) for _ in range(2)]
        for o in outs:
            batch.render(o, kind, _abi.RENDER_DETERMINISTIC | _abi.RENDER_CLIP01)
        a, b = (o.download((rows, cols, 4), dt) for o in outs)
        assert np.array_equal(a, b), f"{case.name}: two deterministic renders differ"
        _check(a, _ref(case, True), f"{case.name} deterministic")
        for o in outs:
            o.free()
    batch.destroy()


@pytest.mark.parametrize("case", cc.CASES, ids=cc.IDS)
def test_window_equals_the_references_pixels(S, case):
    from svgrasterize_amd import _abi

    ctx, batch = _planned(S, case)
    win = _window(case)
    for kind, dt, px in _kinds():
        out = ctx.alloc(win[2] * win[3] * px)
        for flags in (0, _abi.RENDER_CLIP01):
            batch.render(out, kind, flags, window=win)
            _check(out.download((win[2], win[3], 4), dt), _cut(_ref(case, bool(flags)), case, win), f"{case.name} window {win} flags {flags}")
        out.free()
    batch.destroy()


@pytest.mark.parametrize("case", cc.CASES, ids=cc.IDS)
def test_window_table_equals_the_references_pixels(S, case):
    """Three windows in one launch (k_tile_render_windows for every variant but the production one): the unaligned window through
    the tile under test, one pixel inside that tile, and all of the canvas but its rim."""
    from svgrasterize_amd import _abi

    ctx, batch = _planned(S, case)
    r0, c0, rows, cols = case.viewport
    band, ct = case.tiles[0]
    wins = [_window(case), (r0 + band * cc.TR + 9, c0 + ct * cc.TC + 33, 1, 1), (r0 + 1, c0 + 2, rows - 2, cols - 3)]
    for kind, dt, px in _kinds():
        for flags in (0, _abi.RENDER_CLIP01):
            outs = [ctx.alloc(w[2] * w[3] * px) for w in wins]
            batch.render_windows(outs, kind, wins, flags)
            for w, o in zip(wins, outs):
                _check(o.download((w[2], w[3], 4), dt), _cut(_ref(case, bool(flags)), case, w), f"{case.name} table window {w} flags {flags}")
                o.free()
    batch.destroy()


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("case", cc.CASES, ids=cc.IDS)
def test_every_rank_of_a_sharded_canvas_equals_the_references_rows(S, case, world):
    """svgr_batch_set_bands(rank, world, 1): rank r draws bands r, r + world, ... packed one under the other.  The library takes
    sharded batches with clip pairs, groups and gradients alike (only a render window and the per-path outputs are refused)."""
    from svgrasterize_amd import _abi

    ctx = S.Context.get()
    batch = cc.build_batch(S, case, ctx)
    _r0, _c0, rows, cols = case.viewport
    n_bands = -(-rows // cc.TR)
    ref = _ref(case, True)
    for rank in range(world):
        bands = [b for b in range(n_bands) if b % world == rank]
        batch.set_bands(rank, world, 1)
        batch.plan()
        assert batch.owned_rows() == len(bands) * cc.TR
        for kind, dt, px in _kinds():
            out = ctx.alloc(len(bands) * cc.TR * cols * px)
            batch.render(out, kind, _abi.RENDER_CLIP01)
            got = out.download((len(bands) * cc.TR, cols, 4), dt)
            for k, b in enumerate(bands):
                n = min(cc.TR, rows - b * cc.TR)   # (the viewport's last band is cut: the rows behind it are not drawn)
                _check(got[k * cc.TR: k * cc.TR + n], ref[b * cc.TR: b * cc.TR + n], f"{case.name} rank {rank} of {world} band {b}")
            out.free()
        with pytest.raises(ValueError):
            batch.render(ctx.alloc(64), _abi.OUT_CANVAS_F64, 0, window=_window(case))   # a window and sharding exclude each other
    batch.destroy()
