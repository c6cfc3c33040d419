"""k_band_entries and k_tile_lists at their launch seams, against the plain float64 reference of tests/canvas_ref.py on the cases of
tests/pathbuild_cases.py:

  band lists   1023 .. 8193 paths on 3 bands x 4 column tiles: one group of 64 paths per wave, several, more than the BE_KEEP = 4
               that stay in registers, a last partial quad of groups (5, 6, 9).  The list's order -- (wave, group, lane) -- is the
               paint order: translucent pairs of differing colours overlap exactly where two pieces of the list meet, and the host
               test shows that a swap of any pair moves a pixel by more than 1e-6.  After the plan and after a second render (`reuse`),
               and sharded (the `plist` route)
  weights      one band whose tiles weigh 62, 63, 64 and 70: the last bin of k_tile_lists' histogram (weight_of saturates at 63)
  wide         20 rows x 65 536 / 65 537 / 65 600 columns: 1024 column tiles are one chunk of k_tile_lists, 1025 are two -- counts
               taken again in pass 2, the item count carried from chunk to chunk, ranks over both --, with a 25-item tile (one more
               than a page holds) in the second chunk; the path over the whole width is 13 column runs per band for k_path_build

(Tiles of 23 .. 26 items, on either side of the page's 24, are cases of tests/canvas_cases.py: tests/test_gpu_tile_variants.py.)
Tolerances and cut clearance as in tests/test_gpu_path_build.py; every comparison is with the reference."""
import numpy as np
import pytest

from tests import canvas_cases as cc
from tests import pathbuild_cases as pc
from tests.test_gpu_path_build import _check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import svgrasterize_amd as S

    S.Context.get()
    return S


def _kinds():
    from svgrasterize_amd import _abi

    return ((_abi.OUT_CANVAS_F64, np.float64, 32), (_abi.OUT_CANVAS_F32, np.float32, 16))


def _plan_and_render_twice(S, case, kinds):
    ctx = S.Context.get()
    batch = cc.build_batch(S, case, ctx)
    batch.plan()
    _r0, _c0, rows, cols = case.viewport
    ref = pc.reference(case)
    for kind, dt, px in kinds:
        out = ctx.alloc(rows * cols * px)
        for nth in (1, 2):
            batch.render(out, kind, 0)
            _check(out.download((rows, cols, 4), dt), ref, f"{case.name} [{dt.__name__}, render {nth}]")
        out.free()
    batch.destroy()


@pytest.mark.parametrize("name", pc.BAND_IDS)
def test_band_lists_keep_the_paint_order(S, name):
    case, _second = pc.list_cases()[name]
    _plan_and_render_twice(S, case, _kinds()[:1])


@pytest.mark.parametrize("origin", cc.ORIGINS, ids=lambda o: "o%d_%d" % o)
def test_band_lists_of_a_sharded_batch_keep_the_paint_order(S, origin):
    """4097 paths, world = 2: every rank's list of paths (`plist`) through five groups per wave"""
    from svgrasterize_amd import _abi

    case, _second = pc.list_cases()["bands_4097-o%d_%d" % origin]
    ctx = S.Context.get()
    batch = cc.build_batch(S, case, ctx)
    _r0, _c0, rows, cols = case.viewport
    n_bands = -(-rows // cc.TR)
    ref = pc.reference(case)
    for rank in range(2):
        bands = [b for b in range(n_bands) if b % 2 == rank]
        batch.set_bands(rank, 2, 1)
        batch.plan()
        assert batch.owned_rows() == len(bands) * cc.TR
        out = ctx.alloc(len(bands) * cc.TR * cols * 32)
        for nth in (1, 2):
            batch.render(out, _abi.OUT_CANVAS_F64, 0)
            got = out.download((len(bands) * cc.TR, cols, 4), np.float64)
            for k, b in enumerate(bands):
                _check(got[k * cc.TR: (k + 1) * cc.TR], ref[b * cc.TR: (b + 1) * cc.TR], f"{case.name} [rank {rank} of 2, render {nth}, band {b}]")
        out.free()
    batch.destroy()


@pytest.mark.parametrize("name", pc.WEIGHT_IDS)
def test_tiles_on_either_side_of_the_saturated_weight(S, name):
    case, _weights = pc.list_cases()[name]
    _plan_and_render_twice(S, case, _kinds())


@pytest.mark.parametrize("name", pc.WIDE_IDS)
def test_viewports_of_one_and_two_chunks_of_column_tiles(S, name):
    case, _ = pc.list_cases()[name]
    _plan_and_render_twice(S, case, _kinds())
