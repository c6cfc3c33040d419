"""What tests/test_gpu_filter_paint_seams.py relies on, shown without a device: which workgroup tile each feConvolveMatrix order
of its cases gets, the pattern restatement (tests/paint_ref.py) against plain tiling, and -- with oracle.gradient_image -- that
the focal gradient of its tall boxes has a negative determinant in the rows of the row-stride loop's second trip and nowhere else."""
import os
import re

import numpy as np
import pytest

from oracle import oracle as orc
from tests import filter_ref as F
from tests import paint_ref as P
from tests.util import ROOT

HIP = os.path.join(ROOT, "svgrasterize.py_amd", "csrc", "svgr_hip.hip")


def test_convolve_matrix_orders_sit_on_both_sides_of_the_tile_switch():
    """The restated rule is the launcher's (its two lines are looked up in the source: if the switch moves, this fails and the
    orders of the device cases are chosen again), and the orders of the cases take the tiles they were chosen for."""
    text = re.sub(r"\s+", " ", open(HIP).read())
    assert "auto lds = [&](int T) { return (size_t)(T + order_y - 1) * (size_t)(T + order_x - 1) * 32 + (size_t)order_x * order_y * 8; };" in text
    assert "const int T = lds(16) <= (64u << 10) ? 16 : 8;" in text
    assert [F.convolve_matrix_tile(*o) for o in [(28, 28), (28, 29), (29, 28), (32, 32), (1, 1)]] == [16, 8, 8, 8, 16]
    assert F.convolve_matrix_lds(16, 28, 28) == 65440 == (64 << 10) - 96   # the largest request of all
    assert F.convolve_matrix_lds(8, 32, 32) == 56864   # (39 x 39 pixels of halo and 1024 weights: the launcher's "56 KiB")
    # no order below (28, 28) in both directions is on the 8 x 8 tile, and the existing cases (3, 4) and (32, 5) are on 16 x 16
    assert all(F.convolve_matrix_tile(oy, ox) == 16 for oy in range(1, 29) for ox in range(1, 29))
    assert F.convolve_matrix_tile(3, 4) == F.convolve_matrix_tile(32, 5) == 16
    assert max(F.convolve_matrix_lds(F.convolve_matrix_tile(oy, ox), oy, ox) for oy in range(1, 33) for ox in range(1, 33)) == 65440


def test_pattern_restatement_tiles_the_plane():
    """Identity transform, whole-pixel cell: the fill is the canvas repeated, np.tile's way, from the cell's origin."""
    rng = np.random.default_rng(3)
    tile = rng.uniform(-0.2, 1.2, (5, 4, 4))
    pat = P.pattern_geometry(np.identity(2), (2.0, -3.0, 7.0, 5.0), (1, 1), tile.shape[:2])
    assert (pat["min_xy"], pat["pat_shape"], pat["tile_bbox"]) == ([0, 0], [8, 6], [1, 1, 5, 4])
    mask = rng.random((19, 30))
    got = P.pattern_fill(pat, tile, mask, (-4, 6, 19, 30))
    canvas = P.pattern_canvas(pat, tile)
    assert canvas.min() == 0.0 and canvas.max() == 1.0 and not canvas[0].any() and not canvas[:, 0].any()
    rr = (np.arange(-4, 15) - 2) % 7   # (pixel centre i + 0.5 - x, modulo the cell, truncated)
    cc = (np.arange(6, 36) + 3) % 5
    assert np.array_equal(got, canvas[rr[:, None], cc[None, :]] * mask[..., None])
    # a canvas too small for the cell: numpy's IndexError
    with pytest.raises(IndexError):
        P.pattern_fill(dict(pat, pat_shape=[4, 6]), tile, mask, (-4, 6, 19, 30))
    # negative offsets wrap once, like numpy's: the canvas moved by (3, 2) reads its last rows / columns for the first offsets
    moved = dict(pat, min_xy=[3, 2], pat_shape=[8, 6])
    got = P.pattern_fill(moved, tile, mask, (-4, 6, 19, 30))
    assert np.array_equal(got, canvas[((rr - 3) % 8)[:, None], ((cc - 2) % 6)[None, :]] * mask[..., None])
    with pytest.raises(IndexError):
        P.pattern_fill(dict(pat, min_xy=[9, 0]), tile, mask, (-4, 6, 19, 30))


def test_fma_rounds_once():
    a, b = 1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30
    assert a * b - 1.0 == 0.0 and P.fma(a, b, -1.0) == -(2.0 ** -60)


def _oracle(name, bbox):
    g = P.GRADIENTS[name]
    off = np.array([o for o, _ in g["stops"]])
    col = np.array([c for _, c in g["stops"]])
    return orc.gradient_image(g["kind"], bbox, np.asarray(g["user"]), None, g["spread"], off, col, **P.oracle_kwargs(g))


def test_tall_focal_gradient_has_its_negative_determinants_in_the_second_trip_only():
    box = P.tall_box(3)
    top = (box[0], box[1], P.FIRST_SECOND_TRIP_ROW, 3)
    rest = (box[0] + P.FIRST_SECOND_TRIP_ROW, box[1], box[2] - P.FIRST_SECOND_TRIP_ROW, 3)
    assert rest[2] == 2
    whole, first, second = _oracle("focal_detneg", box), _oracle("focal_detneg", top), _oracle("focal_detneg", rest)
    # every stop has alpha > 0: a transparent pixel is a masked one
    assert (first[..., 3] > 0).all(), "no pixel of the first 32768 rows is masked: none has det < 0"
    assert np.array_equal(whole[:P.FIRST_SECOND_TRIP_ROW], first) and np.array_equal(whole[P.FIRST_SECOND_TRIP_ROW:], second)
    assert not second.any(), "rows 32768 and 32769 are masked out: det < 0, or det >= 0 with a negative offset beside one"
    # ... and which of the two, from the restated determinant, for both boxes of the device test
    for cols in (3, 257):
        det = P.focal_det(P.GRADIENTS["focal_detneg"], P.tall_box(cols))
        low, high = det[:P.FIRST_SECOND_TRIP_ROW], det[P.FIRST_SECOND_TRIP_ROW:]
        assert (low > 0).all() and (high < 0).any()
        # beyond the line the first column (and the second, in the last row) is in the mirrored cone: masked by the flag alone
        assert (high[:, 0] > 0).all() and high[1, 1] > 0 and (high[0, 1:] < 0).all() and (high[1, 2:] < 0).all()
        # no pixel sits so close to det = 0 that its sign hangs on a rounding (b^2 is up to 1e20 here)
        assert np.abs(det).min() > 1e6
    # the other focal gradient raises no flag anywhere
    for cols in (3, 257):
        assert (P.focal_det(P.GRADIENTS["focal_inside"], P.tall_box(cols)) > 0).all()
