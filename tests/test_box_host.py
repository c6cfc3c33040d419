"""CPU-side checks of csrc/svgr_box.h (host build tests/box_harness.cpp): the box of a layer in device coordinates as the layer,
filter and paint kernels use it -- box_of (what the ABI admits as a box), box_cell (lane i's device pixel), box_find (is a device
pixel in that other box, and where) and box_meet (the in-place window of svgr_layer_mix_blend) -- against restatements in
64-bit numpy integers, up to the extremes box_of admits: origins of +-(2^30 - 1) and extents of 2^30 - 1, where an `int`
subtraction of two coordinates overflows.  No GPU needed."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests.util import host_build

LIM = (1 << 30) - 1   # the largest origin (in size) and the largest extent box_of admits
BOXES = [
    (-7, 11, 300, 517), (3, -5, 1, 1025), (-40, -60, 12, 9), (25, 70, 9, 12),   # origins of both signs
    (5, -3, 1, 1), (0, 0, 1, 1),                                                # one pixel
    (2, -9, 1, 77), (-9, 2, 77, 1),                                             # a row, a column
    (4, 4, 0, 9), (4, 4, 9, 0), (-1, -1, 0, 0),                                 # empty
    (LIM, LIM, LIM, LIM), (-LIM, -LIM, LIM, LIM), (LIM, -LIM, 1, LIM), (-LIM, LIM, LIM, 1), (-LIM, -LIM, 1, 1), (LIM, LIM, 1, 1),
    (0, 0, LIM, LIM),
]
# (name, a, b): the pairs box_meet is asked about
PAIRS = [
    ("identical", (-7, 11, 30, 51), (-7, 11, 30, 51)),
    ("nested", (-7, 11, 30, 51), (0, 20, 5, 7)),
    ("nested, sharing a corner", (-7, 11, 30, 51), (-7, 11, 5, 7)),
    ("overlapping", (-7, 11, 30, 51), (10, -20, 40, 50)),
    ("edge-touching rows", (0, 0, 4, 6), (4, 0, 3, 6)),
    ("edge-touching columns", (0, 0, 4, 6), (0, 6, 4, 2)),
    ("corner-touching", (0, 0, 4, 6), (4, 6, 2, 2)),
    ("corner-touching, before", (0, 0, 4, 6), (-2, -2, 2, 2)),
    ("disjoint", (0, 0, 4, 6), (20, -30, 6, 9)),
    ("disjoint on one axis", (0, 0, 4, 6), (1, 30, 2, 2)),
    ("with an empty box inside", (0, 0, 4, 6), (1, 1, 0, 3)),
    ("both empty", (0, 0, 0, 6), (0, 0, 4, 0)),
    ("a row and a column", (2, -9, 1, 77), (-9, 2, 77, 1)),
    ("opposite extremes", (LIM, LIM, LIM, LIM), (-LIM, -LIM, LIM, LIM)),
    ("extreme extents, a 2 x 2 overlap", (-LIM, -LIM, LIM, LIM), (-2, -2, LIM, LIM)),
    ("extreme, nested", (0, 0, LIM, LIM), (LIM - 5, 3, LIM, 8)),
    ("extreme, identical", (LIM, LIM, LIM, LIM), (LIM, LIM, LIM, LIM)),
]


@pytest.fixture(scope="module")
def L():
    lib = host_build("box_harness")
    i32 = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
    i64 = np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")
    u64 = np.ctypeslib.ndpointer(dtype=np.uint64, flags="C_CONTIGUOUS")
    u8 = np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")
    lib.bx_of.argtypes = [i64, C.c_int, i32]
    lib.bx_of.restype = C.c_int
    lib.bx_px.argtypes = [i32]
    lib.bx_px.restype = C.c_ulonglong
    lib.bx_cell.argtypes = [i32, C.c_long, u64, i32]
    lib.bx_cell.restype = None
    lib.bx_find.argtypes = [i32, C.c_long, i32, u8, u64]
    lib.bx_find.restype = None
    lib.bx_meet.argtypes = [i32, i32, i32]
    lib.bx_meet.restype = None
    return lib


def _b(box):
    return np.array(box, dtype=np.int32)


def _pixels(box, rng, n=200):
    """Flat indices of a box's pixels: the corners, the ends of the first and the last row, and n seeded ones."""
    rows, cols = box[2], box[3]
    total = rows * cols
    if total == 0:
        return np.zeros(0, dtype=np.uint64)
    fixed = [0, cols - 1, min(cols, total - 1), total - cols, total - 1, total // 2]
    return np.array(fixed + [int(v) for v in rng.integers(0, total, n)], dtype=np.uint64)


def _cells(box, idx):
    """box_cell in 64-bit integers: (n, 2) device rows and columns."""
    i = idx.astype(np.int64)
    return np.stack([box[0] + i // box[3], box[1] + i % box[3]], axis=1)


def test_pixel_count_and_cells(L):
    rng = np.random.default_rng(1)
    for box in BOXES:
        assert L.bx_px(_b(box)) == box[2] * box[3]
        idx = _pixels(box, rng)
        if len(idx) == 0:
            continue
        got = np.zeros((len(idx), 2), dtype=np.int32)
        L.bx_cell(_b(box), len(idx), idx, got)
        want = _cells(box, idx)
        assert np.array_equal(got.astype(np.int64), want), box
        assert want[0].tolist() == [box[0], box[1]] and want[4].tolist() == [box[0] + box[2] - 1, box[1] + box[3] - 1]


def _queries(box, others, rng):
    """Device pixels to look for in `box`: its corners and the pixels one step outside each of them (a halo), seeded pixels of the
    box and of a band around it, and pixels of every other box -- their corners among them, the far corner of a box at the
    opposite extreme included."""
    r0, c0, rows, cols = box
    q = []
    for r in (r0 - 1, r0, r0 + rows - 1, r0 + rows):
        for c in (c0 - 1, c0, c0 + cols - 1, c0 + cols):
            q.append((r, c))
    span_r, span_c = max(rows, 1), max(cols, 1)
    for _ in range(300):
        q.append((r0 + int(rng.integers(-span_r, 2 * span_r)), c0 + int(rng.integers(-span_c, 2 * span_c))))
    q = [p for p in q if -LIM - 1 <= p[0] <= 2 * LIM and -LIM - 1 <= p[1] <= 2 * LIM]   # (pixels, or halo pixels, of admitted boxes)
    out = [np.array(q, dtype=np.int64).reshape(-1, 2)]
    for o in others:
        idx = _pixels(o, rng, 40)
        if len(idx):
            out.append(_cells(o, idx))
    return np.concatenate(out)


def test_find_against_64_bit_integers(L):
    rng = np.random.default_rng(2)
    n_in = n_out = 0
    for box in BOXES:
        q = _queries(box, BOXES, rng)
        r, c = q[:, 0] - box[0], q[:, 1] - box[1]
        want_ok = (r >= 0) & (r < box[2]) & (c >= 0) & (c < box[3])
        want_at = r * box[3] + c
        ok = np.zeros(len(q), dtype=np.uint8)
        at = np.full(len(q), 0xABABABABABABABAB, dtype=np.uint64)
        L.bx_find(_b(box), len(q), np.ascontiguousarray(q.astype(np.int32)), ok, at)
        assert np.array_equal(ok.astype(bool), want_ok), (box, q[ok.astype(bool) != want_ok][:3].tolist())
        assert np.array_equal(at[want_ok].astype(np.int64), want_at[want_ok]), box
        assert (at[~want_ok] == 0xABABABABABABABAB).all()
        n_in += int(want_ok.sum())
        n_out += int((~want_ok).sum())
        if box[2] * box[3] == 0:
            assert not want_ok.any()
    assert n_in > 1000 and n_out > 2000   # (the sample has plenty of both)


def test_find_where_an_int_subtraction_would_overflow(L):
    """The far corner of the box at one extreme looked for in the box at the other: R - r0 is 3 * 2^30 - 4, past an int; and the
    other way round, -(2^31 - 2), the most negative difference there is."""
    hi, lo = (LIM, LIM, LIM, LIM), (-LIM, -LIM, LIM, LIM)
    far_hi, first_lo = (2 * LIM - 1, 2 * LIM - 1), (-LIM, -LIM)
    assert far_hi[0] - lo[0] > 2 ** 31 - 1 and first_lo[0] - hi[0] == -(2 ** 31 - 2)
    for box, px, inside in ((lo, far_hi, False), (hi, first_lo, False), (hi, far_hi, True), (lo, first_lo, True),
                            ((-LIM, -LIM, 1, 1), far_hi, False), ((LIM, LIM, 1, 1), first_lo, False), ((0, 0, LIM, LIM), far_hi, False)):
        ok = np.zeros(1, dtype=np.uint8)
        at = np.zeros(1, dtype=np.uint64)
        L.bx_find(_b(box), 1, np.array([px], dtype=np.int32), ok, at)
        assert bool(ok[0]) == inside, (box, px)
        if inside:
            assert int(at[0]) == (px[0] - box[0]) * box[3] + (px[1] - box[1])


@pytest.mark.parametrize("name,a,b", PAIRS, ids=[p[0] for p in PAIRS])
def test_meet(L, name, a, b):
    for x, y in ((a, b), (b, a)):
        got = np.zeros(4, dtype=np.int32)
        L.bx_meet(_b(x), _b(y), got)
        r0, c0 = max(x[0], y[0]), max(x[1], y[1])
        r1, c1 = min(x[0] + x[2], y[0] + y[2]), min(x[1] + x[3], y[1] + y[3])
        if r1 <= r0 or c1 <= c0:
            assert got[2] == 0 or got[3] == 0, (name, got.tolist())
            assert got[2] >= 0 and got[3] >= 0
        else:
            assert got.tolist() == [r0, c0, r1 - r0, c1 - c0], name
    empty = "touching" in name or "disjoint" in name or "empty" in name or name == "opposite extremes"
    assert empty == (min(a[0] + a[2], b[0] + b[2]) <= max(a[0], b[0]) or min(a[1] + a[3], b[1] + b[3]) <= max(a[1], b[1])), name


def _bbox_ok(bb):
    """The rule the layer entries have always refused by."""
    return bb[2] >= 0 and bb[3] >= 0 and bb[2] < (1 << 30) and bb[3] < (1 << 30) and abs(bb[0]) < (1 << 30) and abs(bb[1]) < (1 << 30)


def test_box_of_admits_what_the_entries_always_admitted(L):
    out = np.full(4, -77, dtype=np.int32)
    assert L.bx_of(np.zeros(4, dtype=np.int64), 1, out) == 0 and (out == -77).all()   # a null pointer
    for bad in ((0, 0, -1, 5), (0, 0, 5, -1), (0, 0, 1 << 30, 5), (0, 0, 5, 1 << 30), (1 << 30, 0, 5, 5), (-(1 << 30), 0, 5, 5),
                (0, 1 << 30, 5, 5), (0, -(1 << 30), 5, 5)):
        assert L.bx_of(np.array(bad, dtype=np.int64), 0, out) == 0 and (out == -77).all(), bad
    for good in ((LIM, -LIM, LIM, LIM), (-LIM, LIM, 0, 0), (0, 0, 0, LIM), (-7, 11, 300, 517)):
        assert L.bx_of(np.array(good, dtype=np.int64), 0, out) == 1 and out.tolist() == list(good), good
    # every combination of values on both sides of each limit, and far beyond an int
    edge = [-(1 << 40), -(1 << 31) - 1, -(1 << 30) - 1, -(1 << 30), -LIM, -1, 0, 1, LIM, 1 << 30, (1 << 30) + 1, 1 << 31, 1 << 32, 1 << 40]
    n_ok = 0
    for bb in itertools.product(edge, repeat=4):
        out[:] = -77
        got = L.bx_of(np.array(bb, dtype=np.int64), 0, out)
        assert bool(got) == _bbox_ok(bb), bb
        assert out.tolist() == (list(bb) if got else [-77] * 4)
        n_ok += got
    assert n_ok == 5 * 5 * 3 * 3
