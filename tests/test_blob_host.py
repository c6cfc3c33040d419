"""The layout / blob builder of the pass entries (csrc/svgr_blob.h) on the CPU, through tests/blob_harness.cpp: where the
sections of a block lie, what a HostBlob holds, and that the twelve arrays of the TrueType outline pass keep the offsets the
entry computed by hand before the builder existed."""
import ctypes as C

import numpy as np
import pytest

from tests.util import host_build

DTYPES = {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.float64}


@pytest.fixture(scope="module")
def lib():
    h = host_build("blob_harness")
    for name in ("bh_pad64", "bh_layout", "bh_blob"):
        getattr(h, name).restype = C.c_longlong
    h.bh_pad64.argtypes = [C.c_longlong]
    return h


def pad64(b):
    return (b + 63) // 64 * 64


def layout(lib, arrays):
    """arrays: [(element size, count)] -> (offsets, total) of a Layout."""
    k = len(arrays)
    elem, count = (C.c_int * k)(*[a[0] for a in arrays]), (C.c_longlong * k)(*[a[1] for a in arrays])
    off = (C.c_longlong * k)()
    total = lib.bh_layout(k, elem, count, off)
    return list(off), total


def blob(lib, arrays):
    """arrays: [(element size, numpy array or None, count, reserve?)] -> (offsets, total, the blob's bytes): section by section
    and through HostBlob.build, which must agree -- and build's one allocation is exactly the total."""
    grown, built = _blob(lib, arrays, 0), _blob(lib, arrays, 1)
    assert grown[:2] == built[:2] and grown[2].tobytes() == built[2].tobytes()
    assert built[3] == built[1], "build() allocates once, exactly the sections' total"
    return grown[:3]


def _blob(lib, arrays, built):
    k = len(arrays)
    src = (C.c_void_p * k)(*[None if a[1] is None else a[1].ctypes.data for a in arrays])
    elem, count = (C.c_int * k)(*[a[0] for a in arrays]), (C.c_longlong * k)(*[a[2] for a in arrays])
    mode, off = (C.c_int * k)(*[int(a[3]) for a in arrays]), (C.c_longlong * k)()
    out = np.full(1 << 16, 0xEE, dtype=np.uint8)
    cap = C.c_longlong(-1)
    total = lib.bh_blob(k, src, elem, count, mode, built, off, out.ctypes.data_as(C.c_void_p), out.size, C.byref(cap))
    assert 0 <= total <= out.size, total
    assert (out[total:] == 0xEE).all()
    return list(off), total, out[:total], cap.value


def values(rng, elem, n):
    if elem == 48:
        return rng.standard_normal(6 * n)
    if elem == 8:
        return rng.standard_normal(n)
    info = np.iinfo(DTYPES[elem])
    return rng.integers(info.min, info.max, n, dtype=DTYPES[elem], endpoint=True)


def test_pad64(lib):
    assert [lib.bh_pad64(b) for b in (0, 1, 63, 64, 65, 128, (1 << 40) + 1)] == [0, 64, 64, 64, 128, 128, (1 << 40) + 64]


def test_sections_are_aligned_in_order_and_add_up(lib):
    arrays = [(8, 3), (1, 65), (4, 0), (2, 33), (48, 5), (4, 16), (1, 64), (8, 0), (4, 17)]
    off, total = layout(lib, arrays)
    at = 0
    for (elem, n), o in zip(arrays, off):
        assert o == at and o % 64 == 0, (elem, n, o, at)
        at += pad64(elem * n)
    assert total == at == sum(pad64(e * n) for e, n in arrays)
    assert layout(lib, []) == ([], 0)
    big = (1 << 33) + 5   # all arithmetic is size_t: nothing wraps at 32 bits
    assert layout(lib, [(8, big), (4, 1)]) == ([0, pad64(8 * big)], pad64(8 * big) + 64)
    assert lib.bh_layout(1, (C.c_int * 1)(3), (C.c_longlong * 1)(1), (C.c_longlong * 1)()) == -1   # (the harness's own refusal)


def test_blob_holds_the_arrays_and_zero_padding(lib):
    rng = np.random.default_rng(1)
    arrays = [(e, values(rng, e, n), n, r) for e, n, r in [(8, 3, False), (1, 65, False), (4, 7, True), (2, 33, False), (48, 5, False),
                                                           (4, 16, True), (1, 1, True), (8, 9, True)]]
    off, total, data = blob(lib, arrays)
    want_off, want_total = layout(lib, [(a[0], a[2]) for a in arrays])
    assert off == want_off and total == want_total
    covered = np.zeros(total, dtype=bool)
    for (elem, src, n, _r), o in zip(arrays, off):
        assert data[o:o + elem * n].tobytes() == src.tobytes(), (elem, n)   # put and reserve alike: the n elements, in place
        covered[o:o + elem * n] = True
    assert not data[~covered].any(), "the padding between the sections is zero"


def test_no_elements_from_a_null_pointer(lib):
    rng = np.random.default_rng(2)
    a, b = values(rng, 4, 5), values(rng, 8, 2)
    assert blob(lib, [])[:2] == ([], 0)
    off, total, data = blob(lib, [(8, None, 0, False), (4, a, 5, False), (2, None, 0, False), (1, None, 0, True), (8, b, 2, False), (4, None, 0, False)])
    assert off == [0, 0, 64, 64, 64, 128] and total == 128, "an empty section takes no space beyond alignment"
    assert data[0:20].tobytes() == a.tobytes() and data[64:80].tobytes() == b.tobytes()
    assert blob(lib, [(8, None, 0, False), (1, None, 0, True)])[:2] == ([0, 0], 0)


def test_truetype_outline_upload_keeps_its_offsets(lib):
    """svgr_glyf_outline's upload, as the entry laid it out by hand before the builder: twelve arrays, each padded to 64 bytes."""
    npt, nc, ng, np_ = 65, 3, 2, 5
    i_on = pad64(npt * 4)                       # behind pt_xy: 2 int16 per point
    i_slot = i_on + pad64(npt)                  # pt_on: a byte per point
    i_coff = i_slot + pad64(npt * 4)            # pt_slot
    i_goff = i_coff + pad64((nc + 1) * 4)       # contour_off
    i_pglyph = i_goff + pad64((ng + 1) * 4)     # glyph_contour_off
    i_plane = i_pglyph + pad64(np_ * 4)         # part_glyph
    i_pseg = i_plane + pad64((np_ + 1) * 4)     # part_lane_off
    i_m = i_pseg + pad64((np_ + 1) * 4)         # part_seg_off
    i_pen = i_m + pad64(np_ * 48)               # part_m: 6 doubles per part
    i_sx = i_pen + pad64(np_ * 8)
    i_sy = i_sx + pad64(np_ * 8)
    i_gvar = i_sy + pad64(np_ * 8)              # (where the tuples of a variable font begin)
    old = [0, i_on, i_slot, i_coff, i_goff, i_pglyph, i_plane, i_pseg, i_m, i_pen, i_sx, i_sy]
    assert old == [0, 320, 448, 768, 832, 896, 960, 1024, 1088, 1344, 1408, 1472] and i_gvar == 1536
    shape = [(2, npt * 2), (1, npt), (4, npt), (4, nc + 1), (4, ng + 1), (4, np_), (4, np_ + 1), (4, np_ + 1), (8, np_ * 6), (8, np_),
             (8, np_), (8, np_)]
    rng = np.random.default_rng(3)
    arrays = [(e, values(rng, e, n), n, False) for e, n in shape]
    off, total, data = blob(lib, arrays)
    assert off == old and total == i_gvar
    assert layout(lib, shape) == (old, i_gvar)
    assert layout(lib, shape[:8] + [(48, np_)] + shape[9:]) == (old, i_gvar)   # (the matrices as one 48-byte element each)
    for (elem, src, n, _r), o in zip(arrays, off):
        assert data[o:o + elem * n].tobytes() == src.tobytes()
    # the tuples behind it, as GvarBlob laid them out: n_glyphs + 1 offsets, nt scalars, nt + 1 offsets, ne indices, ne int16 pairs
    nt, ne = 3, 7
    i_scalar = i_gvar + pad64((ng + 1) * 4)
    i_poff = i_scalar + pad64(nt * 8)
    i_index = i_poff + pad64((nt + 1) * 4)
    i_dxy = i_index + pad64(ne * 4)
    i_end = i_dxy + pad64(ne * 4)
    got, end = layout(lib, shape + [(4, ng + 1), (8, nt), (4, nt + 1), (4, ne), (2, ne * 2)])
    assert got[12:] == [i_gvar, i_scalar, i_poff, i_index, i_dxy] and end == i_end
