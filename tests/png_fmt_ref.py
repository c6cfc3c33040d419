"""The PNG sample formats restated in plain numpy (the second part of csrc/svgr_png.h): the quantiser, the luma, a
pixel's sample bytes, the byte-wise scanline filters, and the ctypes front of the host harness (tests/png_fmt_harness.cpp)."""
import ctypes as C

import numpy as np

from tests.util import host_build

FILTERS = ("none", "sub", "up", "average", "paeth", "adaptive")
GREY, RGB, GREY_ALPHA, RGBA = 0, 2, 4, 6                        # PNG colour types
CHANNELS = {GREY: 1, RGB: 3, GREY_ALPHA: 2, RGBA: 4}
RGBA_F64, MASK_F64, RGBA_U8 = 0, 1, 2                           # source kinds
BPPS = (1, 2, 3, 4, 6, 8)
# every source kind x colour x depth the interface allows: a mask is grey only
FORMATS = [(kind, color, depth) for kind in (RGBA_F64, MASK_F64, RGBA_U8) for color in CHANNELS for depth in (8, 16)
           if kind != MASK_F64 or color == GREY]


def quant(v, M):
    """rint(v * M) saturated to [0, M], NaN giving 0: uint32."""
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint(np.asarray(v, dtype=np.float64) * float(M))
        return np.where(r > 0, np.minimum(r, float(M)), 0.0).astype(np.uint32)


def luma(r, g, b):
    """(0.2126 * r + 0.7152 * g) + 0.0722 * b: numpy rounds every product and sum on its own."""
    r, g, b = (np.asarray(x, dtype=np.float64) for x in (r, g, b))
    with np.errstate(invalid="ignore", over="ignore"):
        return (0.2126 * r + 0.7152 * g) + 0.0722 * b


def sample_values(px, color, depth):
    """(..., channels) uint16 or uint8 sample values -- what ``png.read_samples`` returns -- of straight-alpha RGBA doubles
    (..., 4)."""
    px = np.asarray(px, dtype=np.float64)
    M = 65535 if depth == 16 else 255
    first = [luma(px[..., 0], px[..., 1], px[..., 2])] if color in (GREY, GREY_ALPHA) else [px[..., 0], px[..., 1], px[..., 2]]
    chans = first + ([px[..., 3]] if color in (GREY_ALPHA, RGBA) else [])
    return np.stack([quant(c, M) for c in chans], axis=-1).astype(np.uint16 if depth == 16 else np.uint8)


def mask_values(m, depth):
    """(..., 1) sample values of a one-channel mask."""
    return quant(m, 65535 if depth == 16 else 255)[..., None].astype(np.uint16 if depth == 16 else np.uint8)


def file_bytes(values):
    """Sample values (..., channels) -> their bytes in the file (..., bpp): 16-bit samples most significant byte first."""
    values = np.asarray(values)
    if values.dtype == np.uint16:
        return np.ascontiguousarray(values.astype(">u2")).view(np.uint8).reshape(*values.shape[:-1], values.shape[-1] * 2)
    return values.astype(np.uint8)


def samples_ref(src, kind, color, depth):
    """(n, bpp) uint8: svgr_png_samples of `src` -- (n, 4) doubles, (n,) doubles or (n, 4) bytes."""
    if kind == MASK_F64:
        assert color == GREY
        return file_bytes(mask_values(np.asarray(src, dtype=np.float64).reshape(-1), depth))
    px = np.asarray(src).reshape(-1, 4)
    px = px.astype(np.float64) / 255.0 if kind == RGBA_U8 else px.astype(np.float64)
    return file_bytes(sample_values(px, color, depth))


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filtered_rows(img, bpp):
    """(5, rows, row_bytes) uint8: every row of a (rows, row_bytes) uint8 image under each of the five filter types."""
    x = np.asarray(img).astype(np.int64)
    a = np.zeros_like(x)
    a[:, bpp:] = x[:, :-bpp]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, bpp:] = x[:-1, :-bpp]
    pred = (np.zeros_like(x), a, b, (a + b) >> 1, _paeth(a, b, c))
    return np.stack([((x - p) & 255).astype(np.uint8) for p in pred])


def filter_ref(img, bpp, filter):
    """The filtered stream (rows, 1 + row_bytes) uint8 of a (rows, row_bytes) uint8 image at `bpp` bytes a pixel."""
    f = filtered_rows(img, bpp)
    rows = f.shape[1]
    cost = np.minimum(f.astype(np.int64), 256 - f.astype(np.int64)).sum(axis=2).T
    kind = np.argmin(cost, axis=1) if filter == "adaptive" else np.full(rows, FILTERS.index(filter))   # (argmin: the first)
    out = np.empty((rows, 1 + f.shape[2]), dtype=np.uint8)
    out[:, 0] = kind
    out[:, 1:] = f[kind, np.arange(rows)]
    return out


def filter_image(rng, rows, row_bytes):
    """A (rows, row_bytes) uint8 image whose adaptive rows pick different types: noise, rows that repeat the one above, rows of
    small values."""
    img = rng.integers(0, 256, (rows, row_bytes), dtype=np.uint8)
    img[1::3] = img[0::3][:len(img[1::3])]
    img[2::3] = rng.integers(0, 3, (len(img[2::3]), row_bytes))
    return img


# ------------------------------------------------------------------------------------------------------------------------------
# the host harness
# ------------------------------------------------------------------------------------------------------------------------------
def harness():
    lib = host_build("png_fmt_harness")
    lib.h_quant.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
    lib.h_luma.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    lib.h_bpp.argtypes = [C.c_int, C.c_int]
    lib.h_samples.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p]
    lib.h_filter_bytes.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_void_p]
    lib.h_quant.restype = lib.h_luma.restype = None
    return lib


def harness_quant(lib, v, M):
    v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
    out = np.empty(v.size, dtype=np.uint32)
    lib.h_quant(v.ctypes.data, v.size, M, out.ctypes.data)
    return out


def harness_luma(lib, rgb):
    rgb = np.ascontiguousarray(rgb, dtype=np.float64).reshape(-1, 3)
    out = np.empty(len(rgb), dtype=np.float64)
    lib.h_luma(rgb.ctypes.data, len(rgb), out.ctypes.data)
    return out


def source_array(src, kind):
    """`src` as the contiguous array the entry reads: (n, 4) float64, (n,) float64 or (n, 4) uint8."""
    if kind == RGBA_U8:
        return np.ascontiguousarray(src, dtype=np.uint8).reshape(-1, 4)
    return np.ascontiguousarray(src, dtype=np.float64).reshape((-1,) if kind == MASK_F64 else (-1, 4))


def harness_samples(lib, src, kind, color, depth):
    src = source_array(src, kind)
    out = np.empty((len(src), lib.h_bpp(color, depth)), dtype=np.uint8)
    assert lib.h_samples(src.ctypes.data, kind, len(src), color, depth, out.ctypes.data) == 0
    return out


def harness_filter(lib, img, bpp, filter):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    rows, row_bytes = img.shape
    out = np.empty((rows, 1 + row_bytes), dtype=np.uint8)
    assert lib.h_filter_bytes(img.ctypes.data, rows, row_bytes, bpp, FILTERS.index(filter), out.ctypes.data) == 0
    return out


def awkward_values(rng, n):
    """(n, 4) doubles in and around [0, 1] with what a quantiser has to survive: ties, out-of-range values, NaN and infinities."""
    v = rng.random((n, 4))
    k = rng.integers(0, 65535, (n, 4))
    v = np.where(rng.random((n, 4)) < 0.3, (k + 0.5) / 65535.0, v)          # ties at 16 bits
    v = np.where(rng.random((n, 4)) < 0.2, ((k % 255) + 0.5) / 255.0, v)    # ties at 8 bits
    flat = v.reshape(-1)
    special = [np.nan, np.inf, -np.inf, -0.25, 1.5, 0.0, 1.0, -0.0, 1e300, -1e300]
    flat[:min(len(special), flat.size)] = special[:flat.size]
    return flat.reshape(n, 4)
