"""Tensor output restated in numpy (csrc/svgr_tensor.h), and the ctypes face of tests/tensor_harness.cpp.

The restatement is independent of the header where it can be: the element conversions are numpy's own ``astype`` chain (float64 ->
float32 -> float16), bfloat16 is the add-and-shift form of round-to-nearest-even, the one fma of LUMA is exact rational
arithmetic rounded once."""
import ctypes as C
from fractions import Fraction

import numpy as np

from svgrasterize_amd import _abi
from tests.util import host_build

F32, F16, BF16, U8 = _abi.TENSOR_F32, _abi.TENSOR_F16, _abi.TENSOR_BF16, _abi.TENSOR_U8
RGBA, RGB, ALPHA, LUMA = _abi.TENSOR_RGBA, _abi.TENSOR_RGB, _abi.TENSOR_ALPHA, _abi.TENSOR_LUMA
SRC_F64, SRC_F32, SRC_MASK = _abi.TENSOR_SRC_RGBA_F64, _abi.TENSOR_SRC_RGBA_F32, _abi.TENSOR_SRC_MASK_F64
DTYPES = {"f32": F32, "f16": F16, "bf16": BF16, "u8": U8}
CHANNELS = {"rgba": RGBA, "rgb": RGB, "alpha": ALPHA, "luma": LUMA}
N_CH = {RGBA: 4, RGB: 3, ALPHA: 1, LUMA: 1}
STORE = {F32: np.uint32, F16: np.uint16, BF16: np.uint16, U8: np.uint8}   # an element as bits
QNAN = {F32: 0x7FC00000, F16: 0x7E00, BF16: 0x7FC0}


def harness():
    lib = host_build("tensor_harness")
    lib.h_encode.restype, lib.h_encode.argtypes = C.c_uint32, [C.c_int, C.c_double]
    lib.h_decode.restype, lib.h_decode.argtypes = C.c_double, [C.c_int, C.c_uint32]
    for name in ("h_f16_bits", "h_bf16_bits", "h_f16_widen"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = C.c_uint32, [C.c_uint32]
    lib.h_encode_many.restype, lib.h_encode_many.argtypes = None, [C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
    lib.h_pack.restype, lib.h_pack.argtypes = None, [C.POINTER(_abi.TensorDesc), C.c_void_p, C.c_void_p, C.c_void_p]
    lib.h_unpack.restype, lib.h_unpack.argtypes = None, [C.POINTER(_abi.TensorDesc), C.c_void_p, C.c_void_p]
    return lib


def desc(rows, cols, dtype=F32, channels=RGBA, layout="chw", source=SRC_F64, bg=None, scale=None, bias=None, stride_c=None,
         stride_h=None, offset=0, **override):
    """An svgr_tensor_desc: a dense plane of the layout unless strides are given; `override` sets any field as it is."""
    n = N_CH.get(channels, 4)
    d = _abi.TensorDesc()
    d.source, d.dtype, d.channels, d.has_bg = source, dtype, channels, int(bg is not None)
    d.bg = (C.c_double * 3)(*(bg if bg is not None else (0.0, 0.0, 0.0)))
    d.scale = (C.c_double * 4)(*(list(scale) + [1.0] * 4)[:4] if scale is not None else [1.0] * 4)
    d.bias = (C.c_double * 4)(*(list(bias) + [0.0] * 4)[:4] if bias is not None else [0.0] * 4)
    d.rows, d.cols, d.offset = rows, cols, offset
    if layout == "chw":
        d.stride_w = 1
        d.stride_h = cols if stride_h is None else stride_h
        d.stride_c = rows * d.stride_h if stride_c is None else stride_c
    else:
        d.stride_c, d.stride_w = 1, n
        d.stride_h = cols * n if stride_h is None else stride_h
    for k, v in override.items():
        setattr(d, k, v)
    return d


def n_elements(d):
    """One past the largest element index the description reaches."""
    n = N_CH[d.channels]
    return d.offset + (n - 1) * d.stride_c + (d.rows - 1) * d.stride_h + (d.cols - 1) * d.stride_w + 1


def harness_pack(lib, d, src, bbox, dst):
    """`dst` (a uint8 array, the whole buffer) with the plane of `d` written into it by the host build."""
    src = np.ascontiguousarray(src)
    dst = dst.copy()
    assert n_elements(d) * STORE[d.dtype]().itemsize <= dst.nbytes
    lib.h_pack(C.byref(d), src.ctypes.data, (C.c_int64 * 4)(*bbox), dst.ctypes.data)
    return dst


def harness_unpack(lib, d, buf):
    out = np.empty((d.rows, d.cols, 4 if d.channels in (RGBA, RGB) else 1), dtype=np.float64)
    lib.h_unpack(C.byref(d), np.ascontiguousarray(buf).ctypes.data, out.ctypes.data)
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        return a * b + c   # (NaN and infinity: nothing to round)
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def luma_ref(r, g, b):
    """fma(b, 0.072, fma(g, 0.7154, r * 0.2125)) per pixel (svgr_layer_luminance's sum)."""
    r, g, b = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (r, g, b))
    with np.errstate(all="ignore"):
        out = [_fma(b[i], 0.072, _fma(g[i], 0.7154, r[i] * 0.2125)) for i in range(r.size)]
    return np.array(out, dtype=np.float64)


def bf16_bits_ref(f32):
    x = np.asarray(f32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((x + 0x7FFF + ((x >> 16) & 1)) >> 16).astype(np.uint16)


def encode_ref(dtype, y):
    """float64 values -> elements as bits (STORE[dtype])."""
    y = np.asarray(y, dtype=np.float64)
    nan = np.isnan(y)
    with np.errstate(all="ignore"):
        if dtype == U8:
            return np.where(nan, 0.0, np.clip(np.rint(y * 255.0), 0.0, 255.0)).astype(np.uint8)
        f = np.where(nan, 0.0, y).astype(np.float32)
        if dtype == F32:
            bits = f.view(np.uint32)
        elif dtype == F16:
            bits = f.astype(np.float16).view(np.uint16)
        else:
            bits = bf16_bits_ref(f)
    return np.where(nan, QNAN[dtype], bits).astype(STORE[dtype])


def decode_ref(dtype, bits):
    bits = np.asarray(bits)
    with np.errstate(invalid="ignore"):   # (a signalling NaN widened)
        return _decode_ref(dtype, bits)


def _decode_ref(dtype, bits):
    if dtype == U8:
        return bits.astype(np.float64) / 255.0
    if dtype == F32:
        return bits.astype(np.uint32).view(np.float32).astype(np.float64)
    if dtype == F16:
        return bits.astype(np.uint16).view(np.float16).astype(np.float64)
    return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def plane_ref(src, bbox, rows, cols):
    """(rows, cols, 4) float64: the source (an (h, w, 4) RGBA array of float64 or float32, or an (h, w) / (h, w, 1) mask) over
    `bbox` on the plane, zero outside it."""
    src = np.asarray(src)
    if src.ndim == 2 or src.shape[2] == 1:
        src = np.broadcast_to(src.reshape(src.shape[0], src.shape[1], 1), src.shape[:2] + (4,))
    plane = np.zeros((rows, cols, 4), dtype=np.float64)
    r0, c0, h, w = bbox
    ra, rb, ca, cb = max(r0, 0), min(r0 + h, rows), max(c0, 0), min(c0 + w, cols)
    if ra < rb and ca < cb:
        plane[ra:rb, ca:cb] = src[ra - r0:rb - r0, ca - c0:cb - c0].astype(np.float64)
    return plane


def values_ref(plane, channels=RGBA, bg=None, scale=None, bias=None):
    """(rows, cols, n) float64: background, channel selection, affine."""
    with np.errstate(all="ignore"):
        r, g, b, a = (plane[..., k].copy() for k in range(4))
        if bg is not None:
            t = 1.0 - a
            r, g, b, a = r + bg[0] * t, g + bg[1] * t, b + bg[2] * t, np.ones_like(a)
        if channels == RGBA:
            out = np.stack([r, g, b, a], axis=-1)
        elif channels == RGB:
            out = np.stack([r, g, b], axis=-1)
        elif channels == ALPHA:
            out = a[..., None]
        else:
            out = luma_ref(r, g, b).reshape(a.shape)[..., None]
        n = out.shape[-1]
        scale = np.ones(n) if scale is None else np.asarray(scale, dtype=np.float64)[:n]
        bias = np.zeros(n) if bias is None else np.asarray(bias, dtype=np.float64)[:n]
        if (scale != 1.0).any() or (bias != 0.0).any():
            out = out * scale + bias
    return out


def pack_ref(src, bbox, rows, cols, dtype=F32, channels=RGBA, bg=None, scale=None, bias=None):
    """(rows, cols, n) elements as bits."""
    return encode_ref(dtype, values_ref(plane_ref(src, bbox, rows, cols), channels, bg, scale, bias))


def view_of(buf, d):
    """The (rows, cols, n) strided view of the plane of `d` in `buf` (uint8, the whole buffer), as bits."""
    store = np.dtype(STORE[d.dtype])
    elems = buf.view(store)
    n = N_CH[d.channels]
    return np.lib.stride_tricks.as_strided(elems[d.offset:], shape=(d.rows, d.cols, n),
                                           strides=(d.stride_h * store.itemsize, d.stride_w * store.itemsize, d.stride_c * store.itemsize))


def random_layer(rng, h, w, kind=SRC_F64):
    """Pixels with everything the conversions can meet: exact 0 and 1, negatives, values above 1, NaN, tiny and huge ones."""
    shape = (h, w) if kind == SRC_MASK else (h, w, 4)
    v = rng.uniform(-0.25, 1.25, shape)
    pick = rng.integers(0, 16, shape)
    v[pick == 0] = 0.0
    v[pick == 1] = 1.0
    v[pick == 2] = np.nan
    v[pick == 3] = rng.uniform(-3, 3, int((pick == 3).sum()))
    v[pick == 4] = 1e-6 * rng.uniform(0, 1, int((pick == 4).sum()))   # (the halves' subnormal range)
    v[pick == 5] = 7e4 * rng.uniform(0, 1, int((pick == 5).sum()))    # (around float16's largest finite value)
    v[pick == 6] = np.round(rng.uniform(0, 255, int((pick == 6).sum()))) / 255.0
    v[pick == 7] = (np.round(rng.uniform(0, 254, int((pick == 7).sum()))) + 0.5) / 255.0
    return v.astype(np.float32) if kind == SRC_F32 else v
