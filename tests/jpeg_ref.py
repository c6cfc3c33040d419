"""float64 numpy restatement of the JPEG pixel stage (dequantise, exact inverse DCT, level shift and clamp, the centred triangle
filter, the JFIF matrix, rounded once at the end), the fixture list of tests/golden/jpeg, and the loader for the host build of
csrc/svgr_core.h's integer arithmetic (tests/jpeg_harness.cpp).  Test infrastructure only."""
import ctypes as C
import glob
import os

import numpy as np

from svgrasterize_amd import _abi, jpeg
from tests.util import ROOT, host_build

GOLDEN = os.path.join(ROOT, "tests", "golden", "jpeg")
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*.jpg")))


def fixture(name):
    """(the file's bytes, the pixels libjpeg-turbo decoded from it: (h, w) grey or (h, w, 3))"""
    with open(os.path.join(GOLDEN, name + ".jpg"), "rb") as f:
        data = f.read()
    return data, np.load(os.path.join(GOLDEN, name + ".npy"))


def rgba_of(pixels):
    """recorded pixels -> (h, w, 4) as read_jpeg returns them"""
    rgb = np.repeat(pixels[..., None], 3, axis=2) if pixels.ndim == 2 else pixels
    return np.concatenate([rgb, np.full(rgb.shape[:2] + (1,), 255, dtype=np.uint8)], axis=2)


# -- the restatement ---------------------------------------------------------------------------------------------------------
_K = np.arange(8)
_T = 0.5 * np.where(_K == 0, 1.0 / np.sqrt(2.0), 1.0)[None, :] * np.cos((2 * _K[:, None] + 1) * _K[None, :] * np.pi / 16)   # [x][u]


def sample_planes(frame, coef, quant):
    """Each component's samples, exact: float64 in 0 .. 255, (8 * rows of blocks, 8 * blocks per row)."""
    planes = []
    layout, _total = jpeg.coefficient_layout(frame)
    for i, (base, bh, bw) in enumerate(layout):
        f = coef[base * 64:(base + bh * bw) * 64].reshape(bh, bw, 8, 8).astype(np.float64) * quant[i].reshape(8, 8).astype(np.float64)
        s = np.einsum("yv,abvu,xu->abyx", _T, f, _T)
        planes.append(np.clip(s + 128.0, 0.0, 255.0).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8))
    return planes


def _upsample_axis(a, factor, n_out, axis):
    """The centred triangle filter along one axis: weights 3/4, 1/4, the edge sample repeated; `a` holds the component's own
    samples only."""
    a = np.moveaxis(a, axis, 0)
    if factor == 1:
        out = a[:n_out]
    else:
        prev = np.concatenate([a[:1], a[:-1]])
        nxt = np.concatenate([a[1:], a[-1:]])
        out = np.empty((2 * a.shape[0],) + a.shape[1:])
        out[0::2] = 0.75 * a + 0.25 * prev
        out[1::2] = 0.75 * a + 0.25 * nxt
        out = out[:n_out]
    return np.moveaxis(out, 0, axis)


def pixels(frame, coef, quant):
    """(h, w, 4) uint8 from float64 arithmetic, rounded (half up) and clamped once, at the end."""
    n = frame.n_comp
    hmax, vmax = max(frame.h[:n]), max(frame.v[:n])
    full = []
    for i, plane in enumerate(sample_planes(frame, coef, quant)):
        hs, vs = hmax // frame.h[i], vmax // frame.v[i]
        own = plane[:-(-frame.height // vs), :-(-frame.width // hs)]
        full.append(_upsample_axis(_upsample_axis(own, vs, frame.height, 0), hs, frame.width, 1))
    if frame.colour == _abi.JPEG_GREY:
        rgb = [full[0]] * 3
    elif frame.colour == _abi.JPEG_RGB:
        rgb = full
    else:
        y, cb, cr = full[0], full[1] - 128.0, full[2] - 128.0
        rgb = [y + 1.402 * cr, y - 0.344136 * cb - 0.714136 * cr, y + 1.772 * cb]
    out = np.full((frame.height, frame.width, 4), 255, dtype=np.uint8)
    out[..., :3] = np.clip(np.floor(np.stack(rgb, axis=-1) + 0.5), 0, 255).astype(np.uint8)
    return out


# -- the host build of svgr_core.h's JPEG arithmetic -------------------------------------------------------------------------
def harness():
    L = host_build("jpeg_harness")
    L.jh_decode.restype = C.c_int
    L.jh_decode.argtypes = [C.POINTER(_abi.JpegFrame), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def harness_pixels(L, frame, coef, quant, want_samples=False):
    """The host build's (h, w, 4) uint8 for svgr_jpeg_decode's arguments (and the planes of samples, one flat array, if asked)."""
    coef = np.ascontiguousarray(coef, dtype=np.int16)
    quant = np.ascontiguousarray(quant, dtype=np.uint16)
    out = np.empty((frame.height, frame.width, 4), dtype=np.uint8)
    samples = np.empty(coef.size, dtype=np.uint8) if want_samples else None
    rc = L.jh_decode(C.byref(frame), coef.ctypes.data, quant.ctypes.data, None if samples is None else samples.ctypes.data, out.ctypes.data)
    if rc:
        raise ValueError("jh_decode: bad frame")
    return (out, samples) if want_samples else out


def host_read_jpeg(L, data):
    """read_jpeg with the pixel stage on the host harness: container and entropy decoding are the product's own"""
    return harness_pixels(L, *jpeg.decode_coefficients(data))
