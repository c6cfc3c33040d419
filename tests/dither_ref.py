"""Dithering restated in numpy and plain Python integers, and the ctypes side of tests/dither_harness.cpp, the
host build of csrc/svgr_dither.h.

  X          (r a, g a, b a, 255 a) of the canonical pixel (a == 0 -> 0); a target is clamped to 0 .. 65025 per coordinate; the
             pixel takes the entry with the smallest D to its target, a tie to the lowest index
  Bayer      M -> [[4 M, 4 M + 2], [4 M + 3, 4 M + 1]] from [[0]], three times: 8 x 8, indexed (row & 7, col & 7)
  amplitude  d_i = min over j != i of D(entry i, entry j); amp = min(65025, isqrt(sum d_i // (3 n))); 0 for n = 1
  ordered    h = amp a // 255; off = (((2 B + 1) h) >> 7) - (h >> 1); the three colour coordinates move by off, the fourth stays
  diffusion  rows top to bottom, left to right; acc(r, c) = 7 e(r, c-1) + 3 e(r-1, c+1) + 5 e(r-1, c) + e(r-1, c-1), 0 from outside;
             t = clamp(x + floor((acc + 8) / 16)); e = t - X(entry); a == 0: the entry nearest to X = 0, e = 0"""
import ctypes as C
import math

import numpy as np

from tests import quant_ref as Q
from tests.util import host_build

X_MAX = 65025


def harness():
    lib = host_build("dither_harness")
    u32p, u8p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
    lib.h_row_bytes.restype, lib.h_row_bytes.argtypes = C.c_int64, [C.c_int64, C.c_int]
    lib.h_dither.restype, lib.h_dither.argtypes = None, [u32p, C.c_int64, C.c_int64, u32p, C.c_int, C.c_int, C.c_uint32, u8p, u8p]
    return lib


def harness_dither(lib, img, palette, mode, amp=0):
    """(stream (rows, row_bytes), indices (rows, cols)) of the host build; mode is "ordered" or "diffusion"."""
    rows, cols = img.shape[:2]
    src, pal = np.ascontiguousarray(Q.u32(img)), np.ascontiguousarray(Q.u32(palette))
    rb = lib.h_row_bytes(cols, lib.h_depth(len(pal)))
    stream, idx = np.full((rows, rb), 0xAA, dtype=np.uint8), np.full((rows, cols), 0xAA, dtype=np.uint8)
    number = lib.h_mode_ordered() if mode == "ordered" else lib.h_mode_diffusion()
    lib.h_dither(Q._p(src, C.c_uint32), rows, cols, Q._p(pal, C.c_uint32), len(pal), number, int(amp), Q._p(stream, C.c_uint8), Q._p(idx, C.c_uint8))
    return stream, idx


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
def bayer():
    m = np.zeros((1, 1), dtype=np.int64)
    for _ in range(3):
        m = np.block([[4 * m, 4 * m + 2], [4 * m + 3, 4 * m + 1]])
    return m


def coords(px):
    """(..., 4) uint8 -> (..., 4) int64 X of the canonical pixels."""
    p = Q.canon(px).astype(np.int64)
    a = p[..., 3:4]
    return np.concatenate([p[..., :3] * a, 255 * a], axis=-1)


def amplitude_ref(palette):
    pal = [Q.x_of(p) for p in np.asarray(palette).reshape(-1, 4)]
    n = len(pal)
    if n < 2:
        return 0
    total = 0
    for i in range(n):
        total += min(sum((u - v) ** 2 for u, v in zip(pal[i], pal[j])) for j in range(n) if j != i)
    return min(X_MAX, math.isqrt(total // (3 * n)))


def nearest_of(P, t):
    """Index of the row of P ((n, 4) int64) nearest to each row of t ((m, 4) int64): the first of the smallest."""
    return np.argmin(((t[:, None, :] - P[None, :, :]) ** 2).sum(axis=2), axis=1)


def ordered_ref(img, palette, amp):
    img = np.asarray(img, dtype=np.uint8)
    rows, cols = img.shape[:2]
    X, P = coords(img), coords(np.asarray(palette, dtype=np.uint8).reshape(-1, 4))
    a = Q.canon(img)[..., 3].astype(np.int64)
    B = bayer()[np.arange(rows)[:, None] & 7, np.arange(cols)[None, :] & 7]
    h = amp * a // 255
    off = (((2 * B + 1) * h) >> 7) - (h >> 1)
    t = X.copy()
    t[..., :3] = np.clip(X[..., :3] + off[..., None], 0, X_MAX)
    return nearest_of(P, t.reshape(-1, 4)).reshape(rows, cols).astype(np.uint8)


def diffusion_ref(img, palette):
    img = np.asarray(img, dtype=np.uint8)
    rows, cols = img.shape[:2]
    X, P = coords(img), coords(np.asarray(palette, dtype=np.uint8).reshape(-1, 4))
    alpha = img[..., 3]
    clear = int(nearest_of(P, np.zeros((1, 4), dtype=np.int64))[0])
    e = np.zeros((rows + 1, cols + 2, 4), dtype=np.int64)   # e[r + 1, c + 1]: a border of zeros stands for the outside
    out = np.zeros((rows, cols), dtype=np.uint8)
    for r in range(rows):
        for c in range(cols):
            if alpha[r, c] == 0:
                out[r, c] = clear
                continue
            acc = 7 * e[r + 1, c] + 3 * e[r, c + 2] + 5 * e[r, c + 1] + e[r, c]
            t = np.clip(X[r, c] + (acc + 8) // 16, 0, X_MAX)   # (// floors)
            k = int(nearest_of(P, t[None, :])[0])
            out[r, c] = k
            e[r + 1, c + 1] = t - P[k]
    return out


def dither_ref(img, palette, mode, amp=None):
    if mode == "ordered":
        return ordered_ref(img, palette, amplitude_ref(palette) if amp is None else amp)
    return diffusion_ref(img, palette)


def block_mean_error(indices, palette, source, block=8):
    """The mean absolute difference between the block means of palette[indices] and of source (opaque grey: the red channel)."""
    got = np.asarray(palette)[indices][..., 0].astype(np.float64)
    want = np.asarray(source)[..., 0].astype(np.float64)
    rows, cols = got.shape

    def means(v):
        return v.reshape(rows // block, block, cols // block, block).mean(axis=(1, 3))

    return float(np.abs(means(got) - means(want)).mean())
