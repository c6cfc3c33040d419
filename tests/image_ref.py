"""Test helpers for SVG <image>: a PNG encoder (forward scanline filters in numpy, zlib) for every colour type, bit depth
and Adam7, and a numpy restatement of the device image: the mip chain of svgr_image_upload and the per-pixel sampling of
svgr_image_fill (nearest, bilinear, trilinear)."""
import struct
import zlib

import numpy as np

ADAM7 = ((0, 0, 8, 8), (0, 4, 8, 8), (4, 0, 8, 4), (0, 2, 4, 4), (2, 0, 4, 2), (0, 1, 2, 2), (1, 0, 2, 1))
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


# ------------------------------------------------------------------------------------------------------------------------
# encoder
# ------------------------------------------------------------------------------------------------------------------------
def chunk(tag: bytes, body: bytes) -> bytes:
    return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(body, zlib.crc32(tag)) & 0xFFFFFFFF)


def pack_rows(samples: np.ndarray, depth: int) -> np.ndarray:
    """(h, w, ch) sample values -> (h, row_bytes) uint8 scanlines without filter bytes."""
    h, w, ch = samples.shape
    if depth == 16:
        return samples.astype(">u2").view(np.uint8).reshape(h, w * ch * 2)
    if depth == 8:
        return samples.astype(np.uint8).reshape(h, w * ch)
    bits = ((samples.reshape(h, w * ch, 1).astype(np.uint8) >> np.arange(depth - 1, -1, -1, dtype=np.uint8)) & 1)
    return np.packbits(bits.reshape(h, w * ch * depth), axis=1)


def paeth(a, b, c):
    a, b, c = (x.astype(np.int16) for x in (a, b, c))
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c)).astype(np.uint8)


def filter_rows(rows: np.ndarray, bpp: int, types) -> bytes:
    """Forward filters (PNG section 9) of raw scanlines, type `types[r]` on row r; returns the filtered stream."""
    h, n = rows.shape
    out = np.empty((h, n + 1), dtype=np.uint8)
    for r in range(h):
        x = rows[r]
        a = np.concatenate([np.zeros(bpp, np.uint8), x[:-bpp]])[:n] if n else x
        b = rows[r - 1] if r > 0 else np.zeros(n, np.uint8)
        c = np.concatenate([np.zeros(bpp, np.uint8), b[:-bpp]])[:n] if n else b
        t = int(types[r])
        pred = [np.zeros(n, np.uint8), a, b, ((a.astype(np.uint16) + b) >> 1).astype(np.uint8), paeth(a, b, c)][t]
        out[r, 0] = t
        out[r, 1:] = x - pred
    return out.tobytes()


def encode_png(samples, color_type: int, depth: int, palette=None, trns: bytes | None = None, filters="mixed", interlace=False,
               seed=0, extra_chunks=()) -> bytes:
    """PNG bytes of (h, w, ch) raw samples.  `filters`: 0-4 for every row, or "mixed" (seeded per row)."""
    samples = np.asarray(samples)
    h, w, ch = samples.shape
    assert ch == CHANNELS[color_type]
    bpp = max(1, ch * depth // 8)
    rng = np.random.default_rng(seed)
    passes = ADAM7 if interlace else ((0, 0, 1, 1),)
    stream = b""
    for r0, c0, rs, cs in passes:
        sub = samples[r0::rs, c0::cs]
        if sub.shape[0] == 0 or sub.shape[1] == 0:
            continue
        types = rng.integers(0, 5, sub.shape[0]) if filters == "mixed" else [filters] * sub.shape[0]
        stream += filter_rows(pack_rows(sub, depth), bpp, types)
    out = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, color_type, 0, 0, int(interlace)))
    for tag, body in extra_chunks:
        out += chunk(tag, body)
    if palette is not None:
        out += chunk(b"PLTE", np.asarray(palette, dtype=np.uint8).tobytes())
    if trns is not None:
        out += chunk(b"tRNS", trns)
    data = zlib.compress(stream, 9)
    half = len(data) // 2   # (two IDAT chunks: the reader concatenates them)
    return out + chunk(b"IDAT", data[:half]) + chunk(b"IDAT", data[half:]) + chunk(b"IEND", b"")


def to8(v, depth):
    v = np.asarray(v, dtype=np.int64)
    if depth == 16:
        return ((v * 255 + 32767) // 65535).astype(np.uint8)
    return (v * (255 // ((1 << depth) - 1))).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------------------
# device image, restated
# ------------------------------------------------------------------------------------------------------------------------
def prepare(pixels: np.ndarray, linear_rgb: bool) -> np.ndarray:
    t = pixels.astype(np.float64) / 255.0
    rgb = t[..., :3]
    if linear_rgb:
        rgb = np.where(rgb <= 0.04045, rgb / 12.92, np.power((rgb + 0.055) / 1.055, 2.4))
    out = np.empty_like(t)
    out[..., :3] = rgb * t[..., 3:]
    out[..., 3] = t[..., 3]
    return out.astype(np.float32)


def downsample(level: np.ndarray) -> np.ndarray:
    h, w = level.shape[:2]
    dh, dw = (h + 1) // 2, (w + 1) // 2
    r0, c0 = 2 * np.arange(dh), 2 * np.arange(dw)
    r1, c1 = np.minimum(r0 + 1, h - 1), np.minimum(c0 + 1, w - 1)
    L = level.astype(np.float64)
    s = (L[r0][:, c0] + L[r0][:, c1]) + (L[r1][:, c0] + L[r1][:, c1])
    return (s * 0.25).astype(np.float32)


def mip_chain(pixels: np.ndarray, linear_rgb: bool) -> list:
    levels = [prepare(pixels, linear_rgb)]
    while levels[-1].shape[0] > 1 or levels[-1].shape[1] > 1:
        levels.append(downsample(levels[-1]))
    return levels


def lod(inv_m: np.ndarray, n_levels: int) -> float:
    a = np.asarray(inv_m, dtype=np.float64)[:2, :2]
    rho = max(np.hypot(a[0, 0], a[1, 0]), np.hypot(a[0, 1], a[1, 1]))
    return float(np.clip(np.log2(rho), 0, n_levels - 1)) if rho > 0 else 0.0


def _lerp(a, b, f):
    return a + f * (b - a)


def bilinear(level: np.ndarray, k: int, u, v) -> np.ndarray:
    h, w = level.shape[:2]
    s = 2.0 ** -k
    x, y = u * s - 0.5, v * s - 0.5
    xf, yf = np.floor(x), np.floor(y)
    fx, fy = (x - xf)[..., None], (y - yf)[..., None]
    c0, c1 = np.clip(xf, 0, w - 1).astype(np.int64), np.clip(xf + 1, 0, w - 1).astype(np.int64)
    r0, r1 = np.clip(yf, 0, h - 1).astype(np.int64), np.clip(yf + 1, 0, h - 1).astype(np.int64)
    L = level.astype(np.float64)
    return _lerp(_lerp(L[r0, c0], L[r0, c1], fx), _lerp(L[r1, c0], L[r1, c1], fx), fy)


def sample(levels: list, inv_m: np.ndarray, smooth: bool, r0: int, c0: int, rows: int, cols: int, points=None) -> np.ndarray:
    """What svgr_image_fill writes before the mask: (rows, cols, 4) doubles over the pixel grid at (r0, c0), or at the
    (i, j) index arrays `points` of that grid."""
    m = np.asarray(inv_m, dtype=np.float64)
    if points is None:
        i, j = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing="ij")
    else:
        i, j = (np.asarray(p, dtype=np.float64) for p in points)
    px, py = i + (r0 + 0.5), j + (c0 + 0.5)
    u = (py * m[0, 1] + px * m[0, 0]) + m[0, 2]
    v = (py * m[1, 1] + px * m[1, 0]) + m[1, 2]
    if not smooth:
        h, w = levels[0].shape[:2]
        c = np.clip(np.floor(u), 0, w - 1).astype(np.int64)
        r = np.clip(np.floor(v), 0, h - 1).astype(np.int64)
        return levels[0][r, c].astype(np.float64)
    lam = lod(m, len(levels))
    k = int(np.floor(lam))
    out = bilinear(levels[k], k, u, v)
    f = lam - k
    if f > 0:
        k1 = min(k + 1, len(levels) - 1)
        out = _lerp(out, bilinear(levels[k1], k1, u, v), f)
    return out


def random_rgba(shape, seed) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, tuple(shape) + (4,), dtype=np.uint8)
