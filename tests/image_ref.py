"""Test helpers for SVG <image>: a PNG encoder (forward scanline filters in numpy, zlib) for every colour type, bit depth
and Adam7, and a numpy restatement of the device image: the mip chain of svgr_image_upload and the per-pixel sampling of
svgr_image_fill (nearest, bilinear, trilinear), in float64 and (`sample_wide`) in long double, with the tolerance of a smooth
fill against the latter (`fill_tolerance`) and the distance of nearest sampling from its texel boundaries (`clearance`)."""
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


def prepare_wide(pixels: np.ndarray, linear_rgb: bool) -> np.ndarray:
    """`prepare` in long double, before the rounding to float32."""
    t = pixels.astype(np.longdouble) / 255
    rgb = t[..., :3]
    if linear_rgb:
        rgb = np.where(rgb <= np.longdouble(0.04045), rgb / np.longdouble(12.92),
                       np.power((rgb + np.longdouble(0.055)) / np.longdouble(1.055), np.longdouble(2.4)))
    return np.concatenate([rgb * t[..., 3:], t[..., 3:]], axis=-1)


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


def corner(x, n: int):
    """One axis of the bilinear footprint at level coordinate x (texel centres on the integers) of n texels: (i0, i1, f), the
    clamp-to-edge rule with what the kernel's clamps make of the rest -- a NaN samples as one left of / above the level (texel
    0, fraction 0), + inf or anything >= n as the last texel, - inf or anything below -1 as the first.  np.fmax / np.fmin
    return the other operand for a NaN, as fmax / fmin do."""
    with np.errstate(invalid="ignore"):
        xf = np.fmin(np.fmax(np.floor(x), -1), n)
        f = np.fmin(np.fmax(x - xf, 0), 1)   # (inf - inf = NaN -> 0)
    xi = xf.astype(np.int64)
    return np.clip(xi, 0, n - 1), np.minimum(xi + 1, n - 1), f


def nearest_index(u, n: int):
    """Nearest sampling on one axis: floor, clamped to the level; NaN gives index 0."""
    return np.fmin(np.fmax(np.floor(u), 0), n - 1).astype(np.int64)


def bilinear(level: np.ndarray, k: int, u, v, dtype=np.float64) -> np.ndarray:
    h, w = level.shape[:2]
    s = dtype(2.0) ** -k
    x, y = u * s - dtype(0.5), v * s - dtype(0.5)
    c0, c1, fx = corner(x, w)
    r0, r1, fy = corner(y, h)
    fx, fy = fx[..., None], fy[..., None]
    L = level.astype(dtype)
    return _lerp(_lerp(L[r0, c0], L[r0, c1], fx), _lerp(L[r1, c0], L[r1, c1], fx), fy)


def coordinates(inv_m, r0: int, c0: int, rows: int, cols: int, points=None, dtype=np.float64):
    """Image-space (u, v) of the pixel centres of the grid at (r0, c0), or of its (i, j) index arrays `points`: the affine map
    in `dtype`, in the unfused order."""
    m = np.asarray(inv_m, dtype=np.float64).astype(dtype)
    if points is None:
        i, j = np.meshgrid(np.arange(rows, dtype=dtype), np.arange(cols, dtype=dtype), indexing="ij")
    else:
        i, j = (np.asarray(p).astype(dtype) for p in points)
    px, py = i + dtype(r0 + 0.5), j + dtype(c0 + 0.5)
    with np.errstate(invalid="ignore", over="ignore"):
        u = (py * m[0, 1] + px * m[0, 0]) + m[0, 2]
        v = (py * m[1, 1] + px * m[1, 0]) + m[1, 2]
    return u, v


def _sample(levels, u, v, smooth, lam, dtype):
    if not smooth:
        h, w = levels[0].shape[:2]
        return levels[0][nearest_index(v, h), nearest_index(u, w)].astype(dtype)
    k = int(np.floor(lam))
    out = bilinear(levels[k], k, u, v, dtype)
    f = dtype(lam) - k
    if f > 0:
        k1 = min(k + 1, len(levels) - 1)
        out = _lerp(out, bilinear(levels[k1], k1, u, v, dtype), f)
    return out


def sample(levels: list, inv_m: np.ndarray, smooth: bool, r0: int, c0: int, rows: int, cols: int, points=None, lam=None) -> np.ndarray:
    """What svgr_image_fill writes before the mask: (rows, cols, 4) doubles over the pixel grid at (r0, c0), or at the
    (i, j) index arrays `points` of that grid.  `lam`: the level of detail, `lod`'s if None."""
    u, v = coordinates(inv_m, r0, c0, rows, cols, points)
    lam = lod(np.asarray(inv_m, dtype=np.float64), len(levels)) if lam is None else lam
    return _sample(levels, u, v, smooth, lam, np.float64)


LD = np.longdouble
U = 2.0 ** -53   # unit roundoff of a double


def sample_wide(levels: list, inv_m: np.ndarray, smooth: bool, lam: float, r0: int, c0: int, rows: int, cols: int,
                points=None) -> np.ndarray:
    """`sample` in long double, the coordinate transform included: the same formulas, every operation rounded to 64 bits of
    mantissa instead of 53, so its own error is 2^-11 of a double evaluation's.  `levels` is the chain to sample from (the
    GPU tests hand it the chain downloaded from the device: a last bit of level 0's `pow` then stays out of the fill's
    tolerance), `lam` the product's paint.image_lod value as a double.  Returns long doubles."""
    u, v = coordinates(inv_m, r0, c0, rows, cols, points, LD)
    return _sample(levels, u, v, smooth, lam, LD)


# roundings of the smooth fill's arithmetic on texels, counted without contraction: a lerp a + f (b - a) rounds three times,
# a level takes three lerps, the fill two levels, one blend and the product with the mask
LERP_ROUNDINGS = 3
FILL_ROUNDINGS = 2 * 3 * LERP_ROUNDINGS + LERP_ROUNDINGS + 1


def levels_read(n_levels: int, lam: float, smooth: bool):
    """The indices of the levels a fill at level of detail `lam` reads."""
    if not smooth:
        return [0]
    k = int(np.floor(lam))
    return [k] if lam == k else [k, min(k + 1, n_levels - 1)]


def fill_tolerance(case, levels=None) -> float:
    """`fill_tolerance_of` for a tests/image_cases.py FillCase, over `levels` (the restated chain of the case if None)."""
    levels = mip_chain(case.pixels(), case.linear_rgb) if levels is None else levels
    return fill_tolerance_of(levels, case.inv_m, case.smooth, case.lam(), *case.bbox)


def clearance(case) -> float:
    """`clearance_of` for a FillCase (its coordinates in long double)."""
    u, v = coordinates(case.inv_m, *case.bbox, dtype=LD)
    return clearance_of(u, v, *case.shape)


def fill_tolerance_of(levels: list, inv_m, smooth: bool, lam: float, r0: int, c0: int, rows: int, cols: int) -> float:
    """Largest |device - sample_wide| a correct double-precision smooth fill may show over the box, with mask values in
    [0, 1]:

        2^-53 x [ R x T + 2 x S x G ]

    The fill is  mask x blend(bilinear(lo, u, v), bilinear(hi, u, v))  with  (u, v) = A (p0, p1) + b.

    * Arithmetic on the texels.  Texels are float32 and enter exactly.  Every lerp  a + f (b - a)  is a convex combination
      (f in [0, 1]), so every intermediate lies within the texels' range, at most T = the largest texel magnitude of the
      levels read, and an error of an operand passes on with a factor of at most 1.  Each rounding therefore adds at most
      2^-53 T to the result.  Counted without contraction (the bound then holds whether or not a compiler fuses): 3 per lerp,
      3 lerps per level, 2 levels, the blend, the product with the mask: R - 1 = 22 (FILL_ROUNDINGS), plus one for the
      fractions x - floor(x), which round only when |x| < 1 (by at most 2^-53, times a texel difference <= T): R = 23.
    * The coordinates.  The sample is a continuous, piecewise bilinear function of (u, v), also across a cell boundary and
      into the clamped border, so an error du moves it by at most du x (the largest difference between neighbouring texels
      of a level x that level's scale 2^-k); G is the largest such product over the levels read (the blend is a convex
      combination of two levels, so the larger one bounds it).  u is a sum of three terms whose magnitudes add up to at most
      S = max(|p0 m0| + |p1 m1| + |m2|) over the box and both rows of A; the term S G is taken twice, for the two roundings
      of that sum.  (u 2^-k is exact; the - 0.5 rounds by 2^-53 |x|, with |x| <= S 2^-k + 0.5.)

    The second term is not a worst case.  Written out, the kernel's fma form rounds p0 m0, the fused sum and the + m2, each
    by up to 2^-53 of a partial sum <= S, and - 0.5 once more, on both coordinates: a worst case of 8 S G, in which every
    rounding is at its half-ulp limit with the same sign, every partial sum is as large as S, and both coordinates sit on
    the steepest texel pair of the image.  2 S G is the bound the fill is held to; tests/test_image_cases_host.py shows that
    the float64 restatement (unfused: four roundings a coordinate) stays within half of it on every case (at most 0.47 of
    it).  Measured on an MI355X over the cases of tests/image_cases.py: the device's largest error is 0.29 of the bound
    (1.02e-14 against 3.50e-14, a 257 x 3 image magnified 3.3 x; on the 37 x 53 tile-seam boxes 4.5e-15 against 1.66e-14).

    Nearest sampling copies a texel and multiplies once by the mask: it is compared bit for bit, and so is every case whose
    coordinates are non-finite or clamped throughout (all lerps are then a + f (a - a) = a)."""
    if not smooth:
        return 0.0
    m = np.asarray(inv_m, dtype=np.float64)
    p0 = max(abs(r0 + 0.5), abs(r0 + rows - 0.5))
    p1 = max(abs(c0 + 0.5), abs(c0 + cols - 0.5))
    S = max(p0 * abs(m[r, 0]) + p1 * abs(m[r, 1]) + abs(m[r, 2]) for r in (0, 1))
    T = G = 0.0
    for k in levels_read(len(levels), lam, smooth):
        L = levels[k].astype(np.float64)
        T = max(T, float(np.abs(L).max()))
        for axis in (0, 1):
            if L.shape[axis] > 1:
                G = max(G, float(np.abs(np.diff(L, axis=axis)).max()) * 2.0 ** -k)
    return U * ((FILL_ROUNDINGS + 1) * T + 2.0 * S * G)


def clearance_of(u, v, h: int, w: int) -> float:
    """Nearest sampling: the smallest distance of any coordinate from a texel boundary that matters, i.e. of u from the
    integers 1 .. w - 1 and of v from 1 .. h - 1 (on the other side of 0 and of w the clamp gives the same texel).  inf for a
    level of one texel.  A comparison bit for bit needs it well above the coordinates' rounding error."""
    d = np.inf
    for x, n in ((u, w), (v, h)):
        if n > 1:
            x = np.asarray(x, dtype=LD)
            d = min(d, float(np.abs(x - np.clip(np.rint(x), 1, n - 1)).min()))
    return d


def random_rgba(shape, seed) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, tuple(shape) + (4,), dtype=np.uint8)
