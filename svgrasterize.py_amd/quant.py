"""Colour quantisation for indexed PNG output (beyond the reference): ``quantize`` and the palette builder.

The per-pixel stages run on the device (csrc/svgr_quant.h has their arithmetic, DESIGN.md 7t the definitions): the set of
distinct colours (``svgr_quant_distinct``), the histogram over 2^20 bins of (r >> 3, g >> 3, b >> 3, a >> 3) with the sums of the
metric's coordinates (``svgr_quant_bins``), and the nearest palette entry of every pixel (``svgr_quant_index``).  The palette is
built here, on the host, over the bins -- thousands of them, not millions of pixels:

  pixel    straight RGBA8 as ``to_rgba8`` writes it; canonical: a pixel with a == 0 is (0, 0, 0, 0)
  metric   X(p) = (r a, g a, b a, 255 a); D(p, q) = the sum of the squared differences of X
  exact    at most ``max_colors`` distinct colours: they are the palette, the image is kept exactly
  lossy    a count-weighted median cut over the bins' means in X, then ``refine`` Lloyd iterations over the bins, the
           centroids rounded back to RGBA8, duplicates removed
  order    ascending (a, r, g, b): the entries that need a tRNS byte come first

Dithering (``dither=``; csrc/svgr_dither.h) changes the indices only, never the palette, and only on the lossy
route -- an image the palette holds exactly is left alone:

  ordered    the colour coordinates of X move by an offset from the 8 x 8 Bayer matrix, scaled by ``ordered_amplitude`` of the
             palette and the pixel's alpha, before the nearest entry is taken
  diffusion  Floyd-Steinberg, every row left to right, the error of a pixel being its target minus its entry in X

No perceptual or gamma-aware metric."""
from __future__ import annotations

import math

import numpy as np

from . import _abi

MAX_COLORS = 256


# ---------------------------------------------------------------------------------------------------------------------
# arguments
# ---------------------------------------------------------------------------------------------------------------------
def check_max_colors(value, what: str = "max_colors") -> int:
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
        raise TypeError(f"{what} is an int from 2 to {MAX_COLORS}, not {value!r}")
    if not 2 <= value <= MAX_COLORS:
        raise ValueError(f"{what} is an int from 2 to {MAX_COLORS}, not {value!r}")
    return int(value)


def check_refine(value) -> int:
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
        raise TypeError(f"refine is a number of iterations (an int >= 0), not {value!r}")
    if value < 0:
        raise ValueError(f"refine is a number of iterations (an int >= 0), not {value!r}")
    return int(value)


def palette_argument(palette):
    """``palette`` of ``write_png`` and its callers: None (no palette: None and False), or the largest number of entries
    (True: 256; an int from 2 to 256)."""
    if palette is None or palette is False:
        return None
    if palette is True:
        return MAX_COLORS
    return check_max_colors(palette, "palette")


DITHER_MODES = ("none", "ordered", "diffusion")


def dither_argument(dither, with_palette: bool = True):
    """``dither`` of ``quantize``, ``write_png`` and its callers, checked: None (None and "none": every pixel takes its nearest
    entry), "ordered" or "diffusion".  ``with_palette`` False: the call writes no indexed file, and there is nothing to dither."""
    if dither is None:
        return None
    if not isinstance(dither, str):
        raise TypeError(f'dither is None, "none", "ordered" or "diffusion", not {dither!r}')
    if dither not in DITHER_MODES:
        raise ValueError(f'dither is None, "none", "ordered" or "diffusion", not {dither!r}')
    if dither == "none":
        return None
    if not with_palette:
        raise ValueError(f"dither={dither!r} goes with indexed output only: it needs palette=")
    return dither


def ordered_amplitude(palette) -> int:
    """The amplitude of ordered dithering under ``palette`` ((n, 4) uint8): with d_i the smallest D of entry i to another entry,
    ``min(65025, isqrt(sum(d_i) // (3 n)))`` -- the typical gap between neighbouring entries along one colour axis; 0 for a single
    entry."""
    x = coordinates(canonical(np.asarray(palette, dtype=np.uint8).reshape(-1, 4)))
    n = len(x)
    if n < 2:
        return 0
    d = ((x[:, None, :] - x[None, :, :]) ** 2).sum(axis=2)   # (int64 holds 4 * 65025^2)
    d[np.arange(n), np.arange(n)] = np.iinfo(np.int64).max
    total = sum(int(v) for v in d.min(axis=1))
    return min(65025, math.isqrt(total // (3 * n)))


# ---------------------------------------------------------------------------------------------------------------------
# pixels, host side
# ---------------------------------------------------------------------------------------------------------------------
def canonical(rgba8: np.ndarray) -> np.ndarray:
    """The pixels with every fully transparent one set to (0, 0, 0, 0)."""
    out = np.array(rgba8, dtype=np.uint8, copy=True)
    out[out[..., 3] == 0] = 0
    return out


def coordinates(rgba8: np.ndarray) -> np.ndarray:
    """X of every pixel: (..., 4) int64."""
    p = np.asarray(rgba8, dtype=np.uint8).astype(np.int64)
    a = p[..., 3:4]
    return np.concatenate([p[..., :3] * a, 255 * a], axis=-1)


def order_palette(colors: np.ndarray) -> np.ndarray:
    """The distinct rows of ``colors`` ((n, 4) uint8) in ascending (a, r, g, b)."""
    c = np.unique(np.asarray(colors, dtype=np.uint8).reshape(-1, 4), axis=0)
    return np.ascontiguousarray(c[np.lexsort((c[:, 2], c[:, 1], c[:, 0], c[:, 3]))])


def trns(palette: np.ndarray) -> bytes:
    """The tRNS chunk's data: the alphas up to the last entry with a < 255; empty when every entry is opaque."""
    alpha = np.asarray(palette, dtype=np.uint8).reshape(-1, 4)[:, 3]
    below = np.nonzero(alpha < 255)[0]
    return alpha[:below[-1] + 1].tobytes() if len(below) else b""


def depth_of(n_colors: int) -> int:
    return 1 if n_colors <= 2 else 2 if n_colors <= 4 else 4 if n_colors <= 16 else 8


# ---------------------------------------------------------------------------------------------------------------------
# the palette builder ("the cut")
# ---------------------------------------------------------------------------------------------------------------------
def _box(means, count, sums, members):
    """(score, axis, centroid) of a box: the largest of the four weighted sums of squares about the centroid, its axis (the
    lowest on a tie), and the centroid = the members' summed X over their summed count."""
    n = count[members]
    centroid = sums[members].sum(axis=0).astype(np.float64) / float(n.sum())
    v = (n[:, None].astype(np.float64) * (means[members] - centroid) ** 2).sum(axis=0)
    axis = int(np.argmax(v))
    return float(v[axis]), axis, centroid


def median_cut(count: np.ndarray, sums: np.ndarray, max_colors: int) -> np.ndarray:
    """The centroids ((k, 4) float64, k <= max_colors) of the count-weighted median cut over bins with ``count`` ((n,) integer)
    pixels and ``sums`` ((n, 4) integer) of X."""
    count, sums = np.asarray(count).astype(np.int64), np.asarray(sums).astype(np.int64)
    means = sums.astype(np.float64) / count[:, None].astype(np.float64)
    boxes = [np.arange(len(count))]
    stats = [_box(means, count, sums, boxes[0])]
    while len(boxes) < max_colors:
        best, best_v = -1, 0.0
        for i, (v, _, _) in enumerate(stats):
            if len(boxes[i]) >= 2 and v > best_v:
                best, best_v = i, v
        if best < 0:
            break
        members, axis = boxes[best], stats[best][1]
        order = members[np.argsort(means[members, axis], kind="stable")]
        cw = np.cumsum(count[order])
        j = int(np.searchsorted(2 * cw, cw[-1], side="left"))   # the first member at which half the weight is reached
        cut = min(max(j + 1, 1), len(order) - 1)
        boxes[best] = order[:cut]
        boxes.append(order[cut:])
        stats[best] = _box(means, count, sums, boxes[best])
        stats.append(_box(means, count, sums, boxes[-1]))
    return np.array([s[2] for s in stats], dtype=np.float64).reshape(-1, 4)


def assign(means: np.ndarray, centroids: np.ndarray):
    """Per bin the index of the nearest centroid (squared distance in float64, a tie to the lowest index) and that distance."""
    idx = np.empty(len(means), dtype=np.int64)
    dist = np.empty(len(means), dtype=np.float64)
    step = max(1, (1 << 19) // max(len(centroids), 1))
    cols = [np.ascontiguousarray(centroids[:, k])[None, :] for k in range(4)]
    for i0 in range(0, len(means), step):
        m = means[i0:i0 + step]
        d = m[:, 0, None] - cols[0]   # ((d0 + d1) + d2) + d3, an axis at a time: the temporaries stay in the cache
        d *= d
        for k in range(1, 4):
            t = m[:, k, None] - cols[k]
            t *= t
            d += t
        idx[i0:i0 + step] = np.argmin(d, axis=1)
        dist[i0:i0 + step] = d[np.arange(len(d)), idx[i0:i0 + step]]
    return idx, dist


def lloyd(count: np.ndarray, sums: np.ndarray, centroids: np.ndarray, refine: int) -> np.ndarray:
    """``refine`` Lloyd iterations over the bins: every bin's mean goes to its nearest centroid, every centroid becomes the summed
    X over the summed count of its bins (sums of integers below 2^53: exact in float64); a centroid without a bin stays."""
    count, sums = np.asarray(count).astype(np.int64), np.asarray(sums).astype(np.int64)
    means = sums.astype(np.float64) / count[:, None].astype(np.float64)
    c = np.array(centroids, dtype=np.float64, copy=True)
    for _ in range(refine):
        idx, _ = assign(means, c)
        n = np.bincount(idx, weights=count.astype(np.float64), minlength=len(c))
        for k in range(4):
            s = np.bincount(idx, weights=sums[:, k].astype(np.float64), minlength=len(c))
            c[:, k] = np.where(n > 0, s / np.maximum(n, 1.0), c[:, k])
    return c


def objective(count: np.ndarray, sums: np.ndarray, centroids: np.ndarray) -> float:
    """The unrounded objective: the count-weighted sum over the bins of the squared distance of the bin's mean to its nearest
    centroid."""
    count, sums = np.asarray(count).astype(np.int64), np.asarray(sums).astype(np.int64)
    means = sums.astype(np.float64) / count[:, None].astype(np.float64)
    _, dist = assign(means, np.asarray(centroids, dtype=np.float64))
    return float((count.astype(np.float64) * dist).sum())


def centroids_to_rgba8(centroids: np.ndarray) -> np.ndarray:
    """Straight RGBA8 of centroids in X: a = rint(X3 / 255), colour = rint(Xc / a), a == 0 gives all zero."""
    c = np.asarray(centroids, dtype=np.float64).reshape(-1, 4)
    a = np.rint(c[:, 3] / 255.0)
    out = np.zeros((len(c), 4), dtype=np.uint8)
    seen = a > 0
    out[seen, :3] = np.clip(np.rint(c[seen, :3] / a[seen, None]), 0, 255).astype(np.uint8)
    out[seen, 3] = np.clip(a[seen], 0, 255).astype(np.uint8)
    return out


def build_palette(bins: np.ndarray, max_colors: int, refine: int = 3) -> np.ndarray:
    """The lossy route: the palette ((n, 4) uint8, n <= max_colors, ordered) of an image with the non-empty ``bins`` ((m, 5):
    pixels and the four sums of X, in ascending key order)."""
    bins = np.asarray(bins).reshape(-1, 5)
    count, sums = bins[:, 0], bins[:, 1:]
    centroids = lloyd(count, sums, median_cut(count, sums, max_colors), refine)
    return order_palette(centroids_to_rgba8(centroids))


# ---------------------------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------------------------
def _on_device(image):
    """(device buffer, rows, cols) of a Layer or a (rows, cols, 4) uint8 array."""
    from .layer import Layer  # noqa: PLC0415

    if isinstance(image, Layer):
        return image._to_rgba8_device()
    if isinstance(image, _abi.DeviceBuffer):
        raise TypeError("quantize takes a Layer or a (rows, cols, 4) uint8 array")
    px = np.asarray(image)
    if px.dtype != np.uint8 or px.ndim != 3 or px.shape[2] != 4 or px.size == 0:
        raise ValueError("quantize takes a Layer or a non-empty (rows, cols, 4) uint8 array")
    return _abi.Context.get().from_host(np.ascontiguousarray(px)), px.shape[0], px.shape[1]


def colors_of_u32(values: np.ndarray) -> np.ndarray:
    """(n,) uint32 pixels -> (n, 4) uint8 RGBA."""
    return np.ascontiguousarray(values, dtype="<u4").view(np.uint8).reshape(-1, 4)


def palette_and_route(rgba8, rows: int, cols: int, max_colors: int = MAX_COLORS, refine: int = 3):
    """``(palette, exact)`` of the RGBA8 bytes in the DeviceBuffer ``rgba8``: the distinct colours when there are at most
    ``max_colors`` (``exact``: the palette holds the image), the median cut over the bins otherwise."""
    ctx = _abi.Context.get()
    exact = _abi.quant_distinct(ctx, rgba8, rows, cols, max_colors)
    if exact is not None:
        return order_palette(colors_of_u32(exact)), True
    _, bins = _abi.quant_bins(ctx, rgba8, rows, cols)
    return build_palette(bins, max_colors, refine), False


def index_rows(rgba8, rows: int, cols: int, max_colors: int, refine: int, dither, stream: bool, indices: bool):
    """``(palette, stream, indices)`` of the RGBA8 bytes in the DeviceBuffer ``rgba8``: the palette, and the packed scanlines and /
    or the plain indices on the device, dithered as ``dither`` (checked: None, "ordered" or "diffusion") says.  The palette is that
    of the undithered image.  An image that it holds exactly takes the plain route under every ``dither``: diffusion has no error
    to pass on there, and ordered dithering is not let loose on pixels that need none."""
    ctx = _abi.Context.get()
    palette, exact = palette_and_route(rgba8, rows, cols, max_colors, refine)
    if dither is None or exact:
        out = _abi.quant_index(ctx, rgba8, rows, cols, palette, stream=stream, indices=indices)
    else:
        amp = ordered_amplitude(palette) if dither == "ordered" else 0
        out = _abi.quant_dither(ctx, rgba8, rows, cols, palette, dither, amp, stream=stream, indices=indices)
    return (palette, *out)


def quantize(image, max_colors: int = MAX_COLORS, refine: int = 3, dither=None):
    """``(indices, palette)``: ``indices`` (rows, cols) uint8 and ``palette`` (n, 4) uint8 straight RGBA, n <= ``max_colors``,
    with ``palette[indices]`` the quantised image.  ``image`` is a Layer or a (rows, cols, 4) uint8 array as ``to_rgba8`` gives
    it.  An image of at most ``max_colors`` (2 .. 256) colours is kept exactly (fully transparent pixels become (0, 0, 0, 0));
    otherwise the palette is a median cut over the colour histogram, improved by ``refine`` Lloyd iterations, and every pixel gets
    its nearest entry under D, the squared distance of (r a, g a, b a, 255 a).  The palette is in ascending (a, r, g, b)
    order.

    ``dither`` (None or "none": as above) spreads the rounding error of the lossy route over neighbouring pixels, so that a
    gradient shows as a fine pattern instead of bands: "ordered" moves every pixel by an offset from the 8 x 8 Bayer matrix
    before it takes its nearest entry, "diffusion" is Floyd-Steinberg error diffusion, every row left to right.  Both are integer
    arithmetic on the device; the palette does not depend on ``dither``, and an exactly kept image is never touched.  The same
    image gives the same result every time."""
    max_colors, refine, dither = check_max_colors(max_colors), check_refine(refine), dither_argument(dither)
    buf, rows, cols = _on_device(image)
    palette, _, idx = index_rows(buf, rows, cols, max_colors, refine, dither, stream=False, indices=True)
    return idx.download((rows, cols), np.uint8), palette
