"""numpy restatement of the filter primitives beyond the reference (feTurbulence, feComponentTransfer, feConvolveMatrix,
feDisplacementMap), written from the Filter Effects text in the operation order the kernels use, plus the loader for the host
build of their arithmetic (tests/filter_harness.cpp over csrc/svgr_core.h).  Test infrastructure only."""
import ctypes as C
import math

import numpy as np

from tests.util import host_build

BSIZE, BM, PERLIN_N = 0x100, 0xFF, 0x1000
RAND_M, RAND_A, RAND_Q, RAND_R = 2147483647, 16807, 127773, 2836
NAN = float("nan")


def _c_rem(a: int, b: int) -> int:
    """C's a % b (the sign of the dividend)."""
    r = abs(a) % abs(b)
    return -r if a < 0 else r


def setup_seed(s: int) -> int:
    if s <= 0:
        s = -_c_rem(s, RAND_M - 1) + 1
    if s > RAND_M - 1:
        s = RAND_M - 1
    return s


def random(s: int) -> int:
    r = RAND_A * (s % RAND_Q) - RAND_R * (s // RAND_Q)   # (s > 0 here: Python's // and % are C's)
    return r + RAND_M if r <= 0 else r


def lattice(seed):
    """(sel (514,), grad (4, 514, 2)) of the spec's init() for a seed (truncated toward zero first)."""
    s = setup_seed(int(float(seed)) if not isinstance(seed, int) else seed)
    sel = np.zeros(2 * BSIZE + 2, dtype=np.int64)
    grad = np.zeros((4, 2 * BSIZE + 2, 2), dtype=np.float64)
    for k in range(4):
        for i in range(BSIZE):
            sel[i] = i
            for j in range(2):
                s = random(s)
                grad[k, i, j] = float(s % (2 * BSIZE) - BSIZE) / BSIZE
            x, y = float(grad[k, i, 0]), float(grad[k, i, 1])
            length = math.sqrt(x * x + y * y)
            if length > 0.0:
                grad[k, i] = (x / length, y / length)
    for i in range(BSIZE - 1, 0, -1):
        t = sel[i]
        s = random(s)
        j = s % BSIZE
        sel[i] = sel[j]
        sel[j] = t
    for i in range(BSIZE + 2):   # (one by one, as in the spec: entries 512 and 513 read the copies of 0 and 1 made just before)
        sel[BSIZE + i] = sel[i]
        grad[:, BSIZE + i] = grad[:, i]
    return sel, grad


def clamp_unit(x):
    """[0, 1], and NaN -> 0: the final clamp of the primitives (csrc/svgr_core.h clamp_unit)."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(x > 0.0, np.where(x < 1.0, x, 1.0), 0.0)


STATE_MAX = 2 ** 53   # the stitch state of the last octave stays within the exactly representable integers


def turbulence_params(fx, fy, tile, stitch):
    """(fx, fy, width, height, wrap_x, wrap_y) of the first octave: the base frequencies adjusted to the tile and the stitch
    state when stitching.  The state is Python integers (exact whatever its size)."""
    fx, fy = float(fx), float(fy)
    if not stitch:
        return fx, fy, 0, 0, 0, 0

    def adjust(f, w):
        lo, hi = math.floor(w * f) / w, math.ceil(w * f) / w
        return hi if lo == 0.0 or not f / lo < hi / f else lo   # (f / 0 = inf is not below hi / f)

    tx, ty, tw, th = (float(v) for v in tile)
    if fx != 0.0:
        fx = adjust(fx, tw)
    if fy != 0.0:
        fy = adjust(fy, th)
    width = int(tw * fx + 0.5)
    height = int(th * fy + 0.5)
    return fx, fy, width, height, int(tx * fx + PERLIN_N + width), int(ty * fy + PERLIN_N + height)


def turbulence_accepts(base_frequency, octaves, stitch_tile):
    """Whether the parameters are ones the primitive accepts: finite frequencies >= 0, 0..32 octaves and, when stitching, a
    finite tile of positive width and height whose state of the last octave (k = octaves - 1: width_k = 2^k width_0,
    wrap_k = 2^k (wrap_0 - 4096) + 4096) stays within 2^53:  2^(octaves - 1) max(width_0, |wrap_0 - 4096|) + 4096 <= 2^53."""
    fx, fy = (float(f) for f in base_frequency)
    if not (math.isfinite(fx) and math.isfinite(fy) and fx >= 0.0 and fy >= 0.0 and 0 <= octaves <= 32):
        return False
    if stitch_tile is None:
        return True
    tile = [float(v) for v in stitch_tile]
    if not all(math.isfinite(v) for v in tile) or not (tile[2] > 0.0 and tile[3] > 0.0):
        return False
    with np.errstate(all="ignore"):
        for f, t0, tw in ((fx, tile[0], tile[2]), (fy, tile[1], tile[3])):
            f, t0, tw = np.float64(f), np.float64(t0), np.float64(tw)
            if f != 0.0:
                lo, hi = np.floor(tw * f) / tw, np.ceil(tw * f) / tw
                f = hi if lo == 0.0 or not f / lo < hi / f else lo
            w0 = tw * f + 0.5
            if not (math.isfinite(f) and math.isfinite(w0) and w0 < STATE_MAX):
                return False
            width = math.trunc(w0)
            r0 = t0 * f + PERLIN_N + np.float64(width)
            if not (math.isfinite(r0) and abs(r0) < STATE_MAX):
                return False
            wrap = math.trunc(r0)
            if 2 ** max(octaves - 1, 0) * max(width, abs(wrap - PERLIN_N)) + PERLIN_N > STATE_MAX:
                return False
    return True


def turbulence_cell(t: float):
    """(integer part toward zero, fraction) of a lattice coordinate, in Python integers: exact for every finite t.  An infinite
    t (an overflowed product of finite numbers) stands for an integer beyond every stitch wrap that is a multiple of 256;
    its fraction is inf - inf = NaN, so the point's noise is NaN and ends as 0 in every channel."""
    if math.isinf(t):
        return (1 << 2000) * (1 if t > 0 else -1), NAN
    i = math.trunc(t)
    return i, t - float(i)


def turbulence_trace(seed, base_frequency, octaves, stitch_tile, px, py):
    """[(tx, ty, cell x, cell y, wrap_x, wrap_y) per octave] at one point: what a case needs to show that it reaches its edge."""
    fx, fy, width, height, wrap_x, wrap_y = turbulence_params(*base_frequency, stitch_tile, stitch_tile is not None)
    vx, vy = float(px) * fx, float(py) * fy
    rows = []
    for _ in range(octaves):
        tx, ty = vx + PERLIN_N, vy + PERLIN_N
        rows.append((tx, ty, turbulence_cell(tx)[0], turbulence_cell(ty)[0], wrap_x, wrap_y))
        vx, vy = vx * 2.0, vy * 2.0
        wrap_x, wrap_y = 2 * wrap_x - PERLIN_N, 2 * wrap_y - PERLIN_N
    return rows


def turbulence_exact(seed, base_frequency, octaves, fractal, stitch_tile, px, py):
    """`turbulence` point by point in Python floats (IEEE doubles, one rounding per operation) and Python integers: every
    integer part is exact and nothing can overflow, whatever the coordinate.  (n, 4)."""
    sel, grad = lattice(seed)
    sel = [int(v) for v in sel]
    g = grad.tolist()
    stitch = stitch_tile is not None
    fx, fy, width0, height0, wrapx0, wrapy0 = turbulence_params(*base_frequency, stitch_tile, stitch)
    out = np.zeros((len(px), 4))
    for n, (x, y) in enumerate(zip(px, py)):
        vx, vy, ratio = float(x) * fx, float(y) * fy, 1.0
        width, height, wrap_x, wrap_y = width0, height0, wrapx0, wrapy0
        total = [0.0, 0.0, 0.0, 0.0]
        for _ in range(octaves):
            (bx0, rx0), (by0, ry0) = turbulence_cell(vx + PERLIN_N), turbulence_cell(vy + PERLIN_N)
            bx1, by1 = bx0 + 1, by0 + 1
            rx1, ry1 = rx0 - 1.0, ry0 - 1.0
            if stitch:
                bx0 = bx0 - width if bx0 >= wrap_x else bx0
                bx1 = bx1 - width if bx1 >= wrap_x else bx1
                by0 = by0 - height if by0 >= wrap_y else by0
                by1 = by1 - height if by1 >= wrap_y else by1
            bx0, bx1, by0, by1 = bx0 & BM, bx1 & BM, by0 & BM, by1 & BM
            i, j = sel[bx0], sel[bx1]
            b00, b10, b01, b11 = sel[i + by0], sel[j + by0], sel[i + by1], sel[j + by1]
            sx = rx0 * rx0 * (3.0 - 2.0 * rx0)
            sy = ry0 * ry0 * (3.0 - 2.0 * ry0)
            for k in range(4):
                q = g[k]
                u = rx0 * q[b00][0] + ry0 * q[b00][1]
                v = rx1 * q[b10][0] + ry0 * q[b10][1]
                a = u + sx * (v - u)
                u = rx0 * q[b01][0] + ry1 * q[b01][1]
                v = rx1 * q[b11][0] + ry1 * q[b11][1]
                b = u + sx * (v - u)
                r = a + sy * (b - a)
                total[k] = total[k] + (r if fractal else abs(r)) / ratio
            vx, vy, ratio = vx * 2.0, vy * 2.0, ratio * 2.0
            if stitch:
                width, height = width + width, height + height
                wrap_x, wrap_y = 2 * wrap_x - PERLIN_N, 2 * wrap_y - PERLIN_N
        out[n] = [(t + 1.0) * 0.5 if fractal else t for t in total]
    return clamp_unit(out)


def turbulence(seed, base_frequency, octaves, fractal, stitch_tile, px, py):
    """(n, 4) RGBA in [0, 1] at the user-space points (px[i], py[i]); stitch_tile None = noStitch.  The array form, for layers:
    its integer parts are int64, exact while every lattice coordinate is below 2^62 in size (asserted); `turbulence_exact`
    is the form for every coordinate."""
    sel, grad = lattice(seed)
    fx, fy, width, height, wrap_x, wrap_y = turbulence_params(*base_frequency, stitch_tile, stitch_tile is not None)
    px, py = np.asarray(px, dtype=np.float64), np.asarray(py, dtype=np.float64)
    vx, vy, ratio = px * fx, py * fy, 1.0
    total = np.zeros((4,) + px.shape)
    for _ in range(octaves):
        tx, ty = vx + PERLIN_N, vy + PERLIN_N
        assert (np.abs(tx) < 2.0 ** 62).all() and (np.abs(ty) < 2.0 ** 62).all(), "use turbulence_exact"
        bx0, by0 = np.trunc(tx).astype(np.int64), np.trunc(ty).astype(np.int64)
        bx1, by1 = bx0 + 1, by0 + 1
        rx0, ry0 = tx - np.trunc(tx), ty - np.trunc(ty)
        rx1, ry1 = rx0 - 1.0, ry0 - 1.0
        if stitch_tile is not None:
            bx0 = np.where(bx0 >= wrap_x, bx0 - width, bx0)
            bx1 = np.where(bx1 >= wrap_x, bx1 - width, bx1)
            by0 = np.where(by0 >= wrap_y, by0 - height, by0)
            by1 = np.where(by1 >= wrap_y, by1 - height, by1)
        bx0, bx1, by0, by1 = bx0 & BM, bx1 & BM, by0 & BM, by1 & BM
        i, j = sel[bx0], sel[bx1]
        b00, b10, b01, b11 = sel[i + by0], sel[j + by0], sel[i + by1], sel[j + by1]
        sx = rx0 * rx0 * (3.0 - 2.0 * rx0)
        sy = ry0 * ry0 * (3.0 - 2.0 * ry0)
        for k in range(4):
            g = grad[k]
            u = rx0 * g[b00, 0] + ry0 * g[b00, 1]
            v = rx1 * g[b10, 0] + ry0 * g[b10, 1]
            a = u + sx * (v - u)
            u = rx0 * g[b01, 0] + ry1 * g[b01, 1]
            v = rx1 * g[b11, 0] + ry1 * g[b11, 1]
            b = u + sx * (v - u)
            n = a + sy * (b - a)
            total[k] = total[k] + (n if fractal else np.abs(n)) / ratio
        vx, vy, ratio = vx * 2.0, vy * 2.0, ratio * 2.0
        if stitch_tile is not None:
            width, height = width + width, height + height
            wrap_x, wrap_y = 2 * wrap_x - PERLIN_N, 2 * wrap_y - PERLIN_N
    out = (total + 1.0) * 0.5 if fractal else total
    return clamp_unit(out).T.copy()


def pixel_user_points(inv_m6, offset, shape):
    """User-space points of the pixel centres of a (rows, cols) layer at `offset`: (o + i) + 0.5, then the inverse
    transform as plain products and sums, left to right (the kernel's form)."""
    rows, cols = shape
    d0 = (offset[0] + np.arange(rows, dtype=np.int64)[:, None] + np.zeros((1, cols), dtype=np.int64)).astype(np.float64) + 0.5
    d1 = (offset[1] + np.zeros((rows, 1), dtype=np.int64) + np.arange(cols, dtype=np.int64)[None, :]).astype(np.float64) + 0.5
    m = inv_m6
    return m[0] * d0 + m[1] * d1 + m[2], m[3] * d0 + m[4] * d1 + m[5]


def turbulence_layer(transform, offset, shape, base_frequency, octaves, seed, stitch_tile, fractal):
    px, py = pixel_user_points(transform.invert.m6(), offset, shape)
    return turbulence(seed, base_frequency, octaves, fractal, stitch_tile, px.ravel(), py.ravel()).reshape(*shape, 4)


def transfer(c, fn, raw=False):
    """One feComponentTransfer function on a channel array (fn in Layer.component_transfer's form).  A NaN value counts as 0 on
    the way in, and a NaN result -- 0 * inf in gamma, say -- is 0 on the way out (`clamp_unit`).  `raw`: the value before that
    last clamp."""
    c = clamp_unit(c)
    kind = "identity" if fn is None else fn[0]
    r = c
    if kind == "table" and len(fn[1]):
        v = np.asarray(fn[1], dtype=np.float64)
        if len(v) == 1:
            r = np.full_like(c, v[0])
        else:
            m = len(v) - 1
            t = c * m
            k = np.minimum(np.floor(t), m - 1).astype(np.int64)
            with np.errstate(invalid="ignore", over="ignore"):
                r = v[k] + (t - k) * (v[k + 1] - v[k])
    elif kind == "discrete" and len(fn[1]):
        v = np.asarray(fn[1], dtype=np.float64)
        k = np.minimum(np.floor(c * len(v)), len(v) - 1).astype(np.int64)
        r = v[k]
    elif kind == "linear":
        with np.errstate(invalid="ignore", over="ignore"):
            r = fn[1] * c + fn[2]
    elif kind == "gamma":
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            r = fn[1] * np.power(c, fn[2]) + fn[3]
    return r if raw else clamp_unit(r)


def component_transfer(image, funcs):
    return np.stack([transfer(image[..., k], funcs[k]) for k in range(4)], axis=-1)


def convolve_matrix(image, kernel, divisor, bias, target, edge_mode, preserve_alpha):
    """feConvolveMatrix of a (rows, cols, 4) image (premultiplied, or straight with preserve_alpha)."""
    rows, cols = image.shape[:2]
    oy, ox = kernel.shape
    tx, ty = target
    r = np.arange(rows)[:, None]
    c = np.arange(cols)[None, :]
    acc = np.zeros((rows, cols, 4))
    for I in range(oy):
        for J in range(ox):
            rr, cc = r - ty + I, c - tx + J
            if edge_mode == "duplicate":
                v = image[np.clip(rr, 0, rows - 1), np.clip(cc, 0, cols - 1)]
            elif edge_mode == "wrap":
                v = image[rr % rows, cc % cols]
            else:
                inside = (rr >= 0) & (rr < rows) & (cc >= 0) & (cc < cols)
                v = np.where(inside[..., None], image[np.clip(rr, 0, rows - 1), np.clip(cc, 0, cols - 1)], 0.0)
            with np.errstate(invalid="ignore", over="ignore"):
                acc = acc + v * kernel[oy - 1 - I, ox - 1 - J]
    with np.errstate(invalid="ignore", over="ignore"):
        res = acc / divisor + bias
        if preserve_alpha:
            res[..., :3] = clamp_unit(res[..., :3])
            res[..., 3] = image[..., 3]
        else:
            res[..., 3] = clamp_unit(res[..., 3])
            # [0, alpha], NaN -> 0: the form of clamp_unit with alpha as the upper end
            res[..., :3] = np.where(res[..., :3] > 0.0, np.where(res[..., :3] < res[..., 3:], res[..., :3], res[..., 3:]), 0.0)
    return res


def convolve_footprint(shape, kernel_shape, target, edge_mode, at):
    """(rows, cols) bool: the output pixels whose kernel footprint reads the source pixel `at` = (r, c), weights of 0 included.
    Output (R, C) reads (R - ty + I, C - tx + J) for every I < orderY, J < orderX, moved into the image by the edge mode
    (`none` reads nothing outside)."""
    rows, cols = shape
    oy, ox = kernel_shape
    tx, ty = target
    hit = np.zeros(shape, dtype=bool)
    for R in range(rows):
        for Cc in range(cols):
            for I in range(oy):
                for J in range(ox):
                    r, c = R - ty + I, Cc - tx + J
                    if edge_mode == "duplicate":
                        r, c = min(max(r, 0), rows - 1), min(max(c, 0), cols - 1)
                    elif edge_mode == "wrap":
                        r, c = r % rows, c % cols
                    if (r, c) == tuple(at):
                        hit[R, Cc] = True
    return hit


def convolve_matrix_lds(tile, order_y, order_x):
    """Bytes of dynamic LDS of a feConvolveMatrix launch with `tile` x `tile` workgroups: the input tile with its halo
    (RGBA doubles) and the weights."""
    return (tile + order_y - 1) * (tile + order_x - 1) * 32 + order_x * order_y * 8


def convolve_matrix_tile(order_y, order_x):
    """The workgroup tile svgr_layer_convolve_matrix picks: 16 while that fits in 64 KiB of LDS, else 8."""
    return 16 if convolve_matrix_lds(16, order_y, order_x) <= 64 << 10 else 8


def displacement_map(src, src_offset, disp, disp_offset, lin, scale, xc, yc):
    """feDisplacementMap: src premultiplied (rows_s, cols_s, 4) at src_offset, disp straight (rows, cols, 4) at disp_offset,
    lin = the 2 x 2 linear part of the transform; channels 0..3."""
    rows, cols = disp.shape[:2]
    du0 = scale * (disp[..., xc] - 0.5)
    du1 = scale * (disp[..., yc] - 0.5)
    dd0 = lin[0, 0] * du0 + lin[0, 1] * du1
    dd1 = lin[1, 0] * du0 + lin[1, 1] * du1
    p0 = (disp_offset[0] + np.arange(rows)[:, None]).astype(np.float64) + 0.5 + dd0
    p1 = (disp_offset[1] + np.arange(cols)[None, :]).astype(np.float64) + 0.5 + dd1
    r = np.floor(p0) - src_offset[0]
    c = np.floor(p1) - src_offset[1]
    inside = (r >= 0) & (r < src.shape[0]) & (c >= 0) & (c < src.shape[1])
    ri = np.where(inside, r, 0).astype(np.int64)
    ci = np.where(inside, c, 0).astype(np.int64)
    return np.where(inside[..., None], src[ri, ci], 0.0)


def displaced_points(disp, disp_offset, lin, scale, xc, yc, dtype=np.float64):
    """The device points (p0, p1) that feDisplacementMap looks up, in `dtype` (the kernel's order of operations)."""
    rows, cols = disp.shape[:2]
    lin = np.asarray(lin, dtype=np.float64).astype(dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        du0 = dtype(scale) * (disp[..., xc].astype(dtype) - dtype(0.5))
        du1 = dtype(scale) * (disp[..., yc].astype(dtype) - dtype(0.5))
        dd0 = lin[0, 0] * du0 + lin[0, 1] * du1
        dd1 = lin[1, 0] * du0 + lin[1, 1] * du1
        p0 = (disp_offset[0] + np.arange(rows)[:, None]).astype(dtype) + dtype(0.5) + dd0
        p1 = (disp_offset[1] + np.arange(cols)[None, :]).astype(dtype) + dtype(0.5) + dd1
    return p0, p1


def displacement_map_wide(src, src_offset, disp, disp_offset, lin, scale, xc, yc):
    """`displacement_map` with the displaced points in long double.  The output is a copy of source pixels, so it equals a
    double evaluation bit for bit wherever no displaced point lies within that evaluation's rounding error (a few 2^-53 of
    the point's magnitude) of a pixel edge: `displacement_clearance` measures the distance.  A non-finite point compares
    false with everything and gives a transparent pixel, as does a far one."""
    p0, p1 = displaced_points(disp, disp_offset, lin, scale, xc, yc, np.longdouble)
    r = np.floor(p0) - src_offset[0]
    c = np.floor(p1) - src_offset[1]
    with np.errstate(invalid="ignore"):
        inside = (r >= 0) & (r < src.shape[0]) & (c >= 0) & (c < src.shape[1])
    ri = np.where(inside, r, 0).astype(np.int64)
    ci = np.where(inside, c, 0).astype(np.int64)
    return np.where(inside[..., None], src[ri, ci], 0.0)


def displacement_clearance(src_shape, src_offset, disp, disp_offset, lin, scale, xc, yc) -> float:
    """The smallest distance of a finite displaced p0 / p1 from a pixel edge of the source (the integers s .. s + n of its
    axis; beyond them both sides of an edge are transparent).  inf if no point is finite."""
    d = np.inf
    for p, s, n in zip(displaced_points(disp, disp_offset, lin, scale, xc, yc, np.longdouble), src_offset, src_shape):
        p = p[np.isfinite(p)]
        if p.size:
            d = min(d, float(np.abs(p - np.clip(np.rint(p), s, s + n)).min()))
    return d


# -- the host build of svgr_core.h's filter arithmetic ---------------------------------------------------------------------
def harness():
    L = host_build("filter_harness")
    L.fh_dm_index.argtypes = [np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")] * 2 + [C.c_long] + [C.c_int] * 4 + [
        np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")]
    f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
    i32p = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
    L.fh_lattice.argtypes = [C.c_int64, i32p, f64p]
    L.fh_turbulence.argtypes = [C.c_int64, C.c_double, C.c_double, f64p, C.c_int, C.c_int, C.c_int, f64p, C.c_long, f64p]
    L.fh_turbulence_valid.argtypes = [C.c_double, C.c_double, f64p, C.c_int, C.c_int]
    L.fh_turbulence_state.argtypes = [C.c_double, C.c_double, f64p, C.c_int, C.c_int,
                                      np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS"), f64p]
    L.fh_transfer.argtypes = [f64p, C.c_long, C.c_int, f64p, f64p, C.c_int, f64p]
    L.fh_convolve_matrix.argtypes = [f64p, C.c_long, C.c_long, f64p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double,
                                     C.c_int, C.c_int, f64p]
    L.fh_turbulence_layer.argtypes = [C.c_int64, C.c_double, C.c_double, f64p, C.c_int, C.c_int, C.c_int, f64p, C.c_long, C.c_long,
                                      C.c_long, C.c_long, f64p]
    return L


def harness_lattice(L, seed):
    """(sel (514,), grad (4, 514, 2)) from the host build (its lattice-major layout turned into the spec's)."""
    sel = np.zeros(2 * BSIZE + 2, dtype=np.int32)
    grad = np.zeros((2 * BSIZE + 2) * 8)
    L.fh_lattice(seed, sel, grad)
    return sel.astype(np.int64), grad.reshape(2 * BSIZE + 2, 4, 2).transpose(1, 0, 2)


def harness_turbulence(L, seed, base_frequency, octaves, fractal, stitch_tile, px, py):
    pts = np.ascontiguousarray(np.stack([np.asarray(px, np.float64).ravel(), np.asarray(py, np.float64).ravel()], axis=1)).reshape(-1)
    out = np.zeros((len(pts) // 2, 4))
    tile = np.ascontiguousarray((0, 0, 0, 0) if stitch_tile is None else stitch_tile, dtype=np.float64)
    L.fh_turbulence(seed, base_frequency[0], base_frequency[1], tile, octaves, int(fractal), int(stitch_tile is not None), pts,
                    len(pts) // 2, out.reshape(-1))
    return out


def harness_turbulence_layer(L, transform, offset, shape, base_frequency, octaves, seed, stitch_tile, fractal):
    out = np.zeros((shape[0], shape[1], 4))
    tile = np.ascontiguousarray((0, 0, 0, 0) if stitch_tile is None else stitch_tile, dtype=np.float64)
    inv = np.ascontiguousarray(transform.invert.m6(), dtype=np.float64)
    L.fh_turbulence_layer(seed, base_frequency[0], base_frequency[1], tile, octaves, int(fractal), int(stitch_tile is not None), inv,
                          offset[0], offset[1], shape[0], shape[1], out.reshape(-1))
    return out


TRANSFER_TYPES = {"identity": 0, "table": 1, "discrete": 2, "linear": 3, "gamma": 4}
EDGE_MODES = {"duplicate": 0, "wrap": 1, "none": 2}


def transfer_abi(fn):
    """(type, prm (5,), values) of one transfer function, as svgr_layer_component_transfer and the host build take it."""
    prm = np.array([1.0, 0.0, 1.0, 1.0, 0.0])
    kind = "identity" if fn is None else fn[0]
    values = np.zeros(0)
    if kind in ("table", "discrete"):
        values = np.ascontiguousarray(fn[1], dtype=np.float64)
        if values.size == 0:
            kind = "identity"
    elif kind == "linear":
        prm[0:2] = fn[1:3]
    elif kind == "gamma":
        prm[2:5] = fn[1:4]
    return TRANSFER_TYPES[kind], prm, values


def harness_transfer(L, c, fn):
    kind, prm, values = transfer_abi(fn)
    c = np.ascontiguousarray(c, dtype=np.float64).reshape(-1)
    out = np.zeros(c.size)
    L.fh_transfer(c, c.size, kind, prm, values if values.size else np.zeros(1), values.size, out)
    return out


def harness_convolve_matrix(L, image, kernel, divisor, bias, target, edge_mode, preserve_alpha):
    image = np.ascontiguousarray(image, dtype=np.float64)
    kernel = np.ascontiguousarray(kernel, dtype=np.float64)
    out = np.zeros(image.shape)
    L.fh_convolve_matrix(image.reshape(-1), image.shape[0], image.shape[1], kernel.reshape(-1), kernel.shape[1], kernel.shape[0],
                         target[0], target[1], divisor, bias, EDGE_MODES[edge_mode], int(preserve_alpha), out.reshape(-1))
    return out
