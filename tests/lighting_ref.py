"""numpy restatement of feDiffuseLighting / feSpecularLighting, written from the Filter Effects text in the operation order of
csrc/svgr_core.h (light_normal, light_pixel), plus the spec's Sobel table as printed, the mapping of a light source to the device
frame, and the loader for the host build of the arithmetic (tests/lighting_harness.cpp).  Test infrastructure only."""
import ctypes as C
import math

import numpy as np

from tests.util import host_build

DISTANT, POINT, SPOT = 0, 1, 2

# Filter Effects 1's Sobel table, keyed by (row place, column place) with places -1 first, 0 inside, 1 last: (FACTOR1, K1) along
# the columns (the spec's x) and (FACTOR0, K0) along the rows (the spec's y); kernels row by row, top (d0 - 1) to bottom.
SOBEL = {
    (-1, -1): ((2 / 3, [[0, 0, 0], [0, -2, 2], [0, -1, 1]]), (2 / 3, [[0, 0, 0], [0, -2, -1], [0, 2, 1]])),
    (-1, 0): ((1 / 3, [[0, 0, 0], [-2, 0, 2], [-1, 0, 1]]), (1 / 2, [[0, 0, 0], [-1, -2, -1], [1, 2, 1]])),
    (-1, 1): ((2 / 3, [[0, 0, 0], [-2, 2, 0], [-1, 1, 0]]), (2 / 3, [[0, 0, 0], [-1, -2, 0], [1, 2, 0]])),
    (0, -1): ((1 / 2, [[0, -1, 1], [0, -2, 2], [0, -1, 1]]), (1 / 3, [[0, -2, -1], [0, 0, 0], [0, 2, 1]])),
    (0, 0): ((1 / 4, [[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]]), (1 / 4, [[-1, -2, -1], [0, 0, 0], [1, 2, 1]])),
    (0, 1): ((1 / 2, [[-1, 1, 0], [-2, 2, 0], [-1, 1, 0]]), (1 / 3, [[-1, -2, 0], [0, 0, 0], [1, 2, 0]])),
    (1, -1): ((2 / 3, [[0, -1, 1], [0, -2, 2], [0, 0, 0]]), (2 / 3, [[0, -2, -1], [0, 2, 1], [0, 0, 0]])),
    (1, 0): ((1 / 3, [[-1, 0, 1], [-2, 0, 2], [0, 0, 0]]), (1 / 2, [[-1, -2, -1], [1, 2, 1], [0, 0, 0]])),
    (1, 1): ((2 / 3, [[-1, 1, 0], [-2, 2, 0], [0, 0, 0]]), (2 / 3, [[-1, -2, 0], [1, 2, 0], [0, 0, 0]])),
}


def table_normal(a9, place, ss):
    """N of the spec's table for a 3 x 3 neighbourhood (summed as printed, not in the kernel's order)."""
    (f1, k1), (f0, k0) = SOBEL[place]
    a = np.asarray(a9, dtype=np.float64).reshape(3, 3)
    n = np.array([-ss * f0 * (np.array(k0) * a).sum(), -ss * f1 * (np.array(k1) * a).sum(), 1.0])
    return n / np.linalg.norm(n)


def light_frame(transform, kind, light):
    """(params (8,)) of a light in the device frame, from the issue's mapping: positions (transform(x, y), z sqrt|det M|), a
    distant light (v / |v| cos el, sin el) with v = M (cos az, sin az), spot S = normalize(pointsAt - position)."""
    m = np.asarray(transform.m, dtype=np.float64)[:2, :2]
    s = math.sqrt(abs(m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]))
    p = np.zeros(8)
    if kind == DISTANT:
        az, el = math.radians(light[0]), math.radians(light[1])
        v = m @ np.array([math.cos(az), math.sin(az)])
        n = math.sqrt(v[0] * v[0] + v[1] * v[1])
        p[0:2] = v / n * math.cos(el)
        p[2] = math.sin(el)
        return p
    p[0:2] = transform(np.array([float(light[0]), float(light[1])]))
    p[2] = float(light[2]) * s
    if kind == SPOT:
        at = np.array([*transform(np.array([float(light[3]), float(light[4])])), float(light[5]) * s])
        d = at - p[0:3]
        n = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
        if n > 0:   # (a spot that points at its own position has no direction: S = 0, and it lights nothing)
            p[3:6] = d / n
        p[6] = float(light[6])
        p[7] = -1.0 if light[7] is None else math.cos(math.radians(abs(float(light[7]))))
    return p


def region_alpha(src_image, src_offset, offset, shape):
    """The alpha of `src_image` (at `src_offset`) over the region (offset, shape), zero where the source has no pixel."""
    out = np.zeros(shape)
    r0, c0 = src_offset[0] - offset[0], src_offset[1] - offset[1]
    sr, sc = src_image.shape[:2]
    lo0, lo1 = max(r0, 0), max(c0, 0)
    hi0, hi1 = min(r0 + sr, shape[0]), min(c0 + sc, shape[1])
    if lo0 < hi0 and lo1 < hi1:
        out[lo0:hi0, lo1:hi1] = src_image[lo0 - r0: hi0 - r0, lo1 - c0: hi1 - c0, 3]
    return out


def normals(A, ss):
    """(n0, n1, n2) per pixel of the region alpha A, in light_normal's order."""
    rows, cols = A.shape
    P = np.zeros((rows + 2, cols + 2))
    P[1:-1, 1:-1] = A
    R, Cc = np.indices((rows, cols))
    top, bottom, left, right = R == 0, R == rows - 1, Cc == 0, Cc == cols - 1

    def a(k, j):
        return P[R + k, Cc + j]

    r_lo, r_hi = np.where(top, 1, 0), np.where(bottom, 1, 2)
    c_lo, c_hi = np.where(left, 1, 0), np.where(right, 1, 2)
    wt, wb = np.where(top, 0.0, 1.0), np.where(bottom, 0.0, 1.0)
    wl, wr = np.where(left, 0.0, 1.0), np.where(right, 0.0, 1.0)
    g0 = wl * (a(r_hi, 0) - a(r_lo, 0)) + 2.0 * (a(r_hi, 1) - a(r_lo, 1)) + wr * (a(r_hi, 2) - a(r_lo, 2))
    g1 = wt * (a(0, c_hi) - a(0, c_lo)) + 2.0 * (a(1, c_hi) - a(1, c_lo)) + wb * (a(2, c_hi) - a(2, c_lo))
    with np.errstate(invalid="ignore", divide="ignore"):   # (a span of 0: a one-row or one-column region, flat below)
        f0 = 2.0 / ((wl + 2.0 + wr) * (r_hi - r_lo).astype(np.float64))
        f1 = 2.0 / ((wt + 2.0 + wb) * (c_hi - c_lo).astype(np.float64))
        n0, n1 = -ss * f0 * g0, -ss * f1 * g1
        length = np.sqrt(n0 * n0 + n1 * n1 + 1.0)
        n = [n0 / length, n1 / length, 1.0 / length]
    flat = (top & bottom) | (left & right)
    return [np.where(flat, v, x) for v, x in zip((0.0, 0.0, 1.0), n)]


def lighting(A, offset, kind, params, color, ss, constant, se=None):
    """The (rows, cols, 4) result over the region at `offset` whose alpha is A; `se` None = diffuse."""
    rows, cols = A.shape
    with np.errstate(invalid="ignore", over="ignore"):
        n0, n1, n2 = normals(A, ss)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if kind == DISTANT:
            l0, l1, l2 = (np.full((rows, cols), params[k]) for k in range(3))
        else:
            R, Cc = np.indices((rows, cols))
            d0, d1 = (offset[0] + R).astype(np.float64) + 0.5, (offset[1] + Cc).astype(np.float64) + 0.5
            v0, v1, v2 = params[0] - d0, params[1] - d1, params[2] - ss * A
            length = np.sqrt(v0 * v0 + v1 * v1 + v2 * v2)
            ok = length > 0.0
            l0, l1, l2 = np.where(ok, v0 / length, 0.0), np.where(ok, v1 / length, 0.0), np.where(ok, v2 / length, 1.0)
        c = [np.full((rows, cols), float(color[k])) for k in range(3)]
        if kind == SPOT:
            m = -(l0 * params[3] + l1 * params[4] + l2 * params[5])
            on = (m > 0.0) & (m >= params[7])
            f = np.power(np.where(on, m, 1.0), params[6])
            c = [np.where(on, ck * f, 0.0) for ck in c]
        if se is not None:
            h0, h1, h2 = l0, l1, l2 + 1.0
            length = np.sqrt(h0 * h0 + h1 * h1 + h2 * h2)
            nh = np.where(length > 0.0, n0 * (h0 / length) + n1 * (h1 / length) + n2 * (h2 / length), 0.0)
            nh = np.where(nh > 0.0, nh, 0.0)
            k = constant * np.power(nh, se)
        else:
            nl = n0 * l0 + n1 * l1 + n2 * l2
            k = constant * np.where(nl > 0.0, nl, 0.0)
    with np.errstate(invalid="ignore", over="ignore"):   # (NaN -> 0, as svgr_core.h's clamp_unit: a NaN alpha ends as 0)
        rgb = [np.where(k * ck > 0.0, np.where(k * ck < 1.0, k * ck, 1.0), 0.0) for ck in c]
    alpha = np.maximum(np.maximum(rgb[0], rgb[1]), rgb[2]) if se is not None else np.ones((rows, cols))
    return np.stack([*rgb, alpha], axis=-1)


# -- the host build of svgr_core.h's lighting arithmetic ---------------------------------------------------------------------
def harness():
    L = host_build("lighting_harness")
    f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
    L.lh_normal.argtypes = [f64p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, f64p]
    L.lh_layer.argtypes = [C.c_int, f64p, f64p, C.c_double, C.c_double, C.c_double, C.c_int, C.c_long, C.c_long, C.c_long, C.c_long,
                           f64p, f64p]
    return L


def harness_normal(L, a9, top, bottom, left, right, ss):
    n = np.zeros(3)
    L.lh_normal(np.ascontiguousarray(a9, dtype=np.float64).reshape(9), int(top), int(bottom), int(left), int(right), ss, n)
    return n


def harness_layer(L, A, offset, kind, params, color, ss, constant, se=None):
    rows, cols = A.shape
    out = np.zeros((rows, cols, 4))
    L.lh_layer(kind, np.ascontiguousarray(params, dtype=np.float64), np.ascontiguousarray(color, dtype=np.float64), ss, constant,
               1.0 if se is None else se, int(se is not None), offset[0], offset[1], rows, cols,
               np.ascontiguousarray(A, dtype=np.float64), out.reshape(-1))
    return out
