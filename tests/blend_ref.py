"""Numpy restatement of CSS mix-blend-mode (W3C Compositing and Blending Level 1, section 5) for the tests: the blend functions
B(Cb, Cs) of the 16 modes, one premultiplied pixel of a source over a backdrop, and whole layers zero-extended to the union of their
boxes.  Operations are written in the order of csrc/svgr_core.h (mix_blend_px), so that the host build (tests/blend_harness.cpp)
and the kernel can be compared with it bit for bit.  Test infrastructure only."""
import ctypes as C

import numpy as np

from tests.util import host_build

MODES = ["normal", "multiply", "screen", "overlay", "darken", "lighten", "color-dodge", "color-burn", "hard-light", "soft-light",
         "difference", "exclusion", "hue", "saturation", "color", "luminosity"]
CODE = {name: i for i, name in enumerate(MODES)}
NONSEP = {"hue", "saturation", "color", "luminosity"}


def blend_sep(mode: str, b, s):
    """B(Cb, Cs) of a separable mode, elementwise."""
    b, s = np.asarray(b, dtype=np.float64), np.asarray(s, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        if mode == "normal":
            return s.copy()
        if mode == "multiply":
            return b * s
        if mode == "screen":
            return b + s - b * s
        if mode == "overlay":   # HardLight(Cs, Cb)
            b2 = 2.0 * b
            return np.where(b <= 0.5, s * b2, s + (b2 - 1.0) - s * (b2 - 1.0))
        if mode == "darken":
            return np.where(b < s, b, s)
        if mode == "lighten":
            return np.where(b > s, b, s)
        if mode == "color-dodge":
            q = b / (1.0 - s)
            return np.where(b == 0.0, 0.0, np.where(s == 1.0, 1.0, np.where(q < 1.0, q, 1.0)))
        if mode == "color-burn":
            q = (1.0 - b) / s
            return np.where(b == 1.0, 1.0, np.where(s == 0.0, 0.0, 1.0 - np.where(q < 1.0, q, 1.0)))
        if mode == "hard-light":
            s2 = 2.0 * s
            return np.where(s <= 0.5, b * s2, b + (s2 - 1.0) - b * (s2 - 1.0))
        if mode == "soft-light":
            d = np.where(b <= 0.25, ((16.0 * b - 12.0) * b + 4.0) * b, np.sqrt(np.maximum(b, 0.0)))
            return np.where(s <= 0.5, b - (1.0 - 2.0 * s) * b * (1.0 - b), b + (2.0 * s - 1.0) * (d - b))
        if mode == "difference":
            return np.where(b > s, b - s, s - b)
        if mode == "exclusion":
            return b + s - 2.0 * b * s
    raise ValueError(mode)


def lum(c):
    c = np.asarray(c, dtype=np.float64)
    return 0.3 * c[..., 0] + 0.59 * c[..., 1] + 0.11 * c[..., 2]


def clip_color(c):
    c = np.array(c, dtype=np.float64)
    L = lum(c)[..., None]
    n = c.min(axis=-1)[..., None]
    x = c.max(axis=-1)[..., None]
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.where((n < 0.0) & (L - n > 0.0), L + ((c - L) * L) / (L - n), c)
        c = np.where((x > 1.0) & (x - L > 0.0), L + ((c - L) * (1.0 - L)) / (x - L), c)
    return c


def set_lum(c, l):
    c = np.asarray(c, dtype=np.float64)
    d = (np.asarray(l, dtype=np.float64) - lum(c))[..., None]
    return clip_color(c + d)


def sat(c):
    c = np.asarray(c, dtype=np.float64)
    return c.max(axis=-1) - c.min(axis=-1)


def set_sat(c, s):
    c = np.asarray(c, dtype=np.float64)
    n = c.min(axis=-1)[..., None]
    x = c.max(axis=-1)[..., None]
    s = np.asarray(s, dtype=np.float64)[..., None]
    with np.errstate(divide="ignore", invalid="ignore"):
        mid = ((c - n) * s) / (x - n)
    return np.where(x <= n, 0.0, np.where(c == x, s, np.where(c == n, 0.0, mid)))


def blend_nonsep(mode: str, cb, cs):
    cb, cs = np.asarray(cb, dtype=np.float64), np.asarray(cs, dtype=np.float64)
    if mode == "hue":
        return set_lum(set_sat(cs, sat(cb)), lum(cb))
    if mode == "saturation":
        return set_lum(set_sat(cb, sat(cs)), lum(cb))
    if mode == "color":
        return set_lum(cs, lum(cb))
    if mode == "luminosity":
        return set_lum(cb, lum(cs))
    raise ValueError(mode)


def blend(mode: str, cb, cs):
    """B(Cb, Cs) on straight colours (..., 3)."""
    return blend_nonsep(mode, cb, cs) if mode in NONSEP else blend_sep(mode, cb, cs)


def mix_blend_px(mode: str, d, s):
    """Premultiplied pixels (..., 4): the source `s` blended over the backdrop `d`."""
    d, s = np.asarray(d, dtype=np.float64), np.asarray(s, dtype=np.float64)
    ab, as_ = d[..., 3:4], s[..., 3:4]
    ka = 1.0 - as_
    out = np.empty(np.broadcast_shapes(d.shape, s.shape))
    if mode == "normal":   # source-over
        out[..., :3] = s[..., :3] + d[..., :3] * ka
    else:
        with np.errstate(divide="ignore", invalid="ignore"):
            cb = np.where(ab > 0.0, d[..., :3] / ab, 0.0)
            cs = np.where(as_ > 0.0, s[..., :3] / as_, 0.0)
        B = blend(mode, cb, cs)
        out[..., :3] = (s[..., :3] * (1.0 - ab) + d[..., :3] * ka) + (as_ * ab) * B
    out[..., 3:4] = as_ + ab * ka
    return out


def _rgba(img):
    img = np.asarray(img, dtype=np.float64)
    return np.repeat(img, 4, axis=2) if img.shape[2] == 1 else img


def mix_blend_layers(mode: str, b_img, b_off, s_img, s_off, px=None):
    """(image, offset) of the source layer blended over the backdrop layer (premultiplied, 1 or 4 channels, zero outside their
    boxes) on the union of the boxes; `px(mode, d, s)` is the per-pixel function (default: `mix_blend_px`)."""
    px = mix_blend_px if px is None else px
    b_img, s_img = _rgba(b_img), _rgba(s_img)
    r0, c0 = min(b_off[0], s_off[0]), min(b_off[1], s_off[1])
    r1 = max(b_off[0] + b_img.shape[0], s_off[0] + s_img.shape[0])
    c1 = max(b_off[1] + b_img.shape[1], s_off[1] + s_img.shape[1])
    out = np.zeros((r1 - r0, c1 - c0, 4))
    br, bc = b_off[0] - r0, b_off[1] - c0
    out[br:br + b_img.shape[0], bc:bc + b_img.shape[1]] = b_img
    sr, sc = s_off[0] - r0, s_off[1] - c0
    win = out[sr:sr + s_img.shape[0], sc:sc + s_img.shape[1]]
    win[...] = px(mode, win.reshape(-1, 4), s_img.reshape(-1, 4)).reshape(win.shape)
    return out, (r0, c0)


# -- the host build of svgr_core.h's blend arithmetic ----------------------------------------------------------------------
def harness():
    L = host_build("blend_harness")
    f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
    L.bh_px.argtypes = [C.c_int, C.c_long, f64p, f64p, f64p]
    L.bh_b.argtypes = [C.c_int, C.c_long, f64p, f64p, f64p]
    return L


def harness_px(L, mode: str, d, s):
    d = np.ascontiguousarray(np.broadcast_to(d, np.broadcast_shapes(np.shape(d), np.shape(s))), dtype=np.float64).reshape(-1, 4)
    s = np.ascontiguousarray(np.broadcast_to(s, np.broadcast_shapes(np.shape(d), np.shape(s))), dtype=np.float64).reshape(-1, 4)
    out = np.zeros_like(d)
    L.bh_px(CODE[mode], len(d), d, s, out)
    return out


def harness_b(L, mode: str, cb, cs):
    cb = np.ascontiguousarray(cb, dtype=np.float64).reshape(-1, 3)
    cs = np.ascontiguousarray(cs, dtype=np.float64).reshape(-1, 3)
    out = np.zeros_like(cb)
    L.bh_b(CODE[mode], len(cb), cb, cs, out)
    return out


def premultiplied_grid(seed: int = 7, n: int = 4096):
    """Premultiplied RGBA test pixels: random ones plus alpha exactly 0 and 1 and channels exactly 0, 0.25, 0.5 and 1 (the
    branches of dodge, burn, soft-light and hard-light)."""
    rng = np.random.default_rng(seed)
    straight = rng.random((n, 4))
    special = np.array([0.0, 0.25, 0.5, 1.0])
    k = n // 4
    straight[:k, :3] = rng.choice(special, (k, 3))
    straight[k:2 * k, 3] = rng.choice([0.0, 1.0], k)
    straight[2 * k:3 * k, :3] = rng.choice(special, (k, 3))
    straight[2 * k:3 * k, 3] = 1.0
    pre = straight.copy()
    pre[:, :3] *= pre[:, 3:4]
    return pre
