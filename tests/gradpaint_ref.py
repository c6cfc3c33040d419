"""Gradient paints in differentiable compositing restated in numpy (csrc/svgr_gradpaint.h's arithmetic, operation for operation:
numpy fuses nothing, and the header's three fused multiply-adds are tests/paint_ref.py's exact ones), with the rounding bound of
the sums whose order an implementation may choose: every parameter gradient.

point     px = i + (row0 + 0.5), py = j + (col0 + 0.5), x = fma(py, m1, px m0) + m2, y = fma(py, m4, px m3) + m5
offset    linear t = fma(dx, v0, dy v1) / vv;  radial t = sqrt(o0 o0 + o1 o1)
spread    pad, repeat (t - trunc t), reflect (|b - 1|, b = (t + 1) - 2 floor((t + 1) 0.5), slope sigma = +1 where b - 1 >= 0 else -1)
stops     the renderer's three tests; col = 0 + ((1 - ratio) c_s + ratio c_{s+1})
paint     s = (col m) paint, C = s + C (1 - s_3)
backward  the header's comment, line for line.

``fused=False`` replaces the three fma by a product and a sum: one rounding more each.  The central differences use it (they
need a smooth function, not the bits), because the exact fma is a Python-level loop."""
from typing import NamedTuple

import numpy as np

from tests import compose_ref as CR
from tests.paint_ref import fma as _exact_fma

U = CR.U


class GP(NamedTuple):
    """The fields of diff.GradientPaints, on the host."""
    kind: np.ndarray           # (n_paths,) int32: 0 solid, 1 linear, 2 radial
    spread: np.ndarray         # (n_paths,) int32: 0 pad, 1 repeat, 2 reflect
    path_stop_off: np.ndarray  # (n_paths + 1,) int32
    m6: np.ndarray             # (n_paths, 6)
    geom: np.ndarray           # (n_paths, 4)
    stop_pos: np.ndarray       # (n_stops,)
    stop_rgba: np.ndarray      # (n_stops, 4)


PARAMS = ("m6", "geom", "stop_pos", "stop_rgba")


def _fma(a, b, c, fused):
    return _exact_fma(a, b, c) if fused else a * b + c


def colour(gp, p, rows, cols, origin=(0, 0), fused=True):
    """(col (rows, cols, 4), e) of gradient path p: e holds what gradpaint_colour leaves for the backward."""
    m6, geom = gp.m6[p], gp.geom[p]
    s0, s1 = int(gp.path_stop_off[p]), int(gp.path_stop_off[p + 1])
    pos, rgba, n = gp.stop_pos[s0:s1], gp.stop_rgba[s0:s1], s1 - s0
    i, j = np.indices((rows, cols)).astype(np.float64)
    px, py = i + (float(origin[0]) + 0.5), j + (float(origin[1]) + 0.5)
    x = _fma(py, m6[1], px * m6[0], fused) + m6[2]
    y = _fma(py, m6[4], px * m6[3], fused) + m6[5]
    if gp.kind[p] == 1:
        v0, v1 = geom[2] - geom[0], geom[3] - geom[1]
        vv = v0 * v0 + v1 * v1
        a0, a1 = x - geom[0], y - geom[1]
        t = _fma(a0, v0, a1 * v1, fused) / vv
    else:
        a0, a1 = (x - geom[0]) / geom[2], (y - geom[1]) / geom[2]
        t = np.sqrt(a0 * a0 + a1 * a1)
    sigma, u = np.ones_like(t), t
    if gp.spread[p] == 1:
        with np.errstate(invalid="ignore"):
            u = np.where(np.isinf(t), np.copysign(0.0, t), t - np.trunc(t))
    elif gp.spread[p] == 2:
        a = t + 1.0
        b = (a - 2.0 * np.floor(a * 0.5)) - 1.0
        sigma, u = np.where(b >= 0.0, 1.0, -1.0), np.fabs(b)
    col = np.zeros((rows, cols, 4))
    lo, hi, ratio = np.full(t.shape, -1), np.full(t.shape, -1), np.zeros_like(t)
    sel = u <= pos[0]
    col[sel], lo[sel], hi[sel] = rgba[0], 0, 0
    sel = u > pos[n - 1]
    col[sel], lo[sel], hi[sel] = rgba[n - 1], n - 1, n - 1
    for s in range(n - 1):
        o0, o1 = pos[s], pos[s + 1]
        sel = np.logical_and(u > o0, u <= o1)
        if sel.any():
            r = (u[sel] - o0) / (o1 - o0)
            col[sel] = col[sel] + ((1 - r)[:, None] * rgba[s] + r[:, None] * rgba[s + 1])
            lo[sel], hi[sel], ratio[sel] = s, s + 1, r
    return col, dict(px=px, py=py, t=t, u=u, sigma=sigma, a0=a0, a1=a1, ratio=ratio, lo=lo, hi=hi)


def _step(C, m, col, paint):
    s = (col * m[..., None]) * paint
    return s + C * (1.0 - s[..., 3:])


def forward(cover, paints, gp, bg=None, origin=(0, 0), fused=True):
    """image (rows, cols, 4)."""
    cover, paints = np.asarray(cover, dtype=np.float64), np.asarray(paints, dtype=np.float64)
    C = CR._canvas(cover.shape[1], cover.shape[2], bg)
    for p in range(len(cover)):
        if gp.kind[p] == 0:
            C = CR._step(C, cover[p], paints[p])
        else:
            C = _step(C, cover[p], colour(gp, p, cover.shape[1], cover.shape[2], origin, fused)[0], paints[p])
    return C


def offsets(gp, p, rows, cols, origin=(0, 0)):
    """(t before the spread, u after it) of gradient path p, for the case builders' distance conditions."""
    e = colour(gp, p, rows, cols, origin, fused=False)[1]
    return e["t"], e["u"]


def _vjp(gp, p, col, e, paint, t):
    """(dense (n_px, 14), stops (n_px, n, 5)): gradpaint_vjp over every pixel of path p; t is (rows, cols, 4)."""
    geom = gp.geom[p]
    s0, s1 = int(gp.path_stop_off[p]), int(gp.path_stop_off[p + 1])
    pos, rgba, n = gp.stop_pos[s0:s1], gp.stop_rgba[s0:s1], s1 - s0
    shape = e["t"].shape
    dense, stops = np.zeros(shape + (14,)), np.zeros(shape + (n, 5))
    dense[..., :4] = t * col
    q = t * paint
    lo, hi, ratio = e["lo"], e["hi"], e["ratio"]
    clamp, seg = np.logical_and(lo >= 0, lo == hi), np.logical_and(lo >= 0, lo != hi)
    for s in range(n):
        at = np.logical_and(clamp, lo == s)
        stops[at, s, 1:] = q[at]
    for s in range(n - 1):
        at = np.logical_and(seg, lo == s)
        if not at.any():
            continue
        r, qq = ratio[at], q[at]
        w0 = 1 - r
        stops[at, s, 1:] = qq * w0[:, None]
        stops[at, s + 1, 1:] = qq * r[:, None]
        d = rgba[s + 1] - rgba[s]
        D = ((qq[:, 0] * d[0] + qq[:, 1] * d[1]) + qq[:, 2] * d[2]) + qq[:, 3] * d[3]
        E = D / (pos[s + 1] - pos[s])
        stops[at, s, 0] = -(w0 * E)
        stops[at, s + 1, 0] = -(r * E)
        a = e["sigma"][at] * E
        tt, a0, a1 = e["t"][at], e["a0"][at], e["a1"][at]
        g = np.zeros((len(a), 14))
        if gp.kind[p] == 1:
            v0, v1 = geom[2] - geom[0], geom[3] - geom[1]
            vv = v0 * v0 + v1 * v1
            t2 = 2.0 * tt
            gx, gy = a * (v0 / vv), a * (v1 / vv)
            g[:, 12] = a * ((a0 - t2 * v0) / vv)
            g[:, 13] = a * ((a1 - t2 * v1) / vv)
            g[:, 10] = -(gx + g[:, 12])
            g[:, 11] = -(gy + g[:, 13])
        else:
            ok = tt != 0.0
            rt = np.where(ok, geom[2] * tt, 1.0)
            gx, gy = np.where(ok, a * (a0 / rt), 0.0), np.where(ok, a * (a1 / rt), 0.0)
            g[:, 10], g[:, 11] = -gx, -gy
            g[:, 12] = np.where(ok, -(a * (tt / geom[2])), 0.0)
        px, py = e["px"][at], e["py"][at]
        g[:, 4], g[:, 5], g[:, 6], g[:, 7], g[:, 8], g[:, 9] = gx * px, gx * py, gx, gy * px, gy * py, gy
        dense[at, 4:] = g[:, 4:]
    return dense.reshape(-1, 14), stops.reshape(-1, n, 5)


def backward(cover, paints, gp, grad_image, bg=None, origin=(0, 0), fused=True):
    """(grad_cover, sums, tol): sums and tol are dicts over paints, m6, geom, stop_pos, stop_rgba; tol bounds what the order of a
    sum can change, n_terms * 2^-53 * sum |terms| per component (a pixel that does not touch a stop is a term of 0)."""
    cover, paints = np.asarray(cover, dtype=np.float64), np.asarray(paints, dtype=np.float64)
    gi = np.asarray(grad_image, dtype=np.float64)
    n, rows, cols = cover.shape
    cols_of = {p: colour(gp, p, rows, cols, origin, fused) for p in range(n) if gp.kind[p] != 0}
    through = np.empty_like(cover)
    above = np.ones((rows, cols))
    for p in range(n - 1, -1, -1):
        through[p] = above
        if gp.kind[p] == 0:
            above = above * (1.0 - cover[p] * paints[p, 3])
        else:
            above = above * (1.0 - (cols_of[p][0][..., 3] * cover[p]) * paints[p, 3])
    n_stops = len(gp.stop_pos)
    sums = dict(paints=np.zeros((n, 4)), m6=np.zeros((n, 6)), geom=np.zeros((n, 4)), stop_pos=np.zeros(n_stops), stop_rgba=np.zeros((n_stops, 4)))
    tol = {k: np.zeros_like(v) for k, v in sums.items()}
    grad_cover = np.empty_like(cover)
    C = CR._canvas(rows, cols, bg)
    n_px = rows * cols

    def add(name, where, terms):
        sums[name][where] = terms.sum(axis=0)
        tol[name][where] = n_px * U * np.abs(terms).sum(axis=0)

    for p in range(n):
        g = through[p][..., None] * gi
        gc = CR._dot(g, C)
        m = cover[p]
        if gp.kind[p] == 0:
            P = paints[p]
        else:
            col, e = cols_of[p]
            P = col * paints[p]
        gp_dot = CR._dot(g, P)
        grad_cover[p] = gp_dot - P[..., 3] * gc
        t = np.stack([m * g[..., 0], m * g[..., 1], m * g[..., 2], m * (g[..., 3] - gc)], axis=-1)
        if gp.kind[p] == 0:
            add("paints", p, t.reshape(-1, 4))
            C = CR._step(C, m, paints[p])
            continue
        dense, stops = _vjp(gp, p, col, e, paints[p], t)
        add("paints", p, dense[:, :4])
        add("m6", p, dense[:, 4:10])
        add("geom", p, dense[:, 10:])
        s0, s1 = int(gp.path_stop_off[p]), int(gp.path_stop_off[p + 1])
        add("stop_pos", slice(s0, s1), stops[:, :, 0])
        add("stop_rgba", slice(s0, s1), stops[:, :, 1:])
        C = _step(C, m, col, paints[p])
    return grad_cover, sums, tol
