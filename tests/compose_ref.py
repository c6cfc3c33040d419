"""Differentiable compositing restated in numpy (csrc/svgr_compose.h's arithmetic, operation for operation: numpy fuses nothing),
with the rounding bound of the one sum whose order an implementation may choose, the paint gradient's.

forward   C = bg; for p in paint order: s = m_p paint_p, C = s + C (1 - s_3)
backward  u_p = 1 - m_p a_p, T_p = prod_{q > p} u_q, g = T_p grad_image, C_{p-1} the canvas under path p:
            d / d m_p          = g . paint_p - a_p (g . C_{p-1})
            d / d paint_p[k<3] = sum over pixels of m_p g_k
            d / d paint_p[3]   = sum over pixels of m_p (g_3 - g . C_{p-1})
          with g . x = ((g_0 x_0 + g_1 x_1) + g_2 x_2) + g_3 x_3.
"""
import numpy as np

U = 2.0 ** -53   # unit round-off of a double


def _canvas(rows, cols, bg):
    C = np.zeros((rows, cols, 4))
    if bg is not None:
        C[...] = np.asarray(bg, dtype=np.float64)
    return C


def _step(C, m, paint):
    s = m[..., None] * paint
    return s + C * (1.0 - s[..., 3:])


def _dot(g, x):
    x = np.broadcast_to(x, g.shape)
    return ((g[..., 0] * x[..., 0] + g[..., 1] * x[..., 1]) + g[..., 2] * x[..., 2]) + g[..., 3] * x[..., 3]


def forward(cover, paints, bg=None):
    """image (rows, cols, 4) of cover (n_paths, rows, cols) and paints (n_paths, 4)."""
    cover, paints = np.asarray(cover, dtype=np.float64), np.asarray(paints, dtype=np.float64)
    C = _canvas(cover.shape[1], cover.shape[2], bg)
    for p in range(len(cover)):
        C = _step(C, cover[p], paints[p])
    return C


def backward(cover, paints, grad_image, bg=None):
    """(grad_cover, grad_paints, tol_paints): tol_paints bounds what the order of a paint sum can change,
    n_terms * 2^-53 * sum |terms| per (path, channel)."""
    cover, paints = np.asarray(cover, dtype=np.float64), np.asarray(paints, dtype=np.float64)
    gi = np.asarray(grad_image, dtype=np.float64)
    n, rows, cols = cover.shape
    through = np.empty_like(cover)
    above = np.ones((rows, cols))
    for p in range(n - 1, -1, -1):
        through[p] = above
        above = above * (1.0 - cover[p] * paints[p, 3])
    grad_cover, grad_paints, tol = np.empty_like(cover), np.zeros((n, 4)), np.zeros((n, 4))
    C = _canvas(rows, cols, bg)
    for p in range(n):
        g = through[p][..., None] * gi
        gc, gp = _dot(g, C), _dot(g, paints[p])
        grad_cover[p] = gp - paints[p, 3] * gc
        m = cover[p]
        terms = np.stack([m * g[..., 0], m * g[..., 1], m * g[..., 2], m * (g[..., 3] - gc)], axis=-1).reshape(-1, 4)
        grad_paints[p] = terms.sum(axis=0)
        tol[p] = len(terms) * U * np.abs(terms).sum(axis=0)
        C = _step(C, m, paints[p])
    return grad_cover, grad_paints, tol
