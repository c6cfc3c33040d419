"""Isolated groups in differentiable compositing restated in numpy (csrc/svgr_group.h's arithmetic, one operation per line: numpy
fuses nothing), on top of tests/gradpaint_ref.py for the fills, with the rounding bound of the sums whose order an implementation
may choose: every parameter gradient, the opacities' included.

program   items (n_items, 4): {0, p, 0, 0} FILL, {1, its END, 0, 0} BEGIN, {2, its BEGIN, opacity slot or -1, clip or -1} END
forward   FILL: the painted step on the open canvas.  BEGIN: G = 0.  END: k = 1, or m_j0, then m_j + k (1 - m_j);
          S = (G o) k;  X = S + X (1 - S_3)
walk 1    last to first: FILL through = above, above = above u;  END T_end = above, above = 1;
          BEGIN P = above, u_g = 1 - ((1 - P) o) k, above = T_end u_g
walk 2    first to last, X and B per level: FILL as the painted backward with B for the image's gradient;
          BEGIN g = T_end B, gc = g . X, adj = (g_0, g_1, g_2, g_3 - gc), X' = 0, B' = (adj k) o;
          END q = adj . G, d o = sum q k, d k = q o, d m_j = d k ((1 | 1 - k_before) prod_{after} (1 - m_i)), then the forward step"""
from typing import NamedTuple

import numpy as np

from tests import compose_ref as CR
from tests import gradpaint_ref as R

U = CR.U
FILL, BEGIN, END = 0, 1, 2
DEPTH = 4


class GR(NamedTuple):
    """The fields of diff.Groups, on the host."""
    items: np.ndarray        # (n_items, 4) int32
    clip_off: np.ndarray     # (n_clips + 1,) int32
    clip_planes: np.ndarray  # (n_clip_planes,) int32
    opacity: np.ndarray      # (n_opacities,) float64


def _mask(cover, gr, clip):
    """(k, [k before every plane of the clip]) of a clip, or (ones, []) without one."""
    if clip < 0:
        return np.ones(cover.shape[1:]), []
    planes = gr.clip_planes[gr.clip_off[clip]:gr.clip_off[clip + 1]]
    k, before = None, []
    for a, j in enumerate(planes):
        m = cover[j]
        before.append(k)
        if a == 0:
            k = m.copy()
        else:
            t = 1.0 - m
            t = k * t
            k = m + t
    return k, before


def _opacity(gr, slot):
    return 1.0 if slot < 0 else float(gr.opacity[slot])


def _group_step(X, G, o, k):
    S = G * o
    S = S * k[..., None]
    t = 1.0 - S[..., 3:]
    t = X * t
    return S + t


def _fill_step(C, cover, paints, gp, p, origin, fused):
    if gp.kind[p] == 0:
        return CR._step(C, cover[p], paints[p])
    return R._step(C, cover[p], R.colour(gp, p, cover.shape[1], cover.shape[2], origin, fused)[0], paints[p])


def forward(cover, paints, gp, gr, bg=None, origin=(0, 0), fused=True):
    """image (rows, cols, 4)."""
    cover, paints = np.asarray(cover, dtype=np.float64), np.asarray(paints, dtype=np.float64)
    rows, cols = cover.shape[1:]
    X = [CR._canvas(rows, cols, bg)]
    for op, a, slot, clip in np.asarray(gr.items).tolist():
        if op == FILL:
            X[-1] = _fill_step(X[-1], cover, paints, gp, a, origin, fused)
        elif op == BEGIN:
            X.append(np.zeros((rows, cols, 4)))
        else:
            G = X.pop()
            X[-1] = _group_step(X[-1], G, _opacity(gr, slot), _mask(cover, gr, clip)[0])
    assert len(X) == 1
    return X[0]


def backward(cover, paints, gp, gr, grad_image, bg=None, origin=(0, 0), fused=True):
    """(grad_cover, sums, tol): sums and tol are dicts over paints, m6, geom, stop_pos, stop_rgba, opacity; tol bounds what the
    order of a sum can change, n_terms * 2^-53 * sum |terms| per component."""
    cover, paints = np.asarray(cover, dtype=np.float64), np.asarray(paints, dtype=np.float64)
    gi = np.asarray(grad_image, dtype=np.float64)
    n, rows, cols = cover.shape
    items = np.asarray(gr.items).tolist()
    cols_of = {p: R.colour(gp, p, rows, cols, origin, fused) for p in range(n) if gp.kind[p] != 0}
    through, t_end = np.zeros_like(cover), {}
    above = np.ones((rows, cols))
    for q in range(len(items) - 1, -1, -1):
        op, a, slot, clip = items[q]
        if op == FILL:
            through[a] = above
            if gp.kind[a] == 0:
                u = cover[a] * paints[a, 3]
            else:
                u = cols_of[a][0][..., 3] * cover[a]
                u = u * paints[a, 3]
            u = 1.0 - u
            above = above * u
        elif op == END:
            t_end[q] = above
            above = np.ones((rows, cols))
        else:
            _op, _a, slot, clip = items[a]   # (the group's END holds its opacity and clip)
            k = _mask(cover, gr, clip)[0]
            u = 1.0 - above
            u = u * _opacity(gr, slot)
            u = u * k
            u = 1.0 - u
            above = t_end[a] * u
    n_stops, n_op = len(gp.stop_pos), len(gr.opacity)
    sums = dict(paints=np.zeros((n, 4)), m6=np.zeros((n, 6)), geom=np.zeros((n, 4)), stop_pos=np.zeros(n_stops), stop_rgba=np.zeros((n_stops, 4)),
                opacity=np.zeros(n_op))
    tol = {k: np.zeros_like(v) for k, v in sums.items()}
    grad_cover = np.zeros_like(cover)
    n_px = rows * cols

    def add(name, where, terms):
        sums[name][where] = terms.sum(axis=0)
        tol[name][where] = n_px * U * np.abs(terms).sum(axis=0)

    def adjoint(X, T, B):
        g = T[..., None] * B
        gc = CR._dot(g, X)
        return np.stack([g[..., 0], g[..., 1], g[..., 2], g[..., 3] - gc], axis=-1)

    X, B = [CR._canvas(rows, cols, bg)], [gi]
    for q, (op, a, slot, clip) in enumerate(items):
        if op == FILL:
            p, C = a, X[-1]
            g = through[p][..., None] * B[-1]
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
                X[-1] = CR._step(C, m, paints[p])
                continue
            dense, stops = R._vjp(gp, p, col, e, paints[p], t)
            add("paints", p, dense[:, :4])
            add("m6", p, dense[:, 4:10])
            add("geom", p, dense[:, 10:])
            s0, s1 = int(gp.path_stop_off[p]), int(gp.path_stop_off[p + 1])
            add("stop_pos", slice(s0, s1), stops[:, :, 0])
            add("stop_rgba", slice(s0, s1), stops[:, :, 1:])
            X[-1] = R._step(C, m, col, paints[p])
        elif op == BEGIN:
            _op, _a, slot, clip = items[a]
            adj = adjoint(X[-1], t_end[a], B[-1])
            k = _mask(cover, gr, clip)[0]
            b = adj * k[..., None]
            b = b * _opacity(gr, slot)
            X.append(np.zeros((rows, cols, 4)))
            B.append(b)
        else:
            G = X.pop()
            B.pop()
            o = _opacity(gr, slot)
            adj = adjoint(X[-1], t_end[q], B[-1])
            qd = CR._dot(adj, G)
            dk = qd * o
            k, before = _mask(cover, gr, clip)
            if clip >= 0:
                planes = gr.clip_planes[gr.clip_off[clip]:gr.clip_off[clip + 1]]
                suffix, suffixes = np.ones((rows, cols)), [None] * len(planes)
                for pos in range(len(planes) - 1, -1, -1):
                    suffixes[pos] = suffix
                    t = 1.0 - cover[planes[pos]]
                    suffix = suffix * t
                for pos, j in enumerate(planes):
                    pre = 1.0 if pos == 0 else 1.0 - before[pos]
                    t = pre * suffixes[pos]
                    grad_cover[j] = dk * t
            if slot >= 0:
                add("opacity", slot, (qd * k).reshape(-1))
            X[-1] = _group_step(X[-1], G, o, k)
    return grad_cover, sums, tol
