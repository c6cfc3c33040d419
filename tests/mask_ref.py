"""Luminance-masked groups in differentiable compositing restated in numpy (csrc/svgr_mask.h's arithmetic, one operation per line:
numpy fuses nothing; the two fused multiply-adds of the luminance are tests.paint_ref.fma, exact), on top of tests/group_ref.py,
with the rounding bound of the sums whose order an implementation may choose.

program   group_ref's items, and {1, its closer, 0, 0} BEGIN with the closer an END, a HOLD or an END_MASK,
          {3, its BEGIN, opacity slot or -1, clip or -1} HOLD, {4, its BEGIN, 0, 0} END_MASK; the BEGIN after a HOLD opens its mask
value     al = M_3;  r_c = M_c / al where al > 0.0001, else M_c;  x_c = clip01(r_c);  a = clip01(al);
          lum = fma(x_2, 0.072, fma(x_1, 0.7154, x_0 * 0.2125));  k = lum a
          s_c = w_c a where 0 <= r_c <= 1, else 0;  dk/dM_c = s_c / al where al > 0.0001, else s_c;
          dk/dM_3 = (lum where 0 <= al <= 1, else 0) - (((s_0 r_0 + s_1 r_1) + s_2 r_2) / al where al > 0.0001, else 0)
forward   HOLD: H = (G o) k_clip.  END_MASK: S = H k_mask;  X = S + X (1 - S_3)
walk 0    the forward, keeping M of every pair
walk 1    END_MASK T_end[target] = above, above = 1;  HOLD above = 1;
          BEGIN of a held target P = above, u_g = 1 - (((1 - P) o) k_clip) k_mask, above = T_end u_g
walk 2    BEGIN of a held target B' = ((adj k_clip) k_mask) o;  HOLD q = adj . G, d o = sum (q k_clip) k_mask,
          d k_clip = (q o) k_mask, qok = (q o) k_clip;  BEGIN of a mask B' = qok dk/dM;  END_MASK the forward step"""
import numpy as np

from tests import compose_ref as CR
from tests import gradpaint_ref as R
from tests import group_ref as GRF
from tests.group_ref import GR  # noqa: F401
from tests.paint_ref import fma as _exact_fma

U = CR.U
FILL, BEGIN, END, HOLD, END_MASK = 0, 1, 2, 3, 4
DEPTH = 4
ALPHA_MIN = 0.0001
W = (0.2125, 0.7154, 0.072)


def _fma(a, b, c, fused):
    return _exact_fma(a, b, c) if fused else a * b + c


def _clip01(x):
    return np.where(x < 0, 0.0, np.where(x > 1, 1.0, x))


def _in01(x):
    return (x >= 0) & (x <= 1)


def _straight(M):
    """(r (..., 3), al, divide)."""
    M = np.asarray(M, dtype=np.float64)
    al = M[..., 3]
    divide = al > ALPHA_MIN
    r = M[..., :3] / np.where(divide, al, 1.0)[..., None]   # (x / 1 is x)
    return r, al, divide


def _lum(r, fused):
    x = _clip01(r)
    t = x[..., 0] * W[0]
    t = _fma(x[..., 1], np.float64(W[1]), t, fused)
    return _fma(x[..., 2], np.float64(W[2]), t, fused)


def mask_value(M, fused=True):
    r, al, _divide = _straight(M)
    return _lum(r, fused) * _clip01(al)


def mask_value_vjp(M, fused=True):
    """dk/dM (..., 4)."""
    r, al, divide = _straight(M)
    lum = _lum(r, fused)
    a = _clip01(al)
    s = [np.where(_in01(r[..., c]), W[c] * a, 0.0) for c in range(3)]
    top = np.where(_in01(al), lum, 0.0)
    safe = np.where(divide, al, 1.0)
    t = s[0] * r[..., 0] + s[1] * r[..., 1]
    t = t + s[2] * r[..., 2]
    t = t / safe
    last = np.where(divide, top - t, top)
    return np.stack([s[0] / safe, s[1] / safe, s[2] / safe, last], axis=-1)


def _over(X, S):
    t = 1.0 - S[..., 3:]
    t = X * t
    return S + t


def _hold(G, o, k):
    S = G * o
    return S * k[..., None]


def forward(cover, paints, gp, gr, bg=None, origin=(0, 0), fused=True, parked=None):
    """image (rows, cols, 4); parked, a dict, gets M per END_MASK item."""
    cover, paints = np.asarray(cover, dtype=np.float64), np.asarray(paints, dtype=np.float64)
    rows, cols = cover.shape[1:]
    X, held = [CR._canvas(rows, cols, bg)], {}
    for q, (op, a, slot, clip) in enumerate(np.asarray(gr.items).tolist()):
        if op == FILL:
            X[-1] = GRF._fill_step(X[-1], cover, paints, gp, a, origin, fused)
        elif op == BEGIN:
            X.append(np.zeros((rows, cols, 4)))
        elif op == END:
            G = X.pop()
            X[-1] = GRF._group_step(X[-1], G, GRF._opacity(gr, slot), GRF._mask(cover, gr, clip)[0])
        elif op == HOLD:
            G = X.pop()
            held[len(X)] = _hold(G, GRF._opacity(gr, slot), GRF._mask(cover, gr, clip)[0])
        else:
            M = X.pop()
            if parked is not None:
                parked[q] = M
            S = held.pop(len(X)) * mask_value(M, fused)[..., None]
            X[-1] = _over(X[-1], S)
    assert len(X) == 1 and not held
    return X[0]


def backward(cover, paints, gp, gr, grad_image, bg=None, origin=(0, 0), fused=True):
    """(grad_cover, sums, tol): group_ref.backward's."""
    cover, paints = np.asarray(cover, dtype=np.float64), np.asarray(paints, dtype=np.float64)
    gi = np.asarray(grad_image, dtype=np.float64)
    n, rows, cols = cover.shape
    items = np.asarray(gr.items).tolist()
    parked = {}
    forward(cover, paints, gp, gr, bg, origin, fused, parked)
    # per HOLD item: k_mask and dk/dM of its pair (the mask's BEGIN follows the HOLD and names its END_MASK)
    k_mask = {h: mask_value(parked[items[h + 1][1]], fused) for h, it in enumerate(items) if it[0] == HOLD}
    dk_dm = {h: mask_value_vjp(parked[items[h + 1][1]], fused) for h in k_mask}
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
        elif op == END_MASK:
            t_end[a - 1] = above   # (of the pair's target: its HOLD sits before the mask's BEGIN)
            above = np.ones((rows, cols))
        elif op == HOLD:
            above = np.ones((rows, cols))
        else:
            closer, _a, slot, clip = items[a]
            if closer == END_MASK:
                continue
            k = GRF._mask(cover, gr, clip)[0]
            u = 1.0 - above
            u = u * GRF._opacity(gr, slot)
            u = u * k
            if closer == HOLD:
                u = u * k_mask[a]
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

    X, B, held, qok = [CR._canvas(rows, cols, bg)], [gi], {}, {}
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
            closer, _a, slot, clip = items[a]
            if closer == END_MASK:
                b = qok[q - 1][..., None] * dk_dm[q - 1]
            else:
                adj = adjoint(X[-1], t_end[a], B[-1])
                k = GRF._mask(cover, gr, clip)[0]
                b = adj * k[..., None]
                if closer == HOLD:
                    b = b * k_mask[a][..., None]
                b = b * GRF._opacity(gr, slot)
            X.append(np.zeros((rows, cols, 4)))
            B.append(b)
        elif op == END_MASK:
            X.pop()
            B.pop()
            S = held.pop(len(X)) * k_mask[a - 1][..., None]
            X[-1] = _over(X[-1], S)
        else:
            hold = op == HOLD
            G = X.pop()
            B.pop()
            o = GRF._opacity(gr, slot)
            adj = adjoint(X[-1], t_end[q], B[-1])
            qd = CR._dot(adj, G)
            dk = qd * o
            if hold:
                dk = dk * k_mask[q]
            k, before = GRF._mask(cover, gr, clip)
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
                t = qd * k
                if hold:
                    t = t * k_mask[q]
                add("opacity", slot, t.reshape(-1))
            if hold:
                t = qd * o
                qok[q] = t * k
                held[len(X)] = _hold(G, o, k)
            else:
                X[-1] = GRF._group_step(X[-1], G, o, k)
    return grad_cover, sums, tol
