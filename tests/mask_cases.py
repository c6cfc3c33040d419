"""Seeded cases of luminance-masked groups in differentiable compositing, shared by tests/test_mask_host.py and the GPU tests:
planes, paints, gradient descriptions and trees with masks, the oracle's image of them, the host build of csrc/svgr_mask.h, and
the central differences of the numpy restatement.

A tree is group_cases' with one more field: ("group", children, opacity or None, clip planes or None, mask children or None);
``program`` makes the ABI's tables of it exactly as diff.mask_program does (a masked group closes with HOLD and is followed by its
mask's group, closed by END_MASK; opacity slots and clips numbered as their groups close).

No pixel of a case sits on a kink of the mask's value (alpha at 0.0001, a straight channel or alpha at 0 or 1): the planes painted
inside a mask group are drawn from [0.15, 0.95] and the paints are translucent, which tests/test_mask_host.py asserts.  Only
"empty_mask", whose mask canvas is 0 everywhere, is at a one-sided point on purpose.

The arrays of a case are shared: leave them unchanged."""
import ctypes as C
import functools

import numpy as np

from oracle import oracle
from tests import compose_cases as M
from tests import gradpaint_cases as G
from tests import group_cases as K
from tests import mask_ref as MR
from tests.group_ref import GR
from tests.paint_ref import fma

BG = M.BG
H = G.H
ROWS, COLS = G.ROWS, G.COLS
GENERIC_ORIGIN = K.GENERIC_ORIGIN


def grp(children, opacity=None, clip=None, mask=None):
    return ("group", list(children), opacity, clip, None if mask is None else list(mask))


def program(tree):
    """GR of a tree."""
    items, clip_off, clip_planes, opacity = [], [0], [], []

    def walk(children):
        for child in children:
            if isinstance(child, tuple):
                _tag, kids, o, clip, mask = child
                begin = len(items)
                items.append([1, -1, 0, 0])
                walk(kids)
                slot = c = -1
                if o is not None:
                    slot = len(opacity)
                    opacity.append(float(o))
                if clip is not None:
                    c = len(clip_off) - 1
                    clip_planes.extend(clip)
                    clip_off.append(len(clip_planes))
                items[begin][1] = len(items)
                items.append([2 if mask is None else 3, begin, slot, c])
                if mask is not None:
                    begin = len(items)
                    items.append([1, -1, 0, 0])
                    walk(mask)
                    items[begin][1] = len(items)
                    items.append([4, begin, 0, 0])
            else:
                items.append([0, int(child), 0, 0])

    walk(tree)
    return GR(np.array(items, dtype=np.int32).reshape(-1, 4), np.array(clip_off, dtype=np.int32), np.array(clip_planes, dtype=np.int32),
              np.array(opacity, dtype=np.float64))


def mask_planes(tree, inside=False):
    """The planes painted inside a mask group, at any depth."""
    out = []
    for child in tree:
        if isinstance(child, tuple):
            out += mask_planes(child[1], inside) + mask_planes(child[4] or [], True)
        elif inside:
            out.append(child)
    return out


def _scene(rng, n, tree, gradients=()):
    """group_cases._solid, with the planes inside mask groups away from 0 and 1 and their paints translucent."""
    cover, paints, gp, tree = K._solid(rng, n, tree, gradients)
    for p in mask_planes(tree):
        cover[p] = rng.uniform(0.15, 0.95, cover[p].shape)
        if gp.kind[p] == 0:
            a = rng.uniform(0.3, 0.9)
            paints[p] = np.append(rng.uniform(0.1, 0.9, 3) * a, a)
    return cover, paints, gp, tree


def _depth4(rng):
    tree = [0, grp([1, grp([2, grp([3, grp([4], opacity=0.8, mask=[5])], opacity=0.9)])]), 6]
    return _scene(rng, 7, tree)


# name -> (builder, seed); every case but "mask_generic" is dyadic and drawn at the origin (0, 0)
CASES = {
    "plain": (lambda r: _scene(r, 5, [0, grp([1, 2], mask=[3]), 4]), 171),
    "opacity_clip": (lambda r: _scene(r, 7, [0, grp([1, 2], opacity=0.7, clip=[3, 4], mask=[5, 6])]), 172),
    "mask_linear": (lambda r: _scene(r, 4, [0, grp([1], opacity=0.8, mask=[2]), 3], {2: K._pad4}), 173),
    "mask_generic": (lambda r: _scene(r, 6, [0, grp([1, 2], opacity=0.75, clip=[3], mask=[4, 5])], {1: K._lin, 4: K._lin, 5: K._rad}), 174),
    "mask_in_mask": (lambda r: _scene(r, 6, [0, grp([1], mask=[2, grp([3], opacity=0.9, mask=[4])]), 5]), 175),
    "pair_in_target": (lambda r: _scene(r, 6, [0, grp([1, grp([2], mask=[3]), 4], opacity=0.6, mask=[5])]), 176),
    "depth4": (_depth4, 177),
    "empty_mask": (lambda r: _scene(r, 3, [0, grp([1], opacity=0.5, mask=[]), 2]), 178),
    "empty_target": (lambda r: _scene(r, 3, [0, grp([], mask=[1]), 2]), 179),
}
ALL = tuple((name, with_bg) for name in CASES for with_bg in (False, True))
BY_VALUE = ("empty_mask",)


@functools.lru_cache(maxsize=None)
def case(name, with_bg):
    """dict(name, cover, paints, gp, tree, gr, origin, bg, g, dyadic)."""
    builder, seed = CASES[name]
    cover, paints, gp, tree = builder(np.random.default_rng(seed))
    dyadic = name != "mask_generic"
    origin = (0, 0) if dyadic else GENERIC_ORIGIN
    if not dyadic:
        gp = G.clear_stops(gp, ROWS, COLS, origin, gp.stop_pos)
    G.check_clear(gp, ROWS, COLS, origin)
    g = np.random.default_rng(3000 + seed).standard_normal((ROWS, COLS, 4))
    return dict(name=name, cover=np.ascontiguousarray(cover), paints=np.ascontiguousarray(paints), gp=gp, tree=tree, gr=program(tree), origin=origin,
                bg=BG if with_bg else None, g=g, dyadic=dyadic)


# ------------------------------------------------------------------------------------------------ the oracle
def oracle_mask(layer):
    """Layer.luminance_mask of a premultiplied layer: the oracle's convert to straight alpha, then the one line of the luminance."""
    s = oracle.convert(layer, True, False, False, False)
    lum = fma(s[..., 2], np.float64(0.072), fma(s[..., 1], np.float64(0.7154), s[..., 0] * 0.2125))
    return np.ascontiguousarray((lum * s[..., 3])[..., None])


def oracle_image(cover, paints, gp, tree, bg=None, origin=(0, 0)):
    """group_cases.oracle_image with masks: after `layer * o` and compose_in with the clip, compose_in with oracle_mask of the
    mask's own layers composed on nothing."""
    rows, cols = cover.shape[1:]

    def layer_of(children, under):
        layers = list(under)
        for child in children:
            if isinstance(child, tuple):
                _tag, kids, o, clip, mask = child
                layer = layer_of(kids, [])
                if o is not None:
                    layer = layer * o
                if clip is not None:
                    m, off = oracle.compose_over([(np.ascontiguousarray(cover[j][..., None]), (0, 0)) for j in clip])
                    assert off == (0, 0)
                    layer, off = oracle.compose_in([(np.ascontiguousarray(m[..., :1]), (0, 0)), (layer, (0, 0))])
                    assert off == (0, 0)
                if mask is not None:
                    layer, off = oracle.compose_in([(oracle_mask(layer_of(mask, [])), (0, 0)), (layer, (0, 0))])
                    assert off == (0, 0)
                layers.append((layer, (0, 0)))
            else:
                layers.append((K._oracle_fill(cover, paints, gp, child, origin), (0, 0)))
        if not layers:
            return np.zeros((rows, cols, 4))
        image, off = oracle.compose_over(layers)
        assert off == (0, 0)
        return image

    return layer_of(tree, [] if bg is None else [(np.tile(np.asarray(bg, dtype=np.float64), (rows, cols, 1)), (0, 0))])


# ------------------------------------------------------------------------------------------------ central differences
NAMES = K.NAMES


def _objective(c, **changed):
    cover, paints = changed.pop("cover", c["cover"]), changed.pop("paints", c["paints"])
    gr = c["gr"]._replace(opacity=changed.pop("opacity")) if "opacity" in changed else c["gr"]
    gp = c["gp"]._replace(**changed) if changed else c["gp"]
    return MR.forward(cover, paints, gp, gr, c["bg"], c["origin"], fused=False)


def central_differences(c):
    """(fd, tol) over NAMES by group_cases.central_differences' scheme (step H and 2 H, tolerance twice the Richardson estimate
    plus the rounding term 2^-50 * sum |g * C| / H), of the masked restatement."""
    g, gp = c["g"], c["gp"]
    base = _objective(c)
    rounding = 2.0 ** -50 * float(np.abs(g * base).sum()) / H
    arrays = dict(cover=c["cover"], paints=c["paints"], m6=gp.m6, geom=gp.geom, stop_pos=gp.stop_pos, stop_rgba=gp.stop_rgba, opacity=c["gr"].opacity)
    fd, tol = {}, {}
    for name, arr in arrays.items():
        fd[name], tol[name] = np.zeros_like(arr), np.zeros_like(arr)
        if name == "cover":   # every pixel of a plane at once: a pixel depends on its own coverage alone
            for p in range(len(arr)):
                d = []
                for h in (H, 2 * H):
                    hi, lo = arr.copy(), arr.copy()
                    hi[p] += h
                    lo[p] -= h
                    d.append((g * (_objective(c, cover=hi) - _objective(c, cover=lo))).sum(axis=-1) / (2 * h))
                fd[name][p], tol[name][p] = d[0], 2.0 * np.abs(d[1] - d[0]) / 3.0 + rounding
            continue
        for idx in np.ndindex(arr.shape):
            d = []
            for h in (H, 2 * H):
                hi, lo = arr.copy(), arr.copy()
                hi[idx] += h
                lo[idx] -= h
                d.append(float((g * (_objective(c, **{name: hi}) - _objective(c, **{name: lo}))).sum()) / (2 * h))
            fd[name][idx], tol[name][idx] = d[0], 2.0 * abs(d[1] - d[0]) / 3.0 + rounding
    return fd, tol


# ------------------------------------------------------------------------------------------------ the host build of the header
def harness():
    from tests.util import host_build

    lib = host_build("mask_harness")
    lib.mkh_depth.restype = C.c_int
    lib.mkh_value.restype = C.c_double
    lib.mkh_value.argtypes = [C.c_void_p]
    lib.mkh_value_vjp.restype = None
    lib.mkh_value_vjp.argtypes = [C.c_void_p, C.c_void_p]
    lib.mkh_check.restype = C.c_char_p
    lib.mkh_check.argtypes = [C.c_void_p] + [C.c_longlong] * 5 + [C.c_void_p] * 4
    lib.mkh_forward.restype = None
    lib.mkh_forward.argtypes = [C.c_void_p] * 10 + [C.c_int] + [C.c_void_p] * 3 + [C.c_longlong, C.c_void_p]
    lib.mkh_backward.restype = None
    lib.mkh_backward.argtypes = [C.c_void_p] * 10 + [C.c_int] * 2 + [C.c_void_p] * 4 + [C.c_int] * 5 + [C.c_longlong] + [C.c_void_p] * 7
    return lib


def harness_value(M):
    """(k, dk/dM) of one premultiplied pixel, as the header computes them."""
    M = np.ascontiguousarray(M, dtype=np.float64)
    assert M.shape == (4,)
    d = np.zeros(4)
    harness().mkh_value_vjp(M.ctypes.data, d.ctypes.data)
    return float(harness().mkh_value(M.ctypes.data)), d


def harness_check(gr, n_paths, n_groups=None, n_clip_planes=None, n_opacities=None):
    """(None or the header's message, the kernels' items, n_clips, n_pairs, index of the last END_MASK) of mask_program_check."""
    items = np.ascontiguousarray(gr.items, dtype=np.int32).reshape(-1, 4)
    clip_off, clip_planes = np.ascontiguousarray(gr.clip_off, dtype=np.int32), np.ascontiguousarray(gr.clip_planes, dtype=np.int32)
    n_groups = int((items[:, 0] == 1).sum()) if n_groups is None else n_groups
    n_clip_planes = len(clip_planes) if n_clip_planes is None else n_clip_planes
    n_opacities = len(gr.opacity) if n_opacities is None else n_opacities
    dev, info = np.zeros((max(len(items), 1), 4), dtype=np.int32), np.zeros(4, dtype=np.int64)
    msg = harness().mkh_check(items.ctypes.data, len(items), n_paths, n_groups, n_clip_planes, n_opacities, clip_off.ctypes.data if len(clip_off) else None,
                              clip_planes.ctypes.data if len(clip_planes) else None, dev.ctypes.data, info.ctypes.data)
    return (None if msg is None else msg.decode()), dev, int(info[0]), int(info[2]), int(info[3])


def _inputs(cover, paints, gp, gr, bg, origin):
    arrays, bg, view = G._inputs(cover, paints, gp, bg, origin)
    msg, dev, _n, n_pairs, last = harness_check(gr, len(arrays[0]))
    assert msg is None, msg
    clip_off = np.ascontiguousarray(gr.clip_off, dtype=np.int32) if len(gr.clip_off) else np.zeros(1, dtype=np.int32)
    clip_planes = np.ascontiguousarray(np.concatenate([gr.clip_planes, [0]]), dtype=np.int32)   # (never empty: a pointer to pass)
    opacity = np.ascontiguousarray(np.concatenate([gr.opacity, [0.0]]), dtype=np.float64)
    return arrays, bg, view, dev, clip_off, clip_planes, opacity, n_pairs, last


def harness_forward(cover, paints, gp, gr, bg=None, origin=(0, 0)):
    """image (rows, cols, 4) in double, as the header composes it on the host."""
    arrays, bg, view, dev, clip_off, clip_planes, opacity, _np, _last = _inputs(cover, paints, gp, gr, bg, origin)
    _n, rows, cols = arrays[0].shape
    image = np.zeros((rows, cols, 4))
    harness().mkh_forward(*[a.ctypes.data for a in arrays], None if bg is None else bg.ctypes.data, view.ctypes.data, dev.ctypes.data, len(dev),
                          clip_off.ctypes.data, clip_planes.ctypes.data, opacity.ctypes.data, rows * cols, image.ctypes.data)
    return image


def harness_backward(cover, paints, gp, gr, grad_image, bg=None, origin=(0, 0)):
    """(grad_cover (n, rows, cols), sums): sums is a dict over paints, m6, geom, stop_pos, stop_rgba, opacity in double, as the
    header gives them on the host in pixel order."""
    arrays, bg, view, dev, clip_off, clip_planes, opacity, n_pairs, last = _inputs(cover, paints, gp, gr, bg, origin)
    n, rows, cols = arrays[0].shape
    g = np.ascontiguousarray(grad_image, dtype=np.float64)
    assert g.shape == (rows, cols, 4)
    ns, nop = len(gp.stop_pos), len(gr.opacity)
    n_groups = int((np.asarray(gr.items)[:, 0] == 1).sum())
    grad_cover = np.zeros_like(arrays[0])
    sums = dict(paints=np.zeros((n, 4)), m6=np.zeros((n, 6)), geom=np.zeros((n, 4)), stop_pos=np.zeros(ns), stop_rgba=np.zeros((ns, 4)), opacity=np.zeros(nop))
    harness().mkh_backward(*[a.ctypes.data for a in arrays], None if bg is None else bg.ctypes.data, view.ctypes.data, dev.ctypes.data, len(dev), last + 1,
                           clip_off.ctypes.data, clip_planes.ctypes.data, opacity.ctypes.data, g.ctypes.data, n, ns, n_groups, n_pairs, nop, rows * cols,
                           grad_cover.ctypes.data, *[sums[k].ctypes.data for k in ("paints", "m6", "geom", "stop_pos", "stop_rgba", "opacity")])
    return grad_cover, sums


# ------------------------------------------------------------------------------------------------ the launch seams
def random_scene(seed, tree, n_paths, rows, cols, first_gradient=None):
    """(cover, paints, gp, gr, g) of gradpaint_cases.random_scene under a tree with masks; the paths from `first_gradient` on are
    solid, linear and radial in turn (all solid by default)."""
    cover, paints, gp, g = G.random_scene(seed, n_paths, rows, cols, first_gradient=n_paths if first_gradient is None else first_gradient)
    return cover, paints, gp, program(tree), g


# ------------------------------------------------------------------------------------------------ the torch tests' cases
@functools.lru_cache(maxsize=None)
def small_case():
    """(cover, paints, gp, gr) at 6 x 5 for gradcheck: a masked pair with opacity and a clip of one plane, a linear-gradient fill
    over a solid one in the mask, a plain group in the target; no pixel near a kink of the mask's value or of the gradient."""
    rng = np.random.default_rng(191)
    cover, paints = M.random_planes(rng, 6, 6, 5), M.random_paints(rng, 6)
    lin = G._linear(rng, 2, (0.1, 0.45, 0.9), m6=(0.95, 0.08, 0.3, -0.06, 1.03, 0.2), geom=(0.4, 0.3, 2.9, 2.3))
    paints[5] = 0.9
    gp = G.make_gp([None, None, None, None, None, lin])
    gp = G.clear_stops(gp, 6, 5, (0, 0), gp.stop_pos)
    G.check_clear(gp, 6, 5, (0, 0))
    tree = [0, grp([1, grp([2], opacity=0.6)], opacity=0.8, clip=[3], mask=[4, 5])]
    for p in (4, 5):
        cover[p] = rng.uniform(0.2, 0.9, cover[p].shape)
    paints[4] = (0.35, 0.2, 0.45, 0.6)
    return cover, paints, gp, program(tree)


@functools.lru_cache(maxsize=None)
def render_case():
    """gradpaint_cases.render_case() -- the blob filled by a linear gradient, the star, at 12 x 11 -- with the blob as the MASK of
    a group that holds the star and has an opacity: (c, paints, gp, gr)."""
    c, paints, gp = G.render_case()
    return c, paints, gp, program([grp([1], opacity=0.7, mask=[0])])


def reference_render(c, segs, m6, paints, gp, gr):
    """The oracle's masks of the paths, composed by the numpy restatement (without its exact fused multiply-adds)."""
    from tests import cover_cases as CK

    off, vp = c["off"], c["viewport"]
    planes = np.stack([CK.oracle_cover(segs[off[p]:off[p + 1]], c["kinds"][off[p]:off[p + 1]], m6[p], int(c["rules"][p]), vp) for p in range(len(m6))])
    return MR.forward(planes, paints, gp, gr, c["bg"], vp[:2], fused=False)


def mask_points(c, index):
    """Which of the distinct points belong to the mask's outline (path 0)."""
    mine = np.zeros(int(index.max()) + 1, dtype=bool)
    mine[np.unique(index[c["off"][0]:c["off"][1]])] = True
    mine[0] = False   # (point 0 stands in for the unused slots of lines)
    return mine


FIT_STEPS, FIT_RATE_OPACITY, FIT_RATE_STOP, FIT_RATE_END = 40, 0.05, 0.02, 1.5   # fixed on the CPU with the harnesses (host_fit's losses)
FIT_OPACITY = 0.45                                   # the target's opacity; the loop starts from render_case's 0.7
FIT_STOP = 0.1                                       # how far the target's middle stop of the mask's gradient lies beyond render_case's
FIT_END = (0.9, -0.7)                                # the translation of the gradient's end point in the target


def fit_target(gp, opacity):
    """(gp, opacity) of the fit's target from the starting values."""
    pos, geom = gp.stop_pos.copy(), gp.geom.copy()
    pos[1] += FIT_STOP
    geom[0, 2:] += FIT_END
    return gp._replace(stop_pos=pos, geom=geom), np.array([FIT_OPACITY])


def host_fit():
    """Plain gradient descent on the target group's opacity and on the middle stop's position and the end point of the mask's
    linear gradient, with the host harnesses of the coverage (once: the outlines stay) and of the masks, towards the image of
    fit_target: the losses of every step, the last one after the final update."""
    from tests import cover_cases as CK

    c, paints, gp, gr = render_case()
    origin = c["viewport"][:2]
    planes, _slope, _acc, st = CK.harness_forward(c["segs"], c["kinds"], c["off"], c["m6"], c["rules"], c["viewport"])
    assert st == 0
    tgp, topacity = fit_target(gp, gr.opacity)
    target = harness_forward(planes, paints, tgp, gr._replace(opacity=topacity), c["bg"], origin)
    opacity, stop, end, losses = float(gr.opacity[0]), float(gp.stop_pos[1]), gp.geom[0, 2:].copy(), []
    for step in range(FIT_STEPS + 1):
        pos, geom = gp.stop_pos.copy(), gp.geom.copy()
        pos[1], geom[0, 2:] = stop, end
        now, g = gp._replace(stop_pos=pos, geom=geom), gr._replace(opacity=np.array([opacity]))
        r = harness_forward(planes, paints, now, g, c["bg"], origin) - target
        losses.append(0.5 * float((r * r).sum()))
        if step == FIT_STEPS:
            break
        _gc, sums = harness_backward(planes, paints, now, g, r, c["bg"], origin)
        opacity = opacity - FIT_RATE_OPACITY * float(sums["opacity"][0])
        stop = stop - FIT_RATE_STOP * float(sums["stop_pos"][1])
        end = end - FIT_RATE_END * sums["geom"][0, 2:]
    return losses
