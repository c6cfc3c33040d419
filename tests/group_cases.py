"""Seeded cases of isolated groups in differentiable compositing, shared by tests/test_group_host.py and the GPU tests: planes,
paints, gradient descriptions and group trees, the oracle's image of them, the host build of csrc/svgr_group.h, and the central
differences of the numpy restatement.

A case's gradient paths are gradpaint_cases' own: the "dyadic" linear ones (identity transform, origin (0, 0): every offset exact,
so the oracle's image is equal bit for bit) or, in the case "gradient_generic", the generic linear and radial ones of its "mixed"
case.  Its builder conditions (no step of a central difference crosses a stop, clamp, wrap or fold) are asserted here as they
are there.  The composite is smooth in every coverage value, paint and opacity: nothing else has a kink.

The tree of a case is a list of plane indices and ("group", children, opacity or None, clip planes or None) tuples; ``program``
makes the ABI's tables of it exactly as diff.group_program does (opacity slots and clips numbered as their groups close).

The arrays of a case are shared: leave them unchanged."""
import ctypes as C
import functools

import numpy as np

from oracle import oracle
from tests import compose_cases as M
from tests import gradpaint_cases as G
from tests import group_ref as GR_
from tests.group_ref import GR

BG = M.BG
H = G.H
ROWS, COLS = G.ROWS, G.COLS
GENERIC_ORIGIN = (8, 2)


def grp(children, opacity=None, clip=None):
    return ("group", list(children), opacity, clip)


def program(tree):
    """GR of a tree."""
    items, clip_off, clip_planes, opacity = [], [0], [], []

    def walk(children):
        for child in children:
            if isinstance(child, tuple):
                _tag, kids, o, clip = child
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
                items.append([2, begin, slot, c])
            else:
                items.append([0, int(child), 0, 0])

    walk(tree)
    return GR(np.array(items, dtype=np.int32).reshape(-1, 4), np.array(clip_off, dtype=np.int32), np.array(clip_planes, dtype=np.int32),
              np.array(opacity, dtype=np.float64))


def _lin(rng):
    return G._linear(rng, 2, (0.1, 0.35, 0.8), m6=(0.93, 0.11, -7.2, -0.07, 1.04, -1.3), geom=(1.2, 0.8, 9.45, 7.7))


def _rad(rng):
    return G._radial(rng, 1, (0.05, 0.4, 0.7, 0.95), m6=(1.02, -0.04, -8.4, 0.06, 0.97, -2.2), geom=(5.3, 4.9, 4.3))


def _pad4(rng):
    return G._linear(rng, 0, (0.0, 0.25, 0.5, 1.0))


def _repeat2(rng):
    return G._linear(rng, 1, (0.125, 0.875))


def _reflect4(rng):
    return G._linear(rng, 2, (0.0625, 0.25, 0.75, 0.9375))


def _solid(rng, n, tree, gradients=()):
    """n planes, solid but for {plane: builder} in gradients."""
    cover, paints = M.random_planes(rng, n, ROWS, COLS), M.random_paints(rng, n)
    paths = [None] * n
    for p, make in dict(gradients).items():
        paths[p] = make(rng)
        paints[p] = rng.uniform(0.5, 1.0)
    return cover, paints, G.make_gp(paths), tree


def _deep(levels):
    """planes 0 .. 2 levels: a fill, then `levels` nested groups with a fill before and after each inner group."""
    def nest(d, p):
        if d == levels:
            return [p], p + 1
        inner, nxt = nest(d + 1, p + 1)
        return [p, grp(inner, opacity=0.9 - 0.1 * d), nxt], nxt + 1

    tree, n = nest(0, 0)
    return tree, n


def _depth4(rng):
    tree, n = _deep(4)
    return _solid(rng, n, tree)


# name -> (builder, seed); every case but "gradient_generic" is dyadic and drawn at the origin (0, 0)
CASES = {
    "flat": (lambda r: _solid(r, 4, [0, 1, 2, 3], {1: _pad4, 2: _reflect4}), 71),
    "opacity": (lambda r: _solid(r, 4, [0, grp([1, 2], opacity=0.6), 3]), 72),
    "clip1": (lambda r: _solid(r, 4, [0, grp([1, 2], clip=[3])]), 73),
    "clip3": (lambda r: _solid(r, 6, [grp([0, 1], clip=[2, 3, 4]), 5]), 74),
    "both": (lambda r: _solid(r, 5, [0, grp([1, 2], opacity=0.7, clip=[3, 4])]), 75),
    "nested": (lambda r: _solid(r, 7, [0, grp([1, grp([2, 3], opacity=0.5, clip=[4]), 5], opacity=0.8), 6]), 76),
    "nested3": (lambda r: _solid(r, 9, [0, grp([1, grp([2, grp([3, 4], opacity=0.6), 5], clip=[6, 7]), 8], opacity=0.85)], {3: _repeat2}), 77),
    "empty": (lambda r: _solid(r, 3, [0, grp([], opacity=0.5, clip=[1]), 2]), 78),
    "gradient_in_clip": (lambda r: _solid(r, 5, [0, grp([1, 2], opacity=0.75, clip=[3]), 4], {1: _pad4, 2: _reflect4}), 79),
    "gradient_generic": (lambda r: _solid(r, 5, [0, grp([1, 2], opacity=0.75, clip=[3]), 4], {1: _lin, 2: _rad}), 81),
    "depth4": (_depth4, 80),
}
ALL = tuple((name, with_bg) for name in CASES for with_bg in (False, True))


@functools.lru_cache(maxsize=None)
def case(name, with_bg):
    """dict(name, cover, paints, gp, tree, gr, origin, bg, g, dyadic)."""
    builder, seed = CASES[name]
    cover, paints, gp, tree = builder(np.random.default_rng(seed))
    dyadic = name != "gradient_generic"
    origin = (0, 0) if dyadic else GENERIC_ORIGIN
    if not dyadic:
        gp = G.clear_stops(gp, ROWS, COLS, origin, gp.stop_pos)
    G.check_clear(gp, ROWS, COLS, origin)
    g = np.random.default_rng(3000 + seed).standard_normal((ROWS, COLS, 4))
    return dict(name=name, cover=np.ascontiguousarray(cover), paints=np.ascontiguousarray(paints), gp=gp, tree=tree, gr=program(tree), origin=origin,
                bg=BG if with_bg else None, g=g, dyadic=dyadic)


# ------------------------------------------------------------------------------------------------ the oracle
def _oracle_fill(cover, paints, gp, p, origin):
    rows, cols = cover.shape[1:]
    if gp.kind[p] == 0:
        return oracle.fill_solid(cover[p], paints[p])
    s0, s1 = gp.path_stop_off[p], gp.path_stop_off[p + 1]
    geo = dict(p0=gp.geom[p, :2], p1=gp.geom[p, 2:]) if gp.kind[p] == 1 else dict(center=gp.geom[p, :2], radius=float(gp.geom[p, 2]))
    grad = oracle.gradient_image(G.KINDS[gp.kind[p]], (origin[0], origin[1], rows, cols), G._m33(gp.m6[p]), None, G.SPREADS[gp.spread[p]],
                                 gp.stop_pos[s0:s1], gp.stop_rgba[s0:s1], **geo)
    return (grad * cover[p][..., None]) * paints[p]


def oracle_image(cover, paints, gp, tree, bg=None, origin=(0, 0)):
    """The oracle's layers in the tree's order: fill_solid (or gradient_image * cover * paint) layers composed by compose_over;
    a group is its members' compose_over on nothing, `layer * o`, then compose_in with the one-channel compose_over of its clip's
    planes as the first layer."""
    rows, cols = cover.shape[1:]

    def layer_of(children, under):
        layers = list(under)
        for child in children:
            if isinstance(child, tuple):
                _tag, kids, o, clip = child
                layer = layer_of(kids, [])
                if o is not None:
                    layer = layer * o
                if clip is not None:
                    mask, off = oracle.compose_over([(np.ascontiguousarray(cover[j][..., None]), (0, 0)) for j in clip])
                    assert off == (0, 0)
                    layer, off = oracle.compose_in([(np.ascontiguousarray(mask[..., :1]), (0, 0)), (layer, (0, 0))])
                    assert off == (0, 0)
                layers.append((layer, (0, 0)))
            else:
                layers.append((_oracle_fill(cover, paints, gp, child, origin), (0, 0)))
        if not layers:
            return np.zeros((rows, cols, 4))
        image, off = oracle.compose_over(layers)
        assert off == (0, 0)
        return image

    return layer_of(tree, [] if bg is None else [(np.tile(np.asarray(bg, dtype=np.float64), (rows, cols, 1)), (0, 0))])


# ------------------------------------------------------------------------------------------------ central differences
NAMES = ("cover", "paints", "m6", "geom", "stop_pos", "stop_rgba", "opacity")


def _objective(c, **changed):
    cover, paints = changed.pop("cover", c["cover"]), changed.pop("paints", c["paints"])
    gr = c["gr"]._replace(opacity=changed.pop("opacity")) if "opacity" in changed else c["gr"]
    gp = c["gp"]._replace(**changed) if changed else c["gp"]
    return GR_.forward(cover, paints, gp, gr, c["bg"], c["origin"], fused=False)


def central_differences(c):
    """(fd, tol) over NAMES: gradpaint_cases.central_differences' scheme -- central differences at H of sum(g * image) from the
    numpy restatement, tolerance twice the Richardson estimate |fd(2H) - fd(H)| / 3 plus the rounding term
    2^-50 * sum |g * C| / H -- with the clip planes among the cover and the opacities as one more array."""
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

    lib = host_build("group_harness")
    lib.grh_depth.restype = C.c_int
    lib.grh_check.restype = C.c_char_p
    lib.grh_check.argtypes = [C.c_void_p] + [C.c_longlong] * 5 + [C.c_void_p] * 4
    lib.grh_forward.restype = None
    lib.grh_forward.argtypes = [C.c_void_p] * 10 + [C.c_int] + [C.c_void_p] * 3 + [C.c_longlong, C.c_void_p]
    lib.grh_backward.restype = None
    lib.grh_backward.argtypes = [C.c_void_p] * 10 + [C.c_int] + [C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_longlong] + [C.c_void_p] * 7
    return lib


def harness_check(gr, n_paths, n_groups=None, n_clip_planes=None, n_opacities=None):
    """(None or the header's message, the kernels' items, n_clips) of group_program_check."""
    items = np.ascontiguousarray(gr.items, dtype=np.int32).reshape(-1, 4)
    clip_off, clip_planes = np.ascontiguousarray(gr.clip_off, dtype=np.int32), np.ascontiguousarray(gr.clip_planes, dtype=np.int32)
    n_groups = int((items[:, 0] == 1).sum()) if n_groups is None else n_groups
    n_clip_planes = len(clip_planes) if n_clip_planes is None else n_clip_planes
    n_opacities = len(gr.opacity) if n_opacities is None else n_opacities
    dev, info = np.zeros((max(len(items), 1), 4), dtype=np.int32), np.zeros(2, dtype=np.int64)
    msg = harness().grh_check(items.ctypes.data, len(items), n_paths, n_groups, n_clip_planes, n_opacities, clip_off.ctypes.data if len(clip_off) else None,
                              clip_planes.ctypes.data if len(clip_planes) else None, dev.ctypes.data, info.ctypes.data)
    return (None if msg is None else msg.decode()), dev, int(info[0])


def _inputs(cover, paints, gp, gr, bg, origin):
    arrays, bg, view = G._inputs(cover, paints, gp, bg, origin)
    msg, dev, _n = harness_check(gr, len(arrays[0]))
    assert msg is None, msg
    clip_off = np.ascontiguousarray(gr.clip_off, dtype=np.int32) if len(gr.clip_off) else np.zeros(1, dtype=np.int32)
    clip_planes = np.ascontiguousarray(np.concatenate([gr.clip_planes, [0]]), dtype=np.int32)   # (never empty: a pointer to pass)
    opacity = np.ascontiguousarray(np.concatenate([gr.opacity, [0.0]]), dtype=np.float64)
    return arrays, bg, view, dev, clip_off, clip_planes, opacity


def harness_forward(cover, paints, gp, gr, bg=None, origin=(0, 0)):
    """image (rows, cols, 4) in double, as the header composes it on the host."""
    arrays, bg, view, dev, clip_off, clip_planes, opacity = _inputs(cover, paints, gp, gr, bg, origin)
    _n, rows, cols = arrays[0].shape
    image = np.zeros((rows, cols, 4))
    harness().grh_forward(*[a.ctypes.data for a in arrays], None if bg is None else bg.ctypes.data, view.ctypes.data, dev.ctypes.data, len(dev),
                          clip_off.ctypes.data, clip_planes.ctypes.data, opacity.ctypes.data, rows * cols, image.ctypes.data)
    return image


def harness_backward(cover, paints, gp, gr, grad_image, bg=None, origin=(0, 0)):
    """(grad_cover (n, rows, cols), sums): sums is a dict over paints, m6, geom, stop_pos, stop_rgba, opacity in double, as the
    header gives them on the host in pixel order."""
    arrays, bg, view, dev, clip_off, clip_planes, opacity = _inputs(cover, paints, gp, gr, bg, origin)
    n, rows, cols = arrays[0].shape
    g = np.ascontiguousarray(grad_image, dtype=np.float64)
    assert g.shape == (rows, cols, 4)
    ns, nop = len(gp.stop_pos), len(gr.opacity)
    n_groups = int((dev[:, 0] == 1).sum())
    grad_cover = np.zeros_like(arrays[0])
    sums = dict(paints=np.zeros((n, 4)), m6=np.zeros((n, 6)), geom=np.zeros((n, 4)), stop_pos=np.zeros(ns), stop_rgba=np.zeros((ns, 4)), opacity=np.zeros(nop))
    harness().grh_backward(*[a.ctypes.data for a in arrays], None if bg is None else bg.ctypes.data, view.ctypes.data, dev.ctypes.data, len(dev),
                           clip_off.ctypes.data, clip_planes.ctypes.data, opacity.ctypes.data, g.ctypes.data, n, ns, n_groups, nop, rows * cols,
                           grad_cover.ctypes.data, *[sums[k].ctypes.data for k in ("paints", "m6", "geom", "stop_pos", "stop_rgba", "opacity")])
    return grad_cover, sums


# ------------------------------------------------------------------------------------------------ the launch seams
def random_scene(seed, tree, n_paths, rows, cols, first_gradient=None):
    """(cover, paints, gp, gr, g) of gradpaint_cases.random_scene under a tree; the paths from `first_gradient` on are solid,
    linear and radial in turn (all solid by default)."""
    cover, paints, gp, g = G.random_scene(seed, n_paths, rows, cols, first_gradient=n_paths if first_gradient is None else first_gradient)
    return cover, paints, gp, program(tree), g


# ------------------------------------------------------------------------------------------------ the torch tests' cases
@functools.lru_cache(maxsize=None)
def small_case():
    """(cover, paints, gp, gr) at 6 x 5 for gradcheck: two nested groups, one clip of two planes, one gradient fill; the
    gradient builder's conditions hold."""
    rng = np.random.default_rng(91)
    cover, paints = M.random_planes(rng, 6, 6, 5), M.random_paints(rng, 6)
    lin = G._linear(rng, 2, (0.1, 0.45, 0.9), m6=(0.95, 0.08, 0.3, -0.06, 1.03, 0.2), geom=(0.4, 0.3, 2.9, 2.3))
    paints[2] = 0.9
    gp = G.make_gp([None, None, lin, None, None, None])
    gp = G.clear_stops(gp, 6, 5, (0, 0), gp.stop_pos)
    G.check_clear(gp, 6, 5, (0, 0))
    tree = [0, grp([1, grp([2], opacity=0.6, clip=[4, 5]), 3], opacity=0.8)]
    return cover, paints, gp, program(tree)


@functools.lru_cache(maxsize=None)
def render_case():
    """gradpaint_cases.render_case() -- the blob filled by a linear gradient, the star, at 12 x 11 -- with the star as the CLIP of
    a group that holds the blob and has an opacity: (c, paints, gp, gr).  The star's paint is not looked at."""
    c, paints, gp = G.render_case()
    return c, paints, gp, program([grp([0], opacity=0.7, clip=[1])])


def point_index(c):
    """(points (n, 2), index (n_segs, 4)): the distinct control points of a case and where each segment's points are among them
    (an unused slot of a line points at point 0: its gradient is 0)."""
    index = np.zeros((len(c["segs"]), 4), dtype=np.int64)
    points = np.zeros((len(c["groups"]), 2))
    for i, members in enumerate(c["groups"]):
        for s, k in members:
            index[s, k] = i
        points[i] = c["segs"][members[0][0], members[0][1]]
    return points, index


def reference_render(c, segs, m6, paints, gp, gr):
    """The oracle's masks of the paths, composed by the numpy restatement (without its exact fused multiply-adds)."""
    from tests import cover_cases as CK

    off, vp = c["off"], c["viewport"]
    planes = np.stack([CK.oracle_cover(segs[off[p]:off[p + 1]], c["kinds"][off[p]:off[p + 1]], m6[p], int(c["rules"][p]), vp) for p in range(len(m6))])
    return GR_.forward(planes, paints, gp, gr, c["bg"], vp[:2], fused=False)


FIT_STEPS, FIT_RATE_OPACITY, FIT_RATE_POINTS, FIT_RATE_PAINT = 40, 0.03, 0.15, 0.04   # fixed on the CPU with the harnesses (host_fit's losses)
FIT_OPACITY = 0.45                                   # the target's opacity; the loop starts from render_case's 0.7
FIT_SHIFT = (0.5, -0.4)                              # the clip outline's translation in the target
FIT_PAINT = (0.9, 0.75, 0.6, 0.85)                   # the target's multiplier of the gradient fill; the loop starts from ones


def clip_points(c, index):
    """Which of the distinct points belong to the clip outline (path 1)."""
    mine = np.zeros(int(index.max()) + 1, dtype=bool)
    mine[np.unique(index[c["off"][1]:c["off"][2]])] = True
    mine[np.unique(index[c["off"][0]:c["off"][1]])] = False   # (point 0 stands in for the unused slots of lines)
    return mine


def host_fit():
    """Plain gradient descent on the group's opacity, the clip outline's points and the gradient fill's multiplier with the host
    harnesses of the coverage and of the groups, towards the image of FIT_OPACITY, FIT_SHIFT and FIT_PAINT: the losses of every
    step, the last one after the final update."""
    from tests import cover_cases as CK

    c, paints, gp, gr = render_case()
    origin = c["viewport"][:2]
    points, index = point_index(c)
    mine = clip_points(c, index)

    def render(pts, opacity, paint0):
        planes, slope, _acc, st = CK.harness_forward(pts[index], c["kinds"], c["off"], c["m6"], c["rules"], c["viewport"])
        assert st == 0
        p = paints.copy()
        p[0] = paint0
        g = gr._replace(opacity=np.array([opacity]))
        return harness_forward(planes, p, gp, g, c["bg"], origin), planes, slope, p, g

    target = render(points + np.where(mine[:, None], np.array(FIT_SHIFT), 0.0), FIT_OPACITY, np.array(FIT_PAINT))[0]
    pts, opacity, paint0, losses = points.copy(), float(gr.opacity[0]), paints[0].copy(), []
    for step in range(FIT_STEPS + 1):
        image, planes, slope, p, g = render(pts, opacity, paint0)
        r = image - target
        losses.append(0.5 * float((r * r).sum()))
        if step == FIT_STEPS:
            break
        grad_planes, sums = harness_backward(planes, p, gp, g, r, c["bg"], origin)
        gs, _gm, st = CK.harness_backward(pts[index], c["kinds"], c["off"], c["m6"], c["viewport"], slope, grad_planes)
        assert st == 0
        gpts = np.zeros_like(pts)
        np.add.at(gpts, index.ravel(), np.asarray(gs).reshape(-1, 2))
        pts = pts - FIT_RATE_POINTS * np.where(mine[:, None], gpts, 0.0)
        opacity = opacity - FIT_RATE_OPACITY * float(sums["opacity"][0])
        paint0 = paint0 - FIT_RATE_PAINT * sums["paints"][0]
    return losses
