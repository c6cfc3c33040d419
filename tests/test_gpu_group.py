"""Isolated groups in differentiable compositing on the device (svgr_compose_grouped_forward / svgr_compose_grouped_backward
through svgrasterize_amd.diff): the image and grad_cover bit for bit against the host build of the same header, every summed
output within what the order of its sum can change and the same on every run, a program without groups against
compose_painted, a lowered scene against the library's own layer calls, the launch seams, and errors that launch nothing."""
import ctypes as C

import numpy as np
import pytest

from tests import compose_cases as M
from tests import gradpaint_cases as G
from tests import group_cases as K
from tests import group_ref as R
from tests.group_cases import grp

pytestmark = pytest.mark.gpu
SUMS = ("paints", "m6", "geom", "stop_pos", "stop_rgba", "opacity")


def _diff():
    from svgrasterize_amd import diff

    return diff


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _sums(grad_paints, grad_gp, grad_opacity):
    return dict(paints=grad_paints, m6=grad_gp.m6, geom=grad_gp.geom, stop_pos=grad_gp.stop_pos, stop_rgba=grad_gp.stop_rgba, opacity=grad_opacity)


def _check(cover, paints, gp, gr, g, bg, origin, what, fused=True):
    """Forward and backward of the device against the harness, in double and in float planes (widened: the harness works in
    double, the device rounds once at its stores).  ``fused=False``: the bound of the sums comes from the restatement without
    its exact fused multiply-adds, for the seams of many pixels."""
    diff = _diff()
    dgp, dgr = diff.GradientPaints(*gp), diff.Groups(*gr)
    for dtype in (np.float64, np.float32):
        cov, grad = cover.astype(dtype), g.astype(dtype)
        himage = K.harness_forward(cov, paints, gp, gr, bg, origin)
        hcover, hsums = K.harness_backward(cov, paints, gp, gr, grad, bg, origin)
        tol = R.backward(cov, paints, gp, gr, grad, bg, origin, fused=fused)[2]
        image = diff.compose_grouped(cov, paints, dgp, dgr, bg=bg, origin=origin)
        assert image.dtype == dtype and image.shape == cover.shape[1:] + (4,)
        assert np.array_equal(_bits(image), _bits(himage.astype(dtype))), f"{what} {dtype.__name__}: image differs, max {np.abs(image - himage).max():.3e}"
        grad_cover, grad_paints, grad_gp, grad_opacity = diff.compose_grouped_backward(cov, paints, dgp, dgr, grad, bg=bg, origin=origin)
        assert grad_cover.dtype == dtype and grad_cover.shape == cover.shape and isinstance(grad_gp, diff.GradientPaints)
        assert np.array_equal(_bits(grad_cover), _bits(hcover.astype(dtype))), f"{what} {dtype.__name__}: grad_cover differs, max {np.abs(grad_cover - hcover).max():.3e}"
        got = _sums(grad_paints, grad_gp, grad_opacity)
        for k in SUMS:
            assert got[k].dtype == np.float64 and got[k].shape == hsums[k].shape, k
            err = np.abs(got[k] - hsums[k])
            assert (err <= tol[k]).all(), f"{what} {dtype.__name__}: grad {k} off by {err.max():.3e}, bound {tol[k].flat[err.argmax()]:.3e}"
        clip = gr.clip_planes
        assert not got["paints"][clip].any() and not got["m6"][clip].any() and not got["geom"][clip].any()
        again = diff.compose_grouped_backward(cov, paints, dgp, dgr, grad, bg=bg, origin=origin)
        assert np.array_equal(_bits(again[0]), _bits(grad_cover)), f"{what}: two runs differ"
        again = _sums(*again[1:])
        assert all(np.array_equal(_bits(again[k]), _bits(got[k])) for k in SUMS), f"{what}: two runs differ"
    return got


@pytest.mark.parametrize("name,with_bg", K.ALL)
def test_cases_forward_backward(name, with_bg):
    c = K.case(name, with_bg)
    _check(c["cover"], c["paints"], c["gp"], c["gr"], c["g"], c["bg"], c["origin"], name)
    if name in ("nested3", "gradient_generic"):   # and the device's own gradients against the central differences of the restatement
        diff = _diff()
        out = diff.compose_grouped_backward(c["cover"], c["paints"], diff.GradientPaints(*c["gp"]), diff.Groups(*c["gr"]), c["g"], bg=c["bg"], origin=c["origin"])
        fd, tol = K.central_differences(c)
        got = dict(_sums(*out[1:]), cover=out[0])
        for k in got:
            assert (np.abs(got[k] - fd[k]) <= tol[k]).all(), k


def test_a_program_without_groups_equals_the_painted_entries():
    diff = _diff()
    for c in (K.case("flat", True), G.case("mixed", False)):
        gp = diff.GradientPaints(*c["gp"])
        flat = diff.group_program(list(range(len(c["cover"]))))
        for dtype in (np.float64, np.float32):
            cov, g = c["cover"].astype(dtype), c["g"].astype(dtype)
            want = diff.compose_painted(cov, c["paints"], gp, bg=c["bg"], origin=c["origin"])
            assert np.array_equal(_bits(diff.compose_grouped(cov, c["paints"], gp, flat, bg=c["bg"], origin=c["origin"])), _bits(want))
            want_cover, want_paints, want_gp = diff.compose_painted_backward(cov, c["paints"], gp, g, bg=c["bg"], origin=c["origin"])
            grad_cover, grad_paints, grad_gp, grad_opacity = diff.compose_grouped_backward(cov, c["paints"], gp, flat, g, bg=c["bg"], origin=c["origin"])
            assert np.array_equal(_bits(grad_cover), _bits(want_cover)) and np.array_equal(_bits(grad_paints), _bits(want_paints))
            for k in ("m6", "geom", "stop_pos", "stop_rgba"):
                assert np.array_equal(_bits(getattr(grad_gp, k)), _bits(getattr(want_gp, k))), k
            assert grad_opacity.shape == (0,)


def test_a_lowered_scene_is_what_the_librarys_own_layer_calls_draw():
    """CLIP(OPACITY(GROUP)) of a solid and a gradient fill under a clip of two paths with different rules, between a fill and an
    OPACITY over a fill: the planes are Path.mask's own, the image of the lowered program equals, bit for bit, Path.fill,
    Path.mask, Layer.opacity, Layer.compose(IN) and Layer.compose(OVER) applied in the lowered order, in float64."""
    import svgrasterize_amd as S
    from svgrasterize_amd.layer import COMPOSE_IN, COMPOSE_OVER, Layer
    from svgrasterize_amd.paint import GradLinear

    diff = _diff()
    rng = np.random.default_rng(95)
    stops = [(float(o), c) for o, c in zip((0.0, 0.3, 0.55, 1.0), G.stop_colours(rng, 4))]
    lin = GradLinear((1.5, 0.75), (9.5, 8.75), stops, None, "reflect", False, None)
    red, green, blue = (np.array(c) for c in ((0.8, 0.1, 0.1, 0.9), (0.1, 0.7, 0.2, 1.0), (0.1, 0.2, 0.9, 0.5)))
    p0, p1, p2, p3 = (S.Path.from_svg(d) for d in ("M3,4 C9,2 14,6 12,12 L4,15 Z", "M2,2 L15,3 L9,14 Z", "M5,1 C12,3 13,9 8,15 L3,9 Z", "M8,6 L16,8 L10,16 Z"))
    c1, c2 = S.Path.from_svg("M1,1 L13,2 L12,13 L2,12 Z"), S.Path.from_svg("M4,4 L16,4 L16,16 L4,16 Z M7,7 L12,7 L12,12 L7,12 Z")
    scene = S.Scene.group([
        S.Scene.fill(p0, red),
        S.Scene.group([S.Scene.fill(p1, green), S.Scene.fill(p2, lin)]).opacity(0.5).clip(S.Scene.group([S.Scene.fill(c1, None), S.Scene.fill(c2, None, "evenodd")])),
        S.Scene.fill(p3, blue).opacity(0.75)])
    tr = S.Transform().translate(1.5, 0.5).scale(1.2)
    vp = [0, 0, 24, 22]
    low = diff.lower_scene(scene, tr, linear_rgb=False)
    assert low.groups.items[:, 0].tolist() == [0, 1, 0, 0, 2, 1, 0, 2] and low.groups.clip_planes.tolist() == [1, 2] and low.rules.tolist() == [0, 0, 1, 0, 0, 0]

    def mask(p):
        return low.sources[p][1].mask(tr, "evenodd" if low.rules[p] else None, viewport=vp)[0]

    def paste(layer):
        out = np.zeros((vp[2], vp[3], layer.channels))
        r0, c0 = (int(v) for v in layer.offset)
        out[r0:r0 + layer.height, c0:c0 + layer.width] = np.array(layer.image)
        return out

    planes = np.ascontiguousarray(np.stack([paste(mask(p))[..., 0] for p in range(6)]))
    image = diff.compose_grouped(planes, low.paints, low.gp, low.groups)

    def fill(path, paint):
        return path.fill(tr, paint, viewport=vp, linear_rgb=False)[0]

    clip = Layer.compose([mask(1), mask(2)], COMPOSE_OVER, False)
    group = Layer.compose([fill(p1, green), fill(p2, lin)], COMPOSE_OVER, False).opacity(0.5, False)
    group = Layer.compose([clip, group], COMPOSE_IN, False)
    want = paste(Layer.compose([fill(p0, red), group, fill(p3, blue).opacity(0.75, False)], COMPOSE_OVER, False))
    assert want[..., 3].max() > 0.5 and len(np.unique(want[..., 3])) > 40 and np.count_nonzero(planes[2]) > 20
    assert np.array_equal(image, want), float(np.abs(image - want).max())


GROUPED = [0, grp([1, 2], opacity=0.6, clip=[3])]


def test_pixel_count_seams():
    block, groups = _diff().compose_block(), _diff().compose_groups()
    for n in (block - 1, block, block + 1, groups * block + 1):
        cover, paints, gp, gr, g = K.random_scene(100 + n % 1000, GROUPED, 4, 1, n)
        _check(cover, paints, gp, gr, g, M.BG if n % 2 else None, (3, -5), f"{n} pixels")


def test_viewport_seams():
    for rows, cols in ((1, 1), (3, 85), (1, 257)):
        cover, paints, gp, gr, g = K.random_scene(200 + cols, [grp([0, grp([1], clip=[2])], opacity=0.7)], 3, rows, cols, first_gradient=0)
        _check(cover, paints, gp, gr, g, None, (0, 0), f"{rows} x {cols}")


def test_a_group_whose_planes_are_zero_over_whole_waves():
    block = _diff().compose_block()
    cover, paints, gp, gr, g = K.random_scene(400, [0, grp([1, 2], opacity=0.5, clip=[3]), 4], 5, 1, 3 * block + 17)
    cover[1, :, :block] = 0.0             # a whole workgroup step of a member
    cover[2, :, 64:128] = 0.0             # one wave
    cover[3, :, : 2 * block] = 0.0        # the clip: nothing of the group shows over two steps
    cover[4] = 0.0
    got = _check(cover, paints, gp, gr, g, None, (0, 0), "sparse planes")
    assert not got["paints"][4].any() and got["paints"][1].all() and got["opacity"].all()


def test_65_fills_inside_one_group():
    cover, paints, gp, gr, g = K.random_scene(600, [grp(list(range(65)), opacity=0.8, clip=[65]), 66], 67, 3, 43, first_gradient=60)
    assert set(gp.kind[60:].tolist()) == {0, 1, 2}
    got = _check(cover, paints, gp, gr, g, M.BG, (0, 0), "65 fills in a group", fused=False)
    assert got["opacity"].all() and got["stop_rgba"].any()


def test_40_groups_in_a_row_cross_an_lds_run():
    """Two fills and an opacity per group: 29 slots each, 1160 in all, so the runs of 1024 slots end inside the row of groups."""
    tree = [grp([2 * q, 2 * q + 1], opacity=0.3 + 0.015 * q) for q in range(40)]
    cover, paints, gp, gr, g = K.random_scene(700, tree, 80, 5, 67)
    got = _check(cover, paints, gp, gr, g, None, (0, 0), "40 groups")
    assert got["opacity"].shape == (40,) and got["opacity"].all()


def test_clips_of_1_and_33_planes():
    tree = [0, grp([1], clip=[2]), grp([3], opacity=0.9, clip=list(range(4, 37)))]
    cover, paints, gp, gr, g = K.random_scene(800, tree, 37, 5, 67)
    cover[4:37] *= 0.08                   # (33 planes OVER each other: keep the mask away from 1)
    _check(cover, paints, gp, gr, g, M.BG, (0, 0), "clips of 1 and 33 planes")
    diff = _diff()
    grad_cover = diff.compose_grouped_backward(cover, paints, diff.GradientPaints(*gp), diff.Groups(*gr), g, bg=M.BG)[0]
    assert np.abs(grad_cover[4:37]).min(axis=(1, 2)).shape == (33,) and all(np.count_nonzero(grad_cover[p]) > 100 for p in range(4, 37))


def test_errors_and_overflow_launch_nothing():
    from svgrasterize_amd import _abi
    from tests.test_group_host import BAD, GOOD

    diff = _diff()
    ctx = _abi.Context.get()
    rng = np.random.default_rng(9)
    n, rows, cols = 3, 4, 5
    cover, paints, g = M.random_planes(rng, n, rows, cols), M.random_paints(rng, n), rng.standard_normal((rows, cols, 4))
    gp = G.make_gp([None] * n)
    topo = tuple(np.ascontiguousarray(a, dtype=np.int32) for a in (gp.kind, gp.spread, gp.path_stop_off))
    ins = [ctx.from_host(a) for a in (cover, paints, gp.m6, gp.geom)] + [None, None, ctx.from_host(np.array([0.5]))]
    d_grad = ctx.from_host(g)
    image = ctx.alloc(rows * cols * 32)
    outs = [ctx.alloc(b) for b in (n * rows * cols * 8, n * 32, n * 48, n * 32)] + [None, None, ctx.alloc(8)]

    def desc(gr=GOOD, n_paths=n, rows=rows, cols=cols, n_groups=1, n_opacities=1, **fields):
        gtopo = tuple(np.ascontiguousarray(a, dtype=np.int32) for a in (gr.items, gr.clip_off, gr.clip_planes))
        d, keep = diff._grouped_desc(n_paths, rows, cols, _abi.COVER_F64, None, (0, 0), topo, 0, gtopo, n_groups, n_opacities)
        for k, v in fields.items():
            setattr(d, k, v)
        return d, keep

    def forward(dk, ins=ins, image=image):
        return ctx.lib.svgr_compose_grouped_forward(ctx.handle, C.byref(dk[0]), *[b.handle if b else None for b in ins], image.handle)

    def backward(dk, ins=ins, grad=d_grad, outs=outs):
        return ctx.lib.svgr_compose_grouped_backward(ctx.handle, C.byref(dk[0]), *[b.handle if b else None for b in ins], grad.handle,
                                                     *[b.handle if b else None for b in outs])

    def swap(seq, i, b):
        return [b if j == i else x for j, x in enumerate(seq)]

    n0 = ctx.launches()
    invalid, overflow = -1, -5
    bad = [desc(gr) for gr in BAD.values()]
    bad += [desc(n_groups=2), desc(n_groups=0), desc(n_opacities=2), desc(n_opacities=0), desc(n_clip_planes=2), desc(n_items=3), desc(n_items=0),
            desc(n_groups=-1), desc(n_paths=0), desc(rows=rows + 1), desc(has_bg=2), desc(items=None), desc(clip_off=None), desc(clip_planes=None)]
    tree5, n5 = K._deep(5)
    deep = K.program(tree5)
    bad.append(desc(deep, n_paths=n5, n_groups=5, n_opacities=5))
    for dk in bad:
        assert forward(dk) == invalid and backward(dk) == invalid
    for i, small in ((0, n * rows * cols * 8), (1, n * 32), (2, n * 48), (3, n * 32), (6, 8)):
        assert forward(desc(), ins=swap(ins, i, ctx.alloc(max(small - 8, 8)) if small > 8 else None)) == invalid
        assert backward(desc(), ins=swap(ins, i, None)) == invalid
        assert backward(desc(), outs=swap(outs, i, None)) == invalid
    assert forward(desc(), image=ctx.alloc(rows * cols * 32 - 8)) == invalid and backward(desc(), grad=ctx.alloc(rows * cols * 32 - 8)) == invalid
    for dk in (desc(rows=1 << 15, cols=1 << 15), desc(n_items=(1 << 24) + 1, n_groups=1 << 23)):
        assert forward(dk) == overflow and backward(dk) == overflow
    assert ctx.launches() == n0
    assert forward(desc()) == 0 and ctx.launches() == n0 + 3          # the topology, the program, the composition
    assert backward(desc()) == 0 and ctx.launches() == n0 + 7         # the topology, the program, the two walks in one kernel, the sums
    ctx.sync()
    assert np.array_equal(image.download((rows, cols, 4), np.float64), K.harness_forward(cover, paints, gp, GOOD))
