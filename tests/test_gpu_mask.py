"""Luminance-masked groups in differentiable compositing on the device (svgr_compose_masked_forward / svgr_compose_masked_backward
through svgrasterize_amd.diff): the image and grad_cover bit for bit against the host build of the same header, every summed
output within what the order of its sum can change and the same on every run, a program without masks against compose_grouped,
a lowered masked scene against the library's own layer calls, the launch seams, and errors that launch nothing."""
import ctypes as C

import numpy as np
import pytest

from tests import compose_cases as M
from tests import gradpaint_cases as G
from tests import group_cases as GK
from tests import mask_cases as K
from tests import mask_ref as R
from tests.mask_cases import grp

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
    """test_gpu_group._check through the masked entries: forward and backward of the device against the harness, in double and
    in float planes (widened: the harness works in double, the device rounds once at its stores); the sums within the
    restatement's bound (``fused=False``: without its exact fused multiply-adds, for the seams of many pixels)."""
    diff = _diff()
    dgp, dgr = diff.GradientPaints(*gp), diff.Groups(*gr)
    for dtype in (np.float64, np.float32):
        cov, grad = cover.astype(dtype), g.astype(dtype)
        himage = K.harness_forward(cov, paints, gp, gr, bg, origin)
        hcover, hsums = K.harness_backward(cov, paints, gp, gr, grad, bg, origin)
        tol = R.backward(cov, paints, gp, gr, grad, bg, origin, fused=fused)[2]
        image = diff.compose_masked(cov, paints, dgp, dgr, bg=bg, origin=origin)
        assert image.dtype == dtype and image.shape == cover.shape[1:] + (4,)
        assert np.array_equal(_bits(image), _bits(himage.astype(dtype))), f"{what} {dtype.__name__}: image differs, max {np.abs(image - himage).max():.3e}"
        grad_cover, grad_paints, grad_gp, grad_opacity = diff.compose_masked_backward(cov, paints, dgp, dgr, grad, bg=bg, origin=origin)
        assert grad_cover.dtype == dtype and grad_cover.shape == cover.shape and isinstance(grad_gp, diff.GradientPaints)
        assert np.array_equal(_bits(grad_cover), _bits(hcover.astype(dtype))), f"{what} {dtype.__name__}: grad_cover differs, max {np.abs(grad_cover - hcover).max():.3e}"
        got = _sums(grad_paints, grad_gp, grad_opacity)
        for k in SUMS:
            assert got[k].dtype == np.float64 and got[k].shape == hsums[k].shape, k
            err = np.abs(got[k] - hsums[k])
            assert (err <= tol[k]).all(), f"{what} {dtype.__name__}: grad {k} off by {err.max():.3e}, bound {tol[k].flat[err.argmax()]:.3e}"
        clip = gr.clip_planes
        assert not got["paints"][clip].any() and not got["m6"][clip].any() and not got["geom"][clip].any()
        again = diff.compose_masked_backward(cov, paints, dgp, dgr, grad, bg=bg, origin=origin)
        assert np.array_equal(_bits(again[0]), _bits(grad_cover)), f"{what}: two runs differ"
        again = _sums(*again[1:])
        assert all(np.array_equal(_bits(again[k]), _bits(got[k])) for k in SUMS), f"{what}: two runs differ"
    return got


@pytest.mark.parametrize("name,with_bg", K.ALL)
def test_cases_forward_backward(name, with_bg):
    c = K.case(name, with_bg)
    _check(c["cover"], c["paints"], c["gp"], c["gr"], c["g"], c["bg"], c["origin"], name)
    if name in ("mask_in_mask", "mask_generic"):   # and the device's own gradients against the central differences of the restatement
        diff = _diff()
        out = diff.compose_masked_backward(c["cover"], c["paints"], diff.GradientPaints(*c["gp"]), diff.Groups(*c["gr"]), c["g"], bg=c["bg"], origin=c["origin"])
        fd, tol = K.central_differences(c)
        got = dict(_sums(*out[1:]), cover=out[0])
        for k in got:
            assert (np.abs(got[k] - fd[k]) <= tol[k]).all(), k


def test_a_program_without_masks_equals_the_grouped_entries():
    diff = _diff()
    for c in (GK.case("nested3", True), GK.case("gradient_generic", False), GK.case("flat", True)):
        gp, gr = diff.GradientPaints(*c["gp"]), diff.Groups(*c["gr"])
        for dtype in (np.float64, np.float32):
            cov, g = c["cover"].astype(dtype), c["g"].astype(dtype)
            want = diff.compose_grouped(cov, c["paints"], gp, gr, bg=c["bg"], origin=c["origin"])
            assert np.array_equal(_bits(diff.compose_masked(cov, c["paints"], gp, gr, bg=c["bg"], origin=c["origin"])), _bits(want))
            want_cover, want_paints, want_gp, want_op = diff.compose_grouped_backward(cov, c["paints"], gp, gr, g, bg=c["bg"], origin=c["origin"])
            grad_cover, grad_paints, grad_gp, grad_opacity = diff.compose_masked_backward(cov, c["paints"], gp, gr, g, bg=c["bg"], origin=c["origin"])
            assert np.array_equal(_bits(grad_cover), _bits(want_cover)) and np.array_equal(_bits(grad_paints), _bits(want_paints))
            assert np.array_equal(_bits(grad_opacity), _bits(want_op))
            for k in ("m6", "geom", "stop_pos", "stop_rgba"):
                assert np.array_equal(_bits(getattr(grad_gp, k)), _bits(getattr(want_gp, k))), k


def test_a_lowered_masked_scene_is_what_the_librarys_own_layer_calls_draw():
    """MASK(CLIP(OPACITY(GROUP))) with a radial-gradient mask, between two fills: the planes are Path.mask's own, and the image of
    the lowered program equals, bit for bit, Path.fill, Path.mask, Layer.opacity, Layer.compose(OVER), Layer.luminance_mask and
    Layer.compose(IN) assembled as Scene._render assembles them, in float64."""
    import svgrasterize_amd as S
    from svgrasterize_amd.layer import COMPOSE_IN, COMPOSE_OVER, Layer
    from svgrasterize_amd.paint import GradRadial

    diff = _diff()
    stops = [(0.0, np.array([1.0, 1.0, 1.0, 1.0])), (0.45, np.array([0.9, 0.7, 0.5, 0.9])), (0.8, np.array([0.3, 0.4, 0.2, 0.6])), (1.0, np.array([0.0, 0.0, 0.0, 0.0]))]
    rad = GradRadial((9.0, 8.5), 8.25, None, None, stops, None, "pad", False, None)
    red, green, blue, grey = (np.array(c) for c in ((0.8, 0.1, 0.1, 0.9), (0.1, 0.7, 0.2, 1.0), (0.1, 0.2, 0.9, 0.5), (0.5, 0.5, 0.5, 0.5)))
    p0, p1, p2, p3 = (S.Path.from_svg(d) for d in ("M3,4 C9,2 14,6 12,12 L4,15 Z", "M2,2 L15,3 L9,14 Z", "M5,1 C12,3 13,9 8,15 L3,9 Z", "M8,6 L16,8 L10,16 Z"))
    c1 = S.Path.from_svg("M1,1 L13,2 L12,13 L2,12 Z")
    m1, m2 = S.Path.from_svg("M0,0 L18,0 L18,18 L0,18 Z"), S.Path.from_svg("M6,3 L14,9 L6,15 Z")
    target = S.Scene.group([S.Scene.fill(p1, green), S.Scene.fill(p2, blue)]).opacity(0.5).clip(S.Scene.fill(c1, None))
    scene = S.Scene.group([S.Scene.fill(p0, red), target.mask(S.Scene.group([S.Scene.fill(m1, rad), S.Scene.fill(m2, grey)])), S.Scene.fill(p3, blue)])
    tr = S.Transform().translate(1.5, 0.5).scale(1.2)
    vp = [0, 0, 24, 22]
    low = diff.lower_scene(scene, tr, linear_rgb=False, masks=True)
    assert low.groups.items[:, 0].tolist() == [0, 1, 0, 0, 3, 1, 0, 0, 4, 0] and low.groups.clip_planes.tolist() == [1]
    assert [r for r, _p in low.sources] == ["fill", "clip", "fill", "fill", "mask", "mask", "fill"]

    def mask(p):
        return low.sources[p][1].mask(tr, "evenodd" if low.rules[p] else None, viewport=vp)[0]

    def paste(layer):
        out = np.zeros((vp[2], vp[3], layer.channels))
        r0, c0 = (int(v) for v in layer.offset)
        out[r0:r0 + layer.height, c0:c0 + layer.width] = np.array(layer.image)
        return out

    planes = np.ascontiguousarray(np.stack([paste(mask(p))[..., 0] for p in range(7)]))
    image = diff.compose_masked(planes, low.paints, low.gp, low.groups)

    def fill(path, paint):
        return path.fill(tr, paint, viewport=vp, linear_rgb=False)[0]

    group = Layer.compose([fill(p1, green), fill(p2, blue)], COMPOSE_OVER, False).opacity(0.5, False)
    group = Layer.compose([mask(1), group], COMPOSE_IN, False)
    lum = Layer.compose([fill(m1, rad), fill(m2, grey)], COMPOSE_OVER, False).luminance_mask(False)
    group = Layer.compose([lum, group], COMPOSE_IN, False)
    want = paste(Layer.compose([fill(p0, red), group, fill(p3, blue)], COMPOSE_OVER, False))
    k = paste(lum)[..., 0]
    assert want[..., 3].max() > 0.5 and len(np.unique(want[..., 3])) > 40 and len(np.unique(k)) > 40 and k.max() > 0.5
    assert np.array_equal(image, want), float(np.abs(image - want).max())
    # and the gradient reaches the mask's gradient paint and its outline's plane
    g = np.random.default_rng(96).standard_normal(image.shape)
    grad_cover, grad_paints, grad_gp, grad_opacity = diff.compose_masked_backward(planes, low.paints, low.gp, low.groups, g)
    assert np.abs(grad_cover[4]).max() > 1e-3 and np.abs(grad_gp.geom[4][:3]).min() > 1e-4 and np.abs(grad_gp.stop_rgba).max() > 1e-3 and grad_opacity[0] != 0.0


DOCUMENT = """<svg xmlns="http://www.w3.org/2000/svg" width="20" height="20" viewBox="0 0 20 20">
<defs>
<radialGradient id="g" cx="10" cy="9" r="8" gradientUnits="userSpaceOnUse"><stop offset="0" stop-color="#fff"/><stop offset="0.6" stop-color="#bbb" stop-opacity="0.8"/><stop offset="1" stop-color="#000" stop-opacity="0"/></radialGradient>
<mask id="m" maskUnits="userSpaceOnUse" maskContentUnits="userSpaceOnUse" x="0" y="0" width="20" height="20"><path d="M3,3 L17,4 L16,17 L4,16 Z" fill="url(#g)"/></mask>
</defs>
<rect x="1" y="1" width="18" height="18" fill="#123456"/>
<g mask="url(#m)" opacity="0.5"><path d="M2,2 L18,4 L10,18 Z" fill="#c03020"/></g>
</svg>"""
VIEWPORT = [0, 0, 20, 20]


def document_picture():
    """(scene, Scene.render's picture of DOCUMENT on VIEWPORT, float64 premultiplied)."""
    import svgrasterize_amd as S

    scene = S.svg_scene_from_str(DOCUMENT)[0]
    layer = scene.render(S.Transform(), viewport=VIEWPORT, linear_rgb=False)[0]
    want = np.zeros((VIEWPORT[2], VIEWPORT[3], 4))
    r0, c0 = (int(v) for v in layer.offset)
    want[r0:r0 + layer.height, c0:c0 + layer.width] = np.array(layer.image)
    return scene, want


def test_a_loaded_document_with_a_mask_renders_to_the_renderers_picture_and_back():
    """Within 1e-11, the tolerance of the coverage's known-answer tests against Path.mask: the composition multiplies a plane's
    error by paints and opacities <= 1, and the mask divides by an alpha that is 0.8 or more where its plane is not 0."""
    import svgrasterize_amd as S

    diff = _diff()
    scene, want = document_picture()
    low = diff.lower_scene(scene, S.Transform(), masks=True)
    assert [r for r, _p in low.sources] == ["fill", "fill", "mask"] and low.groups.items[:, 0].tolist() == [0, 1, 1, 0, 2, 3, 1, 0, 4]
    cover, slope = diff.coverage(low.segs, low.kinds, low.path_seg_off, low.m6, low.rules, VIEWPORT)
    image = diff.compose_masked(cover, low.paints, low.gp, low.groups)
    assert want[..., 3].max() == 1.0 and len(np.unique(want)) > 100   # (the masked triangle shows: not just the backdrop's colour)
    assert np.abs(image - want).max() <= 1e-11, float(np.abs(image - want).max())
    g = np.random.default_rng(2).standard_normal(image.shape)
    grad_cover, _gp, grad_gp, grad_opacity = diff.compose_masked_backward(cover, low.paints, low.gp, low.groups, g)
    grad_segs, _gm = diff.coverage_backward(low.segs, low.kinds, low.path_seg_off, low.m6, low.rules, VIEWPORT, slope, grad_cover)
    mine = slice(int(low.path_seg_off[2]), int(low.path_seg_off[3]))   # the mask's outline
    assert np.abs(grad_segs[mine]).max() > 1e-3 and np.abs(grad_gp.geom[2][:3]).min() > 1e-4 and np.abs(grad_gp.stop_rgba).max() > 1e-3
    assert np.abs(grad_gp.stop_pos).max() > 1e-4 and abs(grad_opacity[0]) > 1e-2


MASKED = [0, grp([1, 2], opacity=0.6, clip=[3], mask=[4, 5]), 6]


def test_pixel_count_seams():
    block, groups = _diff().compose_block(), _diff().compose_groups()
    for n in (block - 1, block, block + 1, groups * block + 1):
        cover, paints, gp, gr, g = K.random_scene(100 + n % 1000, MASKED, 7, 1, n, first_gradient=4)
        _check(cover, paints, gp, gr, g, M.BG if n % 2 else None, (3, -5), f"{n} pixels", fused=False)


def test_viewport_seams():
    for rows, cols in ((1, 1), (3, 85), (1, 257)):
        cover, paints, gp, gr, g = K.random_scene(200 + cols, [grp([0, grp([1], clip=[2], mask=[3])], opacity=0.7, mask=[4])], 5, rows, cols, first_gradient=0)
        _check(cover, paints, gp, gr, g, None, (7, 11), f"{rows} x {cols}")


def test_an_lds_run_ends_inside_a_mask_group():
    """Seven fills of 32 stops in one mask: 174 slots each, 1218 in all, more than the 1024 of a run."""
    rng = np.random.default_rng(300)
    rows, cols = 5, 67
    cover, paints, g = M.random_planes(rng, 9, rows, cols), M.random_paints(rng, 9), rng.standard_normal((rows, cols, 4))
    pos = tuple(np.linspace(0.0, 1.0, 32).tolist())
    paths = [None, None] + [G._linear(rng, q % 3, pos) for q in range(7)]
    for p in range(2, 9):
        paints[p] = rng.uniform(0.5, 1.0)
        cover[p] = cover[p] * 0.3   # (seven fills OVER each other: keep the mask's canvas translucent)
    gp = G.make_gp(paths)
    assert int(gp.path_stop_off[-1]) == 7 * 32
    gr = K.program([0, grp([1], opacity=0.8, mask=[2, 3, 4, 5, 6, 7, 8])])
    got = _check(cover, paints, gp, gr, g, M.BG, (0, 0), "seven 32-stop fills in a mask", fused=False)
    assert got["opacity"].all() and all(got["stop_rgba"][32 * q:32 * (q + 1)].any() for q in range(7)) and got["geom"][2:].any(axis=1).all()


def test_40_masked_pairs_in_a_row():
    tree = [grp([3 * q, 3 * q + 1], opacity=0.3 + 0.015 * q, mask=[3 * q + 2]) for q in range(40)]
    cover, paints, gp, gr, g = K.random_scene(700, tree, 120, 5, 67)
    got = _check(cover, paints, gp, gr, g, None, (0, 0), "40 pairs")
    assert got["opacity"].shape == (40,) and got["opacity"].all() and got["paints"][2::3, :3].all()


def test_a_mask_whose_planes_are_zero_over_whole_waves():
    block = _diff().compose_block()
    cover, paints, gp, gr, g = K.random_scene(400, [0, grp([1, 2], opacity=0.5, mask=[3, 4]), 5], 6, 1, 3 * block + 17)
    cover[3, :, :block] = 0.0             # a whole workgroup step of one of the mask's fills
    cover[4, :, : 2 * block] = 0.0        # of both over the first step: M = 0 there, the target is hidden
    cover[3, :, 2 * block:2 * block + 64] = 0.0   # one wave
    cover[5] = 0.0
    got = _check(cover, paints, gp, gr, g, None, (0, 0), "sparse mask planes")
    assert not got["paints"][5].any() and got["paints"][3, :3].all() and got["opacity"].all()
    diff = _diff()
    grad_cover = diff.compose_masked_backward(cover, paints, diff.GradientPaints(*gp), diff.Groups(*gr), g)[0]
    assert not grad_cover[1][:, :block].any() and np.isfinite(grad_cover).all()   # nothing reaches the target under k = 0


def test_both_groups_of_a_pair_empty():
    cover, paints, gp, gr, g = K.random_scene(500, [0, grp([], opacity=0.5, mask=[]), 1, grp([2], mask=[]), grp([], mask=[3])], 4, 3, 43)
    got = _check(cover, paints, gp, gr, g, M.BG, (0, 0), "empty pairs")
    assert got["opacity"][0] == 0.0 and not got["paints"][2:].any()
    diff = _diff()
    image = diff.compose_masked(cover, paints, diff.GradientPaints(*gp), diff.Groups(*gr), bg=M.BG)
    assert np.array_equal(image, GK.harness_forward(cover[:2], paints[:2], G.make_gp([None] * 2), GK.program([0, 1]), M.BG))


def test_errors_and_overflow_launch_nothing():
    from svgrasterize_amd import _abi
    from tests.test_group_host import BAD as GROUP_BAD
    from tests.test_mask_host import BAD, GOOD

    diff = _diff()
    ctx = _abi.Context.get()
    rng = np.random.default_rng(9)
    n, rows, cols = 4, 4, 5
    cover, paints, g = M.random_planes(rng, n, rows, cols), M.random_paints(rng, n), rng.standard_normal((rows, cols, 4))
    gp = G.make_gp([None] * n)
    topo = tuple(np.ascontiguousarray(a, dtype=np.int32) for a in (gp.kind, gp.spread, gp.path_stop_off))
    ins = [ctx.from_host(a) for a in (cover, paints, gp.m6, gp.geom)] + [None, None, ctx.from_host(np.array([0.5]))]
    d_grad = ctx.from_host(g)
    image = ctx.alloc(rows * cols * 32)
    outs = [ctx.alloc(b) for b in (n * rows * cols * 8, n * 32, n * 48, n * 32)] + [None, None, ctx.alloc(8)]

    def desc(gr=GOOD, n_paths=n, rows=rows, cols=cols, n_groups=2, n_opacities=1, **fields):
        gtopo = tuple(np.ascontiguousarray(a, dtype=np.int32) for a in (gr.items, gr.clip_off, gr.clip_planes))
        d, keep = diff._grouped_desc(n_paths, rows, cols, _abi.COVER_F64, None, (0, 0), topo, 0, gtopo, n_groups, n_opacities)
        for k, v in fields.items():
            setattr(d, k, v)
        return d, keep

    def forward(dk, ins=ins, image=image):
        return ctx.lib.svgr_compose_masked_forward(ctx.handle, C.byref(dk[0]), *[b.handle if b else None for b in ins], image.handle)

    def backward(dk, ins=ins, grad=d_grad, outs=outs):
        return ctx.lib.svgr_compose_masked_backward(ctx.handle, C.byref(dk[0]), *[b.handle if b else None for b in ins], grad.handle,
                                                    *[b.handle if b else None for b in outs])

    def swap(seq, i, b):
        return [b if j == i else x for j, x in enumerate(seq)]

    n0 = ctx.launches()
    invalid, overflow = -1, -5
    bad = [desc(gr) for gr in BAD.values()]
    bad += [desc(gr, n_paths=3, n_groups=1) for what, gr in GROUP_BAD.items() if what != "crossed groups"]
    bad += [desc(n_groups=3), desc(n_groups=1), desc(n_opacities=2), desc(n_opacities=0), desc(n_clip_planes=2), desc(n_items=6), desc(n_items=0),
            desc(n_groups=-1), desc(n_paths=0), desc(rows=rows + 1), desc(has_bg=2), desc(items=None), desc(clip_off=None), desc(clip_planes=None)]
    deep = K.program([grp([0, grp([1, grp([2, grp([3], mask=[4, grp([5])])])])])])
    bad.append(desc(deep, n_paths=6, n_groups=6, n_opacities=0))
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
    assert backward(desc()) == 0 and ctx.launches() == n0 + 7         # the topology, the program, the three walks in one kernel, the sums
    ctx.sync()
    assert np.array_equal(image.download((rows, cols, 4), np.float64), K.harness_forward(cover, paints, gp, GOOD))
