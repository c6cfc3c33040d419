"""Gradient paints in differentiable compositing on the device (svgr_compose_painted_forward / svgr_compose_painted_backward
through svgrasterize_amd.diff): the image and grad_cover bit for bit against the host build of the same header, every summed
output within what the order of its sum can change and the same on every run, the renderer's own gradient fill, solid-only input
against svgr_compose_forward / _backward, the launch seams, and errors that launch nothing."""
import ctypes as C

import numpy as np
import pytest

from tests import compose_cases as M
from tests import gradpaint_cases as G
from tests import gradpaint_ref as R

pytestmark = pytest.mark.gpu
SUMS = ("paints", "m6", "geom", "stop_pos", "stop_rgba")


def _diff():
    from svgrasterize_amd import diff

    return diff


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _sums(grad_paints, grad_gp):
    return dict(paints=grad_paints, m6=grad_gp.m6, geom=grad_gp.geom, stop_pos=grad_gp.stop_pos, stop_rgba=grad_gp.stop_rgba)


def _check(cover, paints, gp, g, bg, origin, what, fused=True):
    """Forward and backward of the device against the harness, in double and in float planes.  ``fused=False``: the bound of the
    sums comes from the restatement without its exact fused multiply-adds (a Python loop per pixel), whose terms differ from the
    header's by a rounding: for the seams of many pixels."""
    diff = _diff()
    dgp = diff.GradientPaints(*gp)
    for dtype in (np.float64, np.float32):
        cov, grad = cover.astype(dtype), g.astype(dtype)
        himage = G.harness_forward(cov, paints, gp, bg, origin)   # (float planes widened: the harness works in double)
        hcover, hsums, _used = G.harness_backward(cov, paints, gp, grad, bg, origin)
        _rc, _rs, tol = R.backward(cov, paints, gp, grad, bg, origin, fused=fused)
        image = diff.compose_painted(cov, paints, dgp, bg=bg, origin=origin)
        assert image.dtype == dtype and image.shape == cover.shape[1:] + (4,)
        assert np.array_equal(_bits(image), _bits(himage.astype(dtype))), f"{what} {dtype.__name__}: image differs, max {np.abs(image - himage).max():.3e}"
        grad_cover, grad_paints, grad_gp = diff.compose_painted_backward(cov, paints, dgp, grad, bg=bg, origin=origin)
        assert grad_cover.dtype == dtype and grad_cover.shape == cover.shape and isinstance(grad_gp, diff.GradientPaints)
        assert np.array_equal(_bits(grad_cover), _bits(hcover.astype(dtype))), f"{what} {dtype.__name__}: grad_cover differs, max {np.abs(grad_cover - hcover).max():.3e}"
        got = _sums(grad_paints, grad_gp)
        for k in SUMS:
            assert got[k].dtype == np.float64 and got[k].shape == hsums[k].shape, k
            err = np.abs(got[k] - hsums[k])
            assert (err <= tol[k]).all(), f"{what} {dtype.__name__}: grad {k} off by {err.max():.3e}, bound {tol[k].flat[err.argmax()]:.3e}"
        assert not got["m6"][gp.kind == 0].any() and not got["geom"][gp.kind == 0].any() and not got["geom"][gp.kind == 2, 3].any()
        assert np.array_equal(grad_gp.kind, gp.kind) and np.array_equal(grad_gp.path_stop_off, gp.path_stop_off)
        again = diff.compose_painted_backward(cov, paints, dgp, grad, bg=bg, origin=origin)
        assert np.array_equal(_bits(again[0]), _bits(grad_cover)), f"{what}: two runs differ"
        again = _sums(again[1], again[2])
        assert all(np.array_equal(_bits(again[k]), _bits(got[k])) for k in SUMS), f"{what}: two runs differ"
    return got


@pytest.mark.parametrize("name,with_bg", G.ALL)
def test_cases_forward_backward(name, with_bg):
    c = G.case(name, with_bg)
    _check(c["cover"], c["paints"], c["gp"], c["g"], c["bg"], c["origin"], name)
    if name == "mixed":   # and the device's own gradients against the central differences of the restatement
        diff = _diff()
        grad_cover, grad_paints, grad_gp = diff.compose_painted_backward(c["cover"], c["paints"], diff.GradientPaints(*c["gp"]), c["g"], bg=c["bg"], origin=c["origin"])
        fd, tol = G.central_differences(c)
        got = dict(_sums(grad_paints, grad_gp), cover=grad_cover)
        for k in got:
            assert (np.abs(got[k] - fd[k]) <= tol[k]).all(), k


def test_the_renderer_draws_the_same_gradient():
    """One gradient path, paints of ones, no bg, the plane of Path.mask itself: the image is the layer of Path.fill with that
    gradient on its window, bit for bit.  The linear geometry is dyadic (the renderer takes vec . vec from the host); the radial
    one is not, and neither is the transform: both routes get the same six numbers."""
    import svgrasterize_amd as S
    from svgrasterize_amd.paint import GradLinear, GradRadial

    diff = _diff()
    path = S.Path.from_svg("M3,4 C9,2 14,6 12,12 L4,15 Z")
    tr = S.Transform().translate(1.5, 0.5).scale(1.2)
    vp = [0, 0, 22, 20]
    rng = np.random.default_rng(90)
    stops = [(float(o), c) for o, c in zip((0.0, 0.3, 0.55, 1.0), G.stop_colours(rng, 4))]
    for paint, lin in ((GradLinear((1.5, 0.75), (9.5, 8.75), stops, None, "reflect", False, None), True),
                       (GradLinear((1.5, 0.75), (9.5, 8.75), stops[:2], None, "pad", False, None), False),
                       (GradRadial((7.3, 8.9), 3.7, None, None, stops, None, "repeat", False, None), True),
                       (GradRadial((7.3, 8.9), 5.1, None, None, stops[1:], None, "pad", False, None), False)):
        layer, _hull = path.fill(tr, paint, viewport=vp, linear_rgb=lin)
        mask, _hull = path.mask(tr, None, viewport=vp)
        assert tuple(mask.offset) == tuple(layer.offset)
        want = np.array(layer.image)
        plane = np.ascontiguousarray(np.array(mask.image)[..., 0][None])
        gp, rows = diff.gradient_paints([paint], tr, linear_rgb=lin)
        image = diff.compose_painted(plane, rows, gp, origin=tuple(int(v) for v in layer.offset))
        assert want.shape == image.shape and want[..., 3].max() > 0.2 and len(np.unique(want[..., 3])) > 20
        assert np.array_equal(_bits(image), _bits(want)), float(np.abs(image - want).max())


def test_solid_only_input_equals_the_solid_entries():
    diff = _diff()
    for name, with_bg in (("scene", True), ("opaque_full", False)):
        c = M.case(name, with_bg)
        gp = diff.GradientPaints(*G.make_gp([None] * len(c["cover"])))
        for dtype in (np.float64, np.float32):
            cov, g = c["cover"].astype(dtype), c["g"].astype(dtype)
            assert np.array_equal(_bits(diff.compose_painted(cov, c["paints"], gp, bg=c["bg"])), _bits(diff.compose(cov, c["paints"], bg=c["bg"])))
            grad_cover, grad_paints, grad_gp = diff.compose_painted_backward(cov, c["paints"], gp, g, bg=c["bg"])
            want_cover, want_paints = diff.compose_backward(cov, c["paints"], g, bg=c["bg"])
            tol = M.R.backward(cov, c["paints"], g, c["bg"])[2]
            assert np.array_equal(_bits(grad_cover), _bits(want_cover)) and (np.abs(grad_paints - want_paints) <= tol).all()
            assert not grad_gp.m6.any() and not grad_gp.geom.any() and grad_gp.stop_pos.shape == (0,) and grad_gp.stop_rgba.shape == (0, 4)


def test_pixel_count_seams():
    block, groups = _diff().compose_block(), _diff().compose_groups()
    for n in (block - 1, block, block + 1, groups * block + 1):
        cover, paints, gp, g = G.random_scene(100 + n % 1000, 2, 1, n)
        _check(cover, paints, gp, g, M.BG if n % 2 else None, (3, -5), f"{n} pixels", fused=False)


def test_viewport_seams():
    for rows, cols in ((1, 1), (3, 85), (1, 257)):
        cover, paints, gp, g = G.random_scene(200 + cols, 3, rows, cols)
        _check(cover, paints, gp, g, None, (0, 0), f"{rows} x {cols}")


def test_path_count_seams():
    for n_paths in (1, 2, 65):
        cover, paints, gp, g = G.random_scene(300 + n_paths, n_paths, 5, 67)
        assert n_paths < 3 or set(gp.kind.tolist()) == {0, 1, 2}
        _check(cover, paints, gp, g, M.BG, (-2, 7), f"{n_paths} paths", fused=n_paths < 3)


def test_stop_count_seams():
    cover, paints, gp, g = G.random_scene(500, 4, 5, 67, stops=(1, 2, 32))
    assert np.diff(gp.path_stop_off).tolist() == [1, 2, 0, 32]
    got = _check(cover, paints, gp, g, None, (0, 0), "1, 2 and 32 stops")
    assert np.count_nonzero(got["stop_pos"][3:]) >= 30   # (nearly every one of the 32 stops is used by some pixel)


def test_a_wave_without_coverage_skips_its_path():
    """Planes that are zero over whole waves and whole workgroups: the skipped reductions add nothing, the others are kept, and
    d / d cover is written where the coverage is 0 too."""
    block = _diff().compose_block()
    cover, paints, gp, g = G.random_scene(400, 4, 1, 3 * block + 17, first_gradient=0)
    assert gp.kind.tolist() == [1, 2, 0, 1]
    cover[0, :, :block] = 0.0             # a whole workgroup step
    cover[1, :, 64:128] = 0.0             # one wave of the first step
    cover[2] = 0.0                        # everywhere (a solid)
    cover[3, :, : 3 * block] = 0.0        # all but the ragged end
    got = _check(cover, paints, gp, g, None, (0, 0), "sparse planes", fused=False)
    assert not got["paints"][2].any() and got["paints"][3].all() and got["m6"][3].all()
    diff = _diff()
    grad_cover = diff.compose_painted_backward(cover, paints, diff.GradientPaints(*gp), g)[0]
    assert np.count_nonzero(grad_cover[0, :, :block]) > block // 2 and np.count_nonzero(grad_cover[3, :, : 3 * block]) > block


def test_gradients_after_64_solid_paths():
    cover, paints, gp, g = G.random_scene(600, 67, 3, 43, first_gradient=64)
    assert not gp.kind[:64].any() and gp.kind[64:].tolist() == [1, 2, 0] and gp.path_stop_off[64] == 0
    got = _check(cover, paints, gp, g, M.BG, (0, 0), "64 solid paths first", fused=False)
    assert got["m6"][64:66].all() and got["stop_rgba"].any()


def test_errors_and_overflow_launch_nothing():
    from svgrasterize_amd import _abi

    diff = _diff()
    ctx = _abi.Context.get()
    c = G.case("mixed", False)
    gp = c["gp"]
    n, rows, cols = c["cover"].shape
    ns = len(gp.stop_pos)
    ins = [ctx.from_host(a) for a in (c["cover"], c["paints"], gp.m6, gp.geom, gp.stop_pos, gp.stop_rgba)]
    d_grad = ctx.from_host(c["g"])
    image = ctx.alloc(rows * cols * 32)
    outs = [ctx.alloc(b) for b in (n * rows * cols * 8, n * 32, n * 48, n * 32, ns * 8, ns * 32)]

    def desc(n_paths=n, rows=rows, cols=cols, plane=_abi.COVER_F64, n_stops=ns, kind=gp.kind, spread=gp.spread, off=gp.path_stop_off, has_bg=None):
        topo = tuple(np.ascontiguousarray(a, dtype=np.int32) for a in (kind, spread, off))
        d, keep = diff._painted_desc(n_paths, rows, cols, plane, None, (0, 0), topo, n_stops)
        if has_bg is not None:
            d.has_bg = has_bg
        return d, keep

    def forward(dk, ins=ins, image=image):
        return ctx.lib.svgr_compose_painted_forward(ctx.handle, C.byref(dk[0]), *[b.handle if b else None for b in ins], image.handle)

    def backward(dk, ins=ins, grad=d_grad, outs=outs):
        return ctx.lib.svgr_compose_painted_backward(ctx.handle, C.byref(dk[0]), *[b.handle if b else None for b in ins], grad.handle,
                                                     *[b.handle if b else None for b in outs])

    def swap(seq, i, b):
        return [b if j == i else x for j, x in enumerate(seq)]

    def put(a, i, v):
        a = np.array(a)
        a[i] = v
        return a

    n0 = ctx.launches()
    invalid, overflow = -1, -5
    bad = [desc(n_paths=0), desc(rows=0), desc(cols=-3), desc(plane=2), desc(has_bg=2), desc(rows=rows + 1),
           desc(kind=put(gp.kind, 1, 3)), desc(kind=put(gp.kind, 0, -1)), desc(spread=put(gp.spread, 2, 3)), desc(spread=put(gp.spread, 1, -1)),
           desc(off=put(gp.path_stop_off, 0, 1)), desc(off=put(gp.path_stop_off, 4, 6)), desc(n_stops=ns + 1), desc(off=put(gp.path_stop_off, 2, 8)),
           desc(off=put(gp.path_stop_off, 1, 1)), desc(off=put(gp.path_stop_off, 2, 0)), desc(n_stops=-1),
           desc(off=[0, 0, 33, 40, 40], n_stops=40)]
    for dk in bad:
        assert forward(dk) == invalid and backward(dk) == invalid
    for i, small in enumerate((n * rows * cols * 8, n * 32, n * 48, n * 32, ns * 8, ns * 32)):
        assert forward(desc(), ins=swap(ins, i, ctx.alloc(small - 8))) == invalid and backward(desc(), ins=swap(ins, i, ctx.alloc(small - 8))) == invalid
        assert forward(desc(), ins=swap(ins, i, None)) == invalid and backward(desc(), ins=swap(ins, i, None)) == invalid
        assert backward(desc(), outs=swap(outs, i, ctx.alloc(small - 8))) == invalid and backward(desc(), outs=swap(outs, i, None)) == invalid
    assert forward(desc(), image=ctx.alloc(rows * cols * 32 - 8)) == invalid and backward(desc(), grad=ctx.alloc(rows * cols * 32 - 8)) == invalid
    null = desc()
    null[0].kind = None
    assert forward(null) == invalid and backward(null) == invalid
    for dk in (desc(rows=1 << 15, cols=1 << 15), desc(rows=1 << 31, cols=1), desc(n_paths=1 << 40, rows=1 << 40, cols=1 << 40)):
        assert forward(dk) == overflow and backward(dk) == overflow
    assert ctx.launches() == n0
    assert forward(desc()) == 0 and ctx.launches() == n0 + 2          # the topology, the composition
    assert backward(desc()) == 0 and ctx.launches() == n0 + 5         # the topology, the two walks, the sums
    ctx.sync()
    assert np.array_equal(image.download((rows, cols, 4), np.float64), G.harness_forward(c["cover"], c["paints"], gp))
