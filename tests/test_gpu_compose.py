"""Differentiable compositing on the device (svgr_compose_forward / svgr_compose_backward through svgrasterize_amd.diff): the
forward and grad_cover bit for bit against the host build of the same header, grad_paints within what the order of its sum can
change and the same on every run, the launch seams, and errors that launch nothing."""
import ctypes as C

import numpy as np
import pytest

from tests import compose_cases as M
from tests import compose_ref as R

pytestmark = pytest.mark.gpu


def _diff():
    from svgrasterize_amd import diff

    return diff


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _check(cover, paints, g, bg, what):
    """Forward and backward of the device against the harness, in double and in float planes."""
    diff = _diff()
    for dtype in (np.float64, np.float32):
        cov, grad = cover.astype(dtype), g.astype(dtype)
        himage = M.harness_forward(cov, paints, bg)   # (float planes widened: the harness works in double)
        hcover, hpaints = M.harness_backward(cov, paints, grad, bg)
        _rc, _rp, tol = R.backward(cov, paints, grad, bg)
        image = diff.compose(cov, paints, bg=bg)
        assert image.dtype == dtype and image.shape == cover.shape[1:] + (4,)
        assert np.array_equal(_bits(image), _bits(himage.astype(dtype))), f"{what} {dtype.__name__}: image differs, max {np.abs(image - himage).max():.3e}"
        grad_cover, grad_paints = diff.compose_backward(cov, paints, grad, bg=bg)
        assert grad_cover.dtype == dtype and grad_cover.shape == cover.shape and grad_paints.dtype == np.float64
        assert np.array_equal(_bits(grad_cover), _bits(hcover.astype(dtype))), f"{what} {dtype.__name__}: grad_cover differs, max {np.abs(grad_cover - hcover).max():.3e}"
        err = np.abs(grad_paints - hpaints)
        assert (err <= tol).all(), f"{what} {dtype.__name__}: grad_paints off by {err.max():.3e}, bound {tol.flat[err.argmax()]:.3e}"
        again = diff.compose_backward(cov, paints, grad, bg=bg)
        assert np.array_equal(_bits(again[0]), _bits(grad_cover)) and np.array_equal(_bits(again[1]), _bits(grad_paints)), f"{what}: two runs differ"


@pytest.mark.parametrize("name,with_bg", M.ALL)
def test_cases_forward_backward(name, with_bg):
    c = M.case(name, with_bg)
    _check(c["cover"], c["paints"], c["g"], c["bg"], name)
    image = _diff().compose(c["cover"], c["paints"], bg=c["bg"])
    assert np.array_equal(image, M.oracle_image(c["cover"], c["paints"], c["bg"]))
    grad_cover, grad_paints = _diff().compose_backward(c["cover"], c["paints"], c["g"], bg=c["bg"])
    assert np.isfinite(grad_cover).all() and np.isfinite(grad_paints).all()
    fd_cover, fd_paints, tol = M.central_differences(c)
    assert np.abs(grad_cover - fd_cover).max() <= tol and np.abs(grad_paints - fd_paints).max() <= tol


def test_pixel_count_seams():
    block, groups = _diff().compose_block(), _diff().compose_groups()
    for n in (block - 1, block, block + 1, groups * block + 1):
        cover, paints, g = M.random_scene(100 + n % 1000, 2, 1, n)
        _check(cover, paints, g, M.BG if n % 2 else None, f"{n} pixels")


def test_viewport_seams():
    for rows, cols in ((1, 1), (3, 85), (1, 257)):
        cover, paints, g = M.random_scene(200 + cols, 3, rows, cols)
        _check(cover, paints, g, None, f"{rows} x {cols}")


def test_path_count_seams():
    for n_paths in (1, 2, 65):
        cover, paints, g = M.random_scene(300 + n_paths, n_paths, 5, 67)
        assert 0.25 < (cover == 0.0).mean() < 0.42 and (cover == 1.0).any()
        _check(cover, paints, g, M.BG, f"{n_paths} paths")


def test_a_wave_without_coverage_skips_its_path():
    """Planes that are zero over whole waves and whole workgroups: the skipped reductions add nothing, the others are kept."""
    block = _diff().compose_block()
    cover, paints, g = M.random_scene(400, 4, 1, 3 * block + 17)
    cover[0, :, :block] = 0.0             # a whole workgroup step
    cover[1, :, 64:128] = 0.0             # one wave of the first step
    cover[2] = 0.0                        # everywhere
    cover[3, :, : 3 * block] = 0.0        # all but the ragged end
    _check(cover, paints, g, None, "sparse planes")
    _gc, grad_paints = _diff().compose_backward(cover, paints, g)
    assert not grad_paints[2].any() and grad_paints[3].all()


def test_errors_and_empty_inputs_launch_nothing():
    from svgrasterize_amd import _abi

    diff = _diff()
    ctx = _abi.Context.get()
    c = M.case("opaque_full", False)
    n, rows, cols = c["cover"].shape
    d_cover, d_paints, d_grad = ctx.from_host(c["cover"]), ctx.from_host(c["paints"]), ctx.from_host(c["g"])
    image, g_cover, g_paints = ctx.alloc(rows * cols * 32), ctx.alloc(n * rows * cols * 8), ctx.alloc(n * 32)
    small = ctx.alloc(rows * cols * 32 - 8)

    def forward(desc, cover=d_cover, paints=d_paints, image=image):
        return ctx.lib.svgr_compose_forward(ctx.handle, C.byref(desc), cover.handle if cover else None, paints.handle, image.handle)

    def backward(desc, grad=d_grad, g_cover=g_cover, g_paints=g_paints):
        return ctx.lib.svgr_compose_backward(ctx.handle, C.byref(desc), d_cover.handle, d_paints.handle, grad.handle, g_cover.handle, g_paints.handle)

    def desc(n_paths=n, rows=rows, cols=cols, plane=_abi.COVER_F64, bg=None, has_bg=None):
        d = diff._compose_desc(n_paths, rows, cols, plane, bg)
        if has_bg is not None:
            d.has_bg = has_bg
        return d

    n0 = ctx.launches()
    invalid, overflow = -1, -5
    for d in (desc(n_paths=0), desc(n_paths=-1), desc(rows=0), desc(cols=-3), desc(plane=2), desc(plane=-1), desc(has_bg=2), desc(n_paths=n + 1),
              desc(rows=rows + 1)):
        assert forward(d) == invalid and backward(d) == invalid
    assert forward(desc(), image=small) == invalid and forward(desc(), cover=None) == invalid
    assert forward(desc(), paints=ctx.alloc(n * 32 - 8)) == invalid
    assert backward(desc(), grad=small) == invalid and backward(desc(), g_cover=ctx.alloc(n * rows * cols * 8 - 8)) == invalid
    assert backward(desc(), g_paints=ctx.alloc(n * 32 - 8)) == invalid
    assert forward(desc(plane=_abi.COVER_F32), image=ctx.alloc(rows * cols * 16 - 4)) == invalid
    for d in (desc(n_paths=3, rows=1 << 15, cols=1 << 15), desc(rows=1 << 16, cols=1 << 15), desc(n_paths=1, rows=1 << 31, cols=1),
              desc(n_paths=1 << 40, rows=1 << 40, cols=1 << 40)):
        assert forward(d) == overflow and backward(d) == overflow
    with pytest.raises(_abi.SvgrError):
        diff._n_pixels(3, (0, 0, 1 << 15, 1 << 15))
    assert ctx.launches() == n0
    assert forward(desc()) == 0 and ctx.launches() == n0 + 1
    assert backward(desc()) == 0 and ctx.launches() == n0 + 3
    ctx.sync()
    assert np.array_equal(image.download((rows, cols, 4), np.float64), M.harness_forward(c["cover"], c["paints"]))
