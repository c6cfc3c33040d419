"""Differentiable compositing on the host: csrc/svgr_compose.h compiled by g++ (tests/compose_harness.cpp) against the oracle's
solid fill and source-over, against central differences of the numpy restatement (tests/compose_ref.py), and against that
restatement itself (tests/compose_cases.py has the cases).  No GPU."""
import os
import re

import numpy as np
import pytest

from tests import compose_cases as M
from tests import compose_ref as R
from tests.util import ROOT

CSRC = os.path.join(ROOT, "svgrasterize.py_amd", "csrc")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("name,with_bg", M.ALL)
def test_forward_equals_the_oracle(name, with_bg):
    """The same operations in the same order as orc_fill_solid and orc_compose_over: equal, no tolerance."""
    c = M.case(name, with_bg)
    image = M.harness_forward(c["cover"], c["paints"], c["bg"])
    assert image.shape == c["cover"].shape[1:] + (4,)
    assert np.array_equal(image, M.oracle_image(c["cover"], c["paints"], c["bg"]))
    assert np.array_equal(image, R.forward(c["cover"], c["paints"], c["bg"]))
    if name == "opaque_full":
        assert (1.0 - c["cover"][1] * c["paints"][1, 3] == 0.0).sum() >= 12   # u_p == 0 exactly where the opaque paint covers
    if name == "scene":
        assert c["cover"].shape == (3, 24, 21) and all(0.0 < p.mean() < 1.0 for p in c["cover"])


@pytest.mark.parametrize("name,with_bg", M.ALL)
def test_backward_equals_central_differences(name, with_bg):
    """The composite is affine in every single coverage value and paint component, so a central difference at any step is
    exact up to rounding: h = 2^-10, tolerance 2^-50 * sum |g * C| / h, from the restatement alone."""
    c = M.case(name, with_bg)
    grad_cover, grad_paints = M.harness_backward(c["cover"], c["paints"], c["g"], c["bg"])
    assert np.isfinite(grad_cover).all() and np.isfinite(grad_paints).all()
    fd_cover, fd_paints, tol = M.central_differences(c)
    err_c, err_p = np.abs(grad_cover - fd_cover).max(), np.abs(grad_paints - fd_paints).max()
    print(f"{name} bg {with_bg}: max |grad_cover| {np.abs(grad_cover).max():.3e} err {err_c:.3e}; max |grad_paints| {np.abs(grad_paints).max():.3e} "
          f"err {err_p:.3e}; tol {tol:.3e}")
    assert err_c <= tol and err_p <= tol
    assert np.abs(grad_cover).max() > 1e-3 and np.abs(grad_paints).max() > 1e-3   # (the bound is small against the gradients)
    assert tol < 1e-8


@pytest.mark.parametrize("name,with_bg", M.ALL)
def test_harness_equals_reference(name, with_bg):
    """grad_cover bit for bit (per pixel, the same order); grad_paints within what the order of its sum can change."""
    c = M.case(name, with_bg)
    grad_cover, grad_paints = M.harness_backward(c["cover"], c["paints"], c["g"], c["bg"])
    ref_cover, ref_paints, tol = R.backward(c["cover"], c["paints"], c["g"], c["bg"])
    assert np.array_equal(_bits(grad_cover), _bits(ref_cover)), float(np.abs(grad_cover - ref_cover).max())
    assert (np.abs(grad_paints - ref_paints) <= tol).all(), float((np.abs(grad_paints - ref_paints) - tol).max())
    if name == "zero_plane":
        assert not grad_paints[1].any() and grad_cover[1].any()   # nothing of it is seen; covering more would be
    if name == "alpha_zero":
        assert grad_paints[1].all()


def test_opaque_cover_hides_what_is_under_it():
    """Under u_p == 0 the paths below get no gradient at all, and none is NaN: the case a division would break."""
    c = M.case("opaque_full", True)
    grad_cover, _gp = M.harness_backward(c["cover"], c["paints"], c["g"], c["bg"])
    hidden = c["cover"][1] == 1.0
    assert hidden.sum() >= 12 and (grad_cover[0][hidden] == 0.0).all() and np.abs(grad_cover[0][~hidden]).min() > 0.0
    assert np.abs(grad_cover[1][hidden]).min() > 0.0


def test_float32_planes_widen_exactly():
    cover, paints, g = M.random_scene(7, 3, 4, 9)
    c32 = cover.astype(np.float32)
    assert np.array_equal(M.harness_forward(c32, paints), M.harness_forward(c32.astype(np.float64), paints))


def test_premultiply_round_trip():
    from svgrasterize_amd import diff

    straight = np.array([[0.2, 0.4, 0.6, 0.5], [0.9, 0.1, 0.3, 0.0], [1.0, 1.0, 0.0, 1.0]])
    pre = diff.premultiply(straight)
    assert np.array_equal(pre, [[0.1, 0.2, 0.3, 0.5], [0.0, 0.0, 0.0, 0.0], [1.0, 1.0, 0.0, 1.0]])
    back = diff.unpremultiply(pre)
    assert np.allclose(back[[0, 2]], straight[[0, 2]], rtol=0, atol=2.0 ** -52) and not back[1].any()
    assert diff.premultiply([0.5, 0.5, 0.5, 0.5]).tolist() == [0.25, 0.25, 0.25, 0.5]
    with pytest.raises(ValueError):
        diff.premultiply(np.zeros((2, 3)))


def test_header_rules_and_exports():
    """The header's own rules (no fma, no contraction pragma, SVGR_HD throughout), the ABI additions and the Python surface."""
    text = open(os.path.join(CSRC, "svgr_compose.h")).read()
    assert "fma(" not in text and "fp contract" not in text.lower() and "SVGR_HD" in text
    assert " / " not in re.sub(r"//.*", "", text)   # no division
    hdr = open(os.path.join(ROOT, "include", "svgr.h")).read()
    assert "#define SVGR_ABI_VERSION 6" in hdr
    import svgrasterize_amd as S
    from svgrasterize_amd import _abi, diff

    for name in ("svgr_compose_forward", "svgr_compose_backward", "svgr_compose_block", "svgr_compose_groups"):
        assert name in _abi.EXPORTS and re.search(rf"\b{name}\s*\(", hdr)
    for name in ("compose", "compose_backward", "compose_tensor", "render_tensor"):
        assert callable(getattr(diff, name)) and name in S.__all__
    assert callable(diff.premultiply) and callable(diff.unpremultiply)


def test_python_checks_come_before_any_device_work():
    """Wrong shapes and dtypes, non-finite paints or bg and mismatched n_paths are refused without a context."""
    from svgrasterize_amd import _abi, diff

    c = M.case("opaque_full", False)
    cover, paints, g = c["cover"], c["paints"], c["g"]
    before = dict(_abi.Context._by_device)
    bad_paints = paints.copy()
    bad_paints[1, 2] = np.nan
    for args, kw, exc in (((cover[0], paints), {}, ValueError), ((cover, paints[:2]), {}, ValueError), ((cover, paints[:, :3]), {}, ValueError),
                          ((cover, bad_paints), {}, ValueError), ((cover, paints.astype(np.float32)), {}, TypeError),
                          ((cover.astype(np.float16), paints), {}, TypeError), ((cover.astype(np.int32), paints), {}, TypeError),
                          ((cover, paints), dict(bg=(0.0, 0.0, 0.0)), ValueError), ((cover, paints), dict(bg=(0.0, 0.0, np.inf, 1.0)), ValueError),
                          ((cover, paints), dict(dtype=np.float16), TypeError), ((cover[:, :0], paints), {}, ValueError)):
        with pytest.raises(exc):
            diff.compose(*args, **kw)
        if "dtype" not in kw:
            with pytest.raises(exc):
                diff.compose_backward(*args, g, **kw)
    for grad, exc in ((g[:-1], ValueError), (g[..., :3], ValueError), (g.astype(np.float32), TypeError)):
        with pytest.raises(exc):
            diff.compose_backward(cover, paints, grad)
    assert _abi.Context._by_device == before
