"""Gradient paints in differentiable compositing on the host: csrc/svgr_gradpaint.h compiled by g++ (tests/gradpaint_harness.cpp)
against the oracle's gradient, fill and source-over, against the numpy restatement (tests/gradpaint_ref.py), against central
differences of that restatement, and at the points where the derivative takes one side (tests/gradpaint_cases.py has the cases).
No GPU."""
import os
import re

import numpy as np
import pytest

from tests import compose_cases as M
from tests import gradpaint_cases as G
from tests import gradpaint_ref as R
from tests.util import ROOT

CSRC = os.path.join(ROOT, "svgrasterize.py_amd", "csrc")
SUMS = ("paints", "m6", "geom", "stop_pos", "stop_rgba")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("name,with_bg", G.ALL)
def test_forward_equals_the_oracle(name, with_bg):
    """Dyadic cases: equal.  Generic ones: within 1e-13, the points tolerance of test_gpu_gradient_edges.py (the oracle's affine
    map and dot product are BLAS calls).  The restatement: equal everywhere."""
    c = G.case(name, with_bg)
    image = G.harness_forward(c["cover"], c["paints"], c["gp"], c["bg"], c["origin"])
    want = G.oracle_image(c["cover"], c["paints"], c["gp"], c["bg"], c["origin"])
    assert image.shape == c["cover"].shape[1:] + (4,) and np.isfinite(image).all()
    if c["dyadic"]:
        assert np.array_equal(image, want), float(np.abs(image - want).max())
    else:
        assert np.abs(image - want).max() <= 1e-13, float(np.abs(image - want).max())
    assert np.array_equal(_bits(image), _bits(R.forward(c["cover"], c["paints"], c["gp"], c["bg"], c["origin"])))
    gp = c["gp"]
    used = G.harness_backward(c["cover"], c["paints"], gp, c["g"], c["bg"], c["origin"])[2]
    for p in np.nonzero(gp.kind)[0]:   # every stop of the case is used by some pixel
        assert set(np.unique(used[:, :, p])) >= set(range(gp.path_stop_off[p + 1] - gp.path_stop_off[p])), (name, p)


def test_the_cases_cover_the_issue():
    kinds, spreads, counts = set(), set(), set()
    for name in G.CASES:
        gp = G.case(name, False)["gp"]
        for p in np.nonzero(gp.kind)[0]:
            kinds.add(int(gp.kind[p])), spreads.add((int(gp.kind[p]), int(gp.spread[p]))), counts.add(int(gp.path_stop_off[p + 1] - gp.path_stop_off[p]))
    assert kinds == {1, 2} and spreads == {(k, s) for k in (1, 2) for s in (0, 1, 2)} and counts >= {1, 2, 4}
    step = G.case("linear_step", False)["gp"].stop_pos
    assert step[1] == step[2]                                                   # a hard step
    mixed = G.case("mixed", True)
    assert mixed["gp"].kind.tolist() == [0, 1, 2, 0] and mixed["origin"] != (0, 0)   # a gradient over a solid and under a solid
    assert not np.array_equal(mixed["gp"].m6[1], G.IDENT) and (mixed["paints"][2] == 0.7).all()


def test_solid_only_input_equals_the_compose_harness():
    """kind 0 everywhere: the image, grad_cover and grad_paints of compose_harness bit for bit, and nothing else."""
    for name, with_bg in (("scene", True), ("opaque_full", False)):
        c = M.case(name, with_bg)
        gp = G.make_gp([None] * len(c["cover"]))
        assert np.array_equal(_bits(G.harness_forward(c["cover"], c["paints"], gp, c["bg"])), _bits(M.harness_forward(c["cover"], c["paints"], c["bg"])))
        grad_cover, sums, _used = G.harness_backward(c["cover"], c["paints"], gp, c["g"], c["bg"])
        want_cover, want_paints = M.harness_backward(c["cover"], c["paints"], c["g"], c["bg"])
        assert np.array_equal(_bits(grad_cover), _bits(want_cover)) and np.array_equal(_bits(sums["paints"]), _bits(want_paints))
        assert not sums["m6"].any() and not sums["geom"].any() and sums["stop_pos"].shape == (0,)


@pytest.mark.parametrize("name,with_bg", G.ALL)
def test_harness_equals_reference(name, with_bg):
    """grad_cover bit for bit (per pixel, the same order); every summed output within what the order of its sum can change."""
    c = G.case(name, with_bg)
    grad_cover, sums, _used = G.harness_backward(c["cover"], c["paints"], c["gp"], c["g"], c["bg"], c["origin"])
    ref_cover, ref_sums, tol = R.backward(c["cover"], c["paints"], c["gp"], c["g"], c["bg"], c["origin"])
    assert np.array_equal(_bits(grad_cover), _bits(ref_cover)), float(np.abs(grad_cover - ref_cover).max())
    for k in SUMS:
        assert np.isfinite(sums[k]).all()
        assert (np.abs(sums[k] - ref_sums[k]) <= tol[k]).all(), (k, float((np.abs(sums[k] - ref_sums[k]) - tol[k]).max()))
    gp = c["gp"]
    assert not sums["m6"][gp.kind == 0].any() and not sums["geom"][gp.kind == 0].any() and not sums["geom"][gp.kind == 2, 3].any()
    if name == "linear_one_stop":
        assert not sums["m6"].any() and not sums["geom"].any() and not sums["stop_pos"].any() and sums["stop_rgba"].all()
    elif gp.kind.any():
        assert all(sums[k].any() for k in SUMS)


@pytest.mark.parametrize("name,with_bg", G.FD)
def test_backward_equals_central_differences(name, with_bg):
    """Every component of every parameter array, steps H and 2 H of the restatement: per component twice the Richardson estimate
    |fd(2H) - fd(H)| / 3 plus 2^-50 * sum |g * C| / H.  The builder's conditions keep every difference off the kinks."""
    c = G.case(name, with_bg)
    grad_cover, sums, _used = G.harness_backward(c["cover"], c["paints"], c["gp"], c["g"], c["bg"], c["origin"])
    fd, tol = G.central_differences(c)
    got = dict(sums, cover=grad_cover)
    worst = 0.0
    for k in ("cover",) + SUMS:
        err = np.abs(got[k] - fd[k])
        ratio = float((err / tol[k]).max()) if err.size else 0.0
        worst = max(worst, ratio)
        print(f"{name} bg {with_bg} {k}: max |grad| {np.abs(got[k]).max() if err.size else 0.0:.3e} err {err.max() if err.size else 0.0:.3e} worst err / tol {ratio:.3f}")
        assert (err <= tol[k]).all(), (k, ratio)
    assert np.abs(grad_cover).max() > 1e-3 and float(np.median(tol["paints"])) < 1e-5   # (the bound is small against the gradients)
    print(f"{name} bg {with_bg}: worst err / tol {worst:.3f}")


# ------------------------------------------------------------------------------------------------ the one-sided points
EDGE_GEOM = (0.5, 0.5, 8.5, 8.5)   # vec = (8, 8) from the first pixel's centre: offsets (i + j) / 16 exactly


def _edge(spread, pos, kind=1, geom=EDGE_GEOM, rows=12, cols=11, seed=70):
    rng = np.random.default_rng(seed)
    gp = G.make_gp([dict(kind=kind, spread=spread, geom=geom, pos=pos, rgba=G.stop_colours(rng, len(pos)))])
    cover, g = rng.uniform(0.2, 1.0, (1, rows, cols)), rng.standard_normal((rows, cols, 4))
    paints = np.ones((1, 4))
    image = G.harness_forward(cover, paints, gp)
    grad_cover, sums, used = G.harness_backward(cover, paints, gp, g)
    assert np.isfinite(image).all() and np.isfinite(grad_cover).all() and all(np.isfinite(sums[k]).all() for k in SUMS)
    i, j = np.indices((rows, cols))
    return gp, cover, image, sums, used[:, :, 0], i + j


def test_on_a_stop_and_on_the_clamps_pad():
    """t on the first stop: the low clamp.  t on an inner or the last stop: the segment that ends there, ratio 1, so the colour
    is that stop's.  Beyond the last: the high clamp."""
    gp, cover, image, sums, used, ij = _edge(0, (0.25, 0.5, 1.0))
    assert (used[ij <= 4] == [0, 0]).all() and (used[ij == 5] == [0, 1]).all()       # 4 / 16 is ON pos[0]
    assert (used[ij == 8] == [0, 1]).all() and (used[ij == 9] == [1, 2]).all()       # 8 / 16 is ON pos[1]
    assert (used[ij == 16] == [1, 2]).all() and (used[ij >= 17] == [2, 2]).all()     # 16 / 16 is ON pos[2]
    for at, s in ((4, 0), (8, 1), (16, 2), (20, 2)):
        sel = ij == at
        assert np.array_equal(image[sel], gp.stop_rgba[s] * cover[0][sel][:, None])
    assert sums["stop_pos"].all() and sums["stop_rgba"].all()


def test_on_a_wrap_and_on_a_fold():
    """Repeat: t == 1 wraps to 0, the low clamp.  Reflect: t == 1 folds with slope -1 and belongs to the segment that ends at
    1; t == 0 has slope +1.  Stops no pixel touches have a gradient of exactly 0."""
    gp, cover, image, sums, used, ij = _edge(1, (0.0, 0.5, 1.0, 1.5, 2.0))
    assert (used[ij == 16] == [0, 0]).all() and (used[ij == 0] == [0, 0]).all() and (used[ij == 17] == [0, 1]).all()
    assert np.array_equal(image[ij == 16], gp.stop_rgba[0] * cover[0][ij == 16][:, None])
    assert used.max() == 2 and not sums["stop_pos"][3:].any() and not sums["stop_rgba"][3:].any() and sums["stop_rgba"][:3].all()
    gp, cover, image, sums, used, ij = _edge(2, (0.0, 0.5, 1.0, 1.5, 2.0))
    assert (used[ij == 16] == [1, 2]).all() and (used[ij == 0] == [0, 0]).all() and (used[ij == 17] == [1, 2]).all()
    assert np.array_equal(image[ij == 16], gp.stop_rgba[2] * cover[0][ij == 16][:, None])
    assert not sums["stop_pos"][3:].any() and not sums["stop_rgba"][3:].any()
    # the fold's slope: one pixel on each side of t == 1, alone in the plane, pulls the geometry opposite ways
    for at, sign in ((15, 1.0), (17, -1.0)):
        rgba = np.array([[0.0, 0.0, 0.0, 0.2], [0.0, 0.0, 0.0, 0.6], [0.0, 0.0, 0.0, 1.0]])
        one = G.make_gp([dict(kind=1, spread=2, geom=EDGE_GEOM, pos=(0.0, 0.5, 1.0), rgba=rgba)])
        cover = (ij == at).astype(np.float64)[None]
        g = np.zeros((12, 11, 4))
        g[..., 3] = 1.0   # the loss is the alpha under the pixel(s): it grows with u
        _gc, sums, _used = G.harness_backward(cover, np.ones((1, 4)), one, g)
        assert np.sign(sums["m6"][0, 2]) == sign and np.sign(sums["m6"][0, 5]) == sign, (at, sums["m6"])


def test_the_radial_centre_pixel_and_one_stop():
    """A pixel centre ON the radial centre: t == 0, no geometry or transform terms from it, nothing NaN.  One stop: its colour
    everywhere, weight 1 on it, nothing to its position, the geometry or the transform."""
    gp, cover, image, sums, used, _ij = _edge(0, (-0.5, 0.5, 1.0), kind=2, geom=(3.5, 4.5, 6.0))
    assert (used[3, 4] == [0, 1]).all() and sums["m6"].any() and sums["geom"][0, :3].all()   # t == 0 inside the first segment
    alone = np.zeros_like(cover)
    alone[0, 3, 4] = 1.0
    g = np.random.default_rng(72).standard_normal((12, 11, 4))
    grad_cover, sums, _used = G.harness_backward(alone, np.ones((1, 4)), gp, g)
    assert np.isfinite(grad_cover).all() and all(np.isfinite(sums[k]).all() for k in SUMS)
    assert not sums["m6"].any() and not sums["geom"].any() and sums["stop_pos"][:2].all() and sums["stop_rgba"][:2].all() and not sums["stop_rgba"][2].any()
    gp, cover, image, sums, used, _ij = _edge(0, (0.0, 0.5, 1.0), kind=2, geom=(3.5, 4.5, 6.0))   # t == 0 ON the first stop: the clamp
    assert (used[3, 4] == [0, 0]).all() and np.array_equal(image[3, 4], gp.stop_rgba[0] * cover[0, 3, 4])
    for kind, geom in ((1, EDGE_GEOM), (2, (3.5, 4.5, 6.0))):
        gp, cover, image, sums, used, _ij = _edge(2, (0.5,), kind=kind, geom=geom)
        assert (used == 0).all() and np.array_equal(image, gp.stop_rgba[0] * cover[0][..., None])
        assert not sums["m6"].any() and not sums["geom"].any() and not sums["stop_pos"].any() and sums["stop_rgba"].all()


def test_a_hard_step_never_selects_the_empty_segment():
    c = G.case("linear_step", False)
    _gc, sums, used = G.harness_backward(c["cover"], c["paints"], c["gp"], c["g"])
    pairs = {tuple(u) for u in used[:, :, 0].reshape(-1, 2)}
    assert (1, 2) not in pairs and {(0, 0), (0, 1), (2, 3), (3, 3)} <= pairs
    assert all(np.isfinite(sums[k]).all() for k in SUMS)


def test_float32_planes_widen_exactly():
    cover, paints, gp, _g = G.random_scene(7, 3, 4, 9)
    c32 = cover.astype(np.float32)
    assert np.array_equal(G.harness_forward(c32, paints, gp), G.harness_forward(c32.astype(np.float64), paints, gp))


# ------------------------------------------------------------------------------------------------ the Python surface
def _stops(n, seed=80):
    rng = np.random.default_rng(seed)
    return [(float(o), c) for o, c in zip(np.linspace(0.0, 1.0, n), G.stop_colours(rng, n))]


def test_gradient_paints_against_hand_written_arrays():
    from svgrasterize_amd import Transform, diff
    from svgrasterize_amd.paint import GradLinear, GradRadial, _stops_colorspace

    stops2, stops3 = _stops(2), _stops(3, 81)
    gt = Transform().translate(2.0, -1.0).scale(2.0, 4.0)
    lin = GradLinear((1.5, 0.75), (9.5, 8.75), stops2, None, "reflect", False, None)
    rad = GradRadial((5.0, 4.0), 6.0, None, None, stops3, gt, "repeat", False, True)
    solid = np.array([0.1, 0.2, 0.3, 0.5])
    render = Transform().translate(3.0, 5.0).scale(0.5, 0.25)
    gp, rows = diff.gradient_paints([solid, lin, rad], render, linear_rgb=False)
    assert isinstance(gp, diff.GradientPaints)
    assert gp.kind.tolist() == [0, 1, 2] and gp.spread.tolist() == [0, 2, 1] and gp.path_stop_off.tolist() == [0, 0, 2, 5]
    assert all(a.dtype == np.int32 for a in (gp.kind, gp.spread, gp.path_stop_off))
    assert np.array_equal(rows, [[0.1, 0.2, 0.3, 0.5], [1.0] * 4, [1.0] * 4])
    assert np.array_equal(gp.geom, [[0.0] * 4, [1.5, 0.75, 9.5, 8.75], [5.0, 4.0, 6.0, 0.0]])
    inv = np.linalg.inv(render.m)
    assert np.array_equal(gp.m6[0], [1, 0, 0, 0, 1, 0]) and np.array_equal(gp.m6[1], inv[:2].ravel())
    assert np.array_equal(gp.m6[2], np.dot(np.linalg.inv(gt.m), inv)[:2].ravel())
    point = np.array([7.25, 3.5, 1.0])   # a pixel centre -> user space -> gradient space
    assert np.allclose(gp.m6[2].reshape(2, 3) @ point, (np.linalg.inv(gt.m) @ (inv @ point))[:2], rtol=0, atol=1e-12)
    want2, want3 = _stops_colorspace(stops2, False), _stops_colorspace(stops3, True)   # (the radial's own linear_rgb wins)
    assert np.array_equal(gp.stop_pos, [o for o, _ in want2 + want3]) and np.array_equal(gp.stop_rgba, [c for _, c in want2 + want3])
    assert not np.array_equal(gp.stop_rgba[:2], [c for _, c in stops2])
    ident = diff.gradient_paints([lin])[0]
    assert np.array_equal(ident.m6, [[1, 0, 0, 0, 1, 0]]) and ident.path_stop_off.tolist() == [0, 2]
    for bad in ([GradRadial((5.0, 4.0), 6.0, (4.0, 4.0), None, stops3, None, "pad", False, None)],
                [GradRadial((5.0, 4.0), 6.0, None, 1.0, stops3, None, "pad", False, None)],
                [GradLinear((0.0, 0.0), (1.0, 0.0), stops2, None, "pad", True, None)],
                [GradLinear((0.0, 0.0), (1.0, 0.0), _stops(33), None, "pad", False, None)],
                [GradLinear((0.0, 0.0), (1.0, 0.0), [], None, "pad", False, None)],
                [GradLinear((0.0, 0.0), (1.0, 0.0), stops2, None, "mirror", False, None)],
                [np.zeros(3)], ["red"], []):
        with pytest.raises(ValueError):
            diff.gradient_paints(bad)
    assert diff.gradient_paints([GradLinear((0.0, 0.0), (1.0, 0.0), _stops(32), None, "pad", False, None)])[0].path_stop_off.tolist() == [0, 32]


def test_header_rules_and_exports():
    """The header's own rules (three fused multiply-adds and no contraction pragma, SVGR_HD throughout), the ABI additions, the
    Makefile's dependency lines and the Python surface."""
    text = open(os.path.join(CSRC, "svgr_gradpaint.h")).read()
    code = re.sub(r"//.*", "", text)
    assert code.count("fma(") == 1 and "xform_point(" in code and "fp contract" not in text.lower() and "SVGR_HD" in text   # (xform_point has the other two)
    assert '#include "svgr_core.h"' in text and '#include "svgr_compose.h"' in text
    hdr = open(os.path.join(ROOT, "include", "svgr.h")).read()
    assert "#define SVGR_ABI_VERSION 6" in hdr and "svgr_painted_desc" in hdr
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert sum("svgr_gradpaint.h" in line for line in make.splitlines() if line.startswith(("svgr_hip.o:", "lint:"))) == 2
    import svgrasterize_amd as S
    from svgrasterize_amd import _abi, diff

    for name in ("svgr_compose_painted_forward", "svgr_compose_painted_backward"):
        assert name in _abi.EXPORTS and re.search(rf"\b{name}\s*\(", hdr)
    for name in ("GradientPaints", "gradient_paints", "compose_painted", "compose_painted_backward", "compose_painted_tensor", "render_painted_tensor"):
        assert callable(getattr(diff, name)) and name in S.__all__ and getattr(S, name) is getattr(diff, name)
    assert diff.GradientPaints._fields == ("kind", "spread", "path_stop_off", "m6", "geom", "stop_pos", "stop_rgba") == R.GP._fields


def test_python_checks_come_before_any_device_work():
    """Wrong shapes and dtypes, non-finite values, p0 == p1, r <= 0, decreasing positions and every topology error are refused
    without a context, and without a call into the library."""
    from svgrasterize_amd import _abi, diff

    c = G.case("mixed", False)
    cover, paints, g, origin = c["cover"], c["paints"], c["g"], c["origin"]
    gp = diff.GradientPaints(*c["gp"])
    assert gp.kind.tolist() == [0, 1, 2, 0] and gp.path_stop_off.tolist() == [0, 0, 3, 7, 7]
    before = dict(_abi.Context._by_device)

    def put(name, index, value):
        a = np.array(getattr(gp, name)).copy()
        a[index] = value
        return gp._replace(**{name: a})

    many = gp._replace(path_stop_off=np.array([0, 0, 36, 40, 40], dtype=np.int32), stop_pos=np.linspace(0, 1, 40), stop_rgba=np.ones((40, 4)))
    cases = [
        (put("kind", 1, 3), ValueError), (put("kind", 0, -1), ValueError), (put("spread", 2, 3), ValueError), (put("spread", 1, -1), ValueError),
        (put("path_stop_off", 0, 1), ValueError), (put("path_stop_off", 4, 6), ValueError), (put("path_stop_off", 2, 8), ValueError),
        (put("path_stop_off", 1, 1), ValueError),                                    # the solid path 0 would own a stop
        (put("path_stop_off", 2, 0), ValueError),                                    # the linear path would own none
        (many, ValueError),                                                          # 36 stops on a path
        (gp._replace(kind=gp.kind[:3]), ValueError), (gp._replace(spread=np.zeros(5, dtype=np.int32)), ValueError),
        (gp._replace(path_stop_off=gp.path_stop_off[:4]), ValueError), (gp._replace(kind=gp.kind.astype(np.float64)), TypeError),
        (gp._replace(m6=gp.m6[:3]), ValueError), (gp._replace(m6=gp.m6[:, :5]), ValueError), (gp._replace(geom=gp.geom[:, :3]), ValueError),
        (gp._replace(stop_pos=gp.stop_pos[:6]), ValueError), (gp._replace(stop_rgba=gp.stop_rgba[:, :3]), ValueError),
        (gp._replace(stop_rgba=gp.stop_rgba[:6]), ValueError), (gp._replace(stop_pos=gp.stop_pos.reshape(-1, 1)), ValueError),
        (gp._replace(m6=gp.m6.astype(np.float32)), TypeError), (gp._replace(geom=gp.geom.astype(np.float32)), TypeError),
        (gp._replace(stop_pos=gp.stop_pos.astype(np.float32)), TypeError), (gp._replace(stop_rgba=gp.stop_rgba.astype(np.float16)), TypeError),
        (put("m6", (1, 2), np.nan), ValueError), (put("geom", (2, 0), np.inf), ValueError), (put("stop_pos", 1, np.nan), ValueError),
        (put("stop_rgba", (4, 2), -np.inf), ValueError),
        (put("geom", (1, slice(2, 4)), gp.geom[1, :2]), ValueError),                 # p0 == p1
        (put("geom", (2, 2), 0.0), ValueError), (put("geom", (2, 2), -1.0), ValueError),   # r <= 0
        (put("stop_pos", 1, gp.stop_pos[0] - 0.01), ValueError), (put("stop_pos", 6, gp.stop_pos[5] - 0.01), ValueError),   # decreasing
        (tuple(gp)[:6], TypeError), (None, TypeError),
    ]
    for bad, exc in cases:
        with pytest.raises(exc):
            diff.compose_painted(cover, paints, bad, origin=origin)
        with pytest.raises(exc):
            diff.compose_painted_backward(cover, paints, bad, g, origin=origin)
    bad_paints = paints.copy()
    bad_paints[1, 2] = np.nan
    for args, kw, exc in (((cover[0], paints, gp), {}, ValueError), ((cover, paints[:2], gp), {}, ValueError), ((cover, bad_paints, gp), {}, ValueError),
                          ((cover.astype(np.float16), paints, gp), {}, TypeError), ((cover, paints.astype(np.float32), gp), {}, TypeError),
                          ((cover, paints, gp), dict(bg=(0.0, 0.0, 0.0)), ValueError), ((cover, paints, gp), dict(origin=(1,)), ValueError),
                          ((cover, paints, gp), dict(origin=(0, 2 ** 31)), ValueError), ((cover, paints, gp), dict(origin="ab"), ValueError),
                          ((cover, paints, gp), dict(dtype=np.float16), TypeError)):
        with pytest.raises(exc):
            diff.compose_painted(*args, **kw)
        if "dtype" not in kw:
            with pytest.raises(exc):
                diff.compose_painted_backward(*args, g, **kw)
    for grad, exc in ((g[:-1], ValueError), (g[..., :3], ValueError), (g.astype(np.float32), TypeError)):
        with pytest.raises(exc):
            diff.compose_painted_backward(cover, paints, gp, grad)
    same = put("stop_pos", 1, gp.stop_pos[0])   # equal neighbours are a hard step, not an error: checked up to the library call
    assert (np.diff(same.stop_pos[:3]) >= 0).all() and diff._painted_inputs(cover, paints, same, None, origin)[4][2].tolist() == [0, 0, 3, 7, 7]
    assert _abi.Context._by_device == before
