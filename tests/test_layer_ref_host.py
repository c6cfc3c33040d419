"""tests/layer_ref.py pinned on the host: its convolution against scipy's direct sum, and every function against the reference's
own outputs in tests/golden/{filter_kat,gradient_blur_kat,canvasfn_kat}.npz at the tolerances those files are held to elsewhere.
What the GPU comparison in test_gpu_layer_kernels.py rests on."""
import numpy as np
import pytest

from tests import layer_ref as L
from tests.util import assert_close64, load, meta


def _box(offset, img):
    return (int(offset[0]), int(offset[1]), img.shape[0], img.shape[1])


def _img3(a):
    a = np.asarray(a, dtype=np.float64)
    return a[..., None] if a.ndim == 2 else a


def _union_blend(layers, mode, k4=None):
    """canvas_merge_union(full=True) with a blend other than OVER: the first layer on a zero canvas, the others blended in."""
    ub = L._union([b for _, b in layers])
    out, _ = L.over(np.zeros((ub[2], ub[3], 4)), ub, layers[0][0], layers[0][1], first=True)
    for img, b in layers[1:]:
        out, _ = L.blend(out, ub, img, b, mode, k4)
    return np.asarray(out, dtype=np.float64), ub


def _compose(mode, dst, src):
    """canvas_compose (S:277-298) of two images of one size through the per-step functions, RGBA result."""
    d, s = _img3(dst), _img3(src)
    bb = (0, 0, d.shape[0], d.shape[1])
    out, _ = L.crop4(bb, d, bb)
    if mode == 0:
        out, _ = L.over(out, bb, s, bb)
    elif mode == 2:
        out, _ = L.in_(out, bb, s, bb)
    elif isinstance(mode, tuple):
        out, _ = L.blend(out, bb, s, bb, L.COMPOSE_ARITHMETIC, mode)
    else:
        out, _ = L.blend(out, bb, s, bb, mode)
    return np.asarray(out, dtype=np.float64)


def test_convolution_is_scipys_direct_sum():
    from scipy.signal import convolve as sp_convolve

    rng = np.random.default_rng(1)
    for (rows, cols), (kw, kh) in (((9, 14), (3, 5)), ((2, 3), (7, 4)), ((1, 1), (5, 5)), ((20, 6), (1, 9)), ((5, 31), (6, 1)), ((4, 4), (4, 4))):
        img = rng.uniform(-1.0, 2.0, (rows, cols, 4))
        k = rng.uniform(-1.0, 1.0, (kw, kh))
        want, tol = L.convolve(img, k, rank1=False)
        assert want.shape == (rows + kw - 1, cols + kh - 1, 4) and want.dtype == np.longdouble
        sp = sp_convolve(img, k[..., None], mode="full", method="direct")
        # (scipy sums kw * kh products in double: inside the bound of a kw + kh chain only for these small kernels -- its own
        #  first-order bound is used instead)
        assert np.abs(sp - want).max() <= (kw * kh + 1) * L.U * np.abs(img).max() * np.abs(k).sum()
        assert tol == pytest.approx(2.0 ** -52 * np.abs(img).max() * (kw + kh + 4) * np.abs(k).sum(), rel=1e-12)
    # the rank-1 allowance, and the rule that decides it
    g = np.exp(-np.linspace(-2, 2, 7) ** 2)
    k = np.outer(g, g[:5]) / 3.0
    assert L.is_rank1(k) and not L.is_rank1(rng.random((3, 5))) and not L.is_rank1(k[:1]) and not L.is_rank1(np.outer([1.0, 2.0, 1.0], [1.0, 0.0, -1.0]))
    img = rng.random((4, 4, 4))
    assert L.convolve(img, k)[1] - L.convolve(img, k, rank1=False)[1] == pytest.approx(2.0 ** -52 * img.max() * 8 * 35 * k.max())


def test_blur_known_answers():
    g = load("gradient_blur_kat.npz")
    for j, b in enumerate(meta(g)["blur"]):
        img, _ = L.convert(g[f"b{j}_in"], L.convert_ops(True, b["in_linear_rgb"], False, True))
        out, _ = L.convolve(np.asarray(img, dtype=np.float64), g[f"b{j}_kernel"])
        assert_close64(out, g[f"b{j}_out"], atol=1e-14, what=f"blur {j}")


def test_filter_known_answers():
    z = load("filter_kat.npz")
    m = meta(z)
    for k, c in enumerate(m["compose"]):
        arithmetic = isinstance(c["mode"], list)
        layers = []
        for j, l in enumerate(c["layers"]):
            img = z[f"c{k}_in{j}"]
            if img.shape[2] == 4:   # (a single channel is alpha: flags only)
                img = np.asarray(L.convert(img, L.convert_ops(l["pre_alpha"], l["linear_rgb"], not arithmetic, c["linear_rgb"]))[0], dtype=np.float64)
            layers.append((img, _box(l["offset"], img)))
        out, ub = _union_blend(layers, L.COMPOSE_ARITHMETIC if arithmetic else c["mode"], c["mode"] if arithmetic else None)
        assert list(ub[:2]) == c["out_offset"]
        assert_close64(out, z[f"c{k}_out"], atol=1e-14, what=f"compose case {k}")
    for j, c in enumerate(m["cmatrix"]):
        img, _ = L.convert(z[f"m{j}_in"], L.convert_ops(c["pre_alpha"], c["linear_rgb"], False, True))
        out, _ = L.color_matrix(np.asarray(img, dtype=np.float64), z[f"m{j}_matrix"])
        assert_close64(out, z[f"m{j}_out"], atol=1e-14, what=f"color matrix {j}")
    for j, c in enumerate(m["morph"]):
        img, _ = L.convert(z[f"p{j}_in"], L.convert_ops(c["pre_alpha"], c["linear_rgb"], True, True))
        out, tol = L.morphology(np.asarray(img, dtype=np.float64), c["x"], c["y"], c["method"] == "max")
        assert tol == 0
        assert_close64(out, z[f"p{j}_out"], atol=1e-14, what=f"morphology {j}")


def test_canvas_function_known_answers():
    z = load("canvasfn_kat.npz")
    seen = set()
    for i, c in enumerate(meta(z)):
        fn = c["fn"]
        mode = tuple(c["mode"]) if isinstance(c.get("mode"), list) else c.get("mode")
        seen.add((fn, mode if not isinstance(mode, tuple) else 5))
        if fn == "compose":
            got, want = _compose(mode, z[f"{i}_dst"], z[f"{i}_src"]), z[f"{i}_out"]
            if want.shape[-1] == 1:   # (numpy's broadcast kept one channel: it is the alpha of the RGBA form)
                got = got[..., 3:]
            assert_close64(got, want, atol=1e-15, what=f"canvas_compose case {i}")
        elif fn == "merge_at":
            base, ovl = z[f"{i}_base"], z[f"{i}_over"]
            bb, sb = (0, 0) + base.shape[:2], _box(c["offset"], ovl)
            ov = L._overlap(bb, sb)
            assert (ov is None) == c["none"]
            out, _ = L.over(base, bb, ovl, sb)
            out = np.asarray(out, dtype=np.float64)
            if ov is not None:
                out[ov[0]] = L.clip01(out[ov[0]])[0]   # (the touched region is clipped, S:326)
            assert_close64(out, z[f"{i}_out"], atol=1e-15, what=f"canvas_merge_at case {i}")
        elif fn == "union":
            layers = [(z[f"{i}_in{j}"], _box(o, z[f"{i}_in{j}"])) for j, o in enumerate(c["offsets"])]
            if mode == 0:
                out, _, ub = L.compose_over([(im, b, 0) for im, b in layers])
            elif mode == 2:   # (IN on the union canvas: every layer zero-extended first)
                ub = L._union([b for _, b in layers])
                out = L.crop4(ub, *layers[0])[0]
                for im, b in layers[1:]:
                    out, _ = L.in_(out, ub, L.crop4(ub, im, b)[0], ub)
            else:
                out, ub = _union_blend(layers, mode)
            assert list(ub[:2]) == c["offset"]
            assert_close64(out, z[f"{i}_out"], atol=1e-15, what=f"canvas_merge_union case {i}")
        elif fn == "intersect":
            layers = [(_img3(z[f"{i}_in{j}"]), _box(o, z[f"{i}_in{j}"])) for j, o in enumerate(c["offsets"])]
            if mode == 2:
                out, _, ib = L.compose_in([(im, b, 0) for im, b in layers])
            else:
                ib = L._intersection([b for _, b in layers])
                out = L.crop4(ib, *layers[0])[0]
                for im, b in layers[1:]:
                    out, _ = L.over(out, ib, im, b)
            assert list(ib[:2]) == c["offset"]
            assert_close64(out, z[f"{i}_out"], atol=1e-15, what=f"canvas_merge_intersect case {i}")
    assert {("compose", q) for q in (0, 1, 2, 3, 4, 5)} <= seen and ("merge_at", None) in seen and ("intersect", 2) in seen


def test_the_selections_and_single_roundings():
    """The functions no fixture holds, against their definitions written another way."""
    rng = np.random.default_rng(2)
    img = rng.uniform(-0.5, 1.5, (6, 7, 4))
    lum, tol = L.luminance(img)
    assert np.abs(np.asarray(lum, dtype=np.float64) - (img[..., :3] @ np.array([0.2125, 0.7154, 0.072])) * img[..., 3]).max() <= tol.max() and tol.max() < 1e-14
    bg, tol = L.background(img, [0.1, 0.2, 0.3, 1.0])
    assert np.abs(np.asarray(bg, dtype=np.float64) - (img + np.array([0.1, 0.2, 0.3, 1.0]) * (1 - img[..., 3:]))).max() <= tol.max() < 1e-14
    x = np.array([-0.0, -1e-300, 0.5, 1.0, 1.0 + 1e-16, 2.0, -3.0, np.nan, 0.5 / 255, 1.5 / 255, 2.5 / 255])
    assert L.to_rgba8(x)[0].tolist() == [0, 0, 128, 255, 255, 255, 0, 0, 0, 2, 2]
    c = L.clip01(x)[0]
    assert np.signbit(c[0]) and c[1] == 0.0 and c[5] == 1.0 and c[6] == 0.0 and np.isnan(c[7])
    tie = (np.float64(np.float32(0.3)) + np.float64(np.nextafter(np.float32(0.3), np.float32(1)))) / 2
    f = L.to_f32(np.array([tie, 2.0, -1.0, np.nan, 1e-40, 2.0 ** -150, 1.5 * 2.0 ** -149]), False)[0]
    assert f.dtype == np.float32 and f[0] in (np.float32(0.3), np.nextafter(np.float32(0.3), np.float32(1))) and (f[0].view(np.uint32) & 1) == 0
    assert f[1] == 2 and f[2] == -1 and np.isnan(f[3]) and f[4] != 0 and f[5] == 0 and f[6] == np.float32(2.0 ** -148)
    assert L.to_f32(np.array([2.0, -1.0, np.nan]), True)[0].tolist()[:2] == [1.0, 0.0]
    m, _ = L.morphology(np.array([[[1.0], [np.nan], [3.0]], [[np.nan], [np.nan], [0.5]]]), 2, 2, True)
    assert m.shape == (1, 2, 1) and m[0, 0, 0] == 1.0 and m[0, 1, 0] == 3.0
    assert np.isnan(L.morphology(np.full((2, 2, 4), np.nan), 2, 2, False)[0]).all()
    # the sRGB pair in long double against mpmath at 30 digits
    import mpmath

    mpmath.mp.dps = 30
    v = np.array([[0.0, 0.04045, 0.2, 1.0]])
    lin, tol = L.convert(v, L.SRGB_TO_LINEAR)
    assert tol == 1e-14
    for got, s in zip(lin[0, :3], v[0, :3]):
        want = mpmath.mpf(float(s)) / mpmath.mpf(12.92) if s <= 0.04045 else ((mpmath.mpf(float(s)) + mpmath.mpf(0.055)) / mpmath.mpf(1.055)) ** mpmath.mpf(2.4)
        assert abs(mpmath.mpf(float(got)) - want) < 1e-16
    back, _ = L.convert(np.asarray(lin, dtype=np.float64), L.LINEAR_TO_SRGB)
    ok = v != 0.04045   # (the two branches of the sRGB curve meet to 3e-8 only: the round trip is not exact at the joint)
    assert np.abs(np.asarray(back, dtype=np.float64) - v)[ok].max() < 1e-15
    assert [L.convert_ops(*a) for a in ((True, False, False, True), (True, False, True, True), (False, True, True, False), (True, True, False, True))] == [3, 11, 12, 1]
    # the short-arithmetic bounds at unit magnitude stay inside the 1e-14 of the known-answer tests
    one = np.ones((1, 1, 4))
    bb = (0, 0, 1, 1)
    worst = max(float(np.max(t)) for t in (L.over(one, bb, one, bb)[1], L.in_(one, bb, one, bb)[1], L.blend(one, bb, one, bb, 4)[1],
                                           L.blend(one, bb, one, bb, 5, (1, 1, 1, 1))[1], L.background(one, [1, 1, 1, 1])[1],
                                           L.color_matrix(one, np.ones((4, 5)))[1], L.luminance(one)[1]))
    assert worst <= 1e-14
