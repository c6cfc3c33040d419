"""SVG <image> on the device: svgr_image_upload + svgr_image_fill against the numpy restatement in tests/image_ref.py
(nearest, bilinear, trilinear; both colour spaces; odd sizes), documents with <image> rendered through the loader against
the restatement and against the same scene built by hand with Scene.image, the per-paint upload cache, and a 2048^2 image
rotated onto a 4096^2 canvas."""
import base64
import ctypes as C
import math

import numpy as np
import pytest

from tests import image_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-6


@pytest.fixture(scope="module")
def S():
    import svgrasterize_amd as S

    S.Context.get()
    return S


def _device_fill(pixels, inv_m, smooth, linear_rgb, bbox, mask=None):
    """svgr_image_fill over bbox (r0, c0, rows, cols) with the given (rows, cols) mask (ones if None)."""
    from svgrasterize_amd import _abi, paint

    ctx = _abi.Context.get()
    r0, c0, rows, cols = bbox
    if mask is None:
        mask = np.ones((rows, cols))
    levels = _abi.image_upload(ctx, pixels, linear_rgb)
    im = _abi.ImageArgs()
    im.inv_m6 = (C.c_double * 6)(*np.asarray(inv_m, dtype=np.float64)[:2].ravel())
    im.height, im.width = pixels.shape[:2]
    im.smooth = int(smooth)
    im.lod = paint.image_lod(inv_m, len(_abi.image_levels(*pixels.shape[:2]))) if smooth else 0.0
    mbuf = ctx.from_host(np.ascontiguousarray(mask, dtype=np.float64))
    out = ctx.alloc(rows * cols * 32)
    _abi._check(ctx.lib.svgr_image_fill(ctx.handle, C.byref(im), levels.handle, mbuf.handle, (C.c_int64 * 4)(*bbox), out.handle))
    return out.download((rows, cols, 4), np.float64)


def _swap():
    from svgrasterize_amd.geometry import Transform

    return Transform().matrix(0, 1, 0, 1, 0, 0)


def _case_transform(name, h, w):
    """(image -> device transform, bbox) of a named case."""
    from svgrasterize_amd.geometry import Transform

    if name == "identity":
        return Transform(), (0, 0, w, h)   # (used as given: u, the image's columns, runs along the device rows here)
    if name == "up3":
        return _swap().translate(2.5, 1.25).scale(3.0), (0, 0, 3 * h + 6, 3 * w + 6)
    if name == "rot30":
        return _swap().translate(w * 0.9, 4).rotate(math.radians(30)), (-3, -2, int(1.6 * h) + 8, int(1.6 * w) + 8)
    if name == "swap":
        return _swap().translate(3.25, -1.5).scale(1.7, 1.3), (0, -2, int(1.3 * h) + 6, int(1.7 * w) + 6)
    if name == "shrink":
        return _swap().translate(1.0, 2.0).rotate(0.2).scale(0.23), (0, 0, int(0.3 * h) + 4, int(0.3 * w) + 4)
    raise KeyError(name)


@pytest.mark.parametrize("name", ["identity", "up3", "rot30", "swap", "shrink"])
@pytest.mark.parametrize("shape", [(37, 53), (64, 48)])
@pytest.mark.parametrize("linear_rgb", [False, True])
@pytest.mark.parametrize("smooth", [True, False])
def test_image_fill_matches_restatement(S, name, shape, linear_rgb, smooth):
    px = R.random_rgba(shape, seed=shape[0] + len(name))
    fwd, bbox = _case_transform(name, *shape)
    inv = fwd.invert.m
    mask = np.random.default_rng(7).uniform(0, 1, bbox[2:])
    got = _device_fill(px, inv, smooth, linear_rgb, bbox, mask)
    want = R.sample(R.mip_chain(px, linear_rgb), inv, smooth, *bbox) * mask[..., None]
    if smooth:
        assert np.abs(got - want).max() <= TOL
    else:
        assert np.array_equal(got, want)   # (nearest: a texel times the mask, bit for bit)


def test_shrink_uses_two_levels(S):
    from svgrasterize_amd import _abi, paint

    fwd, _ = _case_transform("shrink", 64, 48)
    lam = paint.image_lod(fwd.invert.m, len(_abi.image_levels(64, 48)))
    assert 2 < lam < 3   # (1 / 0.23: between levels 2 and 3)


def test_mip_chain_matches_restatement(S):
    from svgrasterize_amd import _abi

    px = R.random_rgba((37, 53), seed=3)
    for linear_rgb in (False, True):
        buf = _abi.image_upload(_abi.Context.get(), px, linear_rgb)
        want = R.mip_chain(px, linear_rgb)
        layout = _abi.image_levels(37, 53)
        total = layout[-1][0] + 1
        got = buf.download((total, 4), np.float32)
        for (off, h, w), lv in zip(layout, want):
            assert np.abs(got[off:off + h * w].reshape(h, w, 4) - lv).max() <= TOL


@pytest.mark.parametrize("name", ["identity", "up3", "rot30", "shrink"])
@pytest.mark.parametrize("smooth", [True, False])
def test_uniform_image_is_exact(S, name, smooth):
    colour = np.array([200, 90, 17, 153], dtype=np.uint8)
    px = np.broadcast_to(colour, (37, 53, 4)).copy()
    fwd, bbox = _case_transform(name, 37, 53)
    for linear_rgb in (False, True):
        got = _device_fill(px, fwd.invert.m, smooth, linear_rgb, bbox)
        want = R.prepare(colour[None, None], linear_rgb)[0, 0].astype(np.float64)
        assert np.array_equal(got, np.broadcast_to(want, got.shape))


# ------------------------------------------------------------------------------------------------------------------------
# documents
# ------------------------------------------------------------------------------------------------------------------------
def _uri(px):
    return "data:image/png;base64," + base64.b64encode(R.encode_png(px, 6, 8)).decode()


def _doc(body, w=64, h=48):
    return f'<svg xmlns="http://www.w3.org/2000/svg" width="{w}" height="{h}">{body}</svg>'


def _render(S, scene, w=64, h=48, linear_rgb=False):
    res = scene.render(_swap(), viewport=[0, 0, h, w], linear_rgb=linear_rgb)
    return np.zeros((h, w, 4)) if res is None else res[0].on_canvas(h, w).image


def _only_image(scene):
    """(ImagePaint, its FILL path, accumulated transform) of the one image leaf of `scene`."""
    from svgrasterize_amd.geometry import Transform

    kind, args = scene
    tr = Transform()
    while kind != 0:
        if kind == 6:
            tr = tr @ args[1]
        kind, args = args[0]   # (a GROUP's first child, or the target of a decoration)
    return args[1], args[0], tr


@pytest.mark.parametrize("par", ["xMidYMid meet", "xMaxYMin slice", "none"])
@pytest.mark.parametrize("linear_rgb", [False, True])
def test_document_integer_viewport(S, par, linear_rgb):
    px = R.random_rgba((12, 20), seed=5)
    # the placements keep the visible rectangle on whole pixels, so the coverage is 0 / 1
    doc = _doc(f'<image href="{_uri(px)}" x="4" y="6" width="40" height="36" preserveAspectRatio="{par}"/>')
    scene, _, _ = S.svg_scene_from_str(doc)
    paint, _path, tr = _only_image(scene)
    got = _render(S, scene, linear_rgb=linear_rgb)
    inv = (_swap() @ tr @ paint.transform).invert.m
    want = R.sample(R.mip_chain(px, linear_rgb), inv, True, 0, 0, 48, 64)
    _, (x0, y0, x1, y1) = S.scene.image_placement((12, 20), 4, 6, 40, 36, par)
    assert all(float(v).is_integer() for v in (x0, y0, x1, y1))
    inside = np.zeros((48, 64), dtype=bool)
    inside[int(y0):int(y1), int(x0):int(x1)] = True
    want[~inside] = 0
    assert np.abs(got - want).max() <= TOL
    png = S.render_svg(__import__("io").StringIO(doc))
    assert S.read_png(png).shape == (48, 64, 4)


def test_document_fractional_placement(S):
    px = R.random_rgba((9, 14), seed=8)
    doc = _doc(f'<image href="{_uri(px)}" x="3.3" y="5.7" width="30.45" height="20.2" transform="rotate(7 20 20)"/>')
    scene, _, _ = S.svg_scene_from_str(doc)
    paint, path, tr = _only_image(scene)
    got = _render(S, scene)
    full = _swap() @ tr
    mask, _hull = path.mask(full, viewport=[0, 0, 48, 64])
    m = np.zeros((48, 64))
    m[mask.x:mask.x + mask.height, mask.y:mask.y + mask.width] = mask.image[..., 0]
    want = R.sample(R.mip_chain(px, False), (full @ paint.transform).invert.m, True, 0, 0, 48, 64) * m[..., None]
    assert np.abs(got - want).max() <= TOL


def test_document_decorations_match_scene_image(S):
    from svgrasterize_amd.geometry import Path, Transform
    from svgrasterize_amd.scene import Scene

    px = R.random_rgba((10, 16), seed=2)
    doc = _doc(f'<defs><clipPath id="c"><circle cx="30" cy="24" r="17"/></clipPath>'
               f'<image id="im" href="{_uri(px)}" x="2" y="3" width="40" height="30" opacity="0.6" '
               f'transform="rotate(12 30 24)" clip-path="url(#c)"/></defs>'
               f'<use href="#im" x="5" y="-2"/>')
    scene, _, _ = S.svg_scene_from_str(doc)
    got = _render(S, scene)
    circle = Scene.fill(Path.from_svg(S.svg.ellipse_path_data(30, 24, 17, 17)), np.array([0.0, 0, 0, 1]), "nonzero")
    node = Scene.image(px, 2, 3, 40, 30).opacity(0.6).clip(circle).transform(Transform().translate(30, 24).rotate(math.radians(12)).translate(-30, -24))
    node = node.transform(Transform().translate(5, -2))
    want = _render(S, Scene.group([node]))
    assert np.abs(want).max() > 0.1
    assert np.abs(got - want).max() <= 1e-12


def test_second_render_does_not_upload_again(S, monkeypatch):
    from svgrasterize_amd import _abi

    calls = []
    real = _abi.image_upload
    monkeypatch.setattr(_abi, "image_upload", lambda *a, **k: calls.append(a[2]) or real(*a, **k))
    px = R.random_rgba((20, 30), seed=4)
    scene, _, _ = S.svg_scene_from_str(_doc(f'<image href="{_uri(px)}" width="50" height="40"/>'))
    first = _render(S, scene)
    second = _render(S, scene)
    assert len(calls) == 1 and np.array_equal(first, second)
    _render(S, scene, linear_rgb=True)
    _render(S, scene, linear_rgb=True)
    assert calls == [False, True]


def test_large_rotated_image(S):
    px = R.random_rgba((2048, 2048), seed=12)
    fwd = _swap().translate(2048, -400).rotate(math.radians(30)).scale(1.9)
    inv = fwd.invert.m
    bbox = (0, 0, 4096, 4096)
    got = _device_fill(px, inv, True, False, bbox)
    levels = R.mip_chain(px, False)
    rng = np.random.default_rng(1)
    i, j = rng.integers(0, 4096, 20000), rng.integers(0, 4096, 20000)
    want = R.sample(levels, inv, True, 0, 0, 4096, 4096, points=(i, j))
    assert np.abs(got[i, j] - want).max() <= TOL
    rows = rng.choice(4096, 24, replace=False)
    ii, jj = np.meshgrid(rows, np.arange(4096), indexing="ij")
    want_rows = R.sample(levels, inv, True, 0, 0, 4096, 4096, points=(ii, jj))
    assert np.abs(got[rows] - want_rows).max() <= TOL
    np.testing.assert_allclose(got[rows].sum(axis=1), want_rows.sum(axis=1), rtol=0, atol=1e-6 * 4096)
    assert got[rows, :, 3].sum() > 0
