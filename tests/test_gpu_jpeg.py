"""JPEG on the device: read_jpeg (svgr_jpeg_decode: k_jpeg_idct + k_jpeg_colour) on every fixture of tests/golden/jpeg against the
host build of the same integer arithmetic (tests/jpeg_harness.cpp) -- bit for bit --, synthetic frames of every sampling, and
documents with a JPEG <image> against the same document with the decoded pixels embedded as PNG."""
import base64

import numpy as np
import pytest

from tests import image_ref
from tests import jpeg_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import svgrasterize_amd as S

    S.Context.get()
    return S


@pytest.fixture(scope="module")
def jh():
    return R.harness()


@pytest.mark.parametrize("name", R.FIXTURES)
def test_read_jpeg_equals_host_build(S, jh, name):
    data, recorded = R.fixture(name)
    got = S.read_jpeg(data)
    want = R.host_read_jpeg(jh, data)
    assert got.dtype == np.uint8 and got.shape == recorded.shape[:2] + (4,) and got.flags.c_contiguous
    assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ"
    assert (got[..., 3] == 255).all()


@pytest.mark.parametrize("h, v", [(1, 1), (2, 1), (1, 2), (2, 2)])
@pytest.mark.parametrize("size", [(1, 1), (8, 8), (9, 17), (100, 259), (517, 130)])
def test_synthetic_frames_equal_host_build(S, jh, h, v, size):
    """sizes whose block count is no multiple of a workgroup's 32 blocks, tall and wide, every sampling and colour model"""
    from svgrasterize_amd import _abi, jpeg

    rng = np.random.default_rng(h * 1000 + v * 100 + size[1])
    for n_comp, colour in ((3, _abi.JPEG_YCBCR), (3, _abi.JPEG_RGB), (1, _abi.JPEG_GREY)):
        if n_comp == 1 and (h, v) != (1, 1):
            continue
        frame = _abi.JpegFrame()
        frame.height, frame.width, frame.n_comp, frame.colour = size[0], size[1], n_comp, colour
        frame.h[:] = (h, 1, 1)
        frame.v[:] = (v, 1, 1)
        n = jpeg.coefficient_layout(frame)[1]
        falloff = 1.0 + np.add.outer(np.arange(8), np.arange(8)).reshape(64)
        coef = np.rint(rng.normal(0.0, 1.0, (n, 64)) * 500.0 / falloff ** 1.5).astype(np.int16)
        coef[:, 0] = rng.integers(-1100, 1100, n)
        coef[rng.integers(0, n, 4), rng.integers(0, 64, 4)] = (-32768, 32767, 20000, -20000)   # (the clamp's side, too)
        quant = rng.integers(1, 6, (n_comp, 64)).astype(np.uint16)
        quant[0, 5] = 65535
        got = _abi.jpeg_decode(_abi.Context.get(), frame, coef.reshape(-1), quant)
        assert np.array_equal(got, R.harness_pixels(jh, frame, coef.reshape(-1), quant))


def test_decode_rejects_nonsense(S):
    from svgrasterize_amd import _abi, jpeg

    ctx = _abi.Context.get()
    frame, coef, quant = jpeg.decode_coefficients(R.fixture("ycc420_baseline")[0])
    _abi.jpeg_decode(ctx, frame, coef, quant)
    with pytest.raises(ValueError):
        _abi.jpeg_decode(ctx, frame, coef[:-64], quant)
    for field, value in [("n_comp", 2), ("width", 0), ("height", 70000), ("colour", 0), ("colour", 3)]:
        bad = _abi.JpegFrame.from_buffer_copy(frame)
        setattr(bad, field, value)
        with pytest.raises(ValueError):
            _abi.jpeg_decode(ctx, bad, coef, quant if field != "n_comp" else quant[:2])
    bad = _abi.JpegFrame.from_buffer_copy(frame)
    bad.h[1] = 3
    with pytest.raises(ValueError):
        _abi.jpeg_decode(ctx, bad, coef, quant)
    small = ctx.alloc(frame.width * frame.height * 4 - 4)
    with pytest.raises(ValueError, match="buffer too small"):
        _abi._check(ctx.lib.svgr_jpeg_decode(ctx.handle, __import__("ctypes").byref(frame), _abi.ptr(coef), coef.size, _abi.ptr(quant),
                                             small.handle))


# ------------------------------------------------------------------------------------------------------------------------------
# documents
# ------------------------------------------------------------------------------------------------------------------------------
def _doc(body, w=64, h=48):
    return f'<svg xmlns="http://www.w3.org/2000/svg" width="{w}" height="{h}">{body}</svg>'


def _render(S, scene, w=64, h=48, linear_rgb=False):
    from svgrasterize_amd.geometry import Transform

    res = scene.render(Transform().matrix(0, 1, 0, 1, 0, 0), viewport=[0, 0, h, w], linear_rgb=linear_rgb)
    return np.zeros((h, w, 4)) if res is None else res[0].on_canvas(h, w).image


DOCUMENTS = {
    "plain": '<image href="{uri}" x="4" y="6" width="50" height="40"/>',
    "slice": '<image href="{uri}" x="6" y="4" width="30" height="36" preserveAspectRatio="xMidYMid slice"/>',
    "transform": '<g transform="translate(30 2) rotate(25) scale(0.9)"><image href="{uri}" width="50" height="40" opacity="0.7"/></g>',
    "pixelated": '<image href="{uri}" x="1" y="1" width="60" height="45" preserveAspectRatio="none" image-rendering="pixelated"/>',
}


@pytest.mark.parametrize("fixture", ["ycc420_baseline", "grey_progressive", "rgb_adobe"])
@pytest.mark.parametrize("document", sorted(DOCUMENTS))
@pytest.mark.parametrize("linear_rgb", [False, True])
def test_document_equals_png_document(S, fixture, document, linear_rgb):
    data, _ = R.fixture(fixture)
    jpeg_uri = "data:image/jpeg;base64," + base64.b64encode(data).decode()
    png_uri = "data:image/png;base64," + base64.b64encode(image_ref.encode_png(S.read_jpeg(data), 6, 8)).decode()
    got_scene, _, _ = S.svg_scene_from_str(_doc(DOCUMENTS[document].format(uri=jpeg_uri)))
    want_scene, _, _ = S.svg_scene_from_str(_doc(DOCUMENTS[document].format(uri=png_uri)))
    got, want = _render(S, got_scene, linear_rgb=linear_rgb), _render(S, want_scene, linear_rgb=linear_rgb)
    assert np.abs(want).max() > 0.1
    assert np.array_equal(got, want)


def test_render_svg_with_jpeg_file(S, tmp_path):
    data, _ = R.fixture("ycc420_photo")
    (tmp_path / "Photo.JPG").write_bytes(data)
    doc = tmp_path / "doc.svg"
    doc.write_text(_doc('<image href="Photo.JPG" width="64" height="48"/>'))
    png = S.read_png(S.render_svg(str(doc)))
    assert png.shape == (48, 64, 4) and (png[..., 3] == 255).all()
    # the picture, 4 x smaller: each output pixel is near the mean of the decoded pixels under it
    means = S.read_jpeg(data)[..., :3].reshape(48, 4, 64, 4, 3).mean(axis=(1, 3))
    assert np.abs(png[..., :3].astype(np.float64) - means).mean() < 6.0
