"""The device PNG encoder on the device: svgr_png_filter and svgr_deflate against the host build of the same headers
(tests/png_enc_harness.cpp, itself held against numpy, RFC 1951 and zlib by tests/test_png_encode_host.py) byte for byte, at
the shapes where the kernels' launch geometry changes, and the encoder's keywords end to end."""
import io
import os
import zlib

import numpy as np
import pytest

from tests import png_enc_ref as R
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import svgrasterize_amd as S

    S.Context.get()
    return S


@pytest.fixture(scope="module")
def lib():
    return R.harness()


@pytest.fixture(scope="module")
def cases(S, lib):
    from svgrasterize_amd import _abi

    assert _abi.deflate_chunk() == lib.h_deflate_chunk()
    return R.deflate_cases(_abi.deflate_chunk())


# rows x cols: one pixel, one row, one column, a row of one lane short of / exactly / one lane beyond the workgroup's stride (256
# pixels), a row of several strides, and more rows than one (a workgroup per row: row 0 without a row above, the others with)
SHAPES = [(1, 1), (1, 5), (5, 1), (3, 255), (3, 256), (3, 257), (2, 1100), (67, 9)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_filter_is_the_host_build(S, lib, shape):
    from svgrasterize_amd import png

    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    rows, cols = shape
    img = rng.integers(0, 256, (rows, cols, 4), dtype=np.uint8)
    img[1::3] = img[0::3][:len(img[1::3])]                                  # a row that repeats the one above: Up
    img[2::3] = rng.integers(0, 3, (len(img[2::3]), cols, 4))               # small values, sums that lie close together
    kinds = set()
    for filter in R.FILTERS:
        got = png.filter_device(img, filter).download((rows, 1 + 4 * cols), np.uint8)
        want = R.harness_filter(lib, img, filter)
        assert np.array_equal(got, want), filter
        assert np.array_equal(want, R.filter_ref(img, filter))
        kinds |= set(got[:, 0].tolist()) if filter == "adaptive" else set()
    if rows >= 3:
        assert len(kinds) > 1, "the image was made for rows that choose different types"


def test_filter_from_a_device_buffer(S, lib):
    from svgrasterize_amd import png

    img = np.random.default_rng(4).integers(0, 256, (6, 10, 4), dtype=np.uint8)
    buf = S.Context.get().from_host(img)
    got = png.filter_device(buf, "paeth", rows=6, cols=10).download((6, 41), np.uint8)
    assert np.array_equal(got, R.harness_filter(lib, img, "paeth"))
    with pytest.raises(ValueError):
        png.filter_device(buf, "paeth")
    with pytest.raises(ValueError, match="buffer too small"):
        png.filter_device(buf, "paeth", rows=7, cols=10)


@pytest.mark.parametrize("huffman", ["fixed", "dynamic"])
def test_deflate_is_the_host_build(S, lib, cases, huffman):
    from svgrasterize_amd import _abi, png

    ctx = S.Context.get()
    mode = png.HUFFMAN[huffman]
    for name, data in cases.items():
        want = R.harness_deflate(lib, data, mode)[0]
        got = png.deflate_device(data, huffman)
        assert got == want, name
        assert zlib.decompress(got) == data, name
        # one byte short: "no room", the length still reported, nothing written
        buf = ctx.from_host(np.frombuffer(data, dtype=np.uint8)) if data else ctx.alloc(4)
        assert _abi.deflate_once(ctx, buf, len(data), mode, len(want) - 1) == (_abi.DEFLATE_NO_ROOM, len(want), b""), name
        assert _abi.deflate_once(ctx, buf, len(data), mode, len(want)) == (0, len(want), want), name


def test_deflate_arguments(S):
    from svgrasterize_amd import _abi, png

    ctx = S.Context.get()
    buf = ctx.alloc(64)
    for n, mode in ((-1, 1), (65, 1), (8, 2), (8, -1)):
        with pytest.raises(ValueError):
            _abi.deflate(ctx, buf, n, mode)
    arr = np.arange(300, dtype=np.uint8)
    assert zlib.decompress(png.deflate_device(arr)) == arr.tobytes()
    assert zlib.decompress(png.deflate_device(ctx.from_host(arr), "fixed", n_bytes=100)) == arr[:100].tobytes()
    assert zlib.decompress(png.deflate_device(b"")) == b""


def _scene_layer(S, w=64, h=48):
    from svgrasterize_amd.geometry import Transform

    body = ('<defs><linearGradient id="g" x1="0" y1="0" x2="1" y2="1"><stop offset="0" stop-color="#e02010"/>'
            '<stop offset="1" stop-color="#1040f0"/></linearGradient></defs>'
            '<rect x="4" y="3" width="50" height="40" fill="url(#g)"/>'
            '<circle cx="40" cy="26" r="17" fill="#20c040" fill-opacity="0.5"/>')
    scene, _, _ = S.svg_scene_from_str(f'<svg xmlns="http://www.w3.org/2000/svg" width="{w}" height="{h}">{body}</svg>')
    return scene.render(Transform().matrix(0, 1, 0, 1, 0, 0), viewport=[0, 0, h, w])[0].on_canvas(h, w)


def _gradient_layer(S, rows=8, cols=300):
    y, x = np.mgrid[0:rows, 0:cols]
    img = np.stack([x / (cols - 1), y / (rows - 1), (x + 3 * y) / (cols + 3 * rows), 0.25 + 0.75 * x / (cols - 1)], axis=2)
    return S.Layer(img, (0, 0), pre_alpha=False, linear_rgb=False)


@pytest.mark.parametrize("which", ["scene", "gradient"])
def test_layer_write_png_device(S, lib, which):
    layer = _scene_layer(S) if which == "scene" else _gradient_layer(S)
    want = layer.to_rgba8()
    assert len(np.unique(want[..., 0])) > 20
    sizes = {}
    for filter in R.FILTERS:
        data = layer.write_png(encoder="device", filter=filter).getvalue()
        assert np.array_equal(S.read_png(data), want), filter
        sizes[filter] = len(data)
        assert data == S.canvas_to_png(want, encoder="device", filter=filter).getvalue()   # (the uploaded array: the same file)
    fixed = layer.write_png(encoder="device", huffman="fixed").getvalue()
    assert np.array_equal(S.read_png(fixed), want)
    sink = io.BytesIO()
    assert layer.write_png(sink, encoder="device") is sink and len(sink.getvalue()) == sizes["adaptive"]
    # the IDAT payload is the host build's stream of the host build's scanlines
    idat = sink.getvalue()[41:-16]
    assert idat == R.harness_idat(lib, want, 5, 1)
    print(which, "file sizes by filter", sizes, "fixed code", len(fixed), "default route", len(layer.write_png().getvalue()))
    with pytest.raises(TypeError):
        layer.write_png(encoder="device", level=3)
    with pytest.raises(ValueError, match="filter"):
        layer.write_png(encoder="device", filter="best")


def test_render_svg_device(S, tmp_path):
    doc = os.path.join(GOLDEN, "demo", "material-design.svgz")
    default = S.render_svg(doc, width=256)
    device = S.render_svg(doc, tmp_path / "out.png", width=256, encoder="device")
    assert (tmp_path / "out.png").read_bytes() == device and device != default
    px = S.read_png(default)
    assert px.shape[1] == 256 and np.array_equal(S.read_png(device), px)
    print("material-design at width 256: default route", len(default), "bytes, device route", len(device))
    for kw in (dict(filter="none", huffman="fixed"), dict(filter="paeth")):
        assert np.array_equal(S.read_png(S.render_svg(doc, width=256, encoder="device", **kw)), px)


def test_the_default_route_is_unchanged(S):
    layer = _scene_layer(S)
    want = S.canvas_to_png(layer.to_rgba8()).getvalue()
    assert layer.write_png().getvalue() == want == layer.write_png(None, 9, 1).getvalue() == layer.write_png(encoder="host").getvalue()
    raw = b"".join(b"\0" + row.tobytes() for row in layer.to_rgba8())
    assert want[41:-16] == zlib.compress(raw, 9)
