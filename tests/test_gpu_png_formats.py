"""The PNG sample formats on the device: svgr_png_samples and svgr_png_filter_bytes against the host build of the same header
(tests/png_fmt_harness.cpp, itself held against numpy by tests/test_png_formats_host.py) byte for byte, at the shapes where the
kernels' launch geometry changes, and ``color=`` / ``depth=`` end to end."""
import os

import numpy as np
import pytest

from tests import png_fmt_ref as R
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu

COLORS = ("rgba", "rgb", "grey-alpha", "grey")


@pytest.fixture(scope="module")
def S():
    import svgrasterize_amd as S

    S.Context.get()
    return S


@pytest.fixture(scope="module")
def lib():
    return R.harness()


# ------------------------------------------------------------------------------------------------------------------------------
# 1. svgr_png_samples
# ------------------------------------------------------------------------------------------------------------------------------
def _source(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == R.RGBA_U8:
        return rng.integers(0, 256, (n, 4), dtype=np.uint8)
    v = R.awkward_values(rng, n)   # ties, values outside [0, 1], NaN and infinities
    return v[:, 0].copy() if kind == R.MASK_F64 else v


# a lane per pixel, 256 lanes per workgroup: one pixel, one short of a workgroup, exactly one, one past it, several
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1100])
def test_samples_are_the_host_build(S, lib, n):
    from svgrasterize_amd import _abi

    ctx = S.Context.get()
    for kind, color, depth in R.FORMATS:
        src = R.source_array(_source(kind, n, n * 1000 + kind * 100 + color * 10 + depth), kind)
        want = R.harness_samples(lib, src, kind, color, depth)
        got = _abi.png_samples(ctx, ctx.from_host(src), kind, 1, n, color, depth).download(want.shape, np.uint8)
        assert np.array_equal(got, want), (kind, color, depth)
        if n == 257:   # rows x cols is the pixel count whatever its factors
            assert np.array_equal(_abi.png_samples(ctx, ctx.from_host(src), kind, 257, 1, color, depth).download(want.shape, np.uint8), want)


def test_samples_arguments(S):
    from svgrasterize_amd import _abi

    ctx = S.Context.get()
    src = ctx.from_host(np.zeros((4, 4)))
    for kind, rows, cols, color, depth in ((3, 1, 4, 6, 8), (-1, 1, 4, 6, 8), (0, 1, 4, 3, 8), (0, 1, 4, 1, 8), (0, 1, 4, 6, 4), (0, 1, 4, 6, 12),
                                           (1, 1, 4, 2, 8), (1, 1, 4, 6, 16), (0, 0, 4, 6, 8), (0, 1, 0, 6, 8), (0, 1, 5, 6, 8), (0, 1 << 17, 1, 6, 8)):
        with pytest.raises(ValueError):
            _abi.png_samples(ctx, src, kind, rows, cols, color, depth)
    rc = ctx.lib.svgr_png_samples(ctx.handle, src.handle, 0, 1, 4, 6, 8, src.handle)
    assert rc != 0
    small = ctx.alloc(8)
    assert ctx.lib.svgr_png_samples(ctx.handle, src.handle, 0, 1, 4, 6, 8, small.handle) != 0


# ------------------------------------------------------------------------------------------------------------------------------
# 2. svgr_png_filter_bytes
# ------------------------------------------------------------------------------------------------------------------------------
def _filter_shapes(bpp, span):
    """(rows, row_bytes): one pixel, one row, one column, many short rows (row 0 without a row above; rows that begin at every
    alignment when the width is odd), and three-row images around the span seam: a pixel short of it, at it, a pixel past it
    (the left neighbours of the second pass lie in the first) and a little over three spans."""
    at = span // bpp * bpp
    return [(1, bpp), (1, 5 * bpp), (5, bpp), (67, 9 * bpp), (3, at - bpp), (3, at), (3, at + bpp), (3, 3 * at + 7 * bpp)]


@pytest.mark.parametrize("bpp", R.BPPS)
def test_filter_bytes_is_the_host_build(S, lib, bpp):
    from svgrasterize_amd import _abi, png

    ctx = S.Context.get()
    span = _abi.png_filter_span()
    assert span > 0 and span % 4 == 0
    for rows, row_bytes in _filter_shapes(bpp, span):
        img = R.filter_image(np.random.default_rng(bpp * 100000 + rows * 1000 + row_bytes), rows, row_bytes)
        buf = ctx.from_host(img)
        kinds = set()
        for filter in R.FILTERS:
            got = _abi.png_filter_bytes(ctx, buf, rows, row_bytes, bpp, R.FILTERS.index(filter)).download((rows, 1 + row_bytes), np.uint8)
            assert np.array_equal(got, R.harness_filter(lib, img, bpp, filter)), (rows, row_bytes, filter)
            kinds |= set(got[:, 0].tolist()) if filter == "adaptive" else set()
            if bpp == 4:
                old = png.filter_device(img.reshape(rows, row_bytes // 4, 4), filter).download((rows, 1 + row_bytes), np.uint8)
                assert np.array_equal(got, old), (rows, row_bytes, filter)
        if rows >= 3 and row_bytes > 8:
            assert len(kinds) > 1, "the image was made for rows that choose different types"


def test_filter_bytes_arguments(S):
    from svgrasterize_amd import _abi

    ctx = S.Context.get()
    buf = ctx.from_host(np.zeros(240, dtype=np.uint8))
    for rows, row_bytes, bpp, filter in ((2, 10, 5, 0), (2, 14, 7, 0), (2, 10, 0, 0), (2, 10, 3, 0), (2, 10, 4, 1), (2, 0, 1, 0), (0, 8, 4, 0),
                                         (2, 8, 4, 6), (2, 8, 4, -1), (31, 8, 4, 0), (1 << 17, 1, 1, 0)):
        with pytest.raises(ValueError):
            _abi.png_filter_bytes(ctx, buf, rows, row_bytes, bpp, filter)
    assert ctx.lib.svgr_png_filter_bytes(ctx.handle, buf.handle, 2, 8, 4, 0, buf.handle) != 0
    assert ctx.lib.svgr_png_filter_bytes(ctx.handle, buf.handle, 2, 8, 4, 0, ctx.alloc(16).handle) != 0


# ------------------------------------------------------------------------------------------------------------------------------
# 3. end to end
# ------------------------------------------------------------------------------------------------------------------------------
ROWS, COLS = 37, 53
BG = (0.05, 0.2, 0.1, 1.0)


@pytest.fixture(scope="module")
def layer(S):
    """A gradient fill over a half-transparent solid: alpha, colour and, in the flat part, samples on ties (0.5 * 255)."""
    from svgrasterize_amd.geometry import Transform

    body = ('<defs><linearGradient id="g" x1="0" y1="0" x2="1" y2="1"><stop offset="0" stop-color="#e02010"/>'
            '<stop offset="1" stop-color="#1040f0" stop-opacity="0.6"/></linearGradient></defs>'
            '<rect x="0" y="0" width="44" height="30" fill="#ffffff" fill-opacity="0.5"/>'
            '<rect x="9.5" y="6.25" width="40" height="27" fill="url(#g)"/>')
    scene, _, _ = S.svg_scene_from_str(f'<svg xmlns="http://www.w3.org/2000/svg" width="{COLS}" height="{ROWS}">{body}</svg>')
    return scene.render(Transform().matrix(0, 1, 0, 1, 0, 0), viewport=[0, 0, ROWS, COLS])[0].on_canvas(ROWS, COLS)


@pytest.fixture(scope="module")
def converted(S, layer):
    """The layer's own converted images, downloaded once: what the samples are made from (with alpha; over white; over BG)."""
    conv = lambda l: l.convert(pre_alpha=False, linear_rgb=False).image   # noqa: E731
    return {"alpha": conv(layer), None: conv(layer.background((1.0, 1.0, 1.0, 1.0))), BG: conv(layer.background(BG))}


@pytest.mark.parametrize("encoder", ["host", "device"])
@pytest.mark.parametrize("depth", [8, 16])
@pytest.mark.parametrize("color", COLORS)
def test_layer_write_png_formats(S, layer, converted, color, depth, encoder):
    from svgrasterize_amd import png

    colour_type = png.COLORS[color]
    assert (layer.height, layer.width, layer.channels) == (ROWS, COLS, 4)
    for bg in ((None, BG) if color in ("rgb", "grey") else ("alpha",)):
        bg_kw = {} if bg == "alpha" else {"bg": bg}
        data = layer.write_png(encoder=encoder, color=color, depth=depth, **bg_kw).getvalue()
        got, got_type, got_depth = png.read_samples(data)
        assert (got_type, got_depth) == (colour_type, depth) and got.shape == (ROWS, COLS, R.CHANNELS[colour_type])
        want = R.sample_values(converted[bg], colour_type, depth)
        assert got.dtype == want.dtype and np.array_equal(got, want), (color, depth, encoder, bg)
        assert len(np.unique(got[..., 0])) > 20
        rgba8 = S.read_png(data)   # every written file reads back; at depth 8 as the samples themselves
        assert rgba8.shape == (ROWS, COLS, 4)
        if depth == 8:
            expect = np.full((ROWS, COLS, 4), 255, dtype=np.uint8)
            expect[..., :3] = got[..., :3] if color in ("rgb", "rgba") else got[..., :1]
            if color in ("rgba", "grey-alpha"):
                expect[..., 3] = got[..., -1]
            assert np.array_equal(rgba8, expect)
        if color == "rgb" and depth == 8:
            assert np.array_equal(got, layer.background((1.0, 1.0, 1.0, 1.0) if bg is None else bg).to_rgba8()[..., :3])
    if color == "rgba" and depth == 8:
        assert np.array_equal(got, layer.to_rgba8())
        if encoder == "host":
            assert data == layer.write_png().getvalue()
            assert layer.write_png(depth=8).getvalue() == data == layer.write_png(color="rgba").getvalue()
    if encoder == "device":   # every filter word and both codes decode to the same samples
        for kw in (dict(filter="none"), dict(filter="sub"), dict(filter="up"), dict(filter="average"), dict(filter="paeth", huffman="fixed")):
            other = layer.write_png(encoder="device", color=color, depth=depth, **kw, **bg_kw).getvalue()
            assert np.array_equal(png.read_samples(other)[0], got), kw


def test_sixteen_bits_keep_what_eight_round_away(S, layer, converted):
    from svgrasterize_amd import png

    wide = png.read_samples(layer.write_png(color="rgba", depth=16).getvalue())[0]
    err16 = np.abs(wide / 65535.0 - np.clip(converted["alpha"], 0, 1)).max()
    err8 = np.abs(layer.to_rgba8() / 255.0 - np.clip(converted["alpha"], 0, 1)).max()
    assert err16 <= 0.5 / 65535 + 1e-12 and err8 > 0.25 / 255


@pytest.mark.parametrize("depth", [8, 16])
def test_mask_layer_as_grey(S, depth):
    from svgrasterize_amd import png

    mask, _hull = S.Path.from_svg("M3.5,2.25 L40,9 L22.5,30.75 Z").mask(S.Transform(), viewport=(0, 0, 33, 45))
    assert mask.channels == 1
    values = mask.image[..., 0].copy()
    assert ((values > 0) & (values < 1)).any()
    for encoder in ("host", "device"):
        data = mask.write_png(color="grey", depth=depth, encoder=encoder).getvalue()
        got, colour_type, got_depth = png.read_samples(data)
        assert (colour_type, got_depth) == (0, depth)
        assert np.array_equal(got, R.mask_values(values, depth))
    with pytest.raises(ValueError, match="Only RGBA layers are supported"):
        mask.write_png()
    with pytest.raises(ValueError, match="Only RGBA layers are supported"):
        mask.write_png(color="grey-alpha")


def test_sdf_atlas_write_png(S):
    from svgrasterize_amd import png

    with open(os.path.join(GOLDEN, "fonts", "varsynth.ttf"), "rb") as f:
        font = S.read_font(f.read())
    atlas = font.sdf_atlas("AV", 32.0, 3.0, max_cols=100)
    assert len(atlas.cells) == 2 and atlas.image.dtype == np.uint8 and atlas.image.ndim == 2
    for kw in (dict(), dict(encoder="device")):
        got, colour_type, depth = png.read_samples(atlas.write_png(**kw).getvalue())
        assert (colour_type, depth) == (0, 8) and np.array_equal(got[..., 0], atlas.image)
    f32 = font.sdf_atlas("AV", 32.0, 3.0, np.float32, max_cols=100)
    for kw, depth in ((dict(), 16), (dict(depth=8), 8), (dict(encoder="device", filter="up"), 16)):
        got, colour_type, got_depth = png.read_samples(f32.write_png(**kw).getvalue())
        assert (colour_type, got_depth) == (0, depth)
        assert np.array_equal(got, R.mask_values(f32.image.astype(np.float64), depth))
    msdf = font.msdf_atlas("AV", 32.0, 3.0, max_cols=100)
    got, colour_type, depth = png.read_samples(msdf.write_png(encoder="device").getvalue())
    assert (colour_type, depth) == (6, 8) and np.array_equal(got, msdf.image)
    with pytest.raises(TypeError, match="uint8 or float32"):
        font.sdf_atlas("AV", 32.0, 3.0, np.float64, max_cols=100).write_png()


def test_canvas_to_png_forms(S, lib):
    from svgrasterize_amd import png

    rng = np.random.default_rng(57)
    arr = rng.integers(0, 65536, (5, 7, 3)).astype(np.uint16)
    for kw in (dict(), dict(encoder="device"), dict(encoder="device", filter="paeth", huffman="fixed"), dict(depth=16)):
        got, colour_type, depth = png.read_samples(S.canvas_to_png(arr, color="rgb", **kw).getvalue())
        assert (colour_type, depth) == (2, 16) and got.dtype == np.uint16 and np.array_equal(got, arr)
    grey = rng.integers(0, 256, (6, 11), dtype=np.uint8)
    got, colour_type, depth = png.read_samples(S.canvas_to_png(grey, color="grey", encoder="device").getvalue())
    assert (colour_type, depth) == (0, 8) and np.array_equal(got[..., 0], grey)
    # RGBA sources, float and bytes, through the device stage: the host build's samples
    f = R.awkward_values(rng, 9 * 13).reshape(9, 13, 4)
    u = rng.integers(0, 256, (9, 13, 4), dtype=np.uint8)
    for color in COLORS:
        for depth in (8, 16):
            colour_type = png.COLORS[color]
            shape = (9, 13, R.CHANNELS[colour_type] * depth // 8)
            got = png.read_samples(S.canvas_to_png(f, color=color, depth=depth).getvalue())[0]
            assert np.array_equal(R.file_bytes(got), R.harness_samples(lib, f, R.RGBA_F64, colour_type, depth).reshape(shape)), (color, depth)
            if color != "rgba":
                got = png.read_samples(S.canvas_to_png(u, color=color, depth=depth, encoder="device").getvalue())[0]
                assert np.array_equal(R.file_bytes(got), R.harness_samples(lib, u, R.RGBA_U8, colour_type, depth).reshape(shape)), (color, depth)
    got = png.read_samples(S.canvas_to_png(u, color="rgba", depth=16).getvalue())[0]
    assert np.array_equal(got, u.astype(np.uint16) * 257)


def test_render_svg_formats(S, tmp_path):
    from svgrasterize_amd import png

    doc = os.path.join(GOLDEN, "demo", "material-design.svgz")
    default = S.read_png(S.render_svg(doc, width=96))
    rgb = S.render_svg(doc, tmp_path / "out.png", width=96, color="rgb", encoder="device")
    assert (tmp_path / "out.png").read_bytes() == rgb
    got, colour_type, depth = png.read_samples(rgb)
    assert (colour_type, depth) == (2, 8) and got.shape == default.shape[:2] + (3,)
    wide, colour_type, depth = png.read_samples(S.render_svg(doc, width=96, depth=16))
    assert (colour_type, depth) == (6, 16) and wide.shape == default.shape
    assert np.abs(wide.astype(np.int64) - default.astype(np.int64) * 257).max() <= 129
    grey, colour_type, depth = png.read_samples(S.render_svg(doc, width=96, color="grey", bg=(0.0, 0.0, 0.0, 1.0)))
    assert (colour_type, depth) == (0, 8) and grey.shape == default.shape[:2] + (1,)
