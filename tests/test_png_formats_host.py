"""The PNG sample formats on the CPU: the second part of csrc/svgr_png.h, driven serially by tests/png_fmt_harness.cpp, against
the numpy restatement of tests/png_fmt_ref.py; the keywords' argument checks with the device entry points made to fail; and
``png.read_samples``.  The device runs the same header (tests/test_gpu_png_formats.py holds its bytes against this harness)."""
import io
import struct
import zlib

import numpy as np
import pytest

import svgrasterize_amd as S
from svgrasterize_amd import _abi, png
from tests import image_ref, png_enc_ref
from tests import png_fmt_ref as R


@pytest.fixture(scope="module")
def lib():
    return R.harness()


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the quantiser and the luma
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [255, 65535])
def test_quant_every_level_and_tie(lib, M):
    k = np.arange(M + 1, dtype=np.float64)
    assert np.array_equal(R.harness_quant(lib, k / M, M), np.arange(M + 1))
    ties = (k + 0.5) / M
    got = R.harness_quant(lib, ties, M)
    want = np.minimum(np.rint(ties * M), M).astype(np.uint32)
    assert np.array_equal(got, want) and np.array_equal(got, R.quant(ties, M))
    assert set(np.unique(got.astype(np.int64) - np.arange(M + 1))) <= {0, 1}   # (half to even, where the product is the tie exactly)


@pytest.mark.parametrize("M", [255, 65535])
def test_quant_outside_the_range(lib, M):
    v = np.array([-1.0, -1e-9, -0.0, 0.0, 0.4999 / M, 1.0, 1.0 + 1e-9, 2.0, 1e300, -1e300, np.inf, -np.inf, np.nan, -np.nan])
    want = np.array([0, 0, 0, 0, 0, M, M, M, M, 0, M, 0, 0, 0], dtype=np.uint32)
    assert np.array_equal(R.harness_quant(lib, v, M), want)
    assert np.array_equal(R.quant(v, M), want)
    rng = np.random.default_rng(M)
    v = rng.uniform(-0.5, 1.5, 20000)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(R.harness_quant(lib, v, M), np.clip(np.rint(v * M), 0, M).astype(np.uint32))


def test_luma_bits(lib):
    rgb = np.random.default_rng(709).random((50000, 3))
    got = R.harness_luma(lib, rgb)
    want = (0.2126 * rgb[:, 0] + 0.7152 * rgb[:, 1]) + 0.0722 * rgb[:, 2]
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert np.array_equal(R.luma(rgb[:, 0], rgb[:, 1], rgb[:, 2]).view(np.uint64), want.view(np.uint64))


@pytest.mark.parametrize("M", [255, 65535])
def test_grey_in_grey_out(lib, M):
    k = np.arange(M + 1)
    v = k / float(M)
    y = R.harness_luma(lib, np.stack([v, v, v], axis=1))
    assert np.array_equal(R.harness_quant(lib, y, M), k)
    assert np.array_equal(R.quant(R.luma(v, v, v), M), k)
    # the whole pixel path: grey and grey + alpha samples of a grey pixel are its level
    px = np.stack([v, v, v, np.ones_like(v)], axis=1)
    depth = 16 if M == 65535 else 8
    got = R.harness_samples(lib, px, R.RGBA_F64, R.GREY, depth)
    assert np.array_equal(got, R.file_bytes(k.astype(np.uint16 if depth == 16 else np.uint8)[:, None]))


# ------------------------------------------------------------------------------------------------------------------------------
# 2. a pixel's sample bytes
# ------------------------------------------------------------------------------------------------------------------------------
def _source(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == R.RGBA_U8:
        return rng.integers(0, 256, (n, 4), dtype=np.uint8)
    v = R.awkward_values(rng, n)
    return v[:, 0].copy() if kind == R.MASK_F64 else v


@pytest.mark.parametrize("kind, color, depth", R.FORMATS)
def test_samples_against_numpy(lib, kind, color, depth):
    src = _source(kind, 700, kind * 100 + color * 10 + depth)
    got = R.harness_samples(lib, src, kind, color, depth)
    assert got.shape == (700, R.CHANNELS[color] * depth // 8)
    assert np.array_equal(got, R.samples_ref(src, kind, color, depth))


def test_samples_refuses_what_the_interface_rules_out(lib):
    src = np.zeros(8)
    out = np.zeros(64, dtype=np.uint8)
    for kind, color, depth in ((R.MASK_F64, R.RGB, 8), (R.MASK_F64, R.RGBA, 16), (R.MASK_F64, R.GREY_ALPHA, 8), (R.RGBA_F64, 3, 8),
                               (R.RGBA_F64, R.RGB, 4), (R.RGBA_F64, R.RGB, 12), (3, R.RGB, 8), (-1, R.RGB, 8)):
        assert lib.h_samples(src.ctypes.data, kind, 1, color, depth, out.ctypes.data) == -1


def test_sixteen_bit_samples_are_big_endian(lib):
    px = np.array([[0x1234 / 65535.0, 0xABCD / 65535.0, 0x00FF / 65535.0, 0xFF00 / 65535.0]])
    assert R.harness_samples(lib, px, R.RGBA_F64, R.RGBA, 16).tolist() == [[0x12, 0x34, 0xAB, 0xCD, 0x00, 0xFF, 0xFF, 0x00]]
    assert R.harness_samples(lib, px, R.RGBA_F64, R.RGB, 16).tolist() == [[0x12, 0x34, 0xAB, 0xCD, 0x00, 0xFF]]
    assert R.harness_samples(lib, px[:, 3], R.MASK_F64, R.GREY, 16).tolist() == [[0xFF, 0x00]]
    ga = R.harness_samples(lib, px, R.RGBA_F64, R.GREY_ALPHA, 16)[0]
    assert ga[2:].tolist() == [0xFF, 0x00]
    assert (int(ga[0]) << 8 | int(ga[1])) == int(R.quant(R.luma(*px[0, :3]), 65535))


def test_bytes_widen_exactly(lib):
    v = np.arange(256, dtype=np.uint8)
    px = np.stack([v, v[::-1], (v * 7) & 255, 255 - v], axis=1).astype(np.uint8)
    got = R.harness_samples(lib, px, R.RGBA_U8, R.RGBA, 16).reshape(256, 4, 2)
    assert np.array_equal((got[..., 0].astype(np.uint32) << 8) | got[..., 1], px.astype(np.uint32) * 257)
    assert np.array_equal(R.harness_samples(lib, px, R.RGBA_U8, R.RGBA, 8), px)
    assert np.array_equal(R.harness_samples(lib, px, R.RGBA_U8, R.RGB, 8), px[:, :3])
    grey = np.stack([v, v, v, 255 - v], axis=1).astype(np.uint8)
    assert np.array_equal(R.harness_samples(lib, grey, R.RGBA_U8, R.GREY, 8)[:, 0], v)
    assert np.array_equal(R.harness_samples(lib, grey, R.RGBA_U8, R.GREY_ALPHA, 8), grey[:, 2:])


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the byte-wise filters
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bpp", R.BPPS)
@pytest.mark.parametrize("shape", [(1, 1), (1, 5), (5, 1), (12, 9), (7, 40)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_filter_bytes_against_numpy(lib, bpp, shape):
    rows, cols = shape
    img = R.filter_image(np.random.default_rng(bpp * 100 + rows), rows, cols * bpp)
    kinds = set()
    for filter in R.FILTERS:
        got = R.harness_filter(lib, img, bpp, filter)
        assert np.array_equal(got, R.filter_ref(img, bpp, filter)), filter
        if filter != "adaptive":
            assert (got[:, 0] == R.FILTERS.index(filter)).all()
        else:
            kinds = set(got[:, 0].tolist())
        back = _abi.png_unfilter(got.tobytes(), rows, cols * bpp, bpp)   # (the library's own host code)
        assert np.array_equal(back, img), filter
    if rows >= 7:
        assert len(kinds) > 1, "the image was made for rows that choose different types"


@pytest.mark.parametrize("shape", [(1, 1), (9, 40), (12, 9), (11, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_filter_bytes_at_four_bytes_is_the_pixel_filter(lib, shape):
    old = png_enc_ref.harness()
    rows, cols = shape
    img = R.filter_image(np.random.default_rng(rows), rows, cols * 4)
    kinds = set()
    for filter in R.FILTERS:
        got = R.harness_filter(lib, img, 4, filter)
        assert np.array_equal(got, png_enc_ref.harness_filter(old, img.reshape(rows, cols, 4), filter)), filter
        kinds |= set(got[:, 0].tolist()) if filter == "adaptive" else set()
    if rows >= 9:
        assert len(kinds) > 1


def test_filter_bytes_refuses_bad_geometry(lib):
    img = np.zeros(64, dtype=np.uint8)
    out = np.zeros(128, dtype=np.uint8)
    for rows, row_bytes, bpp, mode in ((2, 10, 5, 0), (2, 10, 7, 0), (2, 10, 0, 0), (2, 10, 3, 0), (2, 10, 4, 1), (2, 0, 1, 0), (2, 8, 4, 6),
                                       (2, 8, 4, -1)):
        assert lib.h_filter_bytes(img.ctypes.data, rows, row_bytes, bpp, mode, out.ctypes.data) == -1


# ------------------------------------------------------------------------------------------------------------------------------
# 4. the keywords: every refusal comes before any device work
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("device work before the arguments were checked")

    monkeypatch.setattr(_abi.Context, "get", boom)
    for name in ("png_samples", "png_filter_bytes", "png_filter", "deflate"):
        monkeypatch.setattr(_abi, name, boom)


def _rgba_layer():
    return S.Layer(np.full((3, 4, 4), 0.5), (0, 0), pre_alpha=False, linear_rgb=False)


def _mask_layer():
    return S.Layer(np.full((3, 4, 1), 0.5), (0, 0), pre_alpha=True, linear_rgb=True)


BAD_FORMATS = [(dict(color="cmyk"), ValueError, "PNG color"), (dict(color="RGB"), ValueError, "PNG color"), (dict(color=""), ValueError, "PNG color"),
               (dict(color=2), TypeError, "string"), (dict(color=b"rgb"), TypeError, "string"), (dict(color=("rgb",)), TypeError, "string"),
               (dict(depth=4), ValueError, "depth"), (dict(depth=32), ValueError, "depth"), (dict(depth="16"), ValueError, "depth"),
               (dict(depth=True), ValueError, "depth"), (dict(color="grey", depth=1), ValueError, "depth"),
               (dict(color="rgb", palette=16), ValueError, "palette"), (dict(depth=16, palette=True), ValueError, "palette"),
               (dict(depth=8, palette=256, dither="ordered"), ValueError, "palette")]


@pytest.mark.parametrize("kw, error, match", BAD_FORMATS, ids=lambda v: str(v) if isinstance(v, dict) else None)
def test_bad_formats_on_every_call(no_device, kw, error, match):
    with pytest.raises(error, match=match):
        _rgba_layer().write_png(**kw)
    with pytest.raises(error, match=match):
        S.canvas_to_png(np.zeros((2, 2, 4), dtype=np.uint8), **kw)
    with pytest.raises(error, match=match):   # (before the document is read: there is none)
        S.render_svg("/nonexistent/document.svg", **kw)
    for encoder in ("host", "device"):
        with pytest.raises(error, match=match):
            _rgba_layer().write_png(encoder=encoder, **kw)


def test_encoder_arguments_still_come_first(no_device):
    with pytest.raises(TypeError, match="level and threads"):
        _rgba_layer().write_png(encoder="device", level=3, color="rgb")
    with pytest.raises(TypeError, match="filter and huffman"):
        S.canvas_to_png(np.zeros((2, 2, 3), dtype=np.uint8), filter="sub", color="rgb")
    with pytest.raises(ValueError, match="filter"):
        S.canvas_to_png(np.zeros((2, 2, 3), dtype=np.uint8), encoder="device", filter="best", color="rgb")
    with pytest.raises(ValueError, match="format"):
        S.render_svg("/nonexistent/document.svg", format="jpeg", color="rgb")


def test_layer_bg_and_channels(no_device):
    white = (1.0, 1.0, 1.0, 1.0)
    for kw in (dict(color="rgba"), dict(color="grey-alpha"), dict(color="gray-alpha", depth=16), dict(depth=16), dict(depth=8), dict()):
        with pytest.raises(ValueError, match="bg"):
            _rgba_layer().write_png(bg=white, **kw)
    for kw in (dict(color="rgb"), dict(color="rgba"), dict(color="grey-alpha"), dict(depth=16), dict(depth=8), dict()):
        with pytest.raises(ValueError, match="Only RGBA layers are supported"):
            _mask_layer().write_png(**kw)
    with pytest.raises(ValueError, match="bg"):
        _mask_layer().write_png(color="grey", bg=white)
    with pytest.raises(ValueError, match="bg"):
        _mask_layer().write_png(color="gray", depth=16, bg=white)


def test_canvas_shapes(no_device):
    u8, u16, f64 = (lambda *s: np.zeros(s, dtype=np.uint8)), (lambda *s: np.zeros(s, dtype=np.uint16)), (lambda *s: np.zeros(s))
    bad = [(u16(2, 3, 3), dict(color="rgb", depth=8), "depth"), (u16(2, 3), dict(color="grey", depth=8), "depth"),
           (u8(2, 3, 3), dict(color="rgba"), "takes"), (u8(2, 3), dict(color="rgb"), "takes"), (u8(2, 3, 2), dict(color="grey"), "takes"),
           (u8(2, 3, 1), dict(color="grey-alpha"), "takes"), (u16(2, 3, 4), dict(color="rgb"), "takes"), (u16(2, 3, 4), dict(color="grey"), "takes"),
           (f64(2, 3, 3), dict(color="rgb"), "takes"), (f64(2, 3), dict(color="grey"), "takes"), (f64(2, 3, 1), dict(color="grey", depth=16), "takes"),
           (np.zeros((2, 3, 4), dtype=np.int32), dict(color="rgb"), "takes"), (u8(2, 3, 4, 1), dict(depth=16), "takes"),
           (u8(0, 3, 3), dict(color="rgb"), "at least one pixel"), (f64(2, 0, 4), dict(color="grey"), "at least one pixel")]
    for arr, kw, match in bad:
        with pytest.raises(ValueError, match=match):
            S.canvas_to_png(arr, **kw)
    # without the keywords the old rule, with the old words
    with pytest.raises(ValueError, match="Only RGBA layers are supported"):
        S.canvas_to_png(u8(2, 3, 3))


def test_raw_samples_need_no_device(no_device):
    """The host encoder writes samples that are already there without touching the device."""
    rng = np.random.default_rng(16)
    for color, ch in (("grey", 1), ("grey-alpha", 2), ("rgb", 3), ("rgba", 4)):
        for dtype, top in ((np.uint8, 256), (np.uint16, 65536)):
            arr = rng.integers(0, top, (5, 7, ch)).astype(dtype)
            data = S.canvas_to_png(arr, color=color).getvalue()
            got, colour_type, depth = png.read_samples(data)
            assert (colour_type, depth) == (png.COLORS[color], 8 * arr.itemsize) and got.dtype == dtype and np.array_equal(got, arr)
            assert data[:8] == png.SIGNATURE and data[12:16] == b"IHDR" and data[37:41] == b"IDAT" and data[-8:-4] == b"IEND"
            assert struct.unpack(">IIBBBBB", data[16:29]) == (7, 5, depth, colour_type, 0, 0, 0)
            assert zlib.decompress(data[41:-16]) == b"".join(b"\0" + R.file_bytes(row).tobytes() for row in arr)
    arr = rng.integers(0, 256, (4, 6), dtype=np.uint8)
    got, colour_type, depth = png.read_samples(S.canvas_to_png(arr, color="gray", depth=16, level=1).getvalue())
    assert (colour_type, depth) == (0, 16) and np.array_equal(got[..., 0], arr.astype(np.uint16) * 257)
    assert np.array_equal(png.read_samples(S.canvas_to_png(arr[..., None], color="grey", threads=2).getvalue())[0][..., 0], arr)
    # "rgba" at depth 8 from bytes is the file canvas_to_png has always written
    rgba = rng.integers(0, 256, (4, 6, 4), dtype=np.uint8)
    assert S.canvas_to_png(rgba, color="rgba", depth=8).getvalue() == S.canvas_to_png(rgba).getvalue()


def test_sdf_atlas_arguments(no_device):
    from svgrasterize_amd.sdf import SdfAtlas

    with pytest.raises(TypeError, match="uint8 or float32"):
        SdfAtlas(np.zeros((4, 4)), 16.0, 2.0, {}).write_png()
    with pytest.raises(TypeError, match="unexpected"):
        SdfAtlas(np.zeros((4, 4), dtype=np.uint8), 16.0, 2.0, {}).write_png(color="rgb")
    with pytest.raises(ValueError, match="depth"):
        SdfAtlas(np.zeros((4, 4), dtype=np.float32), 16.0, 2.0, {}).write_png(depth=4)
    img = np.arange(20, dtype=np.uint8).reshape(4, 5)
    got, colour_type, depth = png.read_samples(SdfAtlas(img, 16.0, 2.0, {}).write_png().getvalue())
    assert (colour_type, depth) == (0, 8) and np.array_equal(got[..., 0], img)
    img4 = np.arange(80, dtype=np.uint8).reshape(4, 5, 4)
    sink = io.BytesIO()
    assert SdfAtlas(img4, 16.0, 2.0, {}).write_png(sink, level=6) is sink
    got, colour_type, depth = png.read_samples(sink.getvalue())
    assert (colour_type, depth) == (6, 8) and np.array_equal(got, img4)


# ------------------------------------------------------------------------------------------------------------------------------
# 5. read_samples
# ------------------------------------------------------------------------------------------------------------------------------
ALL_FORMATS = [(0, 1), (0, 2), (0, 4), (0, 8), (0, 16), (2, 8), (2, 16), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8), (4, 16), (6, 8), (6, 16)]


@pytest.mark.parametrize("colour_type, depth", ALL_FORMATS)
@pytest.mark.parametrize("interlace", [False, True])
def test_read_samples_every_format(colour_type, depth, interlace):
    rng = np.random.default_rng(colour_type * 31 + depth)
    ch = image_ref.CHANNELS[colour_type]
    n_pal = min(1 << depth, 7)
    samples = rng.integers(0, n_pal if colour_type == 3 else 1 << depth, (9, 13, ch))
    palette = rng.integers(0, 256, (n_pal, 3)) if colour_type == 3 else None
    data = image_ref.encode_png(samples, colour_type, depth, palette, interlace=interlace, seed=depth)
    got, got_type, got_depth = png.read_samples(data)
    assert (got_type, got_depth) == (colour_type, depth)
    assert got.dtype == (np.uint16 if depth == 16 else np.uint8) and np.array_equal(got, samples)
    # read_png on the same file: the reduction to 8-bit RGBA it has always made
    want = np.full((9, 13, 4), 255, dtype=np.uint8)
    if colour_type == 3:
        want[..., :3] = np.asarray(palette, dtype=np.uint8)[samples[..., 0]]
    else:
        want[..., :3] = image_ref.to8(samples[..., :3] if colour_type in (2, 6) else samples[..., :1], depth)
        if colour_type in (4, 6):
            want[..., 3] = image_ref.to8(samples[..., -1], depth)
    assert np.array_equal(S.read_png(data), want)


def test_read_samples_of_a_hand_built_file():
    def chunk(tag, body):
        return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xFFFFFFFF)

    # 2 x 2 grey + alpha at 16 bits, filter 0: the sample 0x1234 is the bytes 12 34
    rows = [bytes([0, 0x12, 0x34, 0xFF, 0xFF, 0x00, 0x01, 0x80, 0x00]), bytes([0, 0xFF, 0xFE, 0x00, 0x00, 0xAB, 0xCD, 0x00, 0xFF])]
    data = png.SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", 2, 2, 16, 4, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(b"".join(rows))) + chunk(b"IEND", b"")
    got, colour_type, depth = png.read_samples(data)
    assert (colour_type, depth) == (4, 16) and got.dtype == np.uint16
    assert got.tolist() == [[[0x1234, 0xFFFF], [0x0001, 0x8000]], [[0xFFFE, 0x0000], [0xABCD, 0x00FF]]]
    with pytest.raises(ValueError, match="signature"):
        png.read_samples(b"no png")
