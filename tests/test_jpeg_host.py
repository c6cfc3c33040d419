"""CPU-side checks of the JPEG reader: the container's matrix and refusals, the entropy decoder plus the integer pixel arithmetic
of csrc/svgr_core.h (host build, tests/jpeg_harness.cpp) against the float64 restatement in tests/jpeg_ref.py and against the
pixels libjpeg-turbo decoded (tests/golden/jpeg, written by tests/tools/make_jpeg_fixtures.py), and the loader.  No GPU needed:
where pixels are wanted, read_jpeg's device stage is replaced by the host build of the same arithmetic."""
import base64
import struct
import warnings

import numpy as np
import pytest

import svgrasterize_amd as S
from svgrasterize_amd import _abi, jpeg, svg_scene_from_filepath, svg_scene_from_str
from svgrasterize_amd.paint import ImagePaint
from svgrasterize_amd.scene import RENDER_FILL
from tests import jpeg_ref as R

# The largest difference, in 8-bit levels, between the integer pipeline and the float64 restatement over the fixture matrix, as
# measured.  It is what the pipeline's rounding steps explain: a sample is rounded to 8 bits after the inverse DCT
# (up to 1/2 level in Y, and in Cb and Cr, which the matrix scales by up to 1.772: 0.5 + 0.886 = 1.386 in B), the restatement
# rounds once at the end and so does the pipeline (upsampling is exact in both): two integers whose exact values differ by
# less than 1.386 + rounding differ by at most 2.  Grey and RGB have the sample rounding alone: at most 1.
MAX_VS_FLOAT64 = 2
MAX_VS_FLOAT64_NO_MATRIX = 1

# max |difference| per fixture between the host decode and libjpeg-turbo's recorded pixels, as measured; the mean absolute
# differences are in DESIGN.md 7f.  libjpeg-turbo rounds inside its inverse DCT differently (a sample may differ by a level),
# rounds the upsampled chroma to 8 bits before the matrix, and alternates its rounding bias from column to column.
MAX_VS_TURBO = {
    "grey_3x8": 1, "grey_baseline": 1, "grey_progressive": 1, "rgb_adobe": 1, "rgb_component_ids": 1, "ycc420_1x1": 0,
    "ycc420_33x17": 2, "ycc420_7x5": 1, "ycc420_baseline": 3, "ycc420_dqt16_sof1": 2, "ycc420_optimised": 2, "ycc420_photo": 3,
    "ycc420_progressive": 3, "ycc420_progressive_restart": 3, "ycc420_restart": 3, "ycc422_baseline": 2, "ycc422_progressive": 3,
    "ycc422_progressive_31x23": 3, "ycc440_from_422": 3, "ycc444_adobe_transform1": 3, "ycc444_baseline": 3,
    "ycc444_low_quality": 2, "ycc444_progressive": 3, "ycc444_restart_rows": 3,
}


@pytest.fixture(scope="module")
def jh():
    return R.harness()


@pytest.fixture
def host_pixels(jh, monkeypatch):
    """read_jpeg (and with it the loader) with the pixel stage on the host build"""
    monkeypatch.setattr(jpeg, "_pixel_stage", lambda frame, coef, quant: R.harness_pixels(jh, frame, coef, quant))


def _segments(data):
    return list(jpeg.markers(data))


def _replace(data, code, fn):
    """`data` with the body of its first FF`code` segment replaced by fn(body) (the length field follows)"""
    for offset, c, body in _segments(data):
        if c == code:
            new = fn(body)
            return data[:offset + 2] + struct.pack(">H", len(new) + 2) + new + data[offset + 4 + len(body):]
    raise AssertionError(f"no FF{code:02X} segment")


# ------------------------------------------------------------------------------------------------------------------------------
# container
# ------------------------------------------------------------------------------------------------------------------------------
def test_fixture_matrix_is_complete():
    assert set(R.FIXTURES) == set(MAX_VS_TURBO)
    kinds = {}
    for name in R.FIXTURES:
        data, _ = R.fixture(name)
        codes = [c for _o, c, _b in _segments(data)]
        frame, _coef, _quant = jpeg.decode_coefficients(data)
        kinds[name] = (next(c for c in codes if 0xC0 <= c <= 0xC2), tuple(frame.h[:frame.n_comp]), tuple(frame.v[:frame.n_comp]),
                       frame.colour, 0xDD in codes, codes.count(0xDA))
    assert kinds["grey_baseline"] == (0xC0, (1,), (1,), _abi.JPEG_GREY, False, 1)
    assert kinds["ycc444_baseline"][1:4] == ((1, 1, 1), (1, 1, 1), _abi.JPEG_YCBCR)
    assert kinds["ycc422_baseline"][1:3] == ((2, 1, 1), (1, 1, 1))
    assert kinds["ycc440_from_422"][1:3] == ((1, 1, 1), (2, 1, 1))
    assert kinds["ycc420_baseline"][1:3] == ((2, 1, 1), (2, 1, 1))
    assert kinds["ycc420_progressive"][0] == 0xC2 and kinds["ycc420_progressive"][5] > 3   # (several scans, AC ones not interleaved)
    assert kinds["ycc420_dqt16_sof1"][0] == 0xC1
    assert kinds["ycc420_restart"][4] and kinds["ycc420_progressive_restart"][4] and kinds["ycc444_restart_rows"][4]
    assert kinds["rgb_adobe"][3] == kinds["rgb_component_ids"][3] == _abi.JPEG_RGB
    assert kinds["ycc444_adobe_transform1"][3] == _abi.JPEG_YCBCR
    dqt = next(b for _o, c, b in _segments(R.fixture("ycc420_dqt16_sof1")[0]) if c == 0xDB)
    assert dqt[0] >> 4 == 1   # (16-bit entries)
    assert int(jpeg.decode_coefficients(R.fixture("ycc420_dqt16_sof1")[0])[2].max()) > 255


def test_frame_sizes():
    for name, size in [("ycc420_1x1", (1, 1)), ("ycc420_7x5", (5, 7)), ("grey_3x8", (8, 3)), ("ycc420_33x17", (17, 33)),
                       ("ycc420_photo", (192, 256))]:
        frame, coef, quant = jpeg.decode_coefficients(R.fixture(name)[0])
        assert (frame.height, frame.width) == size and quant.shape == (frame.n_comp, 64)
        assert coef.size == 64 * jpeg.coefficient_layout(frame)[1]


def _sof(data, fn):
    code = next(c for _o, c, _b in _segments(data) if 0xC0 <= c <= 0xC2)
    return _replace(data, code, fn)


def test_refusals():
    good = R.fixture("ycc420_baseline")[0]
    grey = R.fixture("grey_baseline")[0]

    def refused(data, why):
        with pytest.raises(ValueError, match=why):
            jpeg.decode_coefficients(data)

    refused(b"", "bad signature")
    refused(b"\x89PNG\r\n\x1a\n", "bad signature")
    refused(_sof(good, lambda b: b"\x0c" + b[1:]), "12-bit precision")
    sof = next(o for o, c, _b in _segments(good) if c == 0xC0)
    for code, why in [(0xC3, "lossless"), (0xC5, "hierarchical"), (0xC9, "arithmetic"), (0xCA, "arithmetic"), (0xCB, "arithmetic"),
                      (0xCD, "arithmetic"), (0xCF, "arithmetic"), (0xC7, "hierarchical")]:
        refused(good[:sof + 1] + bytes([code]) + good[sof + 2:], why)
    refused(_sof(good, lambda b: b[:5] + b"\x04" + b[6:] + b"\x04\x11\x00"), "CMYK / YCCK")
    refused(_sof(good, lambda b: b[:5] + b"\x02" + b[6:12]), "2 components")
    refused(_sof(good, lambda b: b[:7] + b"\x41" + b[8:]), "sampling factors 4 x 1")
    refused(_sof(good, lambda b: b[:7] + b"\x13" + b[8:]), "sampling factors 1 x 3")
    refused(_sof(good, lambda b: b[:1] + struct.pack(">HH", 0, 50) + b[5:]), "image size")
    refused(_sof(good, lambda b: b[:1] + struct.pack(">HH", 40000, 40000) + b[5:]), "image size 40000 x 40000")
    # missing tables: every DQT / DHT segment removed in turn
    for code, why in [(0xDB, "missing quantisation table"), (0xC4, "missing Huffman table")]:
        data = good
        while any(c == code for _o, c, _b in _segments(data)):
            offset, body = next((o, b) for o, c, b in _segments(data) if c == code)
            data = data[:offset] + data[offset + 4 + len(body):]
        refused(data, why)
    refused(_replace(good, 0xDB, lambda b: b[:40]), "damaged DQT")
    refused(_replace(good, 0xC4, lambda b: b[:10]), "damaged DHT")
    refused(_replace(good, 0xC4, lambda b: b[:1] + b"\xff" * 16 + b[17:]), "damaged DHT")
    refused(_replace(grey, 0xDA, lambda b: b[:1] + b"\x09" + b[2:]), "components the frame does not have")
    refused(_replace(good, 0xDA, lambda b: b[:-3] + b"\x00\x3e\x00"), "corrupt JPEG scan")        # (Se = 62 in a sequential scan)
    sos = next(o for o, c, _b in _segments(good) if c == 0xDA)
    refused(good[:sos] + good[sof:], "more than one frame")
    refused(good[:sof] + good[sos:], "scan before the frame header")
    refused(good[:sos] + b"\xff\xd9", "no scan")
    refused(good[:-2], "truncated")
    dqt = next(o for o, c, _b in _segments(good) if c == 0xDB)
    refused(good[:dqt] + b"\x00" + good[dqt:], "where a marker should be")


def test_truncation_everywhere_raises(jh):
    for name in ("ycc420_baseline", "ycc420_progressive_restart", "grey_progressive", "ycc420_dqt16_sof1", "rgb_adobe"):
        good = R.fixture(name)[0]
        R.host_read_jpeg(jh, good)
        cuts = {o for o, _c, _b in _segments(good)} | {o + 2 for o, _c, _b in _segments(good)}
        cuts |= set(np.random.default_rng(len(good)).integers(0, len(good), 200).tolist())
        cuts |= set(range(len(good) - 40, len(good)))
        for cut in sorted(c for c in cuts if c < len(good)):
            with pytest.raises(ValueError):
                R.host_read_jpeg(jh, good[:cut])


def test_corruption_never_crashes(jh):
    """bytes flipped anywhere: a ValueError or some picture of the right size, nothing else"""
    rng = np.random.default_rng(11)
    for name in ("ycc420_restart", "ycc422_progressive", "ycc420_optimised", "grey_baseline"):
        good = R.fixture(name)[0]
        shape = R.rgba_of(R.fixture(name)[1]).shape
        for _ in range(300):
            bad = bytearray(good)
            for at in rng.integers(2, len(good), int(rng.integers(1, 4))):
                bad[at] = int(rng.integers(0, 256))
            try:
                out = R.host_read_jpeg(jh, bytes(bad))
            except ValueError:
                continue
            assert out.dtype == np.uint8 and out.ndim == 3 and out.shape[2] == 4
            assert out.shape == shape or bytes(bad[:600]) != good[:600]   # (only a changed header changes the size)


def test_entropy_abi_rejects_nonsense():
    frame, coef, _quant = jpeg.decode_coefficients(R.fixture("ycc420_baseline")[0])
    counts, symbols = np.zeros((8, 16), dtype=np.uint8), np.zeros((8, 256), dtype=np.uint8)
    counts[:, 1] = 2
    scan = _abi.JpegScan()
    scan.frame = frame
    scan.n_scan, scan.se = 1, 63
    _abi.jpeg_entropy(scan, counts, symbols, b"\x00" * 4000, coef.copy())   # (a stream of zeros decodes: code 00 is an end of block)
    for field, value in [("n_scan", 0), ("n_scan", 4), ("se", 64), ("ss", 5), ("al", 3), ("restart_interval", -1)]:
        bad = _abi.JpegScan.from_buffer_copy(scan)
        setattr(bad, field, value)
        with pytest.raises(ValueError):
            _abi.jpeg_entropy(bad, counts, symbols, b"\x00" * 4000, coef.copy())
    bad = _abi.JpegScan.from_buffer_copy(scan)
    bad.scan_comp[0] = 3
    with pytest.raises(ValueError):
        _abi.jpeg_entropy(bad, counts, symbols, b"\x00" * 4000, coef.copy())
    bad = _abi.JpegScan.from_buffer_copy(scan)
    bad.dc_table[0] = 4
    with pytest.raises(ValueError):
        _abi.jpeg_entropy(bad, counts, symbols, b"\x00" * 4000, coef.copy())
    with pytest.raises(ValueError):
        _abi.jpeg_entropy(scan, counts, symbols, b"\x00" * 4000, coef[:-64].copy())
    with pytest.raises(ValueError, match="ends before"):
        _abi.jpeg_entropy(scan, counts, symbols, b"\x00" * 3, coef.copy())
    over = counts.copy()
    over[0, 0] = 3   # (three codes of one bit)
    with pytest.raises(ValueError, match="Huffman"):
        _abi.jpeg_entropy(scan, over, symbols, b"\x00" * 4000, coef.copy())


# ------------------------------------------------------------------------------------------------------------------------------
# host decode against the float64 restatement and against libjpeg-turbo
# ------------------------------------------------------------------------------------------------------------------------------
def test_host_decode_against_float64(jh):
    worst = {}
    for name in R.FIXTURES:
        frame, coef, quant = jpeg.decode_coefficients(R.fixture(name)[0])
        got = R.harness_pixels(jh, frame, coef, quant)
        want = R.pixels(frame, coef, quant)
        assert got.shape == want.shape and (got[..., 3] == 255).all()
        worst[name] = int(np.abs(got.astype(np.int64) - want.astype(np.int64)).max())
        print(f"{name}: max |integer - float64| = {worst[name]}")
    assert max(worst.values()) == MAX_VS_FLOAT64
    assert max(v for k, v in worst.items() if k.startswith(("grey", "rgb"))) == MAX_VS_FLOAT64_NO_MATRIX
    assert all(v <= (MAX_VS_FLOAT64_NO_MATRIX if k.startswith(("grey", "rgb")) else MAX_VS_FLOAT64) for k, v in worst.items())


def test_samples_are_the_rounded_exact_idct(jh):
    """The 8-bit samples themselves.  The transform's factors are rounded to 2^-15 of 1/2 c cos, an error of at most 2^-16 each;
    a sample is sum T[y][v] T[x][u] F[v][u] with |T| <= 1/2, so the two rounded factors move it by at most
    2 * 2^-16 * 1/2 * sum |F| = 2^-16 sum |F| over its block, and nothing else is rounded before the one shift at the end."""
    for name in ("ycc420_photo", "ycc444_low_quality", "ycc420_dqt16_sof1"):
        frame, coef, quant = jpeg.decode_coefficients(R.fixture(name)[0])
        _px, samples = R.harness_pixels(jh, frame, coef, quant, want_samples=True)
        exact = np.concatenate([p.reshape(-1) for p in R.sample_planes(frame, coef, quant)])
        worst_block = max(float(np.abs(coef[64 * b:64 * (b + bh * bw)].reshape(-1, 64).astype(np.float64) * quant[i]).sum(axis=1).max())
                          for i, (b, bh, bw) in enumerate(jpeg.coefficient_layout(frame)[0]))
        err = np.abs(samples.astype(np.float64) - exact).max()
        print(f"{name}: max |sample - exact| = {err:.5f}, bound 0.5 + {2.0 ** -16 * worst_block:.5f}")
        assert err <= 0.5 + 2.0 ** -16 * worst_block


@pytest.mark.parametrize("h, v", [(1, 1), (2, 1), (1, 2), (2, 2)])
@pytest.mark.parametrize("size", [(1, 1), (2, 3), (9, 16), (17, 31), (40, 33)])
def test_synthetic_coefficients_every_sampling(jh, h, v, size):
    """random coefficients of natural magnitudes under every sampling, YCbCr and RGB: the same bound"""
    rng = np.random.default_rng(h * 100 + v * 10 + size[0])
    for colour in (_abi.JPEG_YCBCR, _abi.JPEG_RGB):
        frame = _abi.JpegFrame()
        frame.height, frame.width, frame.n_comp, frame.colour = size[0], size[1], 3, colour
        frame.h[:] = (h, 1, 1)
        frame.v[:] = (v, 1, 1)
        n = jpeg.coefficient_layout(frame)[1]
        falloff = 1.0 + np.add.outer(np.arange(8), np.arange(8)).reshape(64)
        coef = np.rint(rng.normal(0.0, 1.0, (n, 64)) * 400.0 / falloff ** 1.5).astype(np.int16)
        coef[:, 0] = rng.integers(-900, 900, n)
        quant = rng.integers(1, 4, (3, 64)).astype(np.uint16)
        got = R.harness_pixels(jh, frame, coef.reshape(-1), quant)
        want = R.pixels(frame, coef.reshape(-1), quant)
        bound = MAX_VS_FLOAT64 if colour == _abi.JPEG_YCBCR else MAX_VS_FLOAT64_NO_MATRIX
        assert np.abs(got.astype(np.int64) - want.astype(np.int64)).max() <= bound


def test_extreme_coefficients_stay_defined(jh):
    """the clamp of svgr_core.h: any int16 times any 16-bit table entry gives a picture, and the same one each time"""
    frame = _abi.JpegFrame()
    frame.height, frame.width, frame.n_comp, frame.colour = 16, 16, 3, _abi.JPEG_YCBCR
    frame.h[:] = (2, 1, 1)
    frame.v[:] = (2, 1, 1)
    n = jpeg.coefficient_layout(frame)[1]
    rng = np.random.default_rng(5)
    coef = rng.choice(np.array([-32768, 32767, -1, 1, 0], dtype=np.int16), n * 64)
    quant = np.full((3, 64), 65535, dtype=np.uint16)
    a, b = R.harness_pixels(jh, frame, coef, quant), R.harness_pixels(jh, frame, coef, quant)
    assert np.array_equal(a, b) and (a[..., 3] == 255).all()


def test_host_decode_against_libjpeg_turbo(jh):
    worst = {}
    for name in R.FIXTURES:
        data, recorded = R.fixture(name)
        diff = np.abs(R.host_read_jpeg(jh, data).astype(np.int64) - R.rgba_of(recorded).astype(np.int64))
        worst[name] = int(diff.max())
        print(f"{name}: max {worst[name]}, mean {diff[..., :3].mean():.4f}")
    assert worst == MAX_VS_TURBO


def test_variants_of_one_picture_share_coefficients():
    """restart markers, optimised tables and the scan script change the coding, not the coefficients"""
    a = jpeg.decode_coefficients(R.fixture("ycc420_baseline")[0])
    b = jpeg.decode_coefficients(R.fixture("ycc420_restart")[0])
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    a = jpeg.decode_coefficients(R.fixture("ycc420_progressive")[0])
    b = jpeg.decode_coefficients(R.fixture("ycc420_progressive_restart")[0])
    assert np.array_equal(a[1], b[1])
    a = jpeg.decode_coefficients(R.fixture("rgb_adobe")[0])
    b = jpeg.decode_coefficients(R.fixture("ycc444_baseline")[0])
    assert np.array_equal(a[1], b[1]) and a[0].colour != b[0].colour


def test_read_jpeg_is_public(host_pixels, jh):
    data, recorded = R.fixture("ycc422_baseline")
    got = S.read_jpeg(data)
    assert "read_jpeg" in S.__all__ and got.dtype == np.uint8 and got.shape == recorded.shape[:2] + (4,)
    assert np.array_equal(got, R.host_read_jpeg(jh, data))
    assert np.array_equal(S.read_jpeg(bytearray(data)), got)


# ------------------------------------------------------------------------------------------------------------------------------
# loader
# ------------------------------------------------------------------------------------------------------------------------------
def _doc(body):
    return f'<svg xmlns="http://www.w3.org/2000/svg" xmlns:xlink="http://www.w3.org/1999/xlink" width="64" height="48">{body}</svg>'


def _paints(scene):
    out = []

    def walk(node):
        kind, args = node
        if kind == RENDER_FILL:
            out.append(args[1])
        else:
            for child in (args if isinstance(args, list) else [args[0]] if isinstance(args[0], tuple) else args[0]):
                walk(child)

    walk(scene)
    return out


def _only_image(scene):
    found = []

    def walk(x):
        if isinstance(x, ImagePaint):
            found.append(x)
        elif isinstance(x, (tuple, list)):
            for y in x:
                walk(y)

    walk(scene)
    (paint,) = found
    return paint


@pytest.mark.parametrize("mime", ["image/jpeg", "image/jpg", "IMAGE/JPEG", "image/png"])
def test_loader_data_uri(host_pixels, jh, mime):
    data, _ = R.fixture("ycc420_baseline")
    uri = f"data:{mime};base64,{base64.b64encode(data).decode()}"
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        scene, _ids, _size = svg_scene_from_str(_doc(f'<image href="{uri}" x="2" y="3" width="50" height="40"/>'))
    assert np.array_equal(_only_image(scene).pixels, R.host_read_jpeg(jh, data))   # (image/png: the magic bytes decide)


@pytest.mark.parametrize("filename", ["a.jpg", "b.jpeg", "c.jpe", "D.JPG", "E.JpEg", "named_wrongly.png"])
def test_loader_file(host_pixels, jh, tmp_path, filename):
    data, _ = R.fixture("grey_progressive")
    (tmp_path / filename).write_bytes(data)
    doc = tmp_path / "doc.svg"
    doc.write_text(_doc(f'<image xlink:href="{filename}" width="50" height="40"/>'))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        scene, _ids, _size = svg_scene_from_filepath(str(doc))
    assert np.array_equal(_only_image(scene).pixels, R.host_read_jpeg(jh, data))


def test_loader_png_named_jpg(tmp_path):
    from tests import image_ref

    rgba = image_ref.random_rgba((4, 5), 3)
    (tmp_path / "really_png.jpg").write_bytes(image_ref.encode_png(rgba, 6, 8))
    doc = tmp_path / "doc.svg"
    doc.write_text(_doc('<image href="really_png.jpg" width="5" height="4"/>'))
    scene, _ids, _size = svg_scene_from_filepath(str(doc))
    assert np.array_equal(_only_image(scene).pixels, rgba)


@pytest.mark.parametrize("href, why", [
    ("data:image/jpeg;base64,/9j/4AAQSkZJRgABAQ==", r"unsupported image data: undecodable JPEG \(data URI\): truncated JPEG"),
    ("data:image/jpeg;base64,/9j/4AAQ!!!!", "bad base64 image data"),
    ("data:image/jpeg,/9j/4AAQSkZJRgABAQ==", "unsupported image data"),
    ("data:image/gif;base64,R0lGODlhAQABAAAAACw=", r"unsupported image data: image/gif;base64 \(base64 PNG and JPEG are read\)"),
    ("photo.webp", r"unsupported image format \(PNG and JPEG are read\)"),
    ("missing.jpg", "not readable"),
    ("http://example.com/a.jpg", "only data URIs"),
])
def test_loader_warns_and_draws_nothing(host_pixels, tmp_path, href, why):
    doc = tmp_path / "doc.svg"
    doc.write_text(_doc(f'<image href="{href}" width="6" height="8"/>'))
    with pytest.warns(UserWarning, match=why) as rec:
        scene, _ids, _size = svg_scene_from_filepath(str(doc))
    assert scene is None
    assert not any("only PNG" in str(w.message) or "only base64 PNG" in str(w.message) for w in rec)


def test_loader_undecodable_file(host_pixels, tmp_path):
    data, _ = R.fixture("ycc420_baseline")
    (tmp_path / "cut.jpg").write_bytes(data[:len(data) // 2])
    doc = tmp_path / "doc.svg"
    doc.write_text(_doc('<rect width="4" height="4"/><image href="cut.jpg" width="6" height="8"/>'))
    with pytest.warns(UserWarning, match=r"undecodable JPEG \(cut.jpg\)"):
        scene, _ids, _size = svg_scene_from_filepath(str(doc))
    assert scene is not None
    with pytest.raises(ValueError):
        _only_image(scene)   # (the rectangle alone)
