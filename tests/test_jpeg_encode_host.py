"""CPU-side checks of the JPEG writer: the integer encode arithmetic of csrc/svgr_core.h (host build, tests/jpeg_enc_harness.cpp)
against its numpy restatement and against the exact DCT (tests/jpeg_enc_ref.py), the host entropy coder against the entropy
decoder the reader already has, and the files write_jpeg makes against the project's own reader and, where it is installed, PIL.
No GPU needed: where coefficients are wanted, write_jpeg's device stage is replaced by the host build of the same arithmetic."""
import ctypes as C
import io

import numpy as np
import pytest

import svgrasterize_amd as S
from svgrasterize_amd import _abi, jpeg
from tests import jpeg_enc_ref as E
from tests import jpeg_ref as R

SAMPLINGS = [None, "4:4:4", "4:2:2", "4:4:0", "4:2:0"]   # None: grey

# max |difference| in 8-bit levels between PIL's (libjpeg's) pixels and the project's host decode of the same written file, as
# measured over test_pil_reads_the_files' cases (64 x 48 random-smooth image, quality 90): 4:4:4 2, 4:2:2 3, 4:4:0 3,
# 4:2:0 2, grey 1.  The causes are the decoder's, the ones tests/test_jpeg_host.py lists for MAX_VS_TURBO: libjpeg rounds
# inside its inverse DCT differently, rounds the upsampled chroma to 8 bits before the matrix and alternates a rounding bias.
MAX_VS_PIL = {"4:4:4": 2, "4:2:2": 3, "4:4:0": 3, "4:2:0": 2, None: 1}


@pytest.fixture(scope="module")
def eh():
    return E.harness()


@pytest.fixture(scope="module")
def jh():
    return R.harness()


@pytest.fixture
def host_coefficients(eh, monkeypatch):
    """write_jpeg with the coefficient stage on the host build"""
    monkeypatch.setattr(jpeg, "_coefficient_stage", lambda frame, rgba8, quant: E.harness_coefficients(eh, frame, rgba8, quant))


def _tables(n_comp, kind):
    rng = np.random.default_rng(7)
    if kind == "ones":
        return np.ones((n_comp, 64), dtype=np.uint16)
    if kind == "max":
        return np.full((n_comp, 64), 255, dtype=np.uint16)
    return rng.integers(1, 256, (n_comp, 64)).astype(np.uint16)


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the arithmetic
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling", SAMPLINGS)
@pytest.mark.parametrize("size", E.SIZES_HOST)
def test_harness_equals_numpy(eh, size, sampling):
    frame = E.frame_of(*size, sampling)
    for name, img in E.images(*size).items():
        for kind in ("ones", "max", "mixed"):
            quant = _tables(frame.n_comp, kind)
            got, samples = E.harness_coefficients(eh, frame, img, quant, want_samples=True)
            want_planes = np.concatenate([p.reshape(-1) for p in E.planes(frame, img)])
            assert np.array_equal(samples, want_planes), (name, kind)
            assert np.array_equal(got, E.coefficients(frame, img, quant)), (name, kind)


def test_extremes_reach_the_largest_coefficients(eh):
    """all 0 gives the DC its clamp, -1024; all 255 gives 1016; pure blue and pure red clamp the chroma at 255"""
    frame = E.frame_of(8, 8, "4:4:4")
    q1 = _tables(3, "ones")
    imgs = E.images(8, 8)
    assert E.harness_coefficients(eh, frame, imgs["zeros"], q1)[0] == -1024
    assert E.harness_coefficients(eh, frame, imgs["ones"], q1)[0] == 1016
    blue = np.zeros((8, 8, 4), dtype=np.uint8)
    blue[..., 2] = 255
    _c, samples = E.harness_coefficients(eh, frame, blue, q1, want_samples=True)
    assert (samples[64:128] == 255).all()
    assert int(np.abs(E.harness_coefficients(eh, frame, imgs["checker"], q1)[1:64].astype(np.int64)).max()) > 800   # (F(7, 7) = 837)


@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_transform_accuracy(eh, sampling):
    """At q = 1 a coefficient is the exact F(v, u) = sum_y sum_x T[y][v] T[x][u] (s - 128) rounded once, but for the table:
    the factors are stored as round(2^15 T), each off by at most 2^-16, and |T| <= 1/2, so the product of two stored factors
    differs from T[y][v] T[x][u] by at most 2 * 2^-16 * 1/2 (+ 2^-32, which the slack of |T| < 0.491 covers); summed over the
    block that is 2^-16 sum |s - 128|.  Nothing else is rounded before the quantiser, whose one rounding adds at most 1/2.
    (No value comes near a clamp: |F| < 929 off DC, and DC lies in -1024 .. 1016.)"""
    for size in E.SIZES_HOST:
        frame = E.frame_of(*size, sampling)
        quant = _tables(frame.n_comp, "ones")
        for name, img in E.images(*size).items():
            coef, samples = E.harness_coefficients(eh, frame, img, quant, want_samples=True)
            at = 0
            for plane in E.planes(frame, img):
                n = plane.size
                exact = E.exact_dct(plane)
                bound = 0.5 + 2.0 ** -16 * np.abs(E.blocks_of(plane).astype(np.float64) - 128.0).sum(axis=(2, 3))
                got = coef[at:at + n].reshape(exact.shape).astype(np.float64)
                err = np.abs(got - exact)
                assert (err <= bound[..., None, None] + 1e-9).all(), (size, name, float(err.max()))
                at += n


def test_quality_scaling():
    assert (jpeg.quant_tables(100) == 1).all()
    for q in (1, 10, 49, 50, 75, 90, 99, 100):
        assert np.array_equal(jpeg.quant_tables(q), E.quant_tables(q)), q
    assert jpeg.quant_tables(50)[0, 0] == 16 and jpeg.quant_tables(50)[1, 63] == 99
    assert jpeg.quant_tables(1).max() == 255


def test_standard_huffman_tables_are_the_fixtures():
    """Annex K.3's tables as typed in against the DHT segments libjpeg-turbo wrote into a fixture"""
    counts, symbols = jpeg.standard_huffman()
    seen = 0
    for _o, code, body in jpeg.markers(R.fixture("ycc420_baseline")[0]):
        at = 0
        while code == 0xC4 and at < len(body):
            tc, t = body[at] >> 4, body[at] & 15
            total = sum(body[at + 1:at + 17])
            assert bytes(body[at + 1:at + 17]) == counts[4 * tc + t].tobytes()
            assert bytes(body[at + 17:at + 17 + total]) == symbols[4 * tc + t, :total].tobytes()
            at += 17 + total
            seen += 1
    assert seen == 4


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the entropy coder
# ------------------------------------------------------------------------------------------------------------------------------
def _scan_of(frame, restart):
    scan = _abi.JpegScan()
    scan.frame = frame
    scan.progressive, scan.restart_interval, scan.n_scan = 0, restart, frame.n_comp
    scan.ss, scan.se = 0, 63
    for i in range(frame.n_comp):
        scan.scan_comp[i], scan.dc_table[i], scan.ac_table[i] = i, min(i, 1), min(i, 1)
    return scan


def _hard_coefficients(frame, seed):
    """Blocks built to be awkward: sparse random values over the whole range, then, block by block in turn, a lone coefficient
    at index 63 behind 62 zeros (three ZRL), a run of exactly 16 zeros, AC of +-1023, a full block, an empty block, and DC
    values that swing between -1024 and 1023 (differences of +-2047)."""
    rng = np.random.default_rng(seed)
    n = _abi.jpeg_n_coef(frame) // 64
    c = np.where(rng.random((n, 64)) < 0.15, rng.integers(-1023, 1024, (n, 64)), 0).astype(np.int16)
    c[:, 0] = np.where(np.arange(n) % 2 == 0, -1024, 1023)
    for b in range(n):
        kind = b % 6
        if kind == 0:
            c[b, 1:] = 0
            c[b, 63] = -1        # (natural index 63 is the last of the zigzag too)
        elif kind == 1:
            c[b, 1:] = 0
            c[b, jpeg._ZIGZAG[17]] = 5   # (16 zeros, then a value: one ZRL)
        elif kind == 2:
            c[b, 1:] = 0
            c[b, 1], c[b, 8], c[b, 62] = 1023, -1023, 1023
        elif kind == 3:
            c[b, 1:] = rng.integers(1, 1024, 63) * rng.choice([-1, 1], 63)
        elif kind == 4:
            c[b, 1:] = 0
    return c.reshape(-1)


def _optimised(scan, coef):
    counts, symbols = jpeg.standard_huffman()
    freq = _abi.jpeg_symbol_counts(scan, coef)
    for i in range(8):
        if freq[i].any():
            bits, vals = jpeg.optimal_huffman(freq[i])
            assert int(bits.sum()) == int((freq[i] > 0).sum()) and sorted(vals) == list(np.nonzero(freq[i])[0])
            counts[i], symbols[i] = bits, 0
            symbols[i, :vals.size] = vals
    return counts, symbols


@pytest.mark.parametrize("restart", [0, 1, 7])
@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_entropy_round_trip(sampling, restart):
    for size in [(9, 17), (33, 70)]:
        frame = E.frame_of(*size, sampling)
        scan = _scan_of(frame, restart)
        coef = _hard_coefficients(frame, seed=restart)
        for tables in (jpeg.standard_huffman(), _optimised(scan, coef)):
            data = _abi.jpeg_entropy_encode(scan, *tables, coef)
            assert (b"\xff\xd0" in data) == (restart > 0 and _abi.jpeg_n_coef(frame) // 64 > restart * (frame.h[0] * frame.v[0] + frame.n_comp - 1))
            back = np.zeros_like(coef)
            _abi.jpeg_entropy(scan, *tables, data, back)
            assert np.array_equal(back, coef)


def test_optimal_tables_obey_the_limits():
    """at most 16 bits, and no code of all ones: the Kraft sum of the table leaves room for the reserved code"""
    rng = np.random.default_rng(3)
    for freq in [rng.integers(0, 1000, 256), (2.0 ** np.arange(256) % 2 ** 40).astype(np.int64) + 1, np.r_[1, np.zeros(255, int)],
                 np.r_[[10 ** 9], np.ones(255, int)], np.array([int(1.6 ** k) for k in range(40)] + [0] * 216)]:
        bits, vals = jpeg.optimal_huffman(freq)
        assert bits.shape == (16,) and int(bits.sum()) == int((np.asarray(freq) > 0).sum()) == vals.size
        kraft = sum(int(b) << (16 - l) for l, b in enumerate(bits, 1))
        assert kraft <= (1 << 16) - 1


def test_entropy_buffer_one_byte_short():
    frame = E.frame_of(33, 17, "4:2:0")
    scan = _scan_of(frame, 3)
    coef = _hard_coefficients(frame, seed=5)
    counts, symbols = jpeg.standard_huffman()
    full = _abi.jpeg_entropy_encode(scan, counts, symbols, coef)
    lib, n = _abi.load_library(), C.c_int64()
    for cap in (len(full), len(full) - 1, 0):
        out = np.full(len(full) + 8, 0xA5, dtype=np.uint8)
        rc = lib.svgr_jpeg_entropy_encode(C.byref(scan), _abi.ptr(counts), _abi.ptr(symbols), _abi.ptr(coef), coef.size, _abi.ptr(out), cap,
                                          C.byref(n))
        assert rc == (0 if cap == len(full) else _abi.JPEG_NO_ROOM) and n.value == len(full)
        assert out[:cap].tobytes() == full[:cap] and (out[cap:] == 0xA5).all()


def test_entropy_encode_rejects_nonsense():
    frame = E.frame_of(8, 8, None)
    scan = _scan_of(frame, 0)
    counts, symbols = jpeg.standard_huffman()
    coef = np.zeros(64, dtype=np.int16)
    assert _abi.jpeg_entropy_encode(scan, counts, symbols, coef) == b"\x2b"   # (DC 0: 00, EOB: 1010, filled with ones)
    with pytest.raises(ValueError):
        _abi.jpeg_entropy_encode(scan, counts, symbols, np.zeros(128, dtype=np.int16))   # (not the frame's size)
    scan.se = 62
    with pytest.raises(ValueError):
        _abi.jpeg_entropy_encode(scan, counts, symbols, coef)
    scan.se = 63
    coef[5] = 1024   # (category 11: no AC symbol)
    with pytest.raises(ValueError, match="no code"):
        _abi.jpeg_entropy_encode(scan, counts, symbols, coef)
    coef[5] = 0
    empty = np.zeros_like(counts)
    with pytest.raises(ValueError, match="no code"):
        _abi.jpeg_entropy_encode(scan, empty, symbols, coef)


# ------------------------------------------------------------------------------------------------------------------------------
# 3. whole files
# ------------------------------------------------------------------------------------------------------------------------------
def _picture(height, width, seed=1):
    """smooth colour with some noise and an edge: what a rendered document looks like to the coder"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:height, :width]
    img = np.empty((height, width, 4), dtype=np.uint8)
    img[..., 0] = (255 * xx / max(width - 1, 1)).astype(np.uint8)
    img[..., 1] = (255 * yy / max(height - 1, 1)).astype(np.uint8)
    img[..., 2] = np.where((xx - width / 2) ** 2 + (yy - height / 2) ** 2 < (min(height, width) / 3) ** 2, 230, 40)
    img[..., :3] = np.clip(img[..., :3].astype(int) + rng.integers(-6, 7, (height, width, 3)), 0, 255)
    img[..., 3] = rng.integers(0, 256, (height, width))
    return img


@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_whole_file(host_coefficients, eh, sampling):
    img = _picture(37, 53)
    kw = dict(quality=85, grey=sampling is None, subsampling=sampling or "4:2:0")
    files = {}
    for optimize in (False, True):
        for restart in (0, 2):
            data = files[optimize, restart] = S.write_jpeg(img, optimize=optimize, restart_interval=restart, **kw)
            codes = [c for _o, c, _b in jpeg.markers(data)]
            assert codes == [0xD8, 0xE0, 0xDB, 0xC0, 0xC4] + ([0xDD] if restart else []) + [0xDA, 0xD9]
            app0 = next(b for _o, c, b in jpeg.markers(data) if c == 0xE0)
            assert app0[:7] == b"JFIF\x00\x01\x01"
            frame, coef, quant = jpeg.decode_coefficients(data)
            want = E.frame_of(37, 53, sampling)
            assert (frame.width, frame.height, frame.n_comp, frame.colour) == (53, 37, want.n_comp, want.colour)
            assert list(frame.h) == list(want.h) and list(frame.v) == list(want.v)
            q = jpeg.quant_tables(85)[[0, 1, 1][:frame.n_comp]]
            assert np.array_equal(quant, q)
            assert np.array_equal(coef, E.harness_coefficients(eh, want, img, q))
    assert len(files[True, 0]) <= len(files[False, 0]) and len(files[True, 2]) <= len(files[False, 2])


def test_write_jpeg_outputs(host_coefficients, tmp_path):
    img = _picture(16, 24)
    data = S.write_jpeg(img)
    sink = io.BytesIO()
    assert S.write_jpeg(img, sink) == data and sink.getvalue() == data
    S.write_jpeg(img, tmp_path / "a.jpg")
    assert (tmp_path / "a.jpg").read_bytes() == data
    other = img.copy()
    other[..., 3] = 0   # (alpha is ignored)
    assert S.write_jpeg(other) == data
    assert "write_jpeg" in S.__all__ and "canvas_to_jpeg" in S.__all__


@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_pil_reads_the_files(host_coefficients, jh, sampling):
    Image = pytest.importorskip("PIL.Image")
    img = _picture(48, 64)
    data = S.write_jpeg(img, quality=90, grey=sampling is None, subsampling=sampling or "4:2:0")
    Image.open(io.BytesIO(data)).verify()
    im = Image.open(io.BytesIO(data))
    assert im.format == "JPEG" and im.size == (64, 48) and im.mode == ("L" if sampling is None else "RGB")
    if sampling is not None:
        assert im.layer[0][1:3] == E.SAMPLINGS[sampling] and im.layer[1][1:3] == (1, 1)
    theirs = np.asarray(im.convert("RGB")).astype(int)
    ours = R.host_read_jpeg(jh, data)[..., :3].astype(int)
    worst = int(np.abs(theirs - ours).max())
    print(f"PIL vs host decode, {sampling}: max {worst}")
    assert worst <= MAX_VS_PIL[sampling]


# ------------------------------------------------------------------------------------------------------------------------------
# 4. refusals
# ------------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments(host_coefficients):
    img = _picture(8, 8)
    for quality in (0, 101, -5, 50.5, "90", None, True):
        with pytest.raises(ValueError, match="quality"):
            S.write_jpeg(img, quality=quality)
    for subsampling in ("4:1:1", "420", None, (2, 2)):
        with pytest.raises(ValueError, match="subsampling"):
            S.write_jpeg(img, subsampling=subsampling)
    for bad in (img[..., :3], img[0], img.astype(np.float64), np.zeros((0, 8, 4), dtype=np.uint8), np.zeros((8, 0, 4), dtype=np.uint8)):
        with pytest.raises(ValueError, match="uint8 array"):
            S.write_jpeg(bad)
    for restart in (-1, 65536, 1.5):
        with pytest.raises(ValueError, match="restart"):
            S.write_jpeg(img, restart_interval=restart)
    with pytest.raises(ValueError, match="Only RGBA"):
        S.canvas_to_jpeg(np.zeros((8, 8, 3)))
