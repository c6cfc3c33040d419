"""The colour quantiser on the CPU: csrc/svgr_quant.h (through tests/quant_harness.cpp) against the numpy / Python restatement of
tests/quant_ref.py bit for bit, the palette builder's contract, the indexed container through the project's reader and Pillow,
and the arguments.  No test here touches a device: where the public functions are driven, the three device stages are replaced
by the host build of the same header."""
import ctypes as C
import io
import os
import re
import struct
import zlib

import numpy as np
import pytest

import svgrasterize_amd as S
from svgrasterize_amd import _abi, png, quant
from tests import quant_ref as R
from tests.util import ROOT


@pytest.fixture(scope="module")
def lib():
    return R.harness()


class _Buf:
    """What stands in for a DeviceBuffer: the bytes, on the host."""

    def __init__(self, arr):
        self.arr = np.ascontiguousarray(arr)
        self.nbytes = self.arr.nbytes

    def download(self, shape, dtype, offset=0):
        return self.arr.reshape(-1).view(np.uint8)[offset:].view(dtype)[:int(np.prod(shape))].reshape(shape).copy()


class _Ctx:
    def from_host(self, arr):
        return _Buf(arr)


@pytest.fixture
def host_stages(lib, monkeypatch):
    """The public route with the host build of svgr_quant.h in place of the kernels (and zlib in place of svgr_deflate)."""
    calls = []

    def image(buf, rows, cols):
        return buf.arr.reshape(rows, cols, 4)

    def distinct(ctx, buf, rows, cols, max_colors):
        calls.append("distinct")
        return R.harness_distinct(lib, image(buf, rows, cols), max_colors)

    def bins(ctx, buf, rows, cols):
        calls.append("bins")
        return R.harness_bins(lib, image(buf, rows, cols))

    def index(ctx, buf, rows, cols, palette, stream=True, indices=False):
        calls.append("index")
        s, i = R.harness_index(lib, image(buf, rows, cols), palette)
        return (_Buf(s) if stream else None), (_Buf(i) if indices else None)

    monkeypatch.setattr(_abi.Context, "get", classmethod(lambda cls, device=None: _Ctx()))
    monkeypatch.setattr(_abi, "DeviceBuffer", _Buf)
    monkeypatch.setattr(_abi, "quant_distinct", distinct)
    monkeypatch.setattr(_abi, "quant_bins", bins)
    monkeypatch.setattr(_abi, "quant_index", index)
    monkeypatch.setattr(_abi, "deflate", lambda ctx, buf, n, huffman: zlib.compress(buf.arr.tobytes()[:n], 6))
    return calls


def _pixels(rng, n):
    px = rng.integers(0, 256, (n, 4), dtype=np.uint8)
    px[::7, 3] = 0        # transparent with stray colour
    px[1::7, 3] = 255
    px[2::7, :3] = 255
    return px


def _colors(n, seed=0):
    """n distinct canonical colours, some translucent, one fully transparent."""
    rng = np.random.default_rng(seed)
    vals = rng.choice(1 << 24, size=n, replace=False).astype(np.uint32)
    alpha = np.where(np.arange(n) % 3 == 0, 255, 1 + (np.arange(n) * 37) % 254).astype(np.uint32)
    c = R.rgba(vals | alpha << 24).copy()
    c[0] = 0
    return c


# ---------------------------------------------------------------------------------------------------------------------
# the header against the restatement
# ---------------------------------------------------------------------------------------------------------------------
def test_pixel_arithmetic(lib):
    px = _pixels(np.random.default_rng(1), 400)
    extremes = np.array([[255, 255, 255, 255], [0, 0, 0, 0], [255, 255, 255, 0], [0, 0, 0, 255], [255, 0, 255, 1], [1, 1, 1, 1]], dtype=np.uint8)
    px = np.concatenate([extremes, px])
    vals = R.u32(px)
    x = (C.c_uint32 * 4)()
    for p, v in zip(px, vals):
        v = int(v)
        assert lib.h_canon(v) == int(R.u32(R.canon(p[None]))[0])
        lib.h_x(lib.h_canon(v), x)
        assert tuple(x) == R.x_of(p)
        assert lib.h_bin_key(v) == R.bin_key(p)
    assert np.array_equal(quant.coordinates(R.canon(px)), np.array([R.x_of(p) for p in px]))
    for i in range(0, len(px) - 1):
        assert lib.h_dist(lib.h_canon(int(vals[i])), lib.h_canon(int(vals[i + 1]))) == R.dist(px[i], px[i + 1])
    assert lib.h_canon(lib.h_empty()) != lib.h_empty(), "the empty slot's value is no canonical pixel"


def test_distance_at_the_extremes(lib):
    white, clear = 0xFFFFFFFF, 0
    assert lib.h_dist(white, clear) == 4 * 65025 ** 2 == R.dist((255, 255, 255, 255), (0, 0, 0, 0))
    assert 65025 ** 2 < 2 ** 32 < 4 * 65025 ** 2, "one square fits 32 bits, the sum does not"
    assert lib.h_dist(0xFF0000FF, 0xFF000000) == 65025 ** 2
    assert lib.h_dist(lib.h_canon(0x00123456), clear) == 0, "a transparent pixel's colour does not matter"
    assert R.bin_key((255, 255, 255, 255)) == (1 << 20) - 1 == lib.h_bin_key(white) and lib.h_bin_key(0x00FFFFFF) == 0


def test_ties_go_to_the_lowest_index(lib):
    for pal in ([(10, 0, 0, 255), (30, 0, 0, 255)], [(30, 0, 0, 255), (10, 0, 0, 255)], [(7, 7, 7, 255)] * 3,
                [(0, 0, 0, 0), (9, 9, 9, 0), (0, 0, 0, 0)]):
        pal = np.array(pal, dtype=np.uint8)
        for px in ((20, 0, 0, 255), (7, 7, 7, 255), (0, 0, 0, 0)):
            got = lib.h_nearest(R.u32(pal).ctypes.data_as(C.POINTER(C.c_uint32)), len(pal), int(R.u32(np.array(px, dtype=np.uint8)[None])[0]))
            assert got == R.nearest(pal, px)
    pal = np.array([(10, 0, 0, 255), (30, 0, 0, 255)], dtype=np.uint8)
    assert R.dist(pal[0], (20, 0, 0, 255)) == R.dist(pal[1], (20, 0, 0, 255)) and R.nearest(pal, (20, 0, 0, 255)) == 0


@pytest.mark.parametrize("n_pal,depth", [(2, 1), (3, 2), (4, 2), (5, 4), (16, 4), (17, 8), (256, 8), (1, 1)])
def test_row_packing(lib, n_pal, depth):
    assert lib.h_depth(n_pal) == depth == R.depth_of(n_pal) == quant.depth_of(n_pal)
    pal = _colors(n_pal, seed=n_pal)
    rng = np.random.default_rng(n_pal)
    for cols in (1, 7, 8, 9, 17):
        img = pal[rng.integers(0, n_pal, (3, cols))]
        img[0, 0] = pal[n_pal - 1]
        stream, idx = R.harness_index(lib, img, pal)
        want = R.indices_ref(img, pal)
        assert np.array_equal(idx, want) and np.array_equal(pal[idx], img)
        assert stream.shape[1] == 1 + (cols * depth + 7) // 8 == lib.h_row_bytes(cols, depth)
        assert np.array_equal(stream, R.pack_rows(want, depth))
        assert not stream[:, 0].any()


def test_harness_stages_against_numpy(lib):
    rng = np.random.default_rng(5)
    img = _pixels(rng, 40 * 30).reshape(40, 30, 4)
    img[5:20, 5:20] = (200, 100, 50, 255)
    keys, bins = R.harness_bins(lib, img)
    rkeys, rbins = R.bins_ref(img)
    assert np.array_equal(keys, rkeys) and np.array_equal(bins, rbins)
    assert (np.diff(keys.astype(np.int64)) > 0).all() and int(bins[:, 0].sum()) == 40 * 30
    assert R.harness_distinct(lib, img, 256) is None and R.distinct_ref(img, 256) is None
    few = img.copy()
    few[...] = _colors(9)[rng.integers(0, 9, (40, 30))]
    few[0, 0, :] = (50, 60, 70, 0)
    assert np.array_equal(R.harness_distinct(lib, few, 9), R.distinct_ref(few, 9))
    assert R.harness_distinct(lib, few, 8) is None


# ---------------------------------------------------------------------------------------------------------------------
# the palette builder
# ---------------------------------------------------------------------------------------------------------------------
def _gradient(rows=48, cols=64, seed=11):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:rows, 0:cols]
    img = np.stack([x * 255 // (cols - 1), y * 255 // (rows - 1), (x + y) * 255 // (rows + cols - 2), 255 - x * 200 // (cols - 1)], axis=2)
    return np.clip(img + rng.integers(-6, 7, img.shape), 0, 255).astype(np.uint8)


def test_median_cut_is_the_restated_one():
    _, bins = R.bins_ref(_gradient())
    for max_colors, refine in ((2, 0), (7, 1), (16, 3)):
        cut = quant.median_cut(bins[:, 0], bins[:, 1:], max_colors)
        assert np.array_equal(cut, R.median_cut_ref(bins[:, 0], bins[:, 1:], max_colors)) and len(cut) == max_colors
        assert np.array_equal(quant.lloyd(bins[:, 0], bins[:, 1:], cut, refine), R.lloyd_ref(bins[:, 0], bins[:, 1:], cut, refine))
        got = quant.build_palette(bins, max_colors, refine)
        assert np.array_equal(got, R.build_palette_ref(bins, max_colors, refine))


@pytest.mark.parametrize("max_colors", [2, 5, 64, 256])
def test_palette_contract(max_colors):
    _, bins = R.bins_ref(_gradient())
    pal = quant.build_palette(bins, max_colors, 2)
    assert pal.dtype == np.uint8 and pal.shape[1] == 4 and 1 <= len(pal) <= max_colors
    assert len({tuple(p) for p in pal.tolist()}) == len(pal)
    keys = [(p[3], p[0], p[1], p[2]) for p in pal.tolist()]
    assert keys == sorted(keys)
    assert not pal[pal[:, 3] == 0, :3].any(), "a transparent entry is canonical"


def test_one_bin_and_fewer_bins_than_colours():
    one = np.array([[10, 1000, 2000, 3000, 2550 * 100]], dtype=np.uint64)
    assert quant.build_palette(one, 256, 3).tolist() == [[1, 2, 3, 100]]
    two = np.array([[4, 0, 0, 0, 0], [2, 2 * 255 * 255, 0, 0, 2 * 255 * 255]], dtype=np.uint64)
    assert quant.build_palette(two, 256, 3).tolist() == [[0, 0, 0, 0], [255, 0, 0, 255]]
    assert len(quant.build_palette(two, 2, 0)) == 2


def test_trns():
    assert quant.trns(np.array([[1, 2, 3, 255], [4, 5, 6, 255]])) == b"" == R.trns_ref([[1, 2, 3, 255], [4, 5, 6, 255]])
    pal = quant.order_palette(np.array([[9, 9, 9, 255], [0, 0, 0, 0], [5, 5, 5, 128], [1, 1, 1, 255], [5, 5, 4, 128]], dtype=np.uint8))
    assert pal.tolist() == [[0, 0, 0, 0], [5, 5, 4, 128], [5, 5, 5, 128], [1, 1, 1, 255], [9, 9, 9, 255]]
    assert quant.trns(pal) == bytes([0, 128, 128]) == R.trns_ref(pal)
    assert quant.trns(np.array([[0, 0, 0, 0]])) == b"\0"


def test_refinement_does_not_raise_the_objective():
    # Lloyd's two half steps each minimise the objective over what they change; in float64 the comparison holds to rounding, which
    # for sums of ~1e3 terms of magnitude below 2^47 is far inside 1e-12 relative
    _, bins = R.bins_ref(_gradient())
    count, sums = bins[:, 0], bins[:, 1:]
    for max_colors in (4, 32):
        cut = quant.median_cut(count, sums, max_colors)
        prev = quant.objective(count, sums, cut)
        assert prev == R.objective_ref(count, sums, cut)
        for k in range(1, 6):
            cur = quant.objective(count, sums, quant.lloyd(count, sums, cut, k))
            assert cur <= prev * (1 + 1e-12), (max_colors, k, prev, cur)
            prev = cur


def test_gradient_beats_the_uniform_palette(host_stages):
    img = _gradient()
    levels = np.array([0, 85, 170, 255], dtype=np.uint8)
    uniform = np.stack(np.meshgrid(levels, levels, levels, levels, indexing="ij"), axis=-1).reshape(-1, 4)
    assert len(uniform) == 256

    def error(pal):
        near = pal[R.indices_ref(img, pal)]
        return int(((quant.coordinates(R.canon(img)) - quant.coordinates(R.canon(near))) ** 2).sum())

    idx, pal = S.quantize(img, 256, 3)
    assert host_stages == ["distinct", "bins", "index"]
    assert np.array_equal(idx, R.indices_ref(img, pal)) and np.array_equal(pal, R.palette_ref(img, 256, 3))
    assert error(pal) < error(uniform)
    assert error(pal) * 10 < error(uniform), "a median cut that is not ten times better than the uniform palette here is broken"


# ---------------------------------------------------------------------------------------------------------------------
# the routes and the container, with the host build in the kernels' place
# ---------------------------------------------------------------------------------------------------------------------
def _seam_image(n_colors):
    """16 x 17 pixels with exactly n_colors distinct colours (alpha-0 pixels with stray colour among them)."""
    c = _colors(n_colors, seed=3)
    img = c[np.arange(16 * 17) % n_colors].reshape(16, 17, 4).copy()
    stray = (img[..., 3] == 0)
    img[stray, :3] = (9, 8, 7)
    return img


def test_exact_at_256_and_lossy_at_257(host_stages):
    img = _seam_image(256)
    idx, pal = S.quantize(img)
    assert host_stages == ["distinct", "index"] and len(pal) == 256
    assert np.array_equal(pal[idx], R.canon(img)) and np.array_equal(pal, R.palette_ref(img, 256))
    del host_stages[:]
    img = _seam_image(257)
    idx, pal = S.quantize(img)
    assert host_stages == ["distinct", "bins", "index"] and len(pal) <= 256
    assert not np.array_equal(pal[idx], R.canon(img)) and np.array_equal(pal, R.palette_ref(img, 256))
    assert np.array_equal(idx, R.indices_ref(img, pal))
    idx5, pal5 = S.quantize(_seam_image(256), max_colors=5, refine=0)
    assert len(pal5) <= 5 and idx5.max() < len(pal5)


def test_hand_built_file_reads_back():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(8)
    for n in (1, 2, 4, 16, 17, 256):
        pal = quant.order_palette(_colors(n, seed=n))
        idx = rng.integers(0, n, (5, 9)).astype(np.uint8)
        data = R.indexed_png(idx, pal)
        assert np.array_equal(S.read_png(data), pal[idx])
        out = png.write_indexed_container(io.BytesIO(), 9, 5, pal, zlib.compress(R.pack_rows(idx, R.depth_of(n)).tobytes(), 9)).getvalue()
        assert out == data
        im = Image.open(io.BytesIO(out))
        assert im.mode == "P" and np.array_equal(np.asarray(im.convert("RGBA")), pal[idx])


@pytest.mark.parametrize("encoder", ["host", "device"])
def test_files_of_the_public_route(host_stages, encoder):
    img = _seam_image(16)
    for palette, n_want, depth in ((True, 16, 4), (256, 16, 4), (16, 16, 4), (3, 3, 2)):
        data = S.canvas_to_png(img, palette=palette, encoder=encoder).getvalue()
        idx, pal = S.quantize(img, 256 if palette is True else palette)
        assert len(pal) <= n_want and np.array_equal(S.read_png(data), pal[idx])
        assert data[8:16] == b"\0\0\0\rIHDR" and struct.unpack(">IIBB", data[16:26]) == (17, 16, depth, 3)
        tags = re.findall(rb"IHDR|PLTE|tRNS|IDAT|IEND", data)
        assert tags[:3] == [b"IHDR", b"PLTE", b"tRNS"] and tags.count(b"IDAT") == 1
    assert np.array_equal(S.read_png(S.canvas_to_png(img, palette=True, encoder=encoder).getvalue()), R.canon(img))
    opaque = img.copy()
    opaque[..., 3] = 255
    data = S.canvas_to_png(opaque, palette=True, encoder=encoder).getvalue()
    assert b"tRNS" not in data and np.array_equal(S.read_png(data), opaque)
    as_float = S.canvas_to_png(opaque.astype(np.float64) / 255.0, palette=True, encoder=encoder).getvalue()
    assert as_float == data


def test_host_encoder_honours_level_and_threads(host_stages):
    img = _gradient(32, 40)
    a = S.canvas_to_png(img, palette=64, level=1).getvalue()
    b = S.canvas_to_png(img, palette=64, level=9).getvalue()
    c = S.canvas_to_png(img, palette=64, level=9, threads=2).getvalue()
    assert len(b) <= len(a) and a != b
    assert np.array_equal(S.read_png(a), S.read_png(b)) and np.array_equal(S.read_png(c), S.read_png(b))


# ---------------------------------------------------------------------------------------------------------------------
# arguments, the ABI, and what has not changed
# ---------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_never_reach_the_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(_abi.Context, "get", classmethod(no_device))
    img = _seam_image(4)
    for bad in (1, 0, 257, -3):
        with pytest.raises(ValueError, match="palette"):
            S.canvas_to_png(img, palette=bad)
        with pytest.raises(ValueError, match="max_colors"):
            S.quantize(img, max_colors=bad)
    for bad in (2.0, "256", (4,)):
        with pytest.raises(TypeError, match="palette"):
            S.canvas_to_png(img, palette=bad, encoder="device")
        with pytest.raises(TypeError, match="max_colors"):
            S.quantize(img, max_colors=bad)
    with pytest.raises(TypeError, match="max_colors"):
        S.quantize(img, max_colors=True)
    with pytest.raises(ValueError, match="refine"):
        S.quantize(img, refine=-1)
    for bad in (1.5, None, True):
        with pytest.raises(TypeError, match="refine"):
            S.quantize(img, refine=bad)
    for filter in ("adaptive", "sub", "up", "average", "paeth"):
        with pytest.raises(ValueError, match=filter):
            S.canvas_to_png(img, palette=True, encoder="device", filter=filter)
    with pytest.raises(ValueError, match="filter"):
        S.canvas_to_png(img, palette=True, encoder="device", filter="best")
    with pytest.raises(ValueError, match="Huffman"):
        S.canvas_to_png(img, palette=True, encoder="device", huffman="static")
    with pytest.raises(TypeError, match="filter and huffman"):
        S.canvas_to_png(img, palette=True, filter="none")
    with pytest.raises(TypeError, match="level and threads"):
        S.canvas_to_png(img, palette=True, encoder="device", level=3)
    with pytest.raises(ValueError, match="RGBA"):
        S.canvas_to_png(img[..., :3], palette=True)
    for bad in (img[..., :3], img.astype(np.float32), img[:0], img[0]):
        with pytest.raises(ValueError, match="uint8"):
            S.quantize(bad)
    with pytest.raises(ValueError, match="palette"):   # (before the document is read: the path does not exist)
        S.render_svg("no/such/file.svg", palette=1)
    with pytest.raises(ValueError, match="paeth"):
        S.render_svg("no/such/file.svg", palette=True, encoder="device", filter="paeth")
    with pytest.raises(ValueError, match="palette"):
        S.Layer(np.zeros((2, 2, 4)), (0, 0), pre_alpha=True, linear_rgb=True).write_png(palette=300)


def test_abi_and_exports():
    names = ("svgr_quant_distinct", "svgr_quant_bins", "svgr_quant_index", "svgr_quant_block", "svgr_quant_groups")
    hdr = open(os.path.join(ROOT, "include", "svgr.h")).read()
    lib = _abi.load_library()
    assert lib.svgr_abi_version() == 6 and "#define SVGR_ABI_VERSION 6" in hdr
    for name in names:
        assert name in _abi.EXPORTS and re.search(rf"\b{name}\s*\(", hdr) and hasattr(lib, name)
    assert "quantize" in S.__all__ and S.quantize is quant.quantize
    assert _abi.quant_block() == 256 * R.harness().h_run() and R.harness().h_slots() >= 4 * quant.MAX_COLORS


def test_the_default_file_has_not_changed():
    img = _gradient(19, 23)
    raw = b"".join(b"\0" + img[r].tobytes() for r in range(19))

    def chunk(tag, body):
        return struct.pack("!I", len(body)) + tag + body + struct.pack("!I", zlib.crc32(tag + body) & 0xFFFFFFFF)

    want = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack("!2I5B", 23, 19, 8, 6, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw, 9)) + chunk(b"IEND", b"")
    assert S.canvas_to_png(img).getvalue() == want
    assert S.canvas_to_png(img, palette=None).getvalue() == want == S.canvas_to_png(img, palette=False).getvalue()
