"""The device PNG encoder on the CPU: csrc/svgr_png.h and csrc/svgr_deflate.h, driven serially by tests/png_enc_harness.cpp,
against the numpy / Python restatement of tests/png_enc_ref.py, the tables of RFC 1951 and zlib.  The device runs the same
headers (tests/test_gpu_png_encode.py holds its bytes against this harness), so what is pinned here is the device's too."""
import io
import struct
import zlib

import numpy as np
import pytest

import svgrasterize_amd as S
from svgrasterize_amd import _abi, png
from tests import png_enc_ref as R


@pytest.fixture(scope="module")
def lib():
    return R.harness()


@pytest.fixture(scope="module")
def ch(lib):
    return lib.h_deflate_chunk()


@pytest.fixture(scope="module")
def cases(ch):
    return R.deflate_cases(ch)


@pytest.fixture
def host_idat(lib, monkeypatch):
    """the encoder with its device stage on the host build"""
    monkeypatch.setattr(png, "_idat_stage", lambda rgba8, rows, cols, filter, huffman: R.harness_idat(lib, rgba8, filter, huffman))


# ------------------------------------------------------------------------------------------------------------------------------
# 1. filters
# ------------------------------------------------------------------------------------------------------------------------------
def _images():
    rng = np.random.default_rng(62)
    grad = np.zeros((9, 40, 4), dtype=np.uint8)
    grad[..., 0] = np.arange(40) * 6
    grad[..., 1] = (np.arange(9) * 25)[:, None]
    grad[..., 2] = (np.arange(40)[None, :] * 3 + np.arange(9)[:, None] * 7) & 255
    grad[..., 3] = 255
    return {
        "random": rng.integers(0, 256, (7, 13, 4), dtype=np.uint8),
        "flat": np.full((5, 6, 4), 77, dtype=np.uint8),
        "gradient": grad,
        "column": rng.integers(0, 256, (11, 1, 4), dtype=np.uint8),
        "row": rng.integers(0, 256, (1, 17, 4), dtype=np.uint8),
        "pixel": np.array([[[1, 2, 3, 4]]], dtype=np.uint8),
        # values 0 .. 3: the Paeth distances tie all the time (pa == pb, pb == pc), and so do the rows' sums
        "ties": rng.integers(0, 4, (12, 9, 4), dtype=np.uint8),
        "zero": np.zeros((3, 4, 4), dtype=np.uint8),
    }


@pytest.mark.parametrize("name", list(_images()))
@pytest.mark.parametrize("filter", R.FILTERS)
def test_filter_against_numpy(lib, name, filter):
    img = _images()[name]
    rows, cols, _ = img.shape
    got = R.harness_filter(lib, img, filter)
    assert np.array_equal(got, R.filter_ref(img, filter))
    if filter != "adaptive":
        assert (got[:, 0] == R.FILTERS.index(filter)).all()
    back = _abi.png_unfilter(got.tobytes(), rows, 4 * cols, 4)
    assert np.array_equal(back.reshape(rows, cols, 4), img)


def test_paeth_ties():
    # the order a, b, c: pa == pb goes to a, pb == pc to b.  (pa == pb with a != b needs c = (a + b) / 2, where pc = 0 wins: the
    # first tie shows only with a == b; the ref is the specification's wording, the header is held against it below)
    a, b, c = np.meshgrid(np.arange(0, 256, 3), np.arange(0, 256, 5), np.arange(0, 256, 7), indexing="ij")
    got = R._paeth(a, b, c)
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    tie_bc = (pb == pc) & (pb < pa) & (b != c)
    assert tie_bc.any() and (got[tie_bc] == b[tie_bc]).all()
    tie_ab = (pa == pb) & (pa <= pc)
    assert tie_ab.any() and (got[tie_ab] == a[tie_ab]).all()


def test_paeth_of_the_header(lib):
    rng = np.random.default_rng(5)
    tri = np.concatenate([rng.integers(0, 256, (4000, 3)), rng.integers(0, 4, (500, 3)), [[0, 30, 10], [10, 10, 0], [255, 0, 255], [0, 0, 0]]])
    want = R._paeth(tri[:, 0], tri[:, 1], tri[:, 2])
    assert [lib.h_paeth(int(a), int(b), int(c)) for a, b, c in tri] == want.tolist()


def test_adaptive_ties_go_to_the_lower_type(lib):
    for name in ("ties", "zero", "flat", "gradient"):
        img = _images()[name]
        sums = R.row_sums(img)
        got = np.zeros((img.shape[0], 5), dtype=np.uint32)
        for r in range(img.shape[0]):
            lib.h_row_sums(img.ctypes.data, img.shape[0], img.shape[1], r, got[r].ctypes.data)
        assert np.array_equal(got, sums)
        kind = R.harness_filter(lib, img, "adaptive")[:, 0]
        for r in range(img.shape[0]):
            assert kind[r] == min(t for t in range(5) if sums[r, t] == sums[r].min())
    # row 0 has no row above: Up ties with None and Paeth with Sub, whatever the pixels
    sums = R.row_sums(_images()["random"])
    assert sums[0, 2] == sums[0, 0] and sums[0, 4] == sums[0, 1]
    assert (R.row_sums(_images()["zero"]) == 0).all() and (R.harness_filter(lib, _images()["zero"], "adaptive")[:, 0] == 0).all()
    tied = R.row_sums(_images()["ties"])
    assert any((np.sort(row)[0] == np.sort(row)[1]) for row in tied[1:]), "the image was made for rows whose best types tie"


# ------------------------------------------------------------------------------------------------------------------------------
# 2. symbol maps
# ------------------------------------------------------------------------------------------------------------------------------
def _rfc(value, base, extra):
    s = max(i for i in range(len(base)) if base[i] <= value)
    return s, extra[s], value - base[s]


def test_length_map_is_rfc1951(lib):
    out = (3 * np.ones(3, dtype=np.int32)).copy()
    for length in range(3, 259):
        lib.h_len_sym(length, out.ctypes.data)
        s, nb, val = _rfc(length, R.LEN_BASE, R.LEN_EXTRA)
        assert out.tolist() == [257 + s, nb, val], length
    lib.h_len_sym(258, out.ctypes.data)
    assert out.tolist() == [285, 0, 0]
    lib.h_len_sym(257, out.ctypes.data)
    assert out.tolist() == [284, 5, 30]


def test_distance_map_is_rfc1951(lib):
    out = np.zeros(3, dtype=np.int32)
    base = np.array(R.DIST_BASE)
    for dist in range(1, 32769):
        lib.h_dist_sym(dist, out.ctypes.data)
        s = int(np.searchsorted(base, dist, side="right")) - 1
        assert out[0] == s and out[1] == R.DIST_EXTRA[s] and out[2] == dist - R.DIST_BASE[s], dist


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the code builder
# ------------------------------------------------------------------------------------------------------------------------------
def _lengths(lib, counts, limit):
    counts = np.asarray(counts, dtype=np.uint64)
    out = np.zeros(counts.size, dtype=np.uint8)
    lib.h_lengths(counts.ctypes.data, counts.size, limit, out.ctypes.data)
    return out


def _fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f


@pytest.mark.parametrize("n,limit", [(40, 15), (30, 15), (19, 7), (286, 15)])
def test_fibonacci_counts_meet_the_limit(lib, n, limit):
    counts = (_fib(min(n, 60)) + [1] * n)[:n]   # (an unlimited code would be n - 1 bits deep)
    lens = _lengths(lib, counts, limit)
    assert lens.min() >= 1 and lens.max() == limit and R.kraft(lens) == 1
    order = np.argsort(counts, kind="stable")
    assert (np.diff(lens[order].astype(np.int64)) <= 0).all(), "a rarer symbol never has the shorter code"


def test_unlimited_code_is_huffman(lib):
    # where the limit does not bind the cost is the optimum: against a plain heap Huffman
    import heapq

    rng = np.random.default_rng(3)
    for _ in range(20):
        counts = rng.integers(0, 1000, 60)
        counts[rng.integers(0, 60, 2)] += 1
        lens = _lengths(lib, counts, 15)
        heap = [(int(c), i) for i, c in enumerate(counts) if c]
        heapq.heapify(heap)
        cost = 0
        while len(heap) > 1:
            a, b = heapq.heappop(heap), heapq.heappop(heap)
            cost += a[0] + b[0]
            heapq.heappush(heap, (a[0] + b[0], -1))
        assert R.kraft(lens) == 1 and ((lens == 0) == (counts == 0)).all()
        if lens.max() < 15:
            assert int((lens.astype(np.int64) * counts).sum()) == cost


def _codes(lib, counts, huffman=1):
    c = R.Codes()
    counts = np.ascontiguousarray(counts, dtype=np.uint64)
    lib.h_build_codes(counts.ctypes.data, huffman, c)
    return c


def _check_dynamic(c):
    ll, dl = list(c.llen)[:286], list(c.dlen)[:30]
    assert R.kraft(ll) == 1 and R.kraft(dl) == 1 and max(ll) <= 15 and max(dl) <= 15 and ll[256] > 0
    bits = R._Bits(bytes(c.hdr))
    assert bits.take(1) == 0 and bits.take(2) == 2   # BFINAL clear, BTYPE 10
    rl, rd, cl = R.read_dynamic_header(bits)
    assert bits.pos == c.hdr_bits <= 8 * 320
    assert R.kraft(cl) == 1 and max(cl) <= 7
    assert rl == ll[:len(rl)] and not any(ll[len(rl):]) and rd == dl[:len(rd)] and not any(dl[len(rd):])
    for lens, codes in ((ll, c.lcode), (dl, c.dcode)):   # canonical, stored bit-reversed
        for (length, code), sym in R._decoder(lens).items():
            assert int(f"{codes[sym]:0{length}b}"[::-1], 2) == code
    return ll, dl


def test_code_builder_edge_alphabets(lib):
    counts = np.zeros(316, dtype=np.uint64)
    counts[256] = 1   # nothing but the end of block, and no distance symbol at all
    ll, dl = _check_dynamic(_codes(lib, counts))
    assert [i for i, v in enumerate(ll) if v] == [0, 256] and dl[:2] == [1, 1] and not any(dl[2:])
    counts[65] = 1000   # one literal; one distance symbol that is not 0
    counts[286 + 7] = 3
    ll, dl = _check_dynamic(_codes(lib, counts))
    assert ll[65] == 1 and ll[256] == 1 and dl[0] == 1 and dl[7] == 1
    counts[:] = 0   # every count 0, as the fixed mode passes them: the end of block is put in
    _check_dynamic(_codes(lib, counts))
    fib = _fib(60)
    counts[:60] = fib
    counts[256] = 1
    counts[286:316] = fib[:30]
    ll, dl = _check_dynamic(_codes(lib, counts))
    assert max(ll) == 15 and max(dl) == 15
    rng = np.random.default_rng(9)
    for _ in range(10):
        counts = rng.integers(0, 50, 316).astype(np.uint64) * rng.integers(0, 2, 316).astype(np.uint64)
        _check_dynamic(_codes(lib, counts))


def test_fixed_code(lib):
    c = _codes(lib, np.zeros(316, dtype=np.uint64), huffman=0)
    assert list(c.llen) == [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8 and list(c.dlen) == [5] * 32
    assert c.hdr_bits == 3 and c.hdr[0] == 0b010
    assert c.lcode[0] == int("00110000"[::-1], 2) and c.lcode[256] == 0 and c.lcode[144] == int("110010000"[::-1], 2)
    assert c.dcode[1] == 0b10000


# ------------------------------------------------------------------------------------------------------------------------------
# 4. streams
# ------------------------------------------------------------------------------------------------------------------------------
CASE_NAMES = ["len0", "len1", "len2", "len3", "zeros257", "zeros258", "zeros259", "zeros260", "zeros517", "ch-1", "ch", "ch+1", "2ch+5",
              "random", "period4", "twice32768", "twice32769", "rows"]
# The harness's stream lengths (fixed, dynamic) at the chunk size 16384, as measured on the host build: a regression mark.  DESIGN
# 7n has them beside zlib's.
PINNED = {
    "len0": (8, 18), "len1": (9, 19), "len2": (10, 20), "len3": (11, 21), "zeros257": (11, 21), "zeros258": (11, 21),
    "zeros259": (10, 20), "zeros260": (11, 20), "zeros517": (12, 21), "ch-1": (8488, 7806), "ch": (6781, 6249),
    "ch+1": (6624, 6116), "2ch+5": (13034, 12102), "random": (17296, 16465), "period4": (33, 35),
    "twice32768": (40613, 38681), "twice32769": (69122, 65752), "rows": (1963, 2023),
}


def test_the_cases_are_the_listed_ones(cases, ch):
    assert list(cases) == CASE_NAMES
    assert [len(cases[k]) for k in ("ch-1", "ch", "ch+1", "2ch+5", "random")] == [ch - 1, ch, ch + 1, 2 * ch + 5, ch + 7]
    assert cases["twice32768"][:32768] == cases["twice32768"][32768:] and cases["twice32769"][:32769] == cases["twice32769"][32769:]


@pytest.fixture(scope="module")
def ref_tokens(cases, ch):
    return {name: R.tokens_ref(data, ch) for name, data in cases.items()}


@pytest.mark.parametrize("huffman", [0, 1], ids=["fixed", "dynamic"])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_stream(lib, cases, ref_tokens, ch, name, huffman):
    data = cases[name]
    stream, tokens, counts = R.harness_deflate(lib, data, huffman)
    print(f"{name} huffman {huffman}: {len(data)} -> {len(stream)} bytes, {len(tokens)} tokens; zlib 1: {len(zlib.compress(data, 1))}, "
          f"zlib 9: {len(zlib.compress(data, 9))}")
    assert zlib.decompress(stream) == data
    assert tokens == ref_tokens[name]
    parsed = R.parse_zlib(stream)
    assert parsed["tokens"] == tokens and parsed["adler"] == zlib.adler32(data)
    a, b = R.adler_pieces(data, ch)
    assert (b << 16) | a == zlib.adler32(data)
    # one block per chunk, each on a byte boundary, an empty stored block behind every one but the last
    n_chunks = max(1, -(-len(data) // ch))
    blocks = parsed["blocks"]
    assert [b_["type"] for b_ in blocks] == ([2 if huffman else 1, 0] * n_chunks)[:-1]
    assert [b_["final"] for b_ in blocks] == [0] * (len(blocks) - 1) + [1]
    coded = blocks[::2]
    assert all(b_["bit0"] == 0 for b_ in coded) and all(b_["stored"] == 0 for b_ in blocks[1::2])
    if huffman:
        first = coded[0]
        assert R.kraft(first["ll"]) == 1 and R.kraft(first["dl"]) == 1 and R.kraft(first["cl"]) == 1
        for b_ in coded[1:]:   # the same header, so the tokens begin at the same bit offset
            assert (b_["ll"], b_["dl"], b_["cl"], b_["header_bits"]) == (first["ll"], first["dl"], first["cl"], first["header_bits"])
            n_hdr = first["header_bits"] // 8
            assert stream[b_["byte0"] + 1:b_["byte0"] + n_hdr] == stream[first["byte0"] + 1:first["byte0"] + n_hdr]
    # the tokens: matches stay inside the window and inside their chunk, and the counts are theirs
    pos, want = 0, np.zeros(316, dtype=np.uint64)
    want[256] = n_chunks
    for t in tokens:
        if t < 256:
            want[t] += 1
            pos += 1
        else:
            length, dist = t >> 16, (t & 0xFFFF) + 1
            assert 3 <= length <= 258 and 1 <= dist <= min(pos, 32768) and (pos % ch) + length <= ch
            want[257 + max(i for i in range(29) if R.LEN_BASE[i] <= length) if length < 258 else 285] += 1
            want[286 + max(i for i in range(30) if R.DIST_BASE[i] <= dist)] += 1
            pos += length
    assert pos == len(data) and np.array_equal(want, counts)
    assert ch != 16384 or len(stream) == PINNED[name][huffman]


def test_what_the_cases_exercise(lib, cases, ch):
    tok = {name: R.harness_deflate(lib, cases[name], 1)[1] for name in ("random", "zeros517", "period4", "twice32768", "twice32769", "rows", "zeros258")}
    assert all(t < 256 for t in tok["random"]), "random bytes: no match, the empty distance alphabet"
    assert tok["zeros258"] == [0, (257 << 16) | 0] and tok["zeros517"] == [0, (258 << 16) | 0, (258 << 16) | 0]
    assert tok["period4"][:5] == [10, 200, 30, 255, (258 << 16) | 3]
    far = [(t & 0xFFFF) + 1 for t in tok["twice32768"] if t >= 256]
    assert far and max(far) == 32768, "distance 32768 is legal and is found"
    assert all(t < 256 or (t & 0xFFFF) + 1 < 32768 for t in tok["twice32769"]), "nothing beyond the window"
    stride = 1 + 4 * 301
    pos, across = 0, 0
    for t in tok["rows"]:
        if t >= 256 and (t & 0xFFFF) + 1 == stride and pos // ch > (pos - stride) // ch:
            across += 1
        pos += 1 if t < 256 else t >> 16
    assert across > 0, "a match whose source row lies in the chunk before"


@pytest.mark.parametrize("huffman", [0, 1])
def test_short_output(lib, cases, huffman):
    for name in ("len0", "zeros517", "ch+1"):
        stream = R.harness_deflate(lib, cases[name], huffman)[0]
        assert R.harness_deflate(lib, cases[name], huffman, out_cap=len(stream) - 1) == (5, len(stream))
        assert R.harness_deflate(lib, cases[name], huffman, out_cap=len(stream)) == (0, len(stream))


# ------------------------------------------------------------------------------------------------------------------------------
# 5. whole files
# ------------------------------------------------------------------------------------------------------------------------------
def _picture(height, width):
    rng = np.random.default_rng(11)
    y, x = np.mgrid[0:height, 0:width]
    img = np.zeros((height, width, 4), dtype=np.uint8)
    img[..., 0] = (x * 255) // max(width - 1, 1)
    img[..., 1] = (y * 255) // max(height - 1, 1)
    img[..., 2] = np.where((x // 8 + y // 8) % 2, 200, 30)
    img[..., 3] = np.where(x > width // 3, 255, rng.integers(0, 256, (height, width)))
    return img


@pytest.mark.parametrize("huffman", ["fixed", "dynamic"])
@pytest.mark.parametrize("filter", R.FILTERS)
def test_whole_file(host_idat, filter, huffman):
    img = _picture(37, 53)
    data = S.canvas_to_png(img, encoder="device", filter=filter, huffman=huffman).getvalue()
    assert np.array_equal(S.read_png(data), img)
    assert data[:8] == b"\x89PNG\r\n\x1a\n" and data[12:16] == b"IHDR" and struct.unpack("!2I5B", data[16:29]) == (53, 37, 8, 6, 0, 0, 0)
    kinds = [data[i + 4:i + 8] for i in (8, 33)] + [data[-8:-4]]
    assert kinds == [b"IHDR", b"IDAT", b"IEND"]


def test_outputs_and_defaults(host_idat, lib):
    img = _picture(16, 24)
    data = S.canvas_to_png(img, encoder="device").getvalue()
    assert data == S.canvas_to_png(img, encoder="device", filter="adaptive", huffman="dynamic").getvalue()
    sink = io.BytesIO()
    assert S.canvas_to_png(img, sink, encoder="device") is sink and sink.getvalue() == data
    assert np.array_equal(S.read_png(S.canvas_to_png(img.astype(np.float64) / 255.0, encoder="device").getvalue()), img)
    assert len(data) < len(S.canvas_to_png(img, encoder="device", filter="none", huffman="fixed").getvalue())


def test_pil_reads_the_files(host_idat):
    Image = pytest.importorskip("PIL.Image")
    img = _picture(48, 64)
    for filter in R.FILTERS:
        data = S.canvas_to_png(img, encoder="device", filter=filter).getvalue()
        Image.open(io.BytesIO(data)).verify()
        im = Image.open(io.BytesIO(data))
        assert im.format == "PNG" and im.size == (64, 48) and im.mode == "RGBA"
        assert np.array_equal(np.asarray(im), img)


def test_bad_arguments(host_idat):
    img = _picture(8, 8)
    for kw in (dict(level=6), dict(threads=4), dict(level=9, threads=1)):
        with pytest.raises(TypeError, match="level and threads"):
            S.canvas_to_png(img, encoder="device", **kw)
    for kw in (dict(filter="sub"), dict(huffman="fixed")):
        with pytest.raises(TypeError, match="filter and huffman"):
            S.canvas_to_png(img, **kw)
    for encoder in ("gpu", None, 1, "Device"):
        with pytest.raises(ValueError, match="encoder"):
            S.canvas_to_png(img, encoder=encoder)
    for filter in ("best", 4, "Paeth", b"up"):
        with pytest.raises(ValueError, match="filter"):
            S.canvas_to_png(img, encoder="device", filter=filter)
    for huffman in ("static", 1, True):
        with pytest.raises(ValueError, match="Huffman"):
            S.canvas_to_png(img, encoder="device", huffman=huffman)
    with pytest.raises(ValueError, match="RGBA"):
        S.canvas_to_png(img[..., :3], encoder="device")
    with pytest.raises(ValueError, match="filter"):
        png.filter_device(img, "best")
    with pytest.raises(ValueError, match="Huffman"):
        png.deflate_device(b"abc", "best")
    with pytest.raises(ValueError, match="encoder"):   # (before the document is read: the path does not exist)
        S.render_svg("no/such/file.svg", encoder="gpu")
    with pytest.raises(TypeError, match="level and threads"):
        S.render_svg("no/such/file.svg", encoder="device", level=1)


def test_the_default_route_is_the_reference_file():
    img = _picture(19, 23)
    raw = b"".join(b"\0" + img[r].tobytes() for r in range(19))

    def chunk(tag, body):
        return struct.pack("!I", len(body)) + tag + body + struct.pack("!I", zlib.crc32(tag + body) & 0xFFFFFFFF)

    want = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack("!2I5B", 23, 19, 8, 6, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw, 9)) + chunk(b"IEND", b"")
    assert S.canvas_to_png(img).getvalue() == want == S.canvas_to_png(img, None, 9, 1, encoder="host").getvalue()
    assert np.array_equal(S.read_png(S.canvas_to_png(img, level=1, threads=2).getvalue()), img)
