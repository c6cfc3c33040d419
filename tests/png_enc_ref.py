"""The device PNG encoder restated in plain numpy / Python (csrc/svgr_png.h, csrc/svgr_deflate.h), the tables of
RFC 1951 written out, a small inflate parser that gives back a stream's tokens and headers, the test cases both test files
share, and the ctypes front of the host harness (tests/png_enc_harness.cpp)."""
import ctypes as C
from fractions import Fraction

import numpy as np

from tests.util import host_build

FILTERS = ("none", "sub", "up", "average", "paeth", "adaptive")
WINDOW, MIN_MATCH, MAX_MATCH, TOO_FAR, HASH_BITS, SUB = 32768, 3, 258, 4096, 13, 256

# RFC 1951 3.2.5: symbol 257 + i codes lengths from LEN_BASE[i] with LEN_EXTRA[i] extra bits; distance symbol i likewise
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


# ------------------------------------------------------------------------------------------------------------------------------
# filters
# ------------------------------------------------------------------------------------------------------------------------------
def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filtered_rows(img):
    """(5, rows, 4 * cols) uint8: every row of an (rows, cols, 4) uint8 image under each of the five filter types."""
    rows, cols, _ = img.shape
    x = img.reshape(rows, cols * 4).astype(np.int64)
    a = np.zeros_like(x)
    a[:, 4:] = x[:, :-4]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, 4:] = x[:-1, :-4]
    pred = (np.zeros_like(x), a, b, (a + b) >> 1, _paeth(a, b, c))
    return np.stack([((x - p) & 255).astype(np.uint8) for p in pred])


def row_sums(img):
    """(rows, 5): libpng's heuristic, the sum of min(v, 256 - v) over each row's filtered bytes, per type."""
    f = filtered_rows(img).astype(np.int64)
    return np.minimum(f, 256 - f).sum(axis=2).T


def filter_ref(img, filter):
    """The filtered stream (rows, 1 + 4 * cols) uint8 of an (rows, cols, 4) uint8 image."""
    f = filtered_rows(img)
    rows = img.shape[0]
    kind = np.argmin(row_sums(img), axis=1) if filter == "adaptive" else np.full(rows, FILTERS.index(filter))   # (argmin: the first)
    out = np.empty((rows, 1 + 4 * img.shape[1]), dtype=np.uint8)
    out[:, 0] = kind
    out[:, 1:] = f[kind, np.arange(rows)]
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# the token rule
# ------------------------------------------------------------------------------------------------------------------------------
def _match(data, p, d, cap):
    x = int.from_bytes(data[p:p + cap], "little") ^ int.from_bytes(data[p - d:p - d + cap], "little")
    return cap if x == 0 else ((x & -x).bit_length() - 1) // 8


def tokens_ref(data, ch):
    """The flat token list of `data` (bytes) at chunk size `ch`: a literal is its byte, a match (length << 16) | (distance - 1)."""
    data = bytes(data)
    n = len(data)
    b = np.frombuffer(data, dtype=np.uint8).astype(np.uint32)
    pos = np.arange(n, dtype=np.int64)
    hashed = pos + 2 < np.minimum((pos // ch + 1) * ch, n)
    h = np.zeros(n, dtype=np.int64)
    if n >= 3:
        v = b[:-2] | (b[1:-1] << np.uint32(8)) | (b[2:] << np.uint32(16))
        h[:n - 2] = (v * np.uint32(0x9E3779B1)) >> np.uint32(32 - HASH_BITS)
    tokens = []
    for start in range(0, max(n, 1), ch):
        end = min(n, start + ch)
        table = np.full(1 << HASH_BITS, -1, dtype=np.int64)
        q = np.arange(max(0, start - WINDOW), start)
        q = q[hashed[q]]
        np.maximum.at(table, h[q], q)
        cand = np.full(end - start, -1, dtype=np.int64)
        for w in range(start, end, SUB):
            q = np.arange(w, min(w + SUB, end))
            q = q[hashed[q]]
            cand[q - start] = table[h[q]]
            np.maximum.at(table, h[q], q)
        p = start
        while p < end:
            cap = min(MAX_MATCH, end - p)
            best, best_d = 0, 0
            if cap >= MIN_MATCH:
                c = int(cand[p - start])
                for d in (1 if p >= 1 else 0, 4 if p >= 4 else 0, p - c if c >= 0 and p - c <= WINDOW else 0):
                    if best == cap:
                        break
                    if d:
                        length = _match(data, p, d, cap)
                        if length > best:
                            best, best_d = length, d
            if best < MIN_MATCH or (best == MIN_MATCH and best_d > TOO_FAR):
                tokens.append(data[p])
                p += 1
            else:
                tokens.append((best << 16) | (best_d - 1))
                p += best
    return tokens


def adler_pieces(data, ch):
    """(a, b) of Adler-32 put together from per-chunk sums by the header's combine rule, in plain integers."""
    a, b = 1, 0
    for start in range(0, len(data), ch):
        piece = data[start:start + ch]
        n = len(piece)
        A = sum(piece) % 65521
        B = sum((n - i) * v for i, v in enumerate(piece)) % 65521
        b = (b + n * a + B) % 65521
        a = (a + A) % 65521
    return a, b


# ------------------------------------------------------------------------------------------------------------------------------
# inflate, as a parser: the stream's tokens and what its block headers say
# ------------------------------------------------------------------------------------------------------------------------------
class _Bits:
    def __init__(self, data, pos=0):
        self.data, self.pos = data, pos

    def take(self, n):
        v = 0
        for i in range(n):
            v |= ((self.data[self.pos >> 3] >> (self.pos & 7)) & 1) << i
            self.pos += 1
        return v


def kraft(lengths):
    return sum((Fraction(1, 1 << int(l)) for l in lengths if l), Fraction(0))


def _decoder(lengths):
    """{(length, code): symbol} of the canonical code (RFC 1951 3.2.2)."""
    lengths = [int(l) for l in lengths]
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    table = {}
    for s, l in enumerate(lengths):
        if l:
            table[l, nxt[l]] = s
            nxt[l] += 1
    return table


def _symbol(bits, table):
    code = 0
    for l in range(1, 16):
        code = (code << 1) | bits.take(1)   # (a Huffman code comes most significant bit first)
        if (l, code) in table:
            return table[l, code]
    raise ValueError("bits that are no code of the table")


def read_dynamic_header(bits):
    """After BTYPE 10: (literal / length lengths, distance lengths, code-length-code lengths)."""
    hlit, hdist, hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
    clen = [0] * 19
    for i in range(hclen):
        clen[CL_ORDER[i]] = bits.take(3)
    table, seq = _decoder(clen), []
    while len(seq) < hlit + hdist:
        s = _symbol(bits, table)
        if s < 16:
            seq.append(s)
        elif s == 16:
            seq += [seq[-1]] * (3 + bits.take(2))
        else:
            seq += [0] * (3 + bits.take(3) if s == 17 else 11 + bits.take(7))
    if len(seq) != hlit + hdist:
        raise ValueError("a run of code lengths beyond the alphabets")
    return seq[:hlit], seq[hlit:], clen


def parse_zlib(stream):
    """dict(tokens, blocks, adler): the flat token list of a zlib stream, one record per block -- dict(type, final, byte0 (the
    byte the block begins in), bit0, and for a dynamic block ll, dl, cl and header_bits) -- and the Adler-32 it ends with."""
    if stream[:2] != b"\x78\x01":
        raise ValueError("not the zlib header 78 01")
    bits, tokens, blocks = _Bits(stream, 16), [], []
    fixed_ll = _decoder([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
    fixed_dl = _decoder([5] * 32)
    while True:
        at = bits.pos
        final, kind = bits.take(1), bits.take(2)
        rec = dict(type=kind, final=final, byte0=at >> 3, bit0=at & 7)
        blocks.append(rec)
        if kind == 0:
            bits.pos = (bits.pos + 7) & ~7
            n, nn = bits.take(16), bits.take(16)
            if n ^ nn != 0xFFFF:
                raise ValueError("a stored block whose lengths disagree")
            tokens += list(stream[bits.pos >> 3:(bits.pos >> 3) + n])
            bits.pos += 8 * n
            rec["stored"] = n
        elif kind in (1, 2):
            if kind == 2:
                ll, dl, cl = read_dynamic_header(bits)
                rec.update(ll=ll, dl=dl, cl=cl, header_bits=bits.pos - at)
                lt, dt = _decoder(ll), _decoder(dl)
            else:
                lt, dt = fixed_ll, fixed_dl
            while True:
                s = _symbol(bits, lt)
                if s < 256:
                    tokens.append(s)
                elif s == 256:
                    break
                else:
                    length = LEN_BASE[s - 257] + bits.take(LEN_EXTRA[s - 257])
                    d = _symbol(bits, dt)
                    tokens.append((length << 16) | (DIST_BASE[d] + bits.take(DIST_EXTRA[d]) - 1))
        else:
            raise ValueError("block type 11")
        if final:
            break
    bits.pos = (bits.pos + 7) & ~7
    end = bits.pos >> 3
    if len(stream) != end + 4:
        raise ValueError("bytes behind the Adler-32")
    return dict(tokens=tokens, blocks=blocks, adler=int.from_bytes(stream[end:], "big"))


# ------------------------------------------------------------------------------------------------------------------------------
# the cases of the deflate tests (CPU: harness against zlib and the ref; GPU: device against harness)
# ------------------------------------------------------------------------------------------------------------------------------
def deflate_cases(ch):
    """{name: bytes}: the inputs both deflate tests run."""
    rng = np.random.default_rng(1951)
    rand = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()   # noqa: E731
    cases = {f"len{n}": bytes(range(65, 65 + n)) for n in (0, 1, 2, 3)}
    cases.update({f"zeros{n}": bytes(n) for n in (257, 258, 259, 260, 517)})
    for name, n in (("ch-1", ch - 1), ("ch", ch), ("ch+1", ch + 1), ("2ch+5", 2 * ch + 5)):
        # runs, a short alphabet and noise by turns: matches at every candidate, literals, and both at the chunk seams
        parts, size = [], 0
        while size < n:
            k = int(rng.integers(1, 400))
            kind = int(rng.integers(0, 4))
            part = (bytes([int(rng.integers(0, 256))]) * k if kind == 0 else bytes(rng.integers(0, 3, k, dtype=np.uint8)) if kind == 1
                    else rand(4) * (k // 4 + 1) if kind == 2 else rand(k))
            parts.append(part)
            size += len(part)
        cases[name] = b"".join(parts)[:n]
    noise, seen = bytearray(), set()   # random bytes in which no three bytes come twice: no match whatever the matcher
    while len(noise) < ch + 7:
        noise.append(int(rng.integers(0, 256)))
        if len(noise) >= 3:
            if bytes(noise[-3:]) in seen:
                noise.pop()
            else:
                seen.add(bytes(noise[-3:]))
    cases["random"] = bytes(noise)
    cases["period4"] = bytes([10, 200, 30, 255]) * 700 + b"\x01\x02\x03"
    block = rand(32768)
    cases["twice32768"] = block + block
    block = rand(32769)
    cases["twice32769"] = block + block
    stride = 1 + 4 * 301   # a row of 301 pixels: the row above the first rows of chunk 1 lies in chunk 0
    row, rows = bytearray(bytes([0]) + rand(stride - 1)), []
    for _ in range(2 * ch // stride + 3):   # each row repeats the one above but for three bytes
        for k in rng.integers(1, stride, 3):
            row[int(k)] = int(rng.integers(0, 256))
        rows.append(bytes(row))
    cases["rows"] = b"".join(rows)
    return cases


# ------------------------------------------------------------------------------------------------------------------------------
# the host harness
# ------------------------------------------------------------------------------------------------------------------------------
class Codes(C.Structure):   # DeflateCodes of csrc/svgr_deflate.h
    _fields_ = [("lcode", C.c_uint16 * 288), ("dcode", C.c_uint16 * 32), ("llen", C.c_uint8 * 288), ("dlen", C.c_uint8 * 32),
                ("hdr_bits", C.c_uint32), ("pad", C.c_uint32), ("hdr", C.c_uint8 * 320)]


def harness():
    lib = host_build("png_enc_harness")
    lib.h_deflate.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_void_p, C.c_int64,
                              C.POINTER(C.c_int64), C.c_void_p]
    lib.h_png_filter.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p]
    lib.h_row_sums.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p]
    lib.h_lengths.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.h_build_codes.argtypes = [C.c_void_p, C.c_int, C.POINTER(Codes)]
    lib.h_adler_combine.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int64]
    lib.h_len_sym.argtypes = lib.h_dist_sym.argtypes = [C.c_int, C.c_void_p]
    for f in (lib.h_png_filter, lib.h_row_sums, lib.h_lengths, lib.h_build_codes, lib.h_adler_combine, lib.h_len_sym, lib.h_dist_sym):
        f.restype = None
    assert lib.h_codes_size() == C.sizeof(Codes)
    return lib


def harness_filter(lib, img, filter):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    rows, cols, _ = img.shape
    out = np.empty((rows, 1 + 4 * cols), dtype=np.uint8)
    lib.h_png_filter(img.ctypes.data, rows, cols, FILTERS.index(filter), out.ctypes.data)
    return out


def harness_deflate(lib, data, huffman, out_cap=None):
    """(stream, tokens, counts) of the harness for `data`; with `out_cap`, (status, needed) of that one call."""
    src = np.frombuffer(bytes(data) + b"\0", dtype=np.uint8)   # (never empty: its address is taken)
    n = len(data)
    n_out, n_tok = C.c_int64(), C.c_int64()
    if out_cap is not None:
        out = np.zeros(max(out_cap, 1), dtype=np.uint8)
        return lib.h_deflate(src.ctypes.data, n, huffman, out.ctypes.data, out_cap, C.byref(n_out), None, 0, C.byref(n_tok), None), n_out.value
    out = np.zeros(2 * n + 1024, dtype=np.uint8)
    tok = np.zeros(n + 1, dtype=np.uint32)
    counts = np.zeros(316, dtype=np.uint64)
    rc = lib.h_deflate(src.ctypes.data, n, huffman, out.ctypes.data, out.size, C.byref(n_out), tok.ctypes.data, tok.size, C.byref(n_tok),
                       counts.ctypes.data)
    assert rc == 0
    return out[:n_out.value].tobytes(), tok[:n_tok.value].tolist(), counts


def harness_idat(lib, img, filter, huffman):
    """png._idat_stage on the host build: what the CPU tests put in its place."""
    return harness_deflate(lib, harness_filter(lib, img, FILTERS[filter]).tobytes(), huffman)[0]
