"""JPEG reader for SVG <image> (beyond the reference): bytes in, an (h, w, 4) uint8 array out, alpha 255, sRGB as stored.

The split is the PNG reader's.  The markers are read here: SOI / EOI / COM / APPn (the Adobe APP14 `transform` byte is kept,
everything else in them -- JFIF density, EXIF orientation, ICC profiles -- is ignored), DQT with 8- and 16-bit entries, DHT,
DRI, the frame headers SOF0 / SOF1 / SOF2 at 8 bits per sample and every SOS.  The entropy-coded data of each scan is a serial
walk over bits and runs in native host code (``svgr_jpeg_entropy``, csrc/svgr_jpeg.cpp): baseline, extended sequential and
progressive, interleaved or not, with restart intervals.  What it leaves -- int16 DCT coefficients -- goes to the device,
where ``svgr_jpeg_decode`` dequantises, runs the inverse DCT, upsamples the chroma with the centred triangle filter and
converts YCbCr to RGB, all in integer arithmetic, and the pixels are downloaded.

One component (grey) or three are read; three are YCbCr unless an Adobe marker says ``transform == 0`` or the component
ids spell ``RGB``.  Sampling factors are 1 or 2 per axis (4:4:4, 4:2:2, 4:4:0, 4:2:0).  Everything else -- 12-bit samples,
lossless, hierarchical and arithmetic-coded frames, four components -- and malformed input raise ValueError with the
reason.

The writer (``write_jpeg``, further down) is the same split the other way round: ``svgr_jpeg_encode`` makes the quantised
coefficients on the device, ``svgr_jpeg_entropy_encode`` codes them on the host, the markers are written here."""
from __future__ import annotations

import os
import re
import struct

import numpy as np

from . import _abi
from .png import _MAX_PIXELS

SIGNATURE = b"\xff\xd8\xff"
_ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                    28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54,
                    47, 55, 62, 63])
# the end of an entropy-coded segment: FF followed by anything but a stuffed zero, a restart marker or one more FF
_SEGMENT_END = re.compile(rb"\xff[^\x00\xd0-\xd7\xff]")
_UNSUPPORTED_FRAMES = {
    0xC3: "lossless (SOF3)", 0xC5: "hierarchical (SOF5)", 0xC6: "hierarchical (SOF6)", 0xC7: "hierarchical lossless (SOF7)",
    0xC9: "arithmetic-coded (SOF9)", 0xCA: "arithmetic-coded (SOF10)", 0xCB: "arithmetic-coded lossless (SOF11)",
    0xCD: "arithmetic-coded hierarchical (SOF13)", 0xCE: "arithmetic-coded hierarchical (SOF14)",
    0xCF: "arithmetic-coded hierarchical lossless (SOF15)", 0xCC: "arithmetic-coded (DAC)", 0xDE: "hierarchical (DHP)",
}


def markers(data: bytes):
    """(offset of the marker's FF, marker code, body) for every marker of `data` in order, SOI first and EOI last; the body of
    SOS is its header alone (the entropy-coded segment behind it is skipped).  ValueError on a damaged structure."""
    if data[:3] != SIGNATURE:
        raise ValueError("not a JPEG image: bad signature")
    yield 0, 0xD8, b""
    pos, n = 2, len(data)
    while True:
        if pos + 2 > n:
            raise ValueError("truncated JPEG: no EOI marker")
        if data[pos] != 0xFF:
            raise ValueError(f"bad JPEG: byte {data[pos]:#04x} at offset {pos} where a marker should be")
        start = pos
        while pos < n and data[pos] == 0xFF:   # (fill bytes)
            pos += 1
        if pos >= n:
            raise ValueError("truncated JPEG: no EOI marker")
        code = data[pos]
        pos += 1
        if code == 0xD9:
            yield start, code, b""
            return
        if code == 0x00 or code == 0x01 or 0xD0 <= code <= 0xD8:   # (stand-alone codes have no business between segments)
            raise ValueError(f"bad JPEG: stray marker FF{code:02X} at offset {start}")
        if pos + 2 > n:
            raise ValueError(f"truncated JPEG: the FF{code:02X} segment has no length")
        (length,) = struct.unpack(">H", data[pos:pos + 2])
        if length < 2 or pos + length > n:
            raise ValueError(f"truncated JPEG: the FF{code:02X} segment runs past the end of the data")
        yield start, code, data[pos + 2:pos + length]
        pos += length
        if code == 0xDA:
            m = _SEGMENT_END.search(data, pos)
            if m is None:
                raise ValueError("truncated JPEG: a scan runs to the end of the data")
            pos = m.start()


def coefficient_layout(frame: _abi.JpegFrame):
    """[(first block, rows of blocks, blocks per row)] per component and the total number of blocks: the layout of
    include/svgr.h (component after component, each padded to whole MCUs)."""
    hmax, vmax = max(frame.h[:frame.n_comp]), max(frame.v[:frame.n_comp])
    mcus_x, mcus_y = -(-frame.width // (8 * hmax)), -(-frame.height // (8 * vmax))
    out, total = [], 0
    for i in range(frame.n_comp):
        bh, bw = mcus_y * frame.v[i], mcus_x * frame.h[i]
        out.append((total, bh, bw))
        total += bh * bw
    return out, total


def decode_coefficients(data: bytes):
    """The container and the entropy-coded data of a JPEG image: (frame, coef, quant) as svgr_jpeg_decode takes them -- the
    frame's description, its int16 coefficients (coefficient_layout) and each component's quantisation table in natural order,
    (n_comp, 64) uint16.  Host work only.  ValueError on input that is malformed or not supported."""
    data = bytes(data)
    qtables: dict = {}
    huff_counts, huff_symbols = np.zeros((8, 16), dtype=np.uint8), np.zeros((8, 256), dtype=np.uint8)
    restart_interval = 0
    adobe_transform = None
    frame = coef = None
    progressive = False
    ids: list = []
    tq: list = []
    quant: list = []
    scanned: set = set()
    seen_eoi = False
    view = memoryview(data)

    for offset, code, body in markers(data):
        if code in (0xD8, 0xFE) or (0xE0 <= code <= 0xEF and code != 0xEE):
            continue
        if code == 0xD9:
            seen_eoi = True
        elif code == 0xEE:
            if body[:5] == b"Adobe" and len(body) >= 12:
                adobe_transform = body[11]
        elif code == 0xDB:
            at = 0
            while at < len(body):
                pq, t = body[at] >> 4, body[at] & 15
                size = 64 * (pq + 1)
                if pq > 1 or t > 3 or at + 1 + size > len(body):
                    raise ValueError("bad JPEG: a damaged DQT segment")
                entries = np.frombuffer(body, dtype=">u2" if pq else np.uint8, count=64, offset=at + 1)
                table = np.zeros(64, dtype=np.uint16)
                table[_ZIGZAG] = entries
                qtables[t] = table
                at += 1 + size
        elif code == 0xC4:
            at = 0
            while at < len(body):
                tc, t = body[at] >> 4, body[at] & 15
                counts = np.frombuffer(body[at + 1:at + 17], dtype=np.uint8)
                total = int(counts.sum()) if len(counts) == 16 else -1
                if tc > 1 or t > 3 or not 0 < total <= 256 or at + 17 + total > len(body):
                    raise ValueError("bad JPEG: a damaged DHT segment")
                huff_counts[4 * tc + t] = counts
                huff_symbols[4 * tc + t] = 0
                huff_symbols[4 * tc + t, :total] = np.frombuffer(body[at + 17:at + 17 + total], dtype=np.uint8)
                at += 17 + total
        elif code == 0xDD:
            if len(body) != 2:
                raise ValueError("bad JPEG: a damaged DRI segment")
            (restart_interval,) = struct.unpack(">H", body)
        elif code in (0xC0, 0xC1, 0xC2):
            if frame is not None:
                raise ValueError("unsupported JPEG: more than one frame")
            if len(body) < 6 or len(body) != 6 + 3 * body[5]:
                raise ValueError("bad JPEG: a damaged frame header")
            precision, height, width, n_comp = struct.unpack(">BHHB", body[:6])
            if precision != 8:
                raise ValueError(f"unsupported JPEG: {precision}-bit precision (only 8-bit samples are read)")
            if n_comp not in (1, 3):
                what = " (CMYK / YCCK)" if n_comp == 4 else ""
                raise ValueError(f"unsupported JPEG: {n_comp} components{what}; one (grey) or three are read")
            if width == 0 or height == 0 or width * height > _MAX_PIXELS:
                raise ValueError(f"bad JPEG frame header: image size {width} x {height}")
            frame = _abi.JpegFrame()
            frame.width, frame.height, frame.n_comp = width, height, n_comp
            for i in range(n_comp):
                cid, hv, t = body[6 + 3 * i:9 + 3 * i]
                h, v = hv >> 4, hv & 15
                if not (1 <= h <= 2 and 1 <= v <= 2):
                    raise ValueError(f"unsupported JPEG: sampling factors {h} x {v} (1 and 2 are read)")
                if t > 3 or cid in ids:
                    raise ValueError("bad JPEG: a damaged frame header")
                ids.append(cid)
                tq.append(t)
                quant.append(None)
                frame.h[i], frame.v[i] = (1, 1) if n_comp == 1 else (h, v)   # (a lone component is stored unsampled)
            progressive = code == 0xC2
            coef = np.zeros(coefficient_layout(frame)[1] * 64, dtype=np.int16)
        elif code == 0xDA:
            if frame is None:
                raise ValueError("bad JPEG: a scan before the frame header")
            if len(body) < 1 or not 1 <= body[0] <= frame.n_comp or len(body) != 4 + 2 * body[0]:
                raise ValueError("bad JPEG: a damaged scan header")
            scan = _abi.JpegScan()
            scan.frame = frame
            scan.progressive, scan.restart_interval, scan.n_scan = int(progressive), restart_interval, body[0]
            ss, se, ahal = body[1 + 2 * body[0]:]
            scan.ss, scan.se, scan.ah, scan.al = ss, se, ahal >> 4, ahal & 15
            need_dc = not progressive or (ss == 0 and scan.ah == 0)
            need_ac = not progressive or ss > 0
            for j in range(body[0]):
                cid, tables = body[1 + 2 * j], body[2 + 2 * j]
                if cid not in ids or (j and ids.index(cid) <= scan.scan_comp[j - 1]):
                    raise ValueError("bad JPEG: a scan of components the frame does not have, or out of order")
                ci = ids.index(cid)
                td, ta = tables >> 4, tables & 15
                if td > 3 or ta > 3:
                    raise ValueError("bad JPEG: a damaged scan header")
                if (need_dc and not huff_counts[td].any()) or (need_ac and not huff_counts[4 + ta].any()):
                    raise ValueError("bad JPEG: missing Huffman table")
                scan.scan_comp[j], scan.dc_table[j], scan.ac_table[j] = ci, td, ta
                if quant[ci] is None:   # (the table in force when the component is first seen)
                    if tq[ci] not in qtables:
                        raise ValueError("bad JPEG: missing quantisation table")
                    quant[ci] = qtables[tq[ci]]
                scanned.add(ci)
            first = offset + 4 + len(body)   # (FF DA, the length, the header)
            m = _SEGMENT_END.search(data, first)
            if m is None:
                raise ValueError("truncated JPEG: a scan runs to the end of the data")
            try:
                _abi.jpeg_entropy(scan, huff_counts, huff_symbols, view[first:m.start()], coef)
            except ValueError as e:
                raise ValueError(f"corrupt JPEG scan at offset {offset}: {e}") from None
        elif code in _UNSUPPORTED_FRAMES:
            raise ValueError(f"unsupported JPEG: {_UNSUPPORTED_FRAMES[code]} coding (baseline, extended and progressive Huffman are read)")
        elif code == 0xDC:
            raise ValueError("unsupported JPEG: the number of lines comes in a DNL segment")
        else:
            raise ValueError(f"bad JPEG: unknown marker FF{code:02X} at offset {offset}")
    if not seen_eoi:
        raise ValueError("truncated JPEG: no EOI marker")
    if frame is None:
        raise ValueError("bad JPEG: no frame header")
    if len(scanned) != frame.n_comp:
        raise ValueError("truncated JPEG: no scan for some component")
    if frame.n_comp == 1:
        frame.colour = _abi.JPEG_GREY
    elif adobe_transform == 0 or (adobe_transform is None and bytes(ids) == b"RGB"):
        frame.colour = _abi.JPEG_RGB
    else:
        frame.colour = _abi.JPEG_YCBCR
    return frame, coef, np.stack(quant)


def _pixel_stage(frame, coef, quant) -> np.ndarray:
    """Coefficients -> (h, w, 4) uint8 on the device (svgr_jpeg_decode), downloaded."""
    return _abi.jpeg_decode(_abi.Context.get(), frame, coef, quant)


def read_jpeg(data: bytes) -> np.ndarray:
    """Decode a JPEG image: ``(height, width, 4) uint8`` RGBA with alpha 255, the stored sRGB values (EXIF orientation and
    ICC profiles are ignored).  Baseline, extended sequential and progressive Huffman coding at 8 bits per sample; grey or
    three components (YCbCr by the JFIF matrix, or RGB); chroma subsampled by up to 2 per axis is brought back with the
    centred triangle filter.  The pixel arithmetic is integer and runs on the device: the result is defined to the bit.
    ValueError on malformed or unsupported input."""
    frame, coef, quant = decode_coefficients(data)
    return _pixel_stage(frame, coef, quant)


# ------------------------------------------------------------------------------------------------------------------------------
# JPEG writer (beyond the reference): the reader's split the other way round.  The device turns the pixels into quantised
# DCT coefficients (svgr_jpeg_encode: colour transform, chroma downsampling, forward DCT and quantiser in integer arithmetic),
# native host code walks them into the entropy-coded segment (svgr_jpeg_entropy_encode), and the markers are written here.
# ------------------------------------------------------------------------------------------------------------------------------
# ITU-T T.81 tables K.1 and K.2 in natural (row-major) order
_QUANT_LUMA = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
_QUANT_CHROMA = np.array([
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
    + [99] * 32)
# T.81 tables K.3 - K.6: (codes per length 1 .. 16, the symbols in code order)
_STD_HUFFMAN = {
    (0, 0): ("00010501010101010100000000000000", "000102030405060708090a0b"),
    (0, 1): ("00030101010101010101010000000000", "000102030405060708090a0b"),
    (1, 0): ("0002010303020403050504040000017d",
             "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a"
             "434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aa"
             "b2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"),
    (1, 1): ("00020102040403040705040400010277",
             "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a"
             "434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aa"
             "b2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa"),
}
SUBSAMPLINGS = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:4:0": (1, 2), "4:2:0": (2, 2)}   # the luma sampling factors (h, v)


def quant_tables(quality: int) -> np.ndarray:
    """(2, 64) uint16, natural order: the standard's luminance and chrominance tables (Annex K) scaled the usual way --
    ``scale = 5000 / quality`` below 50, else ``200 - 2 quality``; ``entry = clamp((base * scale + 50) // 100, 1, 255)``.
    Quality 100 gives all ones."""
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or not 1 <= quality <= 100:
        raise ValueError(f"JPEG quality is an integer from 1 to 100, not {quality!r}")
    scale = 5000 // int(quality) if quality < 50 else 200 - 2 * int(quality)
    return np.clip((np.stack([_QUANT_LUMA, _QUANT_CHROMA]) * scale + 50) // 100, 1, 255).astype(np.uint16)


def standard_huffman():
    """(huff_counts (8, 16), huff_symbols (8, 256)) uint8 as svgr_jpeg_entropy takes them: Annex K.3's tables, luminance in
    DC / AC table 0 and chrominance in table 1."""
    counts, symbols = np.zeros((8, 16), dtype=np.uint8), np.zeros((8, 256), dtype=np.uint8)
    for (tc, t), (bits, vals) in _STD_HUFFMAN.items():
        counts[4 * tc + t] = np.frombuffer(bytes.fromhex(bits), dtype=np.uint8)
        v = np.frombuffer(bytes.fromhex(vals), dtype=np.uint8)
        symbols[4 * tc + t, :v.size] = v
    return counts, symbols


def optimal_huffman(freq):
    """A Huffman table made for the symbol counts `freq` (256 of them) by the procedure of T.81 Annex K.2: (codes per
    length 1 .. 16, the symbols in code order).  A reserved 257th symbol of count 1 takes the longest code, so no code is all
    ones; code lengths beyond 16 are shortened by the standard's rebalancing (figure K.3)."""
    freq = [int(x) for x in freq] + [1]
    if len(freq) != 257 or min(freq) < 0 or not any(freq[:256]):
        raise ValueError("optimal_huffman: 256 counts, not all zero")
    codesize, others = [0] * 257, [-1] * 257
    while True:
        live = [(f, -i) for i, f in enumerate(freq) if f > 0]   # (ties: the larger symbol first, as the standard's search)
        if len(live) < 2:
            break
        (_f1, n1), (_f2, n2) = sorted(live)[:2]
        v1, v2 = -n1, -n2
        freq[v1] += freq[v2]
        freq[v2] = 0
        for v, tail in ((v1, v2), (v2, None)):
            while True:
                codesize[v] += 1
                if others[v] < 0:
                    break
                v = others[v]
            if tail is not None:
                others[v] = tail
    bits = [0] * (max(codesize) + 2)
    for size in codesize:
        if size:
            bits[size] += 1
    i = len(bits) - 1
    while i > 16:   # (figure K.3: a pair of the longest codes becomes one shorter code and lends its prefix's sibling)
        if bits[i] == 0:
            i -= 1
            continue
        j = i - 2
        while bits[j] == 0:
            j -= 1
        bits[i] -= 2
        bits[i - 1] += 1
        bits[j + 1] += 2
        bits[j] -= 1
    bits = (bits + [0] * 17)[:17]
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1   # (the reserved symbol)
    order = sorted((s for s in range(256) if codesize[s]), key=lambda s: (codesize[s], s))
    return np.array(bits[1:], dtype=np.uint8), np.array(order, dtype=np.uint8)


def _segment(code: int, body: bytes) -> bytes:
    return struct.pack(">BBH", 0xFF, code, len(body) + 2) + body


def encode_frame(frame: _abi.JpegFrame, coef: np.ndarray, quant: np.ndarray, optimize: bool = True, restart_interval: int = 0) -> bytes:
    """A baseline JFIF file from a frame's coefficients (coefficient_layout) and its components' quantisation tables
    (n_comp, 64), entries 1 .. 255: SOI, APP0, DQT, SOF0, DHT, [DRI], SOS, the entropy-coded data, EOI.  One scan,
    interleaved when there are three components; component 0 uses quantisation and Huffman tables 0, the others tables 1.
    Host work only -- decode_coefficients' inverse."""
    coef = np.ascontiguousarray(coef, dtype=np.int16)
    quant = np.ascontiguousarray(quant, dtype=np.uint16)
    n = frame.n_comp
    if n not in (1, 3) or quant.shape != (n, 64) or quant.min() < 1 or quant.max() > 255:
        raise ValueError("encode_frame: one quantisation table of 64 entries from 1 to 255 per component")
    if n == 3 and not np.array_equal(quant[1], quant[2]):
        raise ValueError("encode_frame: the two chroma components share one quantisation table")
    if coef.size != 64 * coefficient_layout(frame)[1]:
        raise ValueError("encode_frame: the coefficients are not the frame's")
    if isinstance(restart_interval, bool) or not isinstance(restart_interval, (int, np.integer)) or not 0 <= restart_interval <= 65535:
        raise ValueError(f"JPEG restart interval is an integer from 0 to 65535 MCUs, not {restart_interval!r}")
    scan = _abi.JpegScan()
    scan.frame = frame
    scan.progressive, scan.restart_interval, scan.n_scan = 0, int(restart_interval), n
    scan.ss, scan.se, scan.ah, scan.al = 0, 63, 0, 0
    for i in range(n):
        scan.scan_comp[i], scan.dc_table[i], scan.ac_table[i] = i, min(i, 1), min(i, 1)
    tables = [(0, 0), (1, 0)] + ([(0, 1), (1, 1)] if n == 3 else [])
    counts, symbols = standard_huffman()
    if optimize:
        freq = _abi.jpeg_symbol_counts(scan, coef)
        for tc, t in tables:
            bits, vals = optimal_huffman(freq[4 * tc + t])
            counts[4 * tc + t] = bits
            symbols[4 * tc + t] = 0
            symbols[4 * tc + t, :vals.size] = vals
    data = _abi.jpeg_entropy_encode(scan, counts, symbols, coef)

    out = [b"\xff\xd8", _segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")]
    out.append(_segment(0xDB, b"".join(bytes([t]) + quant[t][_ZIGZAG].astype(np.uint8).tobytes() for t in range(min(n, 2)))))
    sof = struct.pack(">BHHB", 8, frame.height, frame.width, n)
    for i in range(n):
        sof += bytes([i + 1, frame.h[i] << 4 | frame.v[i], min(i, 1)])
    out.append(_segment(0xC0, sof))
    out.append(_segment(0xC4, b"".join(
        bytes([tc << 4 | t]) + counts[4 * tc + t].tobytes() + symbols[4 * tc + t, :int(counts[4 * tc + t].sum())].tobytes()
        for tc, t in tables)))
    if restart_interval:
        out.append(_segment(0xDD, struct.pack(">H", int(restart_interval))))
    out.append(_segment(0xDA, bytes([n]) + b"".join(bytes([i + 1, min(i, 1) << 4 | min(i, 1)]) for i in range(n)) + b"\x00\x3f\x00"))
    out += [data, b"\xff\xd9"]
    return b"".join(out)


def _coefficient_stage(frame, rgba8, quant) -> np.ndarray:
    """Pixels (a device buffer or a host array) -> the frame's coefficients on the device (svgr_jpeg_encode), downloaded."""
    return _abi.jpeg_encode(_abi.Context.get(), frame, rgba8, quant)


def _encode_rgba8(rgba8, height: int, width: int, output, quality, subsampling, grey, optimize, restart_interval) -> bytes:
    quant = quant_tables(quality)
    if subsampling not in SUBSAMPLINGS:
        raise ValueError(f"JPEG subsampling is one of {', '.join(SUBSAMPLINGS)}, not {subsampling!r}")
    if not (1 <= height <= 65535 and 1 <= width <= 65535) or width * height > _MAX_PIXELS:
        raise ValueError(f"a JPEG image has 1 to 65535 pixels per side, not {width} x {height}")
    frame = _abi.JpegFrame()
    frame.width, frame.height = width, height
    if grey:
        frame.n_comp, frame.colour = 1, _abi.JPEG_GREY
        frame.h[0] = frame.v[0] = 1
        quant = quant[:1]
    else:
        frame.n_comp, frame.colour = 3, _abi.JPEG_YCBCR
        frame.h[0], frame.v[0] = SUBSAMPLINGS[subsampling]
        frame.h[1] = frame.v[1] = frame.h[2] = frame.v[2] = 1
        quant = quant[[0, 1, 1]]
    if isinstance(restart_interval, bool) or not isinstance(restart_interval, (int, np.integer)) or not 0 <= restart_interval <= 65535:
        raise ValueError(f"JPEG restart interval is an integer from 0 to 65535 MCUs, not {restart_interval!r}")
    data = encode_frame(frame, _coefficient_stage(frame, rgba8, quant), quant, bool(optimize), restart_interval)
    if isinstance(output, (str, os.PathLike)):
        with open(output, "wb") as f:
            f.write(data)
    elif output is not None:
        output.write(data)
    return data


def write_jpeg(image, output=None, quality: int = 90, subsampling: str = "4:2:0", grey: bool = False, optimize: bool = True,
               restart_interval: int = 0) -> bytes:
    """Encode a baseline JFIF JPEG and return its bytes (also written to ``output``: a path or a binary file object).
    ``image`` is an ``(height, width, 4) uint8`` array -- straight-alpha sRGB as ``Layer.to_rgba8`` returns it; alpha is
    ignored, JPEG has none -- or a ``Layer``, which goes over opaque white first (``Layer.write_jpeg`` takes the colour).
    ``quality`` 1 .. 100 scales the standard's quantisation tables (100: all ones); ``subsampling`` is "4:4:4", "4:2:2",
    "4:4:0" or "4:2:0"; ``grey`` writes the luma alone; ``optimize`` builds the Huffman tables for the image instead of
    using the standard's; ``restart_interval`` > 0 puts a restart marker after every so many MCUs.  The pixel arithmetic is
    integer and runs on the device: the file is defined to the bit.  ValueError on bad arguments."""
    from .layer import Layer  # noqa: PLC0415

    if isinstance(image, Layer):
        return image.write_jpeg(output, quality=quality, subsampling=subsampling, grey=grey, optimize=optimize,
                                restart_interval=restart_interval)
    px = np.asarray(image)
    if px.dtype != np.uint8 or px.ndim != 3 or px.shape[2] != 4 or px.shape[0] < 1 or px.shape[1] < 1:
        raise ValueError("write_jpeg takes an (height, width, 4) uint8 array or a Layer")
    return _encode_rgba8(np.ascontiguousarray(px), px.shape[0], px.shape[1], output, quality, subsampling, grey, optimize, restart_interval)
