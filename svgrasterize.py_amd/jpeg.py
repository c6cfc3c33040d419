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
reason."""
from __future__ import annotations

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
