"""PNG reader for SVG <image> and the device PNG encoder (both beyond the reference).

Reader: bytes in, an (h, w, 4) uint8 array out, straight alpha, sRGB as stored.

Chunks are read here (signature, CRC of every chunk, IHDR / PLTE / tRNS / IDAT; ancillary chunks are skipped) and the
image data is inflated with the standard library's zlib.  Reversing the scanline filters is a sequential walk over the
bytes and runs in native host code (``svgr_png_unfilter``, csrc/svgr_png.cpp); unpacking samples below 8 bits, the palette
lookup, 16 -> 8 bit reduction and the Adam7 scatter are numpy.  Every colour type and bit depth of the specification is
read.  Malformed input raises ValueError with the reason.

Encoder (``encoder="device"`` of ``canvas_to_png``, ``Layer.write_png`` and ``render_svg``): the scanline filters and the
deflate stream are made on the device (``svgr_png_filter``, ``svgr_deflate``; csrc/svgr_png.h and csrc/svgr_deflate.h have the
definitions) from the RGBA8 bytes that are already there; only the compressed bytes come back, and the container -- signature,
IHDR, one IDAT, IEND, the CRCs -- is written here.

Indexed output (``palette=`` of the same three): the colour quantiser (quant.py, ``svgr_quant_*``) leaves a palette and the packed
index scanlines on the device, dithered if ``dither=`` says so; either encoder compresses them, and the container gains PLTE and
tRNS.

Sample formats (``color=`` and ``depth=`` of the same three): grey, grey + alpha, RGB and RGBA at 8 or 16 bits.  The samples are
made on the device from the float pixels (``svgr_png_samples``); the device encoder filters rows of any pixel size
(``svgr_png_filter_bytes``), the host encoder writes filter 0 rows.  ``read_samples`` gives a file's samples back as stored."""
from __future__ import annotations

import struct
import zlib

import numpy as np

from . import _abi

SIGNATURE = b"\x89PNG\r\n\x1a\n"
_DEPTHS = {0: (1, 2, 4, 8, 16), 2: (8, 16), 3: (1, 2, 4, 8), 4: (8, 16), 6: (8, 16)}   # colour type -> bit depths
_CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
# Adam7 passes: (first row, first column, row step, column step)
_ADAM7 = ((0, 0, 8, 8), (0, 4, 8, 8), (4, 0, 8, 4), (0, 2, 4, 4), (2, 0, 4, 2), (0, 1, 2, 2), (1, 0, 2, 1))
_MAX_PIXELS = 1 << 30


def _chunks(data: bytes):
    if data[:8] != SIGNATURE:
        raise ValueError("not a PNG image: bad signature")
    pos, n = 8, len(data)
    while True:
        if pos + 8 > n:
            raise ValueError("truncated PNG: no IEND chunk")
        length, ctype = struct.unpack(">I4s", data[pos:pos + 8])
        if length > 0x7FFFFFFF:
            raise ValueError(f"bad PNG chunk length {length}")
        end = pos + 12 + length
        if end > n:
            raise ValueError(f"truncated PNG: the {ctype!r} chunk runs past the end of the data")
        body = data[pos + 8:pos + 8 + length]
        (crc,) = struct.unpack(">I", data[pos + 8 + length:end])
        if zlib.crc32(body, zlib.crc32(ctype)) & 0xFFFFFFFF != crc:
            raise ValueError(f"bad CRC in the {ctype!r} chunk")
        yield ctype, body
        if ctype == b"IEND":
            return
        pos = end


def _samples(rows: np.ndarray, width: int, channels: int, depth: int) -> np.ndarray:
    """Unfiltered scanlines (h, row_bytes) -> samples (h, width, channels): uint8, or uint16 at depth 16."""
    h = rows.shape[0]
    if depth == 8:
        return rows[:, :width * channels].reshape(h, width, channels)
    if depth == 16:
        return rows[:, :width * channels * 2].copy().view(">u2").astype(np.uint16).reshape(h, width, channels)
    per_byte = 8 // depth   # (depths below 8 occur with one channel only)
    shifts = np.arange(8 - depth, -1, -depth, dtype=np.uint8)
    vals = (rows[:, :, None] >> shifts) & np.uint8((1 << depth) - 1)
    return vals.reshape(h, rows.shape[1] * per_byte)[:, :width, None]


def _to8(samples: np.ndarray, depth: int) -> np.ndarray:
    if depth == 16:
        return ((samples.astype(np.uint32) * 255 + 32767) // 65535).astype(np.uint8)
    if depth < 8:
        return (samples * np.uint8(255 // ((1 << depth) - 1))).astype(np.uint8)
    return samples.astype(np.uint8)


def _decode(data: bytes):
    """(samples (h, w, channels) uint8 or uint16 as stored, colour type, depth, PLTE entries or None, tRNS body or None): the one
    decoder under ``read_png`` and ``read_samples``."""
    data = bytes(data)
    ihdr = plte = trns = None
    idat = []
    for ctype, body in _chunks(data):
        if ctype == b"IHDR":
            if ihdr is not None or len(body) != 13:
                raise ValueError("bad IHDR chunk")
            ihdr = struct.unpack(">IIBBBBB", body)
        elif ihdr is None:
            raise ValueError("the first PNG chunk is not IHDR")
        elif ctype == b"PLTE":
            if len(body) % 3 or not 3 <= len(body) <= 768:
                raise ValueError("bad PLTE chunk length")
            plte = np.frombuffer(body, dtype=np.uint8).reshape(-1, 3)
        elif ctype == b"tRNS":
            trns = body
        elif ctype == b"IDAT":
            idat.append(body)
        elif ctype == b"IEND":
            break
        elif not ctype[0] & 0x20:   # (an unknown critical chunk: the image cannot be read correctly without it)
            raise ValueError(f"unsupported critical PNG chunk {ctype!r}")
    if ihdr is None:
        raise ValueError("no IHDR chunk")
    width, height, depth, ctype_, compression, filtering, interlace = ihdr
    if ctype_ not in _DEPTHS or depth not in _DEPTHS[ctype_]:
        raise ValueError(f"bad IHDR: bit depth {depth} with colour type {ctype_}")
    if width == 0 or height == 0 or width > 0x7FFFFFFF or height > 0x7FFFFFFF or width * height > _MAX_PIXELS:
        raise ValueError(f"bad IHDR: image size {width} x {height}")
    if compression != 0 or filtering != 0 or interlace not in (0, 1):
        raise ValueError(f"bad IHDR: compression {compression}, filter method {filtering}, interlace {interlace}")
    if ctype_ == 3 and plte is None:
        raise ValueError("a palette image without a PLTE chunk")
    if not idat:
        raise ValueError("no IDAT chunk")
    channels = _CHANNELS[ctype_]
    bits = channels * depth
    passes = _ADAM7 if interlace else ((0, 0, 1, 1),)
    sizes = []
    for r0, c0, rs, cs in passes:
        ph, pw = (height - r0 + rs - 1) // rs, (width - c0 + cs - 1) // cs
        sizes.append((ph, pw, (pw * bits + 7) // 8))
    need = sum(ph * (rb + 1) for ph, pw, rb in sizes if ph and pw)
    inflater = zlib.decompressobj()
    try:
        raw = inflater.decompress(b"".join(idat), need + 1)
    except zlib.error as e:
        raise ValueError(f"bad PNG image data: {e}") from None
    if len(raw) < need:
        raise ValueError("truncated PNG image data")

    samples = np.empty((height, width, channels), dtype=np.uint16 if depth == 16 else np.uint8)
    pos = 0
    for (r0, c0, rs, cs), (ph, pw, rb) in zip(passes, sizes):
        if ph == 0 or pw == 0:
            continue
        rows = _abi.png_unfilter(raw[pos:pos + ph * (rb + 1)], ph, rb, max(1, bits // 8))
        pos += ph * (rb + 1)
        samples[r0::rs, c0::cs] = _samples(rows, pw, channels, depth)
    return samples, ctype_, depth, plte, trns


def read_samples(data: bytes):
    """``(samples, colour_type, depth)`` of a PNG image: the samples as the file stores them, without ``read_png``'s reduction to
    8-bit RGBA -- ``(height, width, channels)``, uint16 at depth 16 and uint8 otherwise (depths below 8 unpacked, not scaled); for
    a palette image the indices.  PLTE, tRNS and every ancillary chunk are left aside.  ValueError on malformed input."""
    samples, colour_type, depth, _plte, _trns = _decode(data)
    return samples, colour_type, depth


def read_png(data: bytes) -> np.ndarray:
    """Decode a PNG image: ``(height, width, 4) uint8`` RGBA, straight alpha, the stored sRGB values (gAMA, iCCP, sRGB,
    cHRM and text chunks are ignored).  16-bit samples become ``(v * 255 + 32767) // 65535``; gray below 8 bits is scaled
    to 0-255; a tRNS colour key makes its pixels transparent.  ValueError on malformed input."""
    samples, ctype_, depth, plte, trns = _decode(data)
    height, width, channels = samples.shape
    out = np.empty((height, width, 4), dtype=np.uint8)
    if ctype_ == 3:
        idx = samples[..., 0]
        if int(idx.max()) >= len(plte):
            raise ValueError("a palette index beyond the PLTE chunk")
        table = np.full((256, 4), 255, dtype=np.uint8)
        table[:len(plte), :3] = plte
        if trns is not None:
            alpha = np.frombuffer(trns, dtype=np.uint8)[:len(plte)]
            table[:len(alpha), 3] = alpha
        return table[idx]
    colour = samples[..., :3] if ctype_ in (2, 6) else np.repeat(samples[..., :1], 3, axis=2)
    out[..., :3] = _to8(colour, depth)
    if ctype_ in (4, 6):
        out[..., 3] = _to8(samples[..., -1], depth)
    else:
        out[..., 3] = 255
        if trns is not None:   # colour key: one 16-bit value per channel, compared with the samples as stored
            key = np.frombuffer(trns, dtype=">u2").astype(np.int64)
            if len(key) != channels:
                raise ValueError("bad tRNS chunk length")
            out[np.all(samples.astype(np.int64) == key, axis=2), 3] = 0
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the encoder
# ---------------------------------------------------------------------------------------------------------------------
FILTERS = {"none": 0, "sub": 1, "up": 2, "average": 3, "paeth": 4, "adaptive": 5}   # SVGR_PNG_FILTER_*
HUFFMAN = {"fixed": 0, "dynamic": 1}                                                # SVGR_DEFLATE_*


def _filter_number(filter) -> int:
    if not isinstance(filter, str) or filter not in FILTERS:
        raise ValueError(f"PNG filter is one of {', '.join(FILTERS)}, not {filter!r}")
    return FILTERS[filter]


def _huffman_number(huffman) -> int:
    if not isinstance(huffman, str) or huffman not in HUFFMAN:
        raise ValueError(f"deflate Huffman mode is one of {', '.join(HUFFMAN)}, not {huffman!r}")
    return HUFFMAN[huffman]


def write_container(output, width: int, height: int, idat: bytes, colour_type: int = 6, depth: int = 8):
    """The file around a zlib stream of scanlines, 8-bit RGBA unless said otherwise: signature, IHDR, one IDAT, IEND
    (canvas_to_png, S:249-274)."""
    def pack(tag: bytes, data: bytes) -> None:
        output.write(struct.pack("!I", len(data)))
        output.write(tag)
        output.write(data)
        output.write(struct.pack("!I", 0xFFFFFFFF & zlib.crc32(data, zlib.crc32(tag))))

    output.write(SIGNATURE)
    pack(b"IHDR", struct.pack("!2I5B", width, height, depth, colour_type, 0, 0, 0))
    pack(b"IDAT", idat)
    pack(b"IEND", b"")
    return output


def filter_device(rgba8, filter: str = "adaptive", *, rows: int | None = None, cols: int | None = None) -> "_abi.DeviceBuffer":
    """The filtered scanlines of an 8-bit RGBA image, made on the device and left there: ``rows * (1 + 4 * cols)`` bytes.
    ``rgba8`` is a ``(rows, cols, 4)`` uint8 array, which is uploaded, or a DeviceBuffer that holds such bytes (then ``rows``
    and ``cols`` say its shape)."""
    mode = _filter_number(filter)
    ctx = _abi.Context.get()
    if not isinstance(rgba8, _abi.DeviceBuffer):
        px = np.ascontiguousarray(rgba8, dtype=np.uint8)
        if px.ndim != 3 or px.shape[2] != 4 or px.size == 0:
            raise ValueError("filter_device: the pixels are a non-empty (rows, cols, 4) uint8 array")
        rows, cols = px.shape[0], px.shape[1]
        rgba8 = ctx.from_host(px)
    elif rows is None or cols is None:
        raise ValueError("filter_device: a device buffer needs rows and cols")
    return _abi.png_filter(ctx, rgba8, int(rows), int(cols), mode)


def deflate_device(data, huffman: str = "dynamic", *, n_bytes: int | None = None) -> bytes:
    """A complete zlib stream of ``data`` -- bytes or a uint8 array, which are uploaded, or a DeviceBuffer (its first
    ``n_bytes`` bytes; default all of it) -- compressed on the device.  ``zlib.decompress`` returns the input."""
    mode = _huffman_number(huffman)
    ctx = _abi.Context.get()
    if not isinstance(data, _abi.DeviceBuffer):
        arr = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
        n_bytes = arr.size
        data = ctx.from_host(arr) if arr.size else ctx.alloc(4)
    elif n_bytes is None:
        n_bytes = data.nbytes
    return _abi.deflate(ctx, data, int(n_bytes), mode)


def _idat_stage(rgba8, rows: int, cols: int, filter: int, huffman: int) -> bytes:
    """The IDAT payload of an image on the device: ``rgba8`` is a DeviceBuffer of its bytes or a (rows, cols, 4) uint8 array,
    which is uploaded first.  (The CPU tests put the host build of the same headers here.)"""
    ctx = _abi.Context.get()
    if not isinstance(rgba8, _abi.DeviceBuffer):
        rgba8 = ctx.from_host(np.ascontiguousarray(rgba8, dtype=np.uint8))
    filtered = _abi.png_filter(ctx, rgba8, rows, cols, filter)
    return _abi.deflate(ctx, filtered, rows * (1 + 4 * cols), huffman)


def encode_rgba8(rgba8, rows: int, cols: int, output=None, filter=None, huffman=None):
    """``canvas_to_png(encoder="device")``: the PNG of 8-bit RGBA pixels (an array or a DeviceBuffer) into ``output`` (a binary
    file object; default a new BytesIO), which is returned.  Bad arguments are refused before any device work."""
    import io

    mode = _filter_number("adaptive" if filter is None else filter)
    code = _huffman_number("dynamic" if huffman is None else huffman)
    if rows <= 0 or cols <= 0:
        raise ValueError(f"a PNG image has at least one pixel, not {cols} x {rows}")
    idat = _idat_stage(rgba8, int(rows), int(cols), mode, code)
    return write_container(io.BytesIO() if output is None else output, int(cols), int(rows), idat)


def encoder_arguments(encoder, level, threads, filter, huffman):
    """What ``canvas_to_png`` and its callers accept: ("host", level, threads) or ("device", filter, huffman), checked."""
    if encoder == "host":
        if filter is not None or huffman is not None:
            raise TypeError('filter and huffman belong to encoder="device"')
        return "host", 9 if level is None else level, 1 if threads is None else threads
    if encoder != "device":
        raise ValueError(f'PNG encoder is "host" or "device", not {encoder!r}')
    if level is not None or threads is not None:
        raise TypeError('level and threads belong to encoder="host"')
    _filter_number("adaptive" if filter is None else filter)
    _huffman_number("dynamic" if huffman is None else huffman)
    return "device", filter, huffman


# ---------------------------------------------------------------------------------------------------------------------
# indexed output (colour type 3): the quantiser's row stream in a PLTE / tRNS container
# ---------------------------------------------------------------------------------------------------------------------
def palette_argument(palette, encoder, filter):
    """``palette`` of ``canvas_to_png`` and its callers, checked: None (8-bit RGBA as before) or the largest number of entries.
    Indexed rows carry filter 0 only: with a palette the device encoder's ``filter`` is None or "none"."""
    from . import quant  # noqa: PLC0415

    n = quant.palette_argument(palette)
    if n is not None and encoder == "device" and filter not in (None, "none"):
        raise ValueError(f'indexed PNG rows are written with filter "none"; filter {filter!r} does not go with palette')
    return n


def dither_argument(dither, max_colors):
    """``dither`` of the same callers, checked, next to what ``palette_argument`` made of their ``palette``: None, "ordered" or
    "diffusion"; a dither without a palette is a ValueError."""
    from . import quant  # noqa: PLC0415

    return quant.dither_argument(dither, max_colors is not None)


def write_indexed_container(output, width: int, height: int, palette: np.ndarray, idat: bytes):
    """The file around a zlib stream of index scanlines: signature, IHDR (colour type 3, the depth of the palette's length), PLTE,
    tRNS unless every entry is opaque, one IDAT, IEND."""
    from . import quant  # noqa: PLC0415

    palette = np.ascontiguousarray(palette, dtype=np.uint8).reshape(-1, 4)
    if not 1 <= len(palette) <= 256:
        raise ValueError(f"a PNG palette has 1 to 256 entries, not {len(palette)}")

    def pack(tag: bytes, data: bytes) -> None:
        output.write(struct.pack("!I", len(data)))
        output.write(tag)
        output.write(data)
        output.write(struct.pack("!I", 0xFFFFFFFF & zlib.crc32(data, zlib.crc32(tag))))

    output.write(SIGNATURE)
    pack(b"IHDR", struct.pack("!2I5B", width, height, quant.depth_of(len(palette)), 3, 0, 0, 0))
    pack(b"PLTE", palette[:, :3].tobytes())
    alphas = quant.trns(palette)
    if alphas:
        pack(b"tRNS", alphas)
    pack(b"IDAT", idat)
    pack(b"IEND", b"")
    return output


def encode_indexed(rgba8, rows: int, cols: int, output, max_colors: int, *, encoder: str = "host", level=9, threads=1, huffman=None,
                   refine: int = 3, dither=None):
    """``canvas_to_png(palette=...)``: the colour type 3 PNG of 8-bit RGBA pixels (an array or a DeviceBuffer) into ``output``
    (default a new BytesIO), which is returned.  The palette and the packed scanlines are made on the device (quant.py), dithered
    as ``dither`` (checked by ``quant.dither_argument``) says; the "device" encoder deflates them there, the "host" encoder
    downloads them -- a byte or less per pixel -- for zlib."""
    import io

    from . import quant  # noqa: PLC0415

    code = _huffman_number("dynamic" if huffman is None else huffman) if encoder == "device" else None
    if rows <= 0 or cols <= 0:
        raise ValueError(f"a PNG image has at least one pixel, not {cols} x {rows}")
    ctx = _abi.Context.get()
    if not isinstance(rgba8, _abi.DeviceBuffer):
        rgba8 = ctx.from_host(np.ascontiguousarray(rgba8, dtype=np.uint8))
    palette, stream, _ = quant.index_rows(rgba8, int(rows), int(cols), max_colors, refine, dither, stream=True, indices=False)
    n_bytes = int(rows) * (1 + (int(cols) * quant.depth_of(len(palette)) + 7) // 8)
    if encoder == "device":
        idat = _abi.deflate(ctx, stream, n_bytes, code)
    else:
        raw = stream.download((n_bytes,), np.uint8).tobytes()
        if threads > 1:
            from .layer import _deflate_parallel  # noqa: PLC0415

            idat = _deflate_parallel(raw, level, threads)
        else:
            comp = zlib.compressobj(level=level)
            idat = comp.compress(raw) + comp.flush()
    return write_indexed_container(io.BytesIO() if output is None else output, int(cols), int(rows), palette, idat)


# ---------------------------------------------------------------------------------------------------------------------
# sample formats (colour types 0, 2, 4, 6 at depth 8 or 16): color= and depth= of canvas_to_png and its callers.  The samples
# are made on the device (svgr_png_samples; csrc/svgr_png.h has the arithmetic) and either encoder takes their rows.
# ---------------------------------------------------------------------------------------------------------------------
COLORS = {"rgba": 6, "rgb": 2, "grey-alpha": 4, "gray-alpha": 4, "grey": 0, "gray": 0}   # SVGR_PNG_COLOR_*


def format_arguments(color, depth, palette=None):
    """``color`` and ``depth`` of ``canvas_to_png`` and its callers, checked: None when neither is given (8-bit RGBA by the code
    path that has always written it), otherwise ``(colour type, depth or None)``.  An unknown colour word or depth is a ValueError,
    a colour that is no string a TypeError, either of them next to ``palette`` a ValueError."""
    if color is None and depth is None:
        return None
    if color is not None and not isinstance(color, str):
        raise TypeError(f"PNG color is a string or None, not {type(color).__name__}")
    if color is not None and color not in COLORS:
        raise ValueError(f"PNG color is one of {', '.join(COLORS)}, not {color!r}")
    if depth is not None and (isinstance(depth, bool) or not isinstance(depth, (int, np.integer)) or depth not in (8, 16)):
        raise ValueError(f"PNG depth is 8 or 16, not {depth!r}")
    if palette is not None and palette is not False:
        raise ValueError("an indexed PNG has a format of its own: color and depth do not go with palette")
    return COLORS["rgba" if color is None else color], None if depth is None else int(depth)


def layer_format_arguments(fmt, channels: int, bg):
    """What ``Layer.write_png`` checks for a format of ``format_arguments`` before any device work: the svgr_png_samples source
    kind of a layer of `channels` channels.  A one-channel layer is written as grey only; ``bg`` goes with the colour types
    without alpha (2 and 0) of an RGBA layer only."""
    colour_type = fmt[0]
    if channels == 1:
        if colour_type != 0:
            raise ValueError('Only RGBA layers are supported (a one-channel layer is written with color="grey")')
        if bg is not None:
            raise ValueError("a one-channel layer is written as it is: bg does not go with it")
        return _abi.PNG_SRC_MASK_F64
    if channels != 4:
        raise ValueError("Only RGBA layers are supported")
    if colour_type in (4, 6) and bg is not None:
        raise ValueError('bg goes with the formats without alpha, color="rgb" and color="grey"')
    return _abi.PNG_SRC_RGBA_F64


def canvas_source(canvas, fmt):
    """What ``canvas_to_png`` makes of its array under a format of ``format_arguments``, before any device work:
    ``(rows, cols, colour type, depth, raw, source, kind)``.  ``raw`` is the ``(rows, cols * bpp)`` uint8 scanline bytes of an array
    that holds the samples themselves (and ``source`` is None); otherwise ``source`` is the RGBA array to upload for
    svgr_png_samples and ``kind`` its source kind."""
    colour_type, depth = fmt
    ch = _CHANNELS[colour_type]
    a = np.asarray(canvas)
    if a.dtype in (np.uint8, np.uint16) and ((a.ndim == 3 and a.shape[2] == ch) or (a.ndim == 2 and ch == 1)):
        if a.dtype == np.uint16:
            if depth == 8:
                raise ValueError("uint16 samples are written at depth 16; depth=8 does not go with them")
            depth = 16
        depth = 8 if depth is None else depth
        rows, cols = a.shape[:2]
        if rows == 0 or cols == 0:
            raise ValueError(f"a PNG image has at least one pixel, not {cols} x {rows}")
        if depth == 16:   # (most significant byte first; a byte widens exactly: v * 257)
            wide = a.astype(np.uint16) * np.uint16(257) if a.dtype == np.uint8 else a
            raw = np.ascontiguousarray(wide.astype(">u2")).view(np.uint8).reshape(rows, cols * ch * 2)
        else:
            raw = np.ascontiguousarray(a).reshape(rows, cols * ch)
        return rows, cols, colour_type, depth, raw, None, None
    if a.ndim == 3 and a.shape[2] == 4 and (a.dtype == np.uint8 or a.dtype.kind == "f"):
        rows, cols = a.shape[:2]
        if rows == 0 or cols == 0:
            raise ValueError(f"a PNG image has at least one pixel, not {cols} x {rows}")
        depth = 8 if depth is None else depth
        if a.dtype == np.uint8:
            return rows, cols, colour_type, depth, None, np.ascontiguousarray(a), _abi.PNG_SRC_RGBA_U8
        return rows, cols, colour_type, depth, None, np.ascontiguousarray(a, dtype=np.float64), _abi.PNG_SRC_RGBA_F64
    name = next(k for k, v in COLORS.items() if v == colour_type)
    forms = f"(h, w, {ch})" + (" or (h, w)" if ch == 1 else "")
    raise ValueError(f'color="{name}" takes uint8 or uint16 samples shaped {forms}, or straight-alpha sRGB RGBA shaped (h, w, 4), '
                     f"float or uint8; not {a.dtype} {a.shape}")


def samples_device(src, kind: int, rows: int, cols: int, colour_type: int, depth: int) -> "_abi.DeviceBuffer":
    """The packed samples of the pixels in ``src`` (a DeviceBuffer, or an array, which is uploaded), made on the device and left
    there: ``rows * cols * bpp`` bytes."""
    ctx = _abi.Context.get()
    if not isinstance(src, _abi.DeviceBuffer):
        src = ctx.from_host(np.ascontiguousarray(src))
    return _abi.png_samples(ctx, src, kind, int(rows), int(cols), colour_type, depth)


def encode_samples(samples, rows: int, cols: int, colour_type: int, depth: int, output, args):
    """The PNG of packed samples -- a DeviceBuffer of ``rows * cols * bpp`` bytes or a ``(rows, cols * bpp)`` uint8 array -- into
    ``output`` (default a new BytesIO), which is returned.  ``args`` is what ``encoder_arguments`` returned: the host encoder
    downloads the samples and writes filter 0 rows through zlib, the device encoder filters (svgr_png_filter_bytes) and deflates
    them there."""
    import io

    rows, cols = int(rows), int(cols)
    bpp = _CHANNELS[colour_type] * depth // 8
    row_bytes = cols * bpp
    if args[0] == "device":
        mode = _filter_number("adaptive" if args[1] is None else args[1])
        code = _huffman_number("dynamic" if args[2] is None else args[2])
        ctx = _abi.Context.get()
        if not isinstance(samples, _abi.DeviceBuffer):
            samples = ctx.from_host(np.ascontiguousarray(samples, dtype=np.uint8))
        filtered = _abi.png_filter_bytes(ctx, samples, rows, row_bytes, bpp, mode)
        idat = _abi.deflate(ctx, filtered, rows * (1 + row_bytes), code)
    else:
        _, level, threads = args
        if isinstance(samples, _abi.DeviceBuffer):
            samples = samples.download((rows, row_bytes), np.uint8)
        scan = np.zeros((rows, 1 + row_bytes), dtype=np.uint8)   # filter byte 0 in front of every scanline, ONE deflate stream
        scan[:, 1:] = np.asarray(samples, dtype=np.uint8).reshape(rows, row_bytes)
        if threads > 1:
            from .layer import _deflate_parallel  # noqa: PLC0415

            idat = _deflate_parallel(scan.tobytes(), level, threads)
        else:
            comp = zlib.compressobj(level=level)
            idat = comp.compress(scan.tobytes()) + comp.flush()
    return write_container(io.BytesIO() if output is None else output, cols, rows, idat, colour_type, depth)
