"""Test-side pieces of the OpenType / CFF tests: a small writer of ``CFF `` tables and ``OTTO`` files from operator lists
(`charstring`, `index`, `dict_bytes`, `build_cff`, `build_otf`), the decode cases with the contours they expect, the arrays of
the C ABI (`pack`) and the case list of the outline pass (`outline_cases`, `fuzz_case`), shared by the host tests and the GPU
test.

A charstring is a list of numbers and operator names; ``("raw", bytes)`` puts bytes in as they are (mask bytes, a number in a
chosen encoding).  A decoded glyph is a list of contours, a contour a list of ``(x, y, kind)`` with the kinds below."""
import struct

import numpy as np

from tests import ttf_cases as T

B = 256   # output segments (= lanes) per workgroup of k_cff_emit (svgr_cff_block; the first GPU test asserts it)

MOVE, LINE, C1, C2, CURVE = 0, 1, 2, 3, 4
IDENTITY = T.IDENTITY

OPS = {"hstem": 1, "vstem": 3, "vmoveto": 4, "rlineto": 5, "hlineto": 6, "vlineto": 7, "rrcurveto": 8, "callsubr": 10, "return": 11,
       "endchar": 14, "hstemhm": 18, "hintmask": 19, "cntrmask": 20, "rmoveto": 21, "hmoveto": 22, "vstemhm": 23, "rcurveline": 24,
       "rlinecurve": 25, "vvcurveto": 26, "hhcurveto": 27, "callgsubr": 29, "vhcurveto": 30, "hvcurveto": 31,
       "and": (12, 3), "or": (12, 4), "not": (12, 5), "abs": (12, 9), "add": (12, 10), "sub": (12, 11), "div": (12, 12), "neg": (12, 14),
       "eq": (12, 15), "drop": (12, 18), "put": (12, 20), "get": (12, 21), "ifelse": (12, 22), "random": (12, 23), "mul": (12, 24),
       "sqrt": (12, 26), "dup": (12, 27), "exch": (12, 28), "index": (12, 29), "roll": (12, 30), "hflex": (12, 34), "flex": (12, 35),
       "hflex1": (12, 36), "flex1": (12, 37), "reserved": 2, "reserved12": (12, 99)}


def number(v) -> bytes:
    """A charstring operand in its shortest encoding; a value that is not whole as 16.16 (give k / 65536)."""
    if v != int(v):
        fixed = round(v * 65536)
        assert fixed / 65536 == v
        return b"\xff" + struct.pack(">i", fixed)
    v = int(v)
    if -107 <= v <= 107:
        return bytes([v + 139])
    if 108 <= v <= 1131:
        return bytes([247 + ((v - 108) >> 8), (v - 108) & 255])
    if -1131 <= v <= -108:
        return bytes([251 + ((-v - 108) >> 8), (-v - 108) & 255])
    if -32768 <= v <= 32767:
        return b"\x1c" + struct.pack(">h", v)
    return b"\xff" + struct.pack(">i", v * 65536)


def fixed(v) -> tuple:
    """`v` as a 16.16 operand whatever its value."""
    return ("raw", b"\xff" + struct.pack(">i", round(v * 65536)))


def charstring(items) -> bytes:
    out = b""
    for item in items:
        if isinstance(item, tuple):
            out += item[1]
        elif isinstance(item, str):
            op = OPS[item]
            out += bytes(op) if isinstance(op, tuple) else bytes([op])
        else:
            out += number(item)
    return out


def index(objects, off_size=None) -> bytes:
    """An INDEX; `off_size`: the offSize to write (None: the smallest that holds the offsets)."""
    objects = list(objects)
    if not objects:
        return b"\0\0"
    offsets, at = [1], 1
    for o in objects:
        at += len(o)
        offsets.append(at)
    if off_size is None:
        off_size = 1 if at < 256 else 2 if at < 65536 else 3 if at < 1 << 24 else 4
    return (struct.pack(">HB", len(objects), off_size) + b"".join(v.to_bytes(off_size, "big") for v in offsets) + b"".join(objects))


def real(v: float) -> bytes:
    text = repr(float(v)).replace("e-", "c").replace("e", "b").replace("+", "")
    nibbles = ["0123456789.bc?-".index(ch) if ch not in "bc" else (11 if ch == "b" else 12) for ch in text] + [15]
    if len(nibbles) % 2:
        nibbles.append(15)
    return b"\x1e" + bytes(nibbles[i] << 4 | nibbles[i + 1] for i in range(0, len(nibbles), 2))


def dict_bytes(entries) -> bytes:
    """A DICT from ``[(operator or (12, x), [operands])]``: whole numbers as 5-byte operands (29), so that a DICT's size does not
    depend on the offsets it holds; a float as a real (30); ``("raw", bytes)`` as it is."""
    out = b""
    for op, operands in entries:
        for v in operands:
            out += v[1] if isinstance(v, tuple) else real(v) if isinstance(v, float) else b"\x1d" + struct.pack(">i", v)
        out += bytes(op) if isinstance(op, tuple) else bytes([op])
    return out


def build_cff(charstrings, subrs=None, gsubrs=(), *, cid=None, fdselect_format=0, font_matrix=None, charstring_type=None, major=1,
              names=(b"Synthetic",), off_size=None, subrs_pad=3, extra_top=()) -> bytes:
    """A ``CFF `` table.  `charstrings`, `subrs` (None: an empty Private DICT, no Subrs), `gsubrs`: lists of bytes.  `cid`: the local subroutine
    lists of the Font DICTs, with `charstrings` then taking ``(bytes, font dict)`` pairs; `subrs_pad` bytes lie between a Private
    DICT and its Subrs (the offset is relative to the Private DICT)."""
    select = None
    if cid is not None:
        select = [fd for _cs, fd in charstrings]
        charstrings = [cs for cs, _fd in charstrings]
    head = bytes([major, 0, 4, 2]) + index(names) if names else bytes([major, 0, 4, 2]) + index([])

    def private(sub):
        d = dict_bytes([(19, [0])])                      # Subrs: the DICT's own size + the pad
        d = dict_bytes([(19, [len(d) + subrs_pad])])
        return d, d + b"\xaa" * subrs_pad + index(sub, off_size)

    def top(at_charstrings=0, at_private=(0, 0), at_fdarray=0, at_fdselect=0, at_charset=0):
        entries = []
        if cid is not None:
            entries.append(((12, 30), [0, 0, 0]))    # ROS
        if font_matrix is not None:
            entries.append(((12, 7), [float(v) for v in font_matrix]))
        if charstring_type is not None:
            entries.append(((12, 6), [charstring_type]))
        entries.extend(extra_top)
        entries.append((17, [at_charstrings]))
        if cid is not None:
            entries += [((12, 36), [at_fdarray]), ((12, 37), [at_fdselect])]
        else:
            entries.append((18, list(at_private)))
        entries.append((15, [at_charset]))           # charset (not read by the package; fontTools wants one, and a Private)
        return dict_bytes(entries)

    n_tops = len(names) if names else 1
    front = len(head) + len(index([top()] * n_tops)) + len(index([])) + len(index(gsubrs, off_size))
    cs_index = index(charstrings, off_size)
    at_cs = front
    charset = struct.pack(">BHH", 2, 1, max(len(charstrings) - 2, 0))    # format 2: the SIDs / CIDs 1 .. n - 1 in one range
    at_charset = front + len(cs_index)
    at = at_charset + len(charset)
    if cid is None:
        if subrs is not None:
            d, block = private(subrs)
            top_dict, tail = top(at_cs, (len(d), at), at_charset=at_charset), charset + block
        else:   # an empty Private DICT
            top_dict, tail = top(at_cs, (0, at), at_charset=at_charset), charset
    else:
        if fdselect_format == 0:
            fdselect = b"\0" + bytes(select)
        else:
            ranges = [(g, fd) for g, fd in enumerate(select) if g == 0 or select[g - 1] != fd]
            fdselect = struct.pack(">BH", 3, len(ranges)) + b"".join(struct.pack(">HB", g, fd) for g, fd in ranges) + struct.pack(">H", len(select))
        at_fdselect = at
        at += len(fdselect)
        blocks = [private(sub) for sub in cid]
        font_dict_size = len(dict_bytes([(18, [0, 0])]))
        at_fdarray = at
        at += len(index([b"\0" * font_dict_size] * len(cid)))
        font_dicts = []
        for d, block in blocks:
            font_dicts.append(dict_bytes([(18, [len(d), at])]))
            at += len(block)
        tail = charset + fdselect + index(font_dicts) + b"".join(block for _d, block in blocks)
        top_dict = top(at_cs, (0, 0), at_fdarray, at_fdselect, at_charset)
    out = head + index([top_dict] * n_tops) + index([]) + index(gsubrs, off_size)
    assert len(out) == front
    return out + cs_index + tail


def assemble(tables, sfnt=b"OTTO") -> bytes:
    """An sfnt file of `tables`, ``{tag: bytes}``."""
    tags = sorted(tables)
    out, at = sfnt + struct.pack(">HHHH", len(tags), 0, 0, 0), 12 + 16 * len(tags)
    for tag in tags:
        out += struct.pack(">4sIII", tag.encode("latin-1"), 0, at, len(tables[tag]))
        at += len(T._pad4(tables[tag]))
    return out + b"".join(T._pad4(tables[tag]) for tag in tags)


def tables_of(data: bytes) -> dict:
    n, = struct.unpack_from(">H", data, 4)
    out = {}
    for i in range(n):
        tag, _sum, off, length = struct.unpack_from(">4sIII", data, 12 + 16 * i)
        out[tag.decode("latin-1")] = data[off:off + length]
    return out


def build_otf(cff: bytes, cmap, advances, kern=None, *, drop=(), cff_tag="CFF ", sfnt=b"OTTO", **options) -> bytes:
    """An ``OTTO`` file around the table `cff`: the sfnt tables are those of `ttf_cases.build_ttf` for as many empty glyphs as
    there are `advances`, ``glyf`` / ``loca`` left out and ``maxp`` cut to its version 0.5 (6 bytes)."""
    tables = tables_of(T.build_ttf([[] for _ in advances], cmap, advances, kern, **options))
    del tables["glyf"], tables["loca"]
    tables["maxp"] = struct.pack(">IH", 0x00005000, len(advances))
    tables[cff_tag] = cff
    for tag in drop:
        tables.pop(tag, None)
    return assemble(tables, sfnt)


def font_of(charstrings, subrs=None, gsubrs=(), **cff_options) -> bytes:
    """An ``OTTO`` file whose glyphs are the operator lists `charstrings` (glyph 0 first); characters ``A``, ``B``, ... name the
    glyphs 1, 2, ...; every advance is 500."""
    n = len(charstrings)
    cs = [(charstring(c[0]), c[1]) if cff_options.get("cid") is not None else charstring(c) for c in charstrings]
    cff = build_cff(cs, None if subrs is None else [charstring(s) for s in subrs], [charstring(s) for s in gsubrs], **cff_options)
    return build_otf(cff, {ord("A") + g - 1: g for g in range(1, n)}, [500] * n)


# ----------------------------------------------------------------------------------------------------------------------
# the machine, operator by operator: (name, charstring, the contours it draws)
# ----------------------------------------------------------------------------------------------------------------------
def _abs(start, steps):
    """The contour that begins at `start` and takes `steps`, ``(dx, dy, kind)``, as absolute points."""
    x, y = start
    out = [(float(x), float(y), MOVE)]
    for dx, dy, kind in steps:
        x, y = x + dx, y + dy
        out.append((float(x), float(y), kind))
    return out


def _curve(a, b, c, d, e, f):
    return [(a, b, C1), (c, d, C2), (e, f, CURVE)]


NOTDEF = [10, 20, "rmoveto", 100, "hlineto", "endchar"]

DECODE_CASES = [
    # ---- movetos and lines
    ("rmoveto", [10, 20, "rmoveto", 5, 6, "rlineto", "endchar"], [_abs((10, 20), [(5, 6, LINE)])]),
    ("hmoveto_vmoveto", [10, "hmoveto", 1, 2, "rlineto", 7, "vmoveto", 3, 4, "rlineto", "endchar"],
     [_abs((10, 0), [(1, 2, LINE)]), _abs((11, 9), [(3, 4, LINE)])]),
    ("rlineto_two", [0, 0, "rmoveto", 1, 2, 3, 4, "rlineto", "endchar"], [_abs((0, 0), [(1, 2, LINE), (3, 4, LINE)])]),
    ("hlineto_odd", [0, 0, "rmoveto", 5, 6, 7, "hlineto", "endchar"], [_abs((0, 0), [(5, 0, LINE), (0, 6, LINE), (7, 0, LINE)])]),
    ("hlineto_even", [0, 0, "rmoveto", 5, 6, "hlineto", "endchar"], [_abs((0, 0), [(5, 0, LINE), (0, 6, LINE)])]),
    ("vlineto_odd", [0, 0, "rmoveto", 5, "vlineto", "endchar"], [_abs((0, 0), [(0, 5, LINE)])]),
    ("vlineto_even", [0, 0, "rmoveto", 5, 6, 7, 8, "vlineto", "endchar"], [_abs((0, 0), [(0, 5, LINE), (6, 0, LINE), (0, 7, LINE), (8, 0, LINE)])]),
    # ---- curves
    ("rrcurveto_two", [1, 1, "rmoveto", 1, 2, 3, 4, 5, 6, -1, -2, -3, -4, -5, -6, "rrcurveto", "endchar"],
     [_abs((1, 1), _curve(1, 2, 3, 4, 5, 6) + _curve(-1, -2, -3, -4, -5, -6))]),
    ("hhcurveto_plain", [0, 0, "rmoveto", 1, 2, 3, 4, 5, 6, 7, 8, "hhcurveto", "endchar"],
     [_abs((0, 0), _curve(1, 0, 2, 3, 4, 0) + _curve(5, 0, 6, 7, 8, 0))]),
    ("hhcurveto_dy1", [0, 0, "rmoveto", 9, 1, 2, 3, 4, 5, 6, 7, 8, "hhcurveto", "endchar"],
     [_abs((0, 0), _curve(1, 9, 2, 3, 4, 0) + _curve(5, 0, 6, 7, 8, 0))]),
    ("vvcurveto_plain", [0, 0, "rmoveto", 1, 2, 3, 4, "vvcurveto", "endchar"], [_abs((0, 0), _curve(0, 1, 2, 3, 0, 4))]),
    ("vvcurveto_dx1", [0, 0, "rmoveto", 9, 1, 2, 3, 4, 5, 6, 7, 8, "vvcurveto", "endchar"],
     [_abs((0, 0), _curve(9, 1, 2, 3, 0, 4) + _curve(0, 5, 6, 7, 0, 8))]),
    ("hvcurveto_one", [0, 0, "rmoveto", 1, 2, 3, 4, "hvcurveto", "endchar"], [_abs((0, 0), _curve(1, 0, 2, 3, 0, 4))]),
    ("hvcurveto_one_trailing", [0, 0, "rmoveto", 1, 2, 3, 4, 5, "hvcurveto", "endchar"], [_abs((0, 0), _curve(1, 0, 2, 3, 5, 4))]),
    ("hvcurveto_two", [0, 0, "rmoveto", 1, 2, 3, 4, 5, 6, 7, 8, "hvcurveto", "endchar"],
     [_abs((0, 0), _curve(1, 0, 2, 3, 0, 4) + _curve(0, 5, 6, 7, 8, 0))]),
    ("hvcurveto_two_trailing", [0, 0, "rmoveto", 1, 2, 3, 4, 5, 6, 7, 8, 9, "hvcurveto", "endchar"],
     [_abs((0, 0), _curve(1, 0, 2, 3, 0, 4) + _curve(0, 5, 6, 7, 8, 9))]),
    ("hvcurveto_three_trailing", [0, 0, "rmoveto", 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, "hvcurveto", "endchar"],
     [_abs((0, 0), _curve(1, 0, 2, 3, 0, 4) + _curve(0, 5, 6, 7, 8, 0) + _curve(9, 0, 10, 11, 13, 12))]),
    ("vhcurveto_one", [0, 0, "rmoveto", 1, 2, 3, 4, "vhcurveto", "endchar"], [_abs((0, 0), _curve(0, 1, 2, 3, 4, 0))]),
    ("vhcurveto_one_trailing", [0, 0, "rmoveto", 1, 2, 3, 4, 5, "vhcurveto", "endchar"], [_abs((0, 0), _curve(0, 1, 2, 3, 4, 5))]),
    ("vhcurveto_two_trailing", [0, 0, "rmoveto", 1, 2, 3, 4, 5, 6, 7, 8, 9, "vhcurveto", "endchar"],
     [_abs((0, 0), _curve(0, 1, 2, 3, 4, 0) + _curve(5, 0, 6, 7, 9, 8))]),
    ("rcurveline", [0, 0, "rmoveto", 1, 2, 3, 4, 5, 6, 7, 8, "rcurveline", "endchar"], [_abs((0, 0), _curve(1, 2, 3, 4, 5, 6) + [(7, 8, LINE)])]),
    ("rlinecurve", [0, 0, "rmoveto", 7, 8, 9, 10, 1, 2, 3, 4, 5, 6, "rlinecurve", "endchar"],
     [_abs((0, 0), [(7, 8, LINE), (9, 10, LINE)] + _curve(1, 2, 3, 4, 5, 6))]),
    # ---- the flexes: two cubics each, the depth dropped
    ("flex", [0, 0, "rmoveto", 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 50, "flex", "endchar"],
     [_abs((0, 0), _curve(1, 2, 3, 4, 5, 6) + _curve(7, 8, 9, 10, 11, 12))]),
    ("hflex", [0, 5, "rmoveto", 1, 2, 3, 4, 5, 6, 7, "hflex", "endchar"], [_abs((0, 5), _curve(1, 0, 2, 3, 4, 0) + _curve(5, 0, 6, -3, 7, 0))]),
    ("hflex1", [0, 5, "rmoveto", 1, 2, 3, 4, 5, 6, 7, 8, 9, "hflex1", "endchar"],
     [_abs((0, 5), _curve(1, 2, 3, 4, 5, 0) + _curve(6, 0, 7, 8, 9, -(2 + 4 + 8)))]),
    ("flex1_wide", [0, 0, "rmoveto", 10, 1, 10, 1, 10, 1, 10, -1, 10, -1, 7, "flex1", "endchar"],
     [_abs((0, 0), _curve(10, 1, 10, 1, 10, 1) + _curve(10, -1, 10, -1, 7, -1))]),
    ("flex1_tall", [0, 0, "rmoveto", 1, 10, 1, 10, 1, 10, -1, 10, 1, 10, 7, "flex1", "endchar"],
     [_abs((0, 0), _curve(1, 10, 1, 10, 1, 10) + _curve(-1, 10, 1, 10, -3, 7))]),
    # ---- the optional width in front of the first stack-clearing operator
    ("width_rmoveto", [333, 10, 20, "rmoveto", 5, 6, "rlineto", "endchar"], [_abs((10, 20), [(5, 6, LINE)])]),
    ("width_hmoveto", [333, 10, "hmoveto", 5, 6, "rlineto", "endchar"], [_abs((10, 0), [(5, 6, LINE)])]),
    ("width_vmoveto", [333, 10, "vmoveto", 5, 6, "rlineto", "endchar"], [_abs((0, 10), [(5, 6, LINE)])]),
    ("width_hstem", [333, 10, 20, "hstem", 1, 2, "rmoveto", 5, 6, "rlineto", "endchar"], [_abs((1, 2), [(5, 6, LINE)])]),
    ("width_vstem", [333, 10, 20, 30, 40, "vstem", 1, 2, "rmoveto", 5, 6, "rlineto", "endchar"], [_abs((1, 2), [(5, 6, LINE)])]),
    ("width_hstemhm_then_mask", [333, 10, 20, "hstemhm", "hintmask", ("raw", b"\x80"), 1, 2, "rmoveto", 5, 6, "rlineto", "endchar"],
     [_abs((1, 2), [(5, 6, LINE)])]),
    ("width_hintmask", [333, 10, 20, "hintmask", ("raw", b"\x80"), 1, 2, "rmoveto", 5, 6, "rlineto", "endchar"], [_abs((1, 2), [(5, 6, LINE)])]),
    ("width_cntrmask", [333, 10, 20, "cntrmask", ("raw", b"\x80"), 1, 2, "rmoveto", 5, 6, "rlineto", "endchar"], [_abs((1, 2), [(5, 6, LINE)])]),
    ("width_vstemhm", [333, 10, 20, "vstemhm", 1, 2, "rmoveto", 5, 6, "rlineto", "endchar"], [_abs((1, 2), [(5, 6, LINE)])]),
    ("width_endchar", [333, "endchar"], []),
    ("width_endchar_seac", [333, 0, 0, 65, 66, "endchar"], []),    # 5 operands: the width, then the four of the seac form
    ("no_width_second_moveto", [10, 20, "rmoveto", 5, 6, "rlineto", 7, "hmoveto", 1, 1, "rlineto", "endchar"],
     [_abs((10, 20), [(5, 6, LINE)]), _abs((22, 26), [(1, 1, LINE)])]),
    # ---- masks: 8 stems take one byte, 9 take two; the operands in front of a mask are a vstem
    ("hintmask_8_stems", [1, 1, 1, 1, 1, 1, 1, 1, "hstemhm", 1, 1, 1, 1, 1, 1, 1, 1, "vstemhm", "hintmask", ("raw", b"\x15"), 1, 2, "rmoveto", 5, 6,
                          "rlineto", "endchar"], [_abs((1, 2), [(5, 6, LINE)])]),
    ("hintmask_9_stems", [1, 1, 1, 1, 1, 1, 1, 1, "hstemhm", 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, "vstemhm", "hintmask", ("raw", b"\x15\x05"), 1, 2,
                          "rmoveto", 5, 6, "rlineto", "endchar"], [_abs((1, 2), [(5, 6, LINE)])]),
    ("hintmask_implied_vstem", [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, "hstemhm", 1, 1, "hintmask", ("raw", b"\x15\x05"), 1, 2,
                                "rmoveto", 5, 6, "rlineto", "hintmask", ("raw", b"\x0b\x05"), 1, 1, "rlineto", "endchar"],
     [_abs((1, 2), [(5, 6, LINE), (1, 1, LINE)])]),
    # ---- numbers
    ("fixed_operands", [0.5, -0.25, "rmoveto", 1.0 + 1 / 65536, -3 / 65536, "rlineto", fixed(7), 30000, "rlineto", -30000, 1000, "rlineto", "endchar"],
     [_abs((0.5, -0.25), [(1.0 + 1 / 65536, -3 / 65536, LINE), (7, 30000, LINE), (-30000, 1000, LINE)])]),
    # ---- arithmetic and storage
    ("div", [7, 2, "div", 1, 4, "div", "rmoveto", 5, 6, "rlineto", "endchar"], [_abs((3.5, 0.25), [(5, 6, LINE)])]),
    ("add_sub_mul_neg_abs", [1, 2, "add", 10, 4, "sub", "rmoveto", 3, 4, "mul", -5, "abs", "neg", "rlineto", "endchar"],
     [_abs((3, 6), [(12, -5, LINE)])]),
    ("sqrt_dup_exch_drop", [16, "sqrt", "dup", 9, "exch", "drop", "rmoveto", 5, 6, "rlineto", "endchar"], [_abs((4, 9), [(5, 6, LINE)])]),
    ("roll_up", [1, 2, 3, 3, 1, "roll", "drop", "rmoveto", 5, 6, 7, 8, 4, 6, "roll", "rlineto", "endchar"],      # 1 2 3 -> 3 1 2
     [_abs((3, 1), [(7, 8, LINE), (5, 6, LINE)])]),
    ("roll_down", [1, 2, 3, 3, -1, "roll", "drop", "rmoveto", 5, 6, 7, 8, 4, -1, "roll", "rlineto", "endchar"],   # 1 2 3 -> 2 3 1
     [_abs((2, 3), [(6, 7, LINE), (8, 5, LINE)])]),
    ("index", [0, 0, "rmoveto", 7, 8, 1, "index", -1, "index", "rlineto", "endchar"], [_abs((0, 0), [(7, 8, LINE), (7, 7, LINE)])]),
    ("put_get", [42, 3, "put", 17, 31, "put", 3, "get", 31, "get", "rmoveto", 0, "get", 1, "rlineto", "endchar"], [_abs((42, 17), [(0, 1, LINE)])]),
    ("ifelse", [10, 20, 1, 2, "ifelse", 10, 20, 2, 1, "ifelse", "rmoveto", 10, 20, 2, 2, "ifelse", 1, "rlineto", "endchar"],
     [_abs((10, 20), [(10, 1, LINE)])]),
    ("and_or_not_eq", [1, 0, "and", 1, 0, "or", "rmoveto", 0, "not", 3, 3, "eq", "rlineto", 5, "not", 3, 4, "eq", "rlineto", "endchar"],
     [_abs((0, 1), [(1, 1, LINE), (0, 0, LINE)])]),
    # ---- contours
    ("draw_before_moveto", [5, 6, "rlineto", 1, 2, 3, 4, 5, 6, "rrcurveto", "endchar"], [_abs((0, 0), [(5, 6, LINE)] + _curve(1, 2, 3, 4, 5, 6))]),
    ("lone_moveto", [10, 20, "rmoveto", 1, 1, "rmoveto", 2, 2, "rlineto", "endchar"], [[(10.0, 20.0, MOVE)], _abs((11, 21), [(2, 2, LINE)])]),
    ("seac_form", [1, 2, "rmoveto", 3, 4, "rlineto", 0, 0, 65, 66, "endchar"], [_abs((1, 2), [(3, 4, LINE)])]),
    ("empty", ["endchar"], []),
]

# (name, charstring, local subroutines, global subroutines, contours): calls at the biases 107 and 1131
_PAD = [["return"]]


def subr_cases():
    line = [[5, 6, "rlineto", "return"]]
    two = [[1, 1, "rlineto", "return"], [2, 2, "rlineto", -107, "callgsubr", "return"]]
    return [
        ("local_107", [1, 2, "rmoveto", -107, "callsubr", "endchar"], line, [], [_abs((1, 2), [(5, 6, LINE)])]),
        ("global_107", [1, 2, "rmoveto", -107, "callgsubr", "endchar"], None, line, [_abs((1, 2), [(5, 6, LINE)])]),
        ("local_calls_global", [1, 2, "rmoveto", -106, "callsubr", "endchar"], two, [[9, 9, "rlineto", "return"]],
         [_abs((1, 2), [(2, 2, LINE), (9, 9, LINE)])]),
        ("local_1131", [1, 2, "rmoveto", 1240 - 1 - 1131, "callsubr", -1131, "callsubr", "endchar"],
         [[3, 3, "rlineto", "return"]] + _PAD * 1238 + line, [], [_abs((1, 2), [(5, 6, LINE), (3, 3, LINE)])]),
        ("global_1131", [1, 2, "rmoveto", 1240 - 1 - 1131, "callgsubr", "endchar"], None, _PAD * 1239 + line, [_abs((1, 2), [(5, 6, LINE)])]),
        ("subr_ends_in_endchar", [1, 2, "rmoveto", -107, "callsubr"], [[5, 6, "rlineto", "endchar"]], [], [_abs((1, 2), [(5, 6, LINE)])]),
        ("operands_pass_through", [1, 2, "rmoveto", 5, 6, -107, "callsubr", "endchar"], [["rlineto", "return"]], [], [_abs((1, 2), [(5, 6, LINE)])]),
    ]


def nested(levels: int):
    """(charstring, local subroutines): subroutine k calls k + 1, `levels` calls deep; the last draws a line."""
    subrs = [[k + 1 - 107, "callsubr", "return"] for k in range(levels - 1)] + [[5, 6, "rlineto", "return"]]
    return [1, 2, "rmoveto", -107, "callsubr", "endchar"], subrs


def bomb():
    """(charstring, local subroutines): 10 levels, each calling the next 16 times: 16^10 operators if it were run."""
    subrs = [[x for _ in range(16) for x in (k + 1 - 107, "callsubr")] + ["return"] for k in range(9)] + [[1, "drop"] * 16 + ["return"]]
    return [1, 2, "rmoveto", -107, "callsubr", "endchar"], subrs


# (name, charstring, local subroutines, what the error names)
MALFORMED_CHARSTRINGS = [
    ("subr_out_of_range", [1, 2, "rmoveto", 0, "callsubr", "endchar"], [["return"]], "subroutine"),
    ("subr_negative", [1, 2, "rmoveto", -108, "callsubr", "endchar"], [["return"]], "subroutine"),
    ("gsubr_without_index", [1, 2, "rmoveto", -107, "callgsubr", "endchar"], None, "subroutine"),
    ("callsubr_without_private", [1, 2, "rmoveto", -107, "callsubr", "endchar"], None, "subroutine"),
    ("stack_overflow", [1] * 49 + ["rlineto", "endchar"], None, "stack"),
    ("stack_underflow_moveto", [1, "rmoveto", "endchar"], None, "underflow"),
    ("stack_underflow_add", [1, "add", "endchar"], None, "underflow"),
    ("stack_underflow_curve", [1, 2, "rmoveto", 1, 2, 3, "rrcurveto", "endchar"], None, "underflow"),
    ("no_endchar", [1, 2, "rmoveto", 3, 4, "rlineto"], None, "endchar"),
    ("subr_without_return", [1, 2, "rmoveto", -107, "callsubr", "endchar"], [[5, 6, "rlineto"]], "return"),
    ("return_at_top", [1, 2, "rmoveto", "return"], None, "return"),
    ("random", [1, 2, "rmoveto", "random", 1, "rlineto", "endchar"], None, "random"),
    ("unknown_operator", [1, 2, "rmoveto", "reserved", "endchar"], None, "operator"),
    ("unknown_escape", [1, 2, "rmoveto", "reserved12", "endchar"], None, "operator"),
    ("mask_runs_out", [1, 1, "hstemhm", "hintmask"], None, "mask"),
    ("number_runs_out", [("raw", b"\x1c\x00")], None, "operand"),
    ("put_out_of_range", [1, 32, "put", "endchar"], None, "transient"),
    ("div_by_zero", [1, 0, "div", "endchar"], None, "div"),
]


# ----------------------------------------------------------------------------------------------------------------------
# the synthetic font of the loader and document tests: lines and curves, subroutines, a kern table
# ----------------------------------------------------------------------------------------------------------------------
SYNTH_SUBRS = [[100, 0, 60, 80, 0, 100, "rrcurveto", "return"]]
SYNTH_GSUBRS = [[-300, "hlineto", "return"]]
SYNTH = [
    # 0 .notdef: a frame
    [500, 50, 0, "rmoveto", 400, 700, -400, "hlineto", -700, "vlineto", 50, 50, "rmoveto", 600, 300, -600, "vlineto", -300, "hlineto", "endchar"],
    # 1 the space
    [300, "endchar"],
    # 2 A: lines and a hole; the outer contour returns to its start by itself
    [700, 50, 0, "rmoveto", 300, 700, 300, -700, -130, 0, -70, 180, -200, 0, -70, -180, "rlineto", -130, "hlineto",
     240, 300, "rmoveto", 120, 0, -60, 170, "rlineto", "endchar"],
    # 3 o: four curves through a subroutine and hvcurveto, and a flex inside
    [600, 300, 0, "rmoveto", 140, 250, 110, 250, "hvcurveto", 140, -110, 110, -250, "vhcurveto", -140, -250, -110, -250, "hvcurveto",
     -140, 110, -110, 250, "vhcurveto", -150, 150, "rmoveto", 100, 10, 50, 0.5, 50, -10.5, 50, 10, 50, 0, 50, -10, 20, "flex", 200, "vlineto",
     -107, "callgsubr", "endchar"],
    # 4 V: lines, hints with a mask in front
    [600, 0, 20, "hstemhm", 0, 100, "hintmask", ("raw", b"\xc0"), 0, 700, "rmoveto", 100, 0, 200, -600, 200, 600, 100, 0, -250, -700, "rlineto",
     -100, "hlineto", "endchar"],
    # 5 D: a local subroutine
    [650, 100, 0, "rmoveto", 200, "hlineto", -107, "callsubr", 520, "vlineto", -360, "hlineto", "endchar"],
]
SYNTH_ADVANCES = [500, 300, 700, 600, 600, 650]
SYNTH_CMAP = {ord(" "): 1, ord("A"): 2, ord("o"): 3, ord("V"): 4, ord("D"): 5}
SYNTH_KERN = {(2, 4): -80, (4, 2): -70}


def synthetic_otf(**options) -> bytes:
    cff = build_cff([charstring(c) for c in SYNTH], [charstring(s) for s in SYNTH_SUBRS], [charstring(s) for s in SYNTH_GSUBRS])
    return build_otf(cff, SYNTH_CMAP, SYNTH_ADVANCES, SYNTH_KERN, **options)


# ----------------------------------------------------------------------------------------------------------------------
# the outline pass: the arrays of the C ABI, and the cases
# ----------------------------------------------------------------------------------------------------------------------
def pack(atlas, parts):
    """The arrays of svgr_cff_outline.  `atlas`: glyphs as lists of contours of ``(x, y, kind)``; `parts`: ``[(glyph index, (m00,
    m01, m10, m11, dx, dy), pen, sx, sy)]``."""
    pts = [p for g in atlas for c in g for p in c]
    contour_off, glyph_contour_off = [0], [0]
    for g in atlas:
        for c in g:
            contour_off.append(contour_off[-1] + len(c))
        glyph_contour_off.append(len(contour_off) - 1)
    return dict(
        pt_xy=np.array([[p[0], p[1]] for p in pts], dtype=np.float64).reshape(-1, 2),
        pt_kind=np.array([p[2] for p in pts], dtype=np.uint8),
        contour_off=np.array(contour_off, dtype=np.int32),
        glyph_contour_off=np.array(glyph_contour_off, dtype=np.int32),
        part_glyph=np.array([p[0] for p in parts], dtype=np.int32),
        part_m=np.array([p[1] for p in parts], dtype=np.float64).reshape(-1, 6),
        part_pen=np.array([p[2] for p in parts], dtype=np.float64),
        part_sx=np.array([p[3] for p in parts], dtype=np.float64),
        part_sy=np.array([p[4] for p in parts], dtype=np.float64),
    )


def contour_segments(c) -> int:
    return sum(1 for p in c if p[2] in (LINE, CURVE)) + (1 if len(c) >= 2 else 0)


def segments(atlas, parts) -> int:
    return sum(sum(contour_segments(c) for c in atlas[p[0]]) for p in parts)


def ring(rng, n_segments, returns=None):
    """A contour of `n_segments` segments, its closing line among them: random lines and cubics at sixteenths of a unit.
    `returns`: whether the last draw is a line back to the start (None: at random); else the closing line has a length."""
    def coordinate():
        return float(rng.integers(-32000, 32000)) / 16.0

    assert n_segments >= 2
    out = [(coordinate(), coordinate(), MOVE)]
    returns = bool(rng.integers(0, 2)) if returns is None else returns
    for s in range(n_segments - 1):
        if returns and s == n_segments - 2:
            out.append((out[0][0], out[0][1], LINE))
        elif rng.integers(0, 2):
            out.append((coordinate(), coordinate(), LINE))
        else:
            out.extend((coordinate(), coordinate(), kind) for kind in (C1, C2, CURVE))
    assert contour_segments(out) == n_segments
    return out


def _part(rng, g, m=IDENTITY, mirror=True):
    return (g, m, float(rng.integers(0, 5000)), 0.0234375, -0.0234375 if mirror else 0.0234375)


def _total(rng, total):
    """An atlas and parts with `total` segments: one glyph of two contours twice, one glyph for the rest."""
    a = [ring(rng, 37), ring(rng, 63)]
    rest = total - 200
    b = [ring(rng, rest - rest // 2), ring(rng, rest // 2)] if rest >= 4 else [ring(rng, rest)]
    atlas, parts = [a, b], [_part(rng, 0), _part(rng, 1), _part(rng, 0)]
    assert segments(atlas, parts) == total
    return atlas, parts


def outline_cases(b=B):
    """[(name, atlas, parts)]: the seams of the launch, and every branch of the outline rule."""
    rng = np.random.default_rng(20261019)
    cos, sin = T.f2dot14(np.cos(0.5)), T.f2dot14(np.sin(0.5))
    rotated = (cos, sin, -sin, cos, 120.0, -35.0)
    cases = [(f"segments_{name}", *_total(rng, total)) for name, total in (("B-1", b - 1), ("B", b), ("B+1", b + 1), ("2B+1", 2 * b + 1))]
    cases.append(("glyph_larger_than_block", [[ring(rng, b + 44), ring(rng, 7)]], [_part(rng, 0)]))
    cases.append(("same_glyph_B+1_parts", [[ring(rng, 3), ring(rng, 2)]], [_part(rng, 0) for _ in range(b + 1)]))
    # the second contour's draws end the first workgroup; its closing line is lane 0 of the next
    cases.append(("closing_line_first_lane_of_block", [[ring(rng, 100), ring(rng, b - 99, returns=False)], [ring(rng, 20)]],
                  [_part(rng, 0), _part(rng, 1)]))
    glyph, space = [ring(rng, 9), ring(rng, 4)], []
    cases.append(("empty_glyph_between", [glyph, space], [_part(rng, 0), _part(rng, 1), _part(rng, 0)]))
    cases.append(("empty_glyph_first_and_last", [space, glyph], [_part(rng, 0), _part(rng, 1), _part(rng, 1), _part(rng, 0)]))
    cases.append(("lone_move", [[[(5.0, 5.0, MOVE)], ring(rng, 5), [(7.5, -1.0, MOVE)]], [[(1.0, 1.0, MOVE)]]],
                  [_part(rng, 0), _part(rng, 1), _part(rng, 0)]))
    cases.append(("closing_line_of_length_0", [[ring(rng, 6, returns=True)]], [_part(rng, 0)]))
    cases.append(("closing_line_with_length", [[ring(rng, 6, returns=False)]], [_part(rng, 0)]))
    cases.append(("two_points", [[[(0.0, 0.0, MOVE), (10.0, 20.0, LINE)], [(1.0, 1.0, MOVE), (2.0, 2.0, C1), (3.0, 1.0, C2), (4.0, 0.0, CURVE)]]],
                  [_part(rng, 0)]))
    cases.append(("mirrored_and_not", [glyph], [_part(rng, 0, mirror=True), _part(rng, 0, mirror=False)]))
    cases.append(("rotated_part", [glyph, [ring(rng, 6)]], [_part(rng, 0, rotated), _part(rng, 1), _part(rng, 1, (0.5, 0.0, 0.0, -0.75, -8.0, 3.0))]))
    return cases


def fuzz_case(seed: int):
    """A random atlas (1-6 glyphs, 0-5 contours of 1-40 segments or a lone MOVE) and a random part list."""
    rng = np.random.default_rng(seed)

    def contour():
        n = int(rng.integers(1, 41))
        return [(1.5, 2.5, MOVE)] if n == 1 else ring(rng, n)

    atlas = [[contour() for _ in range(int(rng.integers(0, 6)))] for _ in range(int(rng.integers(1, 7)))]
    parts = []
    for _ in range(int(rng.integers(1, 13))):
        m = IDENTITY if rng.integers(0, 2) else tuple(T.f2dot14(v) for v in rng.uniform(-2, 2, 4)) + tuple(float(v) for v in rng.integers(-500, 500, 2))
        parts.append((int(rng.integers(0, len(atlas))), m, float(rng.uniform(0, 8000)), float(rng.uniform(0.001, 0.1)),
                      float(rng.uniform(-0.1, 0.1))))
    return atlas, parts


# ----------------------------------------------------------------------------------------------------------------------
# a real face as CFF (needs fontTools; tests/test_cff_host.py and profiles/bench_cff.py)
# ----------------------------------------------------------------------------------------------------------------------
def truetype_as_cff(path: str, n_glyphs=None, family="DejaVu Sans CFF") -> bytes:
    """The first `n_glyphs` glyphs (None: all) of the TrueType font at `path`, drawn into fontTools' ``T2CharStringPen``s -- its
    quadratics raised to cubics -- and saved as an OpenType / CFF font in memory: every line and curve operator in its specialised
    forms."""
    import io

    from fontTools import ttLib
    from fontTools.fontBuilder import FontBuilder
    from fontTools.pens.t2CharStringPen import T2CharStringPen

    src = ttLib.TTFont(path)
    names = src.getGlyphOrder()[:n_glyphs]
    glyph_set, hmtx = src.getGlyphSet(), src["hmtx"]
    charstrings = {}
    for name in names:
        pen = T2CharStringPen(hmtx[name][0], glyph_set)
        glyph_set[name].draw(pen)    # (the pen raises each quadratic to a cubic and rounds to whole units)
        charstrings[name] = pen.getCharString()
    fb = FontBuilder(src["head"].unitsPerEm, isTTF=False)
    fb.setupGlyphOrder(names)
    fb.setupCharacterMap({code: name for code, name in src.getBestCmap().items() if name in charstrings})
    fb.setupCFF(family.replace(" ", ""), {"FullName": family}, charstrings, {})
    fb.setupHorizontalMetrics({name: hmtx[name] for name in names})
    fb.setupHorizontalHeader(ascent=src["hhea"].ascent, descent=src["hhea"].descent)
    fb.setupNameTable({"familyName": family, "styleName": "Book"})
    fb.setupOS2()
    fb.setupPost()
    out = io.BytesIO()
    fb.save(out)
    return out.getvalue()
