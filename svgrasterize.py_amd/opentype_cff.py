"""OpenType fonts with CFF outlines (beyond the reference): ``read_otf`` parses an ``.otf`` (sfnt version ``OTTO``) into a
``CFFFont``, a ``fonts.Font`` whose glyph outlines come from the Type 2 charstrings of the ``CFF `` table.  ``read_font`` takes
either outline format and picks ``read_ttf`` or ``read_otf`` by the first four bytes.

Host code, pure Python + numpy, with the discipline of ``truetype.py``: a font file is untrusted, every offset, length, count
and offSize is checked against the data before it is used, nothing is allocated by the size a field claims, and a malformed
file raises a ``ValueError`` that says which structure is at fault -- when it is read or, for a glyph's charstring, when that
glyph is first used (glyphs are decoded lazily and cached).  The charstrings are run here; their points become path segments on
the device (``_abi.cff_outline``, svgr_cff_outline; one lane per output segment).  Measuring a string needs no device.

Read: the sfnt directory and ``head``, ``maxp`` (version 0.5), ``hhea`` + ``hmtx``, ``cmap``, ``name``, ``OS/2``, ``kern`` by
``truetype.SfntFont``, the code path of TrueType fonts (its messages begin ``opentype:`` here); of the ``CFF `` table (version 1) the
header, the Name INDEX (one font), the Top DICT, the String INDEX (bounds only), the Global Subr INDEX, ``CharStrings`` (its count
is ``maxp.numGlyphs``), ``CharstringType`` (2), ``Private`` with its ``Subrs`` (an offset relative to the Private DICT), and for
CID-keyed fonts ``ROS``, ``FDArray`` and ``FDSelect`` (formats 0 and 3): a glyph's local subroutines are those of its own Font
DICT's Private DICT.  Glyph id = CharStrings index, characters come from ``cmap``, advances from ``hmtx``.

Not read: charset, Encoding, strings, the charstrings' widths.  Ignored: hints (stems are counted so that the masks can be
stepped over, never applied), ``GPOS`` / ``GSUB`` (so most ``.otf`` files kern nothing: few carry a ``kern`` table), ``FontMatrix``
(``head.unitsPerEm`` is the scale; one warning per font when the matrix is not 1 / unitsPerEm on the diagonal), the deprecated
``seac`` form of ``endchar`` (one warning per font; the glyph's own contours are drawn).  Refused: an ``OTTO`` font without a
``CFF `` table (``CFF2`` is named when that is what it has), a CFF major version other than 1, more than one font in the table,
``CharstringType`` 1, the ``random`` operator.

The Type 2 machine: the current point starts at (0, 0) and is a running sum in double, every delta added in charstring order, x
and y apart -- exact for integer and 16.16 operands.  A glyph decodes to contours of absolute points with a kind each: 0 MOVE,
1 LINE, 2 C1, 3 C2 (a cubic's control points), 4 CURVE (its end point).  A moveto or ``endchar`` ends the open contour; a drawing
operator before any moveto begins one at the current point.  A flex is two cubics, its depth dropped.
"""
from __future__ import annotations

import math
import os
import struct
import warnings

import numpy as np

from . import _abi
from .truetype import SFNT_CFF, SfntFont, TrueTypeGlyph, _IDENTITY, _directory, _reader, read_ttf

MOVE, LINE, C1, C2, CURVE = 0, 1, 2, 3, 4
MAX_STACK = 48         # operands of a charstring (and of a DICT)
MAX_NESTING = 10       # subroutine calls inside one another
MAX_OPS = 1 << 18      # operators executed for one glyph: bounds a subroutine bomb of 10 levels of fan-out
N_TRANSIENT = 32

# Top DICT / Private DICT operators (two-byte operators 12 x as 1200 + x)
_CHARSTRINGS, _PRIVATE, _SUBRS = 17, 18, 19
_CHARSTRING_TYPE, _FONT_MATRIX, _ROS, _FDARRAY, _FDSELECT = 1206, 1207, 1230, 1236, 1237


def is_cff(head: bytes) -> bool:
    """Whether a file that begins with `head` is an sfnt with CFF outlines."""
    return bytes(head[:4]) == SFNT_CFF


def _need(data, off: int, size: int, what: str) -> None:
    if off < 0 or size < 0 or off + size > len(data):
        raise ValueError(f"opentype: CFF: {what}: {size} bytes at {off} leave the {len(data)} bytes there are")


class _Index:
    """An INDEX of the table `data` at `off`: `count`, `end` (the first byte behind it) and `item(i)`, the (begin, end) of object
    i in `data`.  Count 0 is the 2-byte empty form; offSize 1 to 4; the offsets begin at 1, do not decrease and stay inside."""

    __slots__ = ("count", "end", "_base", "_offsets")

    def __init__(self, data, off: int, what: str):
        _need(data, off, 2, f"{what} INDEX")
        self.count, = struct.unpack_from(">H", data, off)
        self._base, self._offsets = off + 2, None
        if self.count == 0:
            self.end = off + 2
            return
        _need(data, off + 2, 1, f"{what} INDEX")
        size = data[off + 2]
        if not 1 <= size <= 4:
            raise ValueError(f"opentype: CFF: {what} INDEX: offSize {size}")
        _need(data, off + 3, (self.count + 1) * size, f"{what} INDEX offsets")
        raw = np.frombuffer(data, dtype=np.uint8, count=(self.count + 1) * size, offset=off + 3).reshape(-1, size).astype(np.int64)
        offsets = np.zeros(self.count + 1, dtype=np.int64)
        for b in range(size):
            offsets = offsets * 256 + raw[:, b]
        self._base = off + 3 + (self.count + 1) * size - 1   # (offset 1 is the first byte behind the offset array)
        if int(offsets[0]) != 1 or (np.diff(offsets) < 0).any() or self._base + int(offsets[-1]) > len(data):
            raise ValueError(f"opentype: CFF: {what} INDEX: the offsets do not begin at 1, decrease or leave the data")
        self._offsets = offsets.tolist()
        self.end = self._base + self._offsets[-1]

    def item(self, i: int):
        return self._base + self._offsets[i], self._base + self._offsets[i + 1]


def _real(data, at: int, end: int, what: str):
    """A DICT's real number (operator 30, packed BCD) at `at`: (value, the byte behind it)."""
    text = ""
    while True:
        if at >= end:
            raise ValueError(f"opentype: CFF: {what}: a real number runs out of the DICT")
        byte = data[at]
        at += 1
        for nibble in (byte >> 4, byte & 15):
            if nibble == 15:
                try:
                    value = float(text)
                except ValueError:
                    raise ValueError(f"opentype: CFF: {what}: a real number written {text!r}") from None
                if not math.isfinite(value):   # (1E999: nothing later has to think of inf or nan)
                    raise ValueError(f"opentype: CFF: {what}: a real number written {text!r} is not finite")
                return value, at
            if nibble == 13:
                raise ValueError(f"opentype: CFF: {what}: a real number with the reserved nibble 13")
            text += "0123456789.EE?-"[nibble] if nibble != 12 else "E-"
            if len(text) > 64:
                raise ValueError(f"opentype: CFF: {what}: a real number of more than 64 characters")


def _read_dict(data, begin: int, end: int, what: str) -> dict:
    """``{operator: [operands]}`` of the DICT in ``data[begin:end]``; a two-byte operator 12 x has the key 1200 + x."""
    out, stack, at = {}, [], begin
    while at < end:
        b = data[at]
        at += 1
        if b <= 21:
            if b == 12:
                if at >= end:
                    raise ValueError(f"opentype: CFF: {what}: an operator runs out of the DICT")
                b = 1200 + data[at]
                at += 1
            out.setdefault(b, stack)
            stack = []
            continue
        if b == 28:
            if at + 2 > end:
                raise ValueError(f"opentype: CFF: {what}: an operand runs out of the DICT")
            value = struct.unpack_from(">h", data, at)[0]
            at += 2
        elif b == 29:
            if at + 4 > end:
                raise ValueError(f"opentype: CFF: {what}: an operand runs out of the DICT")
            value = struct.unpack_from(">i", data, at)[0]
            at += 4
        elif b == 30:
            value, at = _real(data, at, end, what)
        elif 32 <= b <= 246:
            value = b - 139
        elif 247 <= b <= 254:
            if at >= end:
                raise ValueError(f"opentype: CFF: {what}: an operand runs out of the DICT")
            value = (b - 247) * 256 + data[at] + 108 if b <= 250 else -(b - 251) * 256 - data[at] - 108
            at += 1
        else:
            raise ValueError(f"opentype: CFF: {what}: the reserved byte {b}")
        if len(stack) >= MAX_STACK:
            raise ValueError(f"opentype: CFF: {what}: more than {MAX_STACK} operands")
        stack.append(value)
    return out


def _offset(d: dict, op: int, n: int, what: str):
    """The `n` integer operands of operator `op` of a DICT, or None without the operator."""
    args = d.get(op)
    if args is None:
        return None
    if len(args) != n or any(isinstance(a, float) and a != int(a) for a in args):
        raise ValueError(f"opentype: CFF: {what}: {len(args)} operands where {n} whole numbers are needed")
    return [int(a) for a in args]


class CFFOutline:
    """A decoded glyph: `xy` (n, 2) float64 absolute points in font units, `kind` (n,) uint8, `ends` (contours,) int32, the last
    point of each contour."""

    __slots__ = ("xy", "kind", "ends")

    def __init__(self, xy, kind, ends):
        self.xy, self.kind, self.ends = xy, kind, ends

    def contours(self) -> list:
        """``[[(x, y, kind)]]``."""
        out, first = [], 0
        for end in self.ends.tolist():
            out.append([(float(x), float(y), int(k)) for (x, y), k in zip(self.xy[first:end + 1].tolist(), self.kind[first:end + 1].tolist())])
            first = end + 1
        return out


class CFFGlyph(TrueTypeGlyph):
    """A glyph of a ``CFFFont``: `gid`, its advance, and `path` / `arrays` in glyph units (y up), made on the device on first use
    (pen 0, sx = sy = 1).  Its one part is the glyph itself under the identity matrix: CFF has no composites."""

    __slots__ = []

    def __repr__(self) -> str:
        return f"CFFGlyph(unicode={self.unicode}, gid={self.gid})"


class CFFFont(SfntFont):
    """A face read from an ``.otf`` with CFF outlines (``read_otf``).  `hkern` is ``TrueTypeFont``'s: from ``kern`` when present."""

    __slots__ = ["cff", "is_cid", "_charstrings", "_gsubrs", "_fd_subrs", "_fd_select", "_decoded", "_warned_seac"]
    GLYPH = CFFGlyph

    def __init__(self, data: bytes, family=None):
        self.data = data = bytes(data)
        with _reader("opentype"):   # (the shared sfnt code path: its messages name this reader)
            self.tables = tables = _directory(data, cff=True)
        if "CFF " not in tables:
            cause = "it has a CFF2 table, and CFF version 2 is not read" if "CFF2" in tables else "there are no outlines to read"
            raise ValueError(f"opentype: an OTTO font without a CFF table: {cause}")
        with _reader("opentype"):
            units, mac_style, _loc_format, ascent, descent = self._read_metrics(loca=False)
        off, length = tables["CFF "]
        self.cff = cff = data[off:off + length]   # (every offset of the table is relative to its start, and checked against it)
        self._read_cff(cff, units)
        with _reader("opentype"):
            self._read_naming(family, units, mac_style, ascent, descent)
        self._decoded, self._warned_seac = {}, False
        self.missing_glyph = self.glyph(0, None)

    # -- the CFF table ---------------------------------------------------------------------------------------------------
    def _read_cff(self, cff: bytes, units: int) -> None:
        _need(cff, 0, 4, "header")
        major, _minor, header_size, _off_size = cff[0], cff[1], cff[2], cff[3]
        if major != 1:
            raise ValueError(f"opentype: CFF: header: major version {major}, only version 1 is read")
        if header_size < 4:
            raise ValueError(f"opentype: CFF: header: hdrSize {header_size}")
        names = _Index(cff, header_size, "Name")
        if names.count != 1:
            raise ValueError(f"opentype: CFF: Name INDEX: {names.count} fonts in the table, one is read")
        tops = _Index(cff, names.end, "Top DICT")
        if tops.count != 1:
            raise ValueError(f"opentype: CFF: Top DICT INDEX: {tops.count} DICTs for 1 font")
        strings = _Index(cff, tops.end, "String")
        self._gsubrs = _Index(cff, strings.end, "Global Subr")
        top = _read_dict(cff, *tops.item(0), "Top DICT")
        kind = top.get(_CHARSTRING_TYPE, [2])
        if kind != [2]:
            raise ValueError(f"opentype: CFF: Top DICT: CharstringType {kind[0] if len(kind) == 1 else kind}, only Type 2 charstrings are read")
        at = _offset(top, _CHARSTRINGS, 1, "Top DICT: CharStrings")
        if at is None:
            raise ValueError("opentype: CFF: Top DICT: no CharStrings")
        self._charstrings = _Index(cff, at[0], "CharStrings")
        if self._charstrings.count != self.n_glyphs:
            raise ValueError(f"opentype: CFF: CharStrings INDEX: {self._charstrings.count} charstrings where maxp has {self.n_glyphs} glyphs")
        matrix = top.get(_FONT_MATRIX, [0.001, 0.0, 0.0, 0.001, 0.0, 0.0])
        want = 1.0 / units
        if (len(matrix) != 6 or any(abs(matrix[i] - want) > 1e-6 * want for i in (0, 3)) or any(matrix[i] != 0 for i in (1, 2, 4, 5))):
            warnings.warn(f"opentype: CFF: FontMatrix {matrix} is not applied: the scale is 1 / unitsPerEm = 1 / {units}")
        self.is_cid = _ROS in top or _FDARRAY in top
        if self.is_cid:
            at = _offset(top, _FDARRAY, 1, "Top DICT: FDArray")
            if at is None:
                raise ValueError("opentype: CFF: Top DICT: a CID-keyed font (ROS) without FDArray")
            fonts = _Index(cff, at[0], "FDArray")
            if not 1 <= fonts.count <= 256:
                raise ValueError(f"opentype: CFF: FDArray INDEX: {fonts.count} Font DICTs")
            self._fd_subrs = [self._local_subrs(cff, _read_dict(cff, *fonts.item(i), f"Font DICT {i}"), f"Font DICT {i}") for i in range(fonts.count)]
            at = _offset(top, _FDSELECT, 1, "Top DICT: FDSelect")
            if at is None:
                raise ValueError("opentype: CFF: Top DICT: a CID-keyed font without FDSelect")
            self._fd_select = self._read_fd_select(cff, at[0], fonts.count)
        else:
            self._fd_subrs = [self._local_subrs(cff, top, "Top DICT")]
            self._fd_select = None

    @staticmethod
    def _local_subrs(cff: bytes, d: dict, what: str):
        """The Subrs INDEX of the Private DICT that the DICT `d` names, or None."""
        private = _offset(d, _PRIVATE, 2, f"{what}: Private")
        if private is None:
            return None
        size, off = private
        _need(cff, off, size, f"{what}: Private DICT")
        subrs = _offset(_read_dict(cff, off, off + size, "Private DICT"), _SUBRS, 1, "Private DICT: Subrs")
        return None if subrs is None else _Index(cff, off + subrs[0], "Subrs")   # (relative to the Private DICT)

    def _read_fd_select(self, cff: bytes, at: int, n_fonts: int) -> np.ndarray:
        """The Font DICT of every glyph (uint8)."""
        _need(cff, at, 1, "FDSelect")
        n = self.n_glyphs
        if cff[at] == 0:
            _need(cff, at + 1, n, "FDSelect format 0")
            select = np.frombuffer(cff, dtype=np.uint8, count=n, offset=at + 1).copy()
        elif cff[at] == 3:
            _need(cff, at + 1, 2, "FDSelect format 3")
            n_ranges, = struct.unpack_from(">H", cff, at + 1)
            _need(cff, at + 3, 3 * n_ranges + 2, "FDSelect format 3 ranges")
            firsts = [struct.unpack_from(">H", cff, at + 3 + 3 * i)[0] for i in range(n_ranges + 1)]
            if n_ranges < 1 or firsts[0] != 0 or firsts[-1] != n or any(b <= a for a, b in zip(firsts, firsts[1:])):
                raise ValueError("opentype: CFF: FDSelect format 3: ranges that do not begin at glyph 0, increase and end at the glyph count")
            select = np.zeros(n, dtype=np.uint8)
            for i in range(n_ranges):
                select[firsts[i]:firsts[i + 1]] = cff[at + 5 + 3 * i]
        else:
            raise ValueError(f"opentype: CFF: FDSelect: format {cff[at]}")
        if n and int(select.max()) >= n_fonts:
            raise ValueError(f"opentype: CFF: FDSelect: Font DICT {int(select.max())} of {n_fonts}")
        return select

    # -- glyphs ----------------------------------------------------------------------------------------------------------
    def outline_of(self, gid: int) -> CFFOutline:
        """The contours of a glyph, decoded on first use."""
        glyph = self._decoded.get(gid)
        if glyph is None:
            if not 0 <= gid < self.n_glyphs:
                raise ValueError(f"opentype: CFF: glyph {gid} of {self.n_glyphs}")
            glyph = self._decoded[gid] = self._run(gid)
        return glyph

    def glyph_parts(self, gid: int) -> list:
        """``[(glyph id, 1, 0, 0, 1, 0, 0)]``; an empty glyph has no part."""
        return [(gid, *_IDENTITY)] if len(self.outline_of(gid).kind) else []

    def outline(self, parts, sx: float, sy: float):
        """(types, params (n, 8), sizes) of `parts`, ``[((glyph id, m00, m01, m10, m11, dx, dy), pen)]``, through the device."""
        index, atlas = {}, []
        for part, _pen in parts:
            if part[0] not in index:
                index[part[0]] = len(atlas)
                atlas.append(self.outline_of(part[0]))
        n = len(parts)
        contour_off, glyph_contour_off, points = [0], [0], 0
        for glyph in atlas:
            contour_off.extend((glyph.ends.astype(np.int64) + 1 + points).tolist())
            points += len(glyph.kind)
            glyph_contour_off.append(len(contour_off) - 1)
        return _abi.cff_outline(
            pt_xy=np.concatenate([g.xy for g in atlas]) if atlas else np.zeros((0, 2), np.float64),
            pt_kind=np.concatenate([g.kind for g in atlas]) if atlas else np.zeros(0, np.uint8),
            contour_off=contour_off, glyph_contour_off=glyph_contour_off, part_glyph=[index[part[0]] for part, _pen in parts],
            part_m=np.array([part[1:] for part, _pen in parts], dtype=np.float64).reshape(n, 6),
            part_pen=np.array([pen for _part, pen in parts], dtype=np.float64), part_sx=np.full(n, float(sx)), part_sy=np.full(n, float(sy)))

    # -- the Type 2 machine ------------------------------------------------------------------------------------------------
    def _run(self, gid: int) -> CFFOutline:
        cff = self.cff
        gsubrs = self._gsubrs
        subrs = self._fd_subrs[int(self._fd_select[gid]) if self._fd_select is not None else 0]

        def bad(why):
            return ValueError(f"opentype: CFF: charstring of glyph {gid}: {why}")

        stack: list = []
        transient = [0.0] * N_TRANSIENT
        contours, open_contour = [], None
        x = y = 0.0
        stems, width_seen, ops = 0, False, 0
        frames = []                                  # the callers: (at, end)
        at, end = self._charstrings.item(gid)

        def drop_width(odd: bool):
            """The optional width in front of the first stack-clearing operator: there when the count's parity is `odd`."""
            nonlocal width_seen
            if not width_seen:
                width_seen = True
                if stack and (len(stack) % 2 == 1) == odd:
                    del stack[0]

        def take(n: int):
            if len(stack) < n:
                raise bad(f"stack underflow: {len(stack)} operands where {n} are needed")

        def close():
            nonlocal open_contour
            if open_contour is not None:
                contours.append(open_contour)
                open_contour = None

        def move(dx, dy):
            nonlocal x, y, open_contour
            close()
            x += dx
            y += dy
            open_contour = [(x, y, MOVE)]

        def point(dx, dy, kind):
            nonlocal x, y, open_contour
            if open_contour is None:
                open_contour = [(x, y, MOVE)]
            x += dx
            y += dy
            open_contour.append((x, y, kind))

        def line(dx, dy):
            point(dx, dy, LINE)

        def curve(dxa, dya, dxb, dyb, dxc, dyc):
            point(dxa, dya, C1)
            point(dxb, dyb, C2)
            point(dxc, dyc, CURVE)

        def alternating_curves(args, horizontal: bool):
            """hvcurveto / vhcurveto: curves that begin and end along the axes in turn; one more operand ends the last obliquely."""
            n = len(args)
            if n < 4 or n % 4 not in (0, 1):
                raise bad(f"{n} operands for hvcurveto / vhcurveto")
            i = 0
            while i + 4 <= n:
                a, b, c, d = args[i:i + 4]
                last = args[i + 4] if n - i == 5 else 0.0
                if horizontal:
                    curve(a, 0.0, b, c, last, d)
                else:
                    curve(0.0, a, b, c, d, last)
                horizontal = not horizontal
                i += 4

        while True:
            if at >= end:
                raise bad("it ends without endchar" if not frames else "a subroutine ends without return")
            b = cff[at]
            at += 1
            # ---- numbers
            if b >= 32 or b == 28:
                if b == 28:
                    if at + 2 > end:
                        raise bad("an operand runs out of the charstring")
                    value = float(struct.unpack_from(">h", cff, at)[0])
                    at += 2
                elif b <= 246:
                    value = float(b - 139)
                elif b <= 254:
                    if at >= end:
                        raise bad("an operand runs out of the charstring")
                    value = float((b - 247) * 256 + cff[at] + 108 if b <= 250 else -(b - 251) * 256 - cff[at] - 108)
                    at += 1
                else:
                    if at + 4 > end:
                        raise bad("an operand runs out of the charstring")
                    value = struct.unpack_from(">i", cff, at)[0] / 65536.0
                    at += 4
                if len(stack) >= MAX_STACK:
                    raise bad(f"operand stack deeper than {MAX_STACK}")
                stack.append(value)
                continue
            # ---- operators
            ops += 1
            if ops > MAX_OPS:
                raise bad(f"more than {MAX_OPS} operators executed")
            if b == 12:
                if at >= end:
                    raise bad("an operator runs out of the charstring")
                b = 1200 + cff[at]
                at += 1
            if b in (1, 3, 18, 23):                    # hstem vstem hstemhm vstemhm
                drop_width(odd=True)
                stems += len(stack) // 2
                stack.clear()
            elif b in (19, 20):                        # hintmask cntrmask: the implied vstem, then the mask
                drop_width(odd=True)
                stems += len(stack) // 2
                stack.clear()
                at += (stems + 7) // 8
                if at > end:
                    raise bad("a hint mask runs out of the charstring")
            elif b == 21:                              # rmoveto
                drop_width(odd=True)
                take(2)
                move(stack[-2], stack[-1])
                stack.clear()
            elif b in (22, 4):                         # hmoveto vmoveto
                drop_width(odd=False)
                take(1)
                move(*((stack[-1], 0.0) if b == 22 else (0.0, stack[-1])))
                stack.clear()
            elif b == 5:                               # rlineto
                take(2)
                if len(stack) % 2:
                    raise bad(f"{len(stack)} operands for rlineto")
                for i in range(0, len(stack), 2):
                    line(stack[i], stack[i + 1])
                stack.clear()
            elif b in (6, 7):                          # hlineto vlineto: alternating
                take(1)
                horizontal = b == 6
                for value in stack:
                    line(*((value, 0.0) if horizontal else (0.0, value)))
                    horizontal = not horizontal
                stack.clear()
            elif b == 8:                               # rrcurveto
                take(6)
                if len(stack) % 6:
                    raise bad(f"{len(stack)} operands for rrcurveto")
                for i in range(0, len(stack), 6):
                    curve(*stack[i:i + 6])
                stack.clear()
            elif b in (27, 26):                        # hhcurveto vvcurveto
                take(4)
                if len(stack) % 4 not in (0, 1):
                    raise bad(f"{len(stack)} operands for hhcurveto / vvcurveto")
                first = stack.pop(0) if len(stack) % 4 else 0.0
                for i in range(0, len(stack), 4):
                    a, c, d, e = stack[i:i + 4]
                    if b == 27:
                        curve(a, first, c, d, e, 0.0)
                    else:
                        curve(first, a, c, d, 0.0, e)
                    first = 0.0
                stack.clear()
            elif b in (31, 30):                        # hvcurveto vhcurveto
                alternating_curves(stack, b == 31)
                stack.clear()
            elif b == 24:                              # rcurveline
                take(8)
                if (len(stack) - 2) % 6:
                    raise bad(f"{len(stack)} operands for rcurveline")
                for i in range(0, len(stack) - 2, 6):
                    curve(*stack[i:i + 6])
                line(stack[-2], stack[-1])
                stack.clear()
            elif b == 25:                              # rlinecurve
                take(8)
                if (len(stack) - 6) % 2:
                    raise bad(f"{len(stack)} operands for rlinecurve")
                for i in range(0, len(stack) - 6, 2):
                    line(stack[i], stack[i + 1])
                curve(*stack[-6:])
                stack.clear()
            elif b in (10, 29):                        # callsubr callgsubr
                take(1)
                index = subrs if b == 10 else gsubrs
                count = index.count if index is not None else 0
                number = stack.pop()
                bias = 107 if count < 1240 else 1131 if count < 33900 else 32768
                if number != int(number) or not 0 <= int(number) + bias < count:
                    raise bad(f"{'local' if b == 10 else 'global'} subroutine {number} + {bias} outside its INDEX of {count}")
                if len(frames) >= MAX_NESTING:
                    raise bad(f"subroutines nested deeper than {MAX_NESTING}")
                frames.append((at, end))
                at, end = index.item(int(number) + bias)
            elif b == 11:                              # return
                if not frames:
                    raise bad("return outside a subroutine")
                at, end = frames.pop()
            elif b == 14:                              # endchar
                drop_width(odd=True)
                if len(stack) == 4 and not self._warned_seac:
                    self._warned_seac = True
                    warnings.warn(f"opentype: CFF: {self.family}: endchar with four operands (seac) draws the glyph's own contours only")
                close()
                break
            elif b >= 1200:                            # the two-byte operators: the flexes, then arithmetic and storage, in double
                if b == 1235:                              # flex: two cubics, the depth dropped
                    take(13)
                    curve(*stack[0:6])
                    curve(*stack[6:12])
                    stack.clear()
                elif b == 1234:                            # hflex
                    take(7)
                    dx1, dx2, dy2, dx3, dx4, dx5, dx6 = stack[:7]
                    curve(dx1, 0.0, dx2, dy2, dx3, 0.0)
                    curve(dx4, 0.0, dx5, -dy2, dx6, 0.0)
                    stack.clear()
                elif b == 1236:                            # hflex1
                    take(9)
                    dx1, dy1, dx2, dy2, dx3, dx4, dx5, dy5, dx6 = stack[:9]
                    curve(dx1, dy1, dx2, dy2, dx3, 0.0)
                    curve(dx4, 0.0, dx5, dy5, dx6, -(dy1 + dy2 + dy5))
                    stack.clear()
                elif b == 1237:                            # flex1
                    take(11)
                    dx1, dy1, dx2, dy2, dx3, dy3, dx4, dy4, dx5, dy5, d6 = stack[:11]
                    dx, dy = dx1 + dx2 + dx3 + dx4 + dx5, dy1 + dy2 + dy3 + dy4 + dy5
                    curve(dx1, dy1, dx2, dy2, dx3, dy3)
                    if abs(dx) > abs(dy):
                        curve(dx4, dy4, dx5, dy5, d6, -dy)
                    else:
                        curve(dx4, dy4, dx5, dy5, -dx, d6)
                    stack.clear()
                elif b == 1203:                            # and
                    take(2)
                    c = stack.pop()
                    stack[-1] = 1.0 if stack[-1] != 0 and c != 0 else 0.0
                elif b == 1204:                            # or
                    take(2)
                    c = stack.pop()
                    stack[-1] = 1.0 if stack[-1] != 0 or c != 0 else 0.0
                elif b == 1205:                            # not
                    take(1)
                    stack[-1] = 1.0 if stack[-1] == 0 else 0.0
                elif b == 1209:                            # abs
                    take(1)
                    stack[-1] = abs(stack[-1])
                elif b == 1210:                            # add
                    take(2)
                    c = stack.pop()
                    stack[-1] = stack[-1] + c
                elif b == 1211:                            # sub
                    take(2)
                    c = stack.pop()
                    stack[-1] = stack[-1] - c
                elif b == 1212:                            # div
                    take(2)
                    c = stack.pop()
                    if c == 0:
                        raise bad("div by zero")
                    stack[-1] = stack[-1] / c
                elif b == 1214:                            # neg
                    take(1)
                    stack[-1] = -stack[-1]
                elif b == 1215:                            # eq
                    take(2)
                    c = stack.pop()
                    stack[-1] = 1.0 if stack[-1] == c else 0.0
                elif b == 1218:                            # drop
                    take(1)
                    stack.pop()
                elif b == 1220:                            # put
                    take(2)
                    i = stack.pop()
                    value = stack.pop()
                    if i != int(i) or not 0 <= int(i) < N_TRANSIENT:
                        raise bad(f"put at {i} of the {N_TRANSIENT} transient entries")
                    transient[int(i)] = value
                elif b == 1221:                            # get
                    take(1)
                    i = stack[-1]
                    if i != int(i) or not 0 <= int(i) < N_TRANSIENT:
                        raise bad(f"get at {i} of the {N_TRANSIENT} transient entries")
                    stack[-1] = transient[int(i)]
                elif b == 1222:                            # ifelse: s1 s2 v1 v2 -> s1 when v1 <= v2, else s2
                    take(4)
                    v2, v1, s2 = stack.pop(), stack.pop(), stack.pop()
                    if not v1 <= v2:
                        stack[-1] = s2
                elif b == 1223:
                    raise bad("the random operator is not run")
                elif b == 1224:                            # mul
                    take(2)
                    c = stack.pop()
                    stack[-1] = stack[-1] * c
                elif b == 1226:                            # sqrt
                    take(1)
                    if stack[-1] < 0:
                        raise bad("sqrt of a negative number")
                    stack[-1] = math.sqrt(stack[-1])
                elif b == 1227:                            # dup
                    take(1)
                    if len(stack) >= MAX_STACK:
                        raise bad(f"operand stack deeper than {MAX_STACK}")
                    stack.append(stack[-1])
                elif b == 1228:                            # exch
                    take(2)
                    stack[-1], stack[-2] = stack[-2], stack[-1]
                elif b == 1229:                            # index: a negative one counts as 0
                    take(1)
                    i = stack.pop()
                    i = 0 if i < 0 else int(i)
                    take(i + 1)
                    stack.append(stack[-1 - i])
                elif b == 1230:                            # roll: n j -> the top n turned by j, positive towards the top
                    take(2)
                    j, n = stack.pop(), stack.pop()
                    if n != int(n) or j != int(j) or n < 0:
                        raise bad(f"roll of {n} by {j}")
                    n, j = int(n), int(j)
                    take(n)
                    if n:
                        j %= n
                        top = stack[len(stack) - n:]
                        stack[len(stack) - n:] = top[n - j:] + top[:n - j]
                else:
                    raise bad(f"unknown operator 12 {b - 1200}")
            else:
                raise bad(f"unknown operator {b}")
            if stack and not math.isfinite(stack[-1]):
                raise bad("a number that is not finite")
        pts = [p for c in contours for p in c]
        if not pts:
            return _EMPTY
        ends = np.cumsum([len(c) for c in contours]).astype(np.int32) - 1
        xy = np.array([(p[0], p[1]) for p in pts], dtype=np.float64).reshape(-1, 2)
        if not np.isfinite(xy).all():
            raise bad("a coordinate that is not finite")
        return CFFOutline(xy, np.array([p[2] for p in pts], dtype=np.uint8), ends)

    def __repr__(self) -> str:
        return f'CFFFont(family="{self.family}", weight={self.weight}, style={self.style}, glyphs_count={self.n_glyphs})'


_EMPTY = CFFOutline(np.zeros((0, 2), np.float64), np.zeros(0, np.uint8), np.zeros(0, np.int32))


def read_otf(data: bytes, family: "str | None" = None) -> CFFFont:
    """Parse an OpenType font with CFF outlines (the module's docstring says what is read).  `family` replaces the family of the
    ``name`` table; a font that has none needs it."""
    font = CFFFont(data, family)
    if font.family is None:
        raise ValueError("opentype: the font names no family (name id 1): pass family=")
    return font


def read_otf_file(path: str, family: "str | None" = None) -> CFFFont:
    """`read_otf` of a file; a font that names no family takes the file's name without its extension."""
    with open(path, "rb") as f:
        data = f.read()
    font = CFFFont(data, family)
    if font.family is None:
        font.family = os.path.splitext(os.path.basename(path))[0]
    return font


def read_font(data: bytes, family: "str | None" = None):
    """`read_ttf` or `read_otf`, picked by the first four bytes: ``OTTO`` is read as CFF, anything else is `read_ttf`'s to read or
    to refuse."""
    data = bytes(data)
    return read_otf(data, family) if is_cff(data) else read_ttf(data, family)
