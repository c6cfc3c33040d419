"""TrueType fonts (beyond the reference, which knows SVG fonts only): ``read_ttf`` parses a ``.ttf`` into a ``TrueTypeFont``,
a ``fonts.Font`` whose glyph outlines come from the ``glyf`` table instead of ``<glyph d="...">``.

Host code, pure Python + numpy: the tables are parsed here, the contours become path segments on the device
(``_abi.glyf_outline``, svgr_glyf_outline; one lane per point).  Measuring a string -- ``str_to_glyphs``, host arithmetic from
``hmtx`` / ``kern`` -- needs no device, so loading a document does not either.

Read: an sfnt with TrueType outlines (version ``0x00010000`` or ``true``) and its tables ``head`` (unitsPerEm, indexToLocFormat,
macStyle), ``maxp`` (glyph count), ``hhea`` + ``hmtx`` (ascent, descent, advances; a glyph id at or beyond numberOfHMetrics takes
the last advance), ``cmap`` (formats 4 and 12; platform 3 encoding 10 before 3 / 1 before platform 0), ``loca`` + ``glyf``,
``name`` (id 1, the family: platform 3 as UTF-16BE, else platform 1 as Latin-1), ``OS/2`` (usWeightClass; fsSelection bit 0 or
macStyle bit 1 make the style ``italic``; without the table the weight is 700 with macStyle bit 0, else 400) and ``kern``
(format 0, horizontal, not cross-stream; optional).

Refused with a ``ValueError`` that says which: ``ttcf`` collections, WOFF / WOFF2, a font without one of
``head maxp hhea hmtx cmap loca glyf``, and, by ``read_ttf``, ``OTTO`` (CFF outlines: ``opentype_cff.read_otf`` reads those, and
``read_font`` picks the reader by the first four bytes; the sfnt tables around the outlines are read by ``SfntFont`` here for both).

Ignored: hinting (``fpgm``, ``prep``, ``cvt`` and the glyphs' instructions are skipped over, never interpreted), ``GSUB`` / ``GPOS``
(no ligatures, no shaping, no GPOS kerning), vertical metrics, bitmaps and colour tables.  One glyph per character; a character the ``cmap`` does not map takes glyph 0 (``.notdef``).

A font file is untrusted: every offset, length and count is checked against the data before it is used, and a malformed
file raises ``ValueError`` -- when it is read or, for a glyph's outline, when that glyph is first used (glyphs are decoded
lazily).  Nothing is allocated by the size a field claims.

Composite glyphs are flattened on the host into parts ``(simple glyph id, m00, m01, m10, m11, dx, dy)`` in font units, a point
(x, y) of the simple glyph going to ``x' = (m00 x + m10 y) + dx``, ``y' = (m01 x + m11 y) + dy``.  A component C inside a
composite that is itself placed by P gives, in this order of operations,
``n00 = c00 p00 + c01 p10``, ``n01 = c00 p01 + c01 p11``, ``n10 = c10 p00 + c11 p10``, ``n11 = c10 p01 + c11 p11``,
``ndx = (cdx p00 + cdy p10) + pdx``, ``ndy = (cdx p01 + cdy p11) + pdy``.
ARG_1_AND_2_ARE_WORDS, ARGS_ARE_XY_VALUES, the three scale forms (F2Dot14) and MORE_COMPONENTS are handled;
SCALED_COMPONENT_OFFSET is ignored (offsets are unscaled, FreeType's and Microsoft's default); a component placed by point
matching warns once per font and gets the offset (0, 0); nesting deeper than 8, a cycle, or more than ``MAX_PARTS`` glyphs visited while flattening
(components and the composites that hold them) warn and leave the glyph empty; USE_MY_METRICS is ignored (the advance is the glyph's own ``hmtx`` entry).

Variable fonts (``fvar`` / ``avar`` / ``gvar``; ``truetype_var.py``): `TrueTypeFont.axes`, `is_variable`, and
`TrueTypeFont.instance`, the font at a position of its axes.  A font without ``fvar`` takes none of that code.
"""
from __future__ import annotations

import bisect
import os
import struct
import warnings

import numpy as np

from . import _abi
from .fonts import FONT_STYLE_NORMAL, Font, Glyph
from .geometry import Path

FONT_STYLE_ITALIC = "italic"
REQUIRED = ("head", "maxp", "hhea", "hmtx", "cmap", "loca", "glyf")
REQUIRED_CFF = ("head", "maxp", "hhea", "hmtx", "cmap")   # (and ``CFF ``, which opentype_cff.py asks for by name)
SFNT_CFF = b"OTTO"
REFUSED = {   # what `read_ttf` turns away by the first four bytes
    b"OTTO": "OTTO: an OpenType font with CFF outlines, read_ttf reads TrueType (glyf) outlines only: read_otf / read_font read it",
    b"ttcf": "ttcf: a TrueType collection, only single fonts are read",
    b"wOFF": "wOFF: a WOFF container, only plain sfnt files are read",
    b"wOF2": "wOF2: a WOFF2 container, only plain sfnt files are read",
}
SFNT_TRUETYPE = (b"\x00\x01\x00\x00", b"true")
MAX_DEPTH = 8       # nesting of composite glyphs
MAX_PARTS = 4096    # glyphs visited while one composite glyph is flattened (its parts and the composites that hold them)

# simple glyph flags
_ON, _X_SHORT, _Y_SHORT, _REPEAT, _X_SAME, _Y_SAME = 1, 2, 4, 8, 16, 32
# component flags
_WORDS, _XY, _SCALE, _MORE, _XY_SCALE, _TWO_BY_TWO = 0x1, 0x2, 0x8, 0x20, 0x40, 0x80

_IDENTITY = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)


def is_truetype(head: bytes) -> bool:
    """Whether a file that begins with `head` is an sfnt with TrueType outlines."""
    return bytes(head[:4]) in SFNT_TRUETYPE


def _need(data, off: int, size: int, what: str) -> None:
    if off < 0 or size < 0 or off + size > len(data):
        raise ValueError(f"truetype: {what}: {size} bytes at {off} leave the {len(data)} bytes there are")


def _unpack(fmt: str, data, off: int, what: str):
    _need(data, off, struct.calcsize(fmt), what)
    return struct.unpack_from(fmt, data, off)


def _array(data, dtype: str, off: int, count: int, what: str) -> np.ndarray:
    _need(data, off, count * np.dtype(dtype).itemsize, what)
    return np.frombuffer(data, dtype=dtype, count=count, offset=off)


class SimpleGlyph:
    """A decoded simple glyph: `xy` (n, 2) int16, `on` (n,) uint8, `ends` (contours,) int32, the last point of each contour."""

    __slots__ = ("xy", "on", "ends")

    def __init__(self, xy, on, ends):
        self.xy, self.on, self.ends = xy, on, ends


_EMPTY = SimpleGlyph(np.zeros((0, 2), np.int16), np.zeros(0, np.uint8), np.zeros(0, np.int32))


class TrueTypeGlyph(Glyph):
    """A glyph of a ``TrueTypeFont``: `gid`, its advance, and `path` / `arrays` in glyph units (y up), made on the device on
    first use (pen 0, sx = sy = 1)."""

    __slots__ = ["font", "gid"]

    def __init__(self, font, gid: int, unicode, advance: float):
        super().__init__(unicode, advance, None, name=f"gid{gid}")
        self.font, self.gid = font, gid

    @property
    def parts(self) -> list:
        return self.font.glyph_parts(self.gid)

    @property
    def arrays(self):
        if self._arrays is None:
            self._arrays = self.font.outline([(part, 0.0) for part in self.parts], 1.0, 1.0)
        return self._arrays

    @property
    def path(self) -> Path:
        if self._path is None:
            self._path = Path.from_segments(*self.arrays)
        return self._path

    def __repr__(self) -> str:
        return f"TrueTypeGlyph(unicode={self.unicode}, gid={self.gid})"


class _reader:
    """Around the shared sfnt reading of a format other than TrueType: a ``ValueError`` of the shared code path names that
    format's reader (``opentype: head: ...``) in place of ``truetype:``.  `TrueTypeFont` does not use it: its messages are as
    they were."""

    def __init__(self, prefix: str):
        self.prefix = prefix

    def __enter__(self):
        return self

    def __exit__(self, kind, why, _trace):
        if kind is ValueError:
            text = str(why)
            text = text[len("truetype:"):].lstrip() if text.startswith("truetype:") else text
            raise ValueError(text if text.startswith(f"{self.prefix}:") else f"{self.prefix}: {text}") from None
        return False


class SfntFont(Font):
    """What the two outline formats of an sfnt share (``TrueTypeFont``; ``opentype_cff.CFFFont``): the table directory and the
    tables ``head``, ``maxp``, ``hhea`` + ``hmtx``, ``cmap``, ``name``, ``OS/2`` and ``kern``, read by one code path -- a format
    other than TrueType reads them inside ``_reader(prefix)``, which puts its own reader's name in front of the messages --, and
    the string measuring on top of them.  A subclass offers ``glyph_parts(gid)``
    and ``outline(parts, sx, sy)``; `GLYPH` is the type of its glyph objects."""

    __slots__ = ["data", "tables", "n_glyphs", "advances", "_cmap", "_by_gid"]
    GLYPH = None

    def _read_metrics(self, loca: bool):
        """``head``, ``maxp``, ``hhea``, ``hmtx`` of `self.data` / `self.tables`: sets `n_glyphs` and `advances`, returns
        (unitsPerEm, macStyle, indexToLocFormat, ascent, descent).  `loca`: the font has a ``loca`` table, whose format is checked."""
        data, tables = self.data, self.tables
        head, length = tables["head"]
        _need(data, head, 54, "head")
        if length < 54:
            raise ValueError("truetype: head: the table is shorter than 54 bytes")
        units, = _unpack(">H", data, head + 18, "head")
        mac_style, = _unpack(">H", data, head + 44, "head")
        loc_format, = _unpack(">h", data, head + 50, "head")
        if units < 1:
            raise ValueError("truetype: head: unitsPerEm is 0")
        if loca and loc_format not in (0, 1):
            raise ValueError(f"truetype: head: indexToLocFormat is {loc_format}")
        self.n_glyphs, = _unpack(">H", data, _table(tables, "maxp", 6) + 4, "maxp")   # (version 0.5, of a CFF font, has 6 bytes)
        if self.n_glyphs < 1:
            raise ValueError("truetype: maxp: the font has no glyph")
        hhea = _table(tables, "hhea", 36)
        ascent, descent = _unpack(">hh", data, hhea + 4, "hhea")
        n_metrics, = _unpack(">H", data, hhea + 34, "hhea")
        if n_metrics < 1:
            raise ValueError("truetype: hhea: numberOfHMetrics is 0")
        hmtx = _table(tables, "hmtx", 4 * n_metrics)
        self.advances = _array(data, ">u2", hmtx, 2 * n_metrics, "hmtx")[0::2].astype(np.int64)
        return units, mac_style, loc_format, ascent, descent

    def _read_naming(self, family, units, mac_style, ascent, descent) -> None:
        """``cmap``, ``OS/2``, ``name``, ``kern``, and with them ``Font.__init__``."""
        data, tables = self.data, self.tables
        self._cmap = _read_cmap(data, *tables["cmap"])
        weight, italic = (700 if mac_style & 1 else 400), bool(mac_style & 2)
        if "OS/2" in tables:
            os2 = _table(tables, "OS/2", 64)
            weight = _unpack(">H", data, os2 + 4, "OS/2")[0] or 400
            italic = italic or bool(_unpack(">H", data, os2 + 62, "OS/2")[0] & 1)
        if family is None and "name" in tables:
            family = _read_family(data, *tables["name"])
        kern = _read_kern(data, *tables["kern"]) if "kern" in tables else {}
        Font.__init__(self, family, weight, FONT_STYLE_ITALIC if italic else FONT_STYLE_NORMAL, float(ascent), float(descent), float(units),
                      hkern={pair: -float(value) for pair, value in kern.items()})
        self._by_gid = {}

    # -- cmap, metrics -------------------------------------------------------------------------------------------------
    def glyph_id(self, code: int) -> int:
        """The glyph of a character code; 0 (``.notdef``) when the cmap has none or names a glyph the font has not."""
        gid = self._cmap.lookup(code)
        return gid if 0 <= gid < self.n_glyphs else 0

    def cmap(self) -> dict:
        """``{character code: glyph id}`` of every mapped code (glyph 0 left out)."""
        out = {}
        for code in self._cmap.codes():
            gid = self.glyph_id(code)
            if gid:
                out[code] = gid
        return out

    def advance(self, gid: int) -> float:
        return float(self.advances[min(gid, len(self.advances) - 1)])

    def glyph(self, gid: int, char=None):
        glyph = self._by_gid.get(gid)
        if glyph is None:
            glyph = self._by_gid[gid] = self.GLYPH(self, gid, char, self.advance(gid))
            if char is not None:
                self.glyphs[char] = glyph
        return glyph

    def names(self) -> dict:
        return {g.name: g.unicode for g in self._by_gid.values()}

    def str_to_glyphs(self, string: str):
        """``([(pen x, glyph)], total advance)`` in font units: one glyph per character through the cmap, ``kern`` pairs by glyph
        id subtracted from the pen before the right glyph is placed.  Host arithmetic."""
        placed, pen, prev = [], 0.0, None
        for char in string:
            gid = self.glyph_id(ord(char))
            glyph = self.glyph(gid, char if gid else None)
            if prev is not None:
                kern = self.hkern.get((prev, gid))
                if kern is not None:
                    pen -= kern
            placed.append((pen, glyph))
            pen += glyph.advance
            prev = gid
        return placed, pen

    def str_to_path(self, size: float, string: str):
        """Outline of ``string`` at ``size`` user units per em, y flipped to the SVG's y-down: ``(Path, advance)``.  Eager, on the
        device: the parts of all glyphs go through the format's outline pass in one call, with sx = scale and sy = -scale."""
        scale = size / self.units_per_em
        placed, advance = self.str_to_glyphs(string)
        parts = [(part, pen) for pen, glyph in placed for part in glyph.parts]
        return Path.from_segments(*self.outline(parts, scale, -scale)), advance * scale


class TrueTypeFont(SfntFont):
    """A face read from a ``.ttf`` (``read_ttf``).  `hkern` maps ``(left glyph id, right glyph id)`` to what is subtracted from
    the pen, SVG's ``hkern k``: the negated value of the ``kern`` table."""

    __slots__ = ["loca", "_simple", "_parts", "_composite", "_warned_matching", "_var", "_instances"]
    GLYPH = TrueTypeGlyph

    def __init__(self, data: bytes, family=None):
        self.data = data = bytes(data)
        self.tables = tables = _directory(data)
        units, mac_style, loc_format, ascent, descent = self._read_metrics(loca=True)
        loca_off, loca_len = tables["loca"]
        glyf_len = tables["glyf"][1]
        if loc_format == 0:
            _table(tables, "loca", 2 * (self.n_glyphs + 1))
            self.loca = _array(data, ">u2", loca_off, self.n_glyphs + 1, "loca").astype(np.int64) * 2
        else:
            _table(tables, "loca", 4 * (self.n_glyphs + 1))
            self.loca = _array(data, ">u4", loca_off, self.n_glyphs + 1, "loca").astype(np.int64)
        if (np.diff(self.loca) < 0).any() or int(self.loca[-1]) > glyf_len:
            raise ValueError("truetype: loca: the offsets decrease or leave the glyf table")
        self._read_naming(family, units, mac_style, ascent, descent)
        self._simple, self._parts, self._composite = {}, {}, {}
        self._warned_matching = False
        self.missing_glyph = self.glyph(0, None)
        from . import truetype_var  # noqa: PLC0415  (truetype_var.py imports this module)

        self._var, self._instances = truetype_var.read_variations(self), {}

    # -- variable fonts ------------------------------------------------------------------------------------------------
    @property
    def axes(self) -> tuple:
        """The axes of a variable font, ``Axis(tag, minimum, default, maximum)`` in ``fvar`` order; empty for a static font."""
        return self._var.axes if self._var is not None else ()

    @property
    def is_variable(self) -> bool:
        return bool(self.axes)

    def instance(self, coords=None, **axes):
        """The font at a position of its axes, ``{tag: value}`` in user units as `coords` and / or as keywords
        (``font.instance(wght=650)``): a ``truetype_var.TrueTypeInstance``, made once per position; an axis not named stays at
        its default, a value is clamped to the axis' range, a tag the font does not have raises ``ValueError``.  With every axis
        at its default the result is the font itself."""
        from . import truetype_var  # noqa: PLC0415

        return truetype_var.instance(self, coords, axes)

    def glyph_deltas(self, gid: int, coords=None, **axes) -> np.ndarray:
        """(n, 2) float64: what the instance at `coords` adds to each of the n points of the simple glyph `gid` (a composite or
        empty glyph has none), on the device (svgr_gvar_deltas)."""
        from . import truetype_var  # noqa: PLC0415

        _user, normal = truetype_var.coordinates(self, coords, axes)
        glyph = self.simple_glyph(gid)
        if not len(glyph.on):
            return np.zeros((0, 2), dtype=np.float64)
        ends = glyph.ends.astype(np.int64) + 1
        return _abi.gvar_deltas(glyph.xy, [0, *ends.tolist()], [0, len(ends)], **truetype_var.tuple_arrays(self, [gid], normal))

    def point_count(self, gid: int) -> int:
        """The points ``gvar`` numbers in a glyph: the points of a simple glyph, the components of a composite one."""
        components = self._components(gid)
        return len(self.simple_glyph(gid).on) if components is None else len(components)

    def outline(self, parts, sx: float, sy: float):
        """(types, params (n, 8), sizes) of `parts`, ``[((simple glyph id, m00, m01, m10, m11, dx, dy), pen)]``, through the device."""
        index, atlas, gids = {}, [], []
        for part, _pen in parts:
            if part[0] not in index:
                index[part[0]] = len(atlas)
                atlas.append(self.simple_glyph(part[0]))
                gids.append(part[0])
        n = len(parts)
        contour_off, glyph_contour_off, points = [0], [0], 0
        for glyph in atlas:
            contour_off.extend((glyph.ends.astype(np.int64) + 1 + points).tolist())
            points += len(glyph.on)
            glyph_contour_off.append(len(contour_off) - 1)
        xy = np.concatenate([g.xy for g in atlas]) if atlas else np.zeros((0, 2), np.int16)
        on = np.concatenate([g.on for g in atlas]) if atlas else np.zeros(0, np.uint8)
        return self._outline_call(gids, dict(
            pt_xy=xy, pt_on=on, contour_off=contour_off, glyph_contour_off=glyph_contour_off, part_glyph=[index[part[0]] for part, _pen in parts],
            part_m=np.array([part[1:] for part, _pen in parts], dtype=np.float64).reshape(n, 6),
            part_pen=np.array([pen for _part, pen in parts], dtype=np.float64), part_sx=np.full(n, float(sx)), part_sy=np.full(n, float(sy))))

    def _outline_call(self, atlas_gids, args):
        """The device call of `outline`: `args` are svgr_glyf_outline's, `atlas_gids` the glyph ids of the atlas (an instance of a
        variable font adds their tuples)."""
        return _abi.glyf_outline(**args)

    # -- glyf ----------------------------------------------------------------------------------------------------------
    def _glyph_bytes(self, gid: int):
        """(offset in the data, length) of a glyph's record; length 0: the glyph is empty."""
        if not 0 <= gid < self.n_glyphs:
            raise ValueError(f"truetype: glyf: glyph {gid} of {self.n_glyphs}")
        glyf_off, glyf_len = self.tables["glyf"]
        begin, end = int(self.loca[gid]), int(self.loca[gid + 1])
        if begin == end:
            return glyf_off, 0
        if end - begin < 10 or end > glyf_len:
            raise ValueError(f"truetype: glyf: the record of glyph {gid} is short or leaves the table")
        return glyf_off + begin, end - begin

    def simple_glyph(self, gid: int) -> SimpleGlyph:
        """The points of a simple glyph, decoded on first use; a composite or empty glyph has none."""
        glyph = self._simple.get(gid)
        if glyph is None:
            glyph = self._simple[gid] = self._decode_simple(gid)
        return glyph

    def _decode_simple(self, gid: int) -> SimpleGlyph:
        off, length = self._glyph_bytes(gid)
        if length == 0:
            return _EMPTY
        data = self.data[off:off + length]   # (every read below is checked against the glyph's own record)
        n_contours, = _unpack(">h", data, 0, "glyf")
        if n_contours <= 0:
            return _EMPTY
        ends = _array(data, ">u2", 10, n_contours, "glyf: contour ends").astype(np.int32)
        if (np.diff(ends) <= 0).any():
            raise ValueError(f"truetype: glyf: the contour ends of glyph {gid} do not increase")
        n = int(ends[-1]) + 1
        at = 10 + 2 * n_contours
        n_instructions, = _unpack(">H", data, at, "glyf: instruction length")
        at += 2 + n_instructions   # (skipped over, never interpreted)
        flags = np.zeros(n, dtype=np.uint8)
        i = 0
        while i < n:
            _need(data, at, 1, "glyf: flags")
            flag = data[at]
            at += 1
            flags[i] = flag
            i += 1
            if flag & _REPEAT:
                _need(data, at, 1, "glyf: flag repeat")
                repeat = data[at]
                at += 1
                if i + repeat > n:
                    raise ValueError(f"truetype: glyf: a flag of glyph {gid} repeats beyond its points")
                flags[i:i + repeat] = flag
                i += repeat
        xy = np.zeros((n, 2), dtype=np.int64)
        for axis, short, same in ((0, _X_SHORT, _X_SAME), (1, _Y_SHORT, _Y_SAME)):
            value = 0
            for i, flag in enumerate(flags.tolist()):
                if flag & short:
                    _need(data, at, 1, "glyf: coordinates")
                    value += data[at] if flag & same else -data[at]
                    at += 1
                elif not flag & same:
                    value += _unpack(">h", data, at, "glyf: coordinates")[0]
                    at += 2
                xy[i, axis] = value
        if n and (xy.min() < -32768 or xy.max() > 32767):
            raise ValueError(f"truetype: glyf: a coordinate of glyph {gid} leaves 16 bits")
        return SimpleGlyph(xy.astype(np.int16), (flags & _ON).astype(np.uint8), ends)

    def glyph_parts(self, gid: int) -> list:
        """The glyph flattened into ``[(simple glyph id, m00, m01, m10, m11, dx, dy)]``; an empty glyph has no part."""
        parts = self._parts.get(gid)
        if parts is None:
            try:
                parts = self._flatten(gid, (), [0])
            except _TooDeep as why:
                warnings.warn(f"truetype: glyph {gid} of {self.family}: {why}: the glyph is left empty")
                parts = []
            self._parts[gid] = parts
        return parts

    def _components(self, gid: int):
        """None for a simple or empty glyph, else the components of a composite: ``[(glyph id, (c00, c01, c10, c11, dx, dy))]``;
        a glyph's record is read once."""
        if gid not in self._composite:
            self._composite[gid] = self._read_components(gid)
        return self._composite[gid]

    def _placed_components(self, gid: int):
        """`_components` as they are placed: an instance of a variable font moves the offsets."""
        return self._components(gid)

    def _read_components(self, gid: int):
        off, length = self._glyph_bytes(gid)
        if length == 0:
            return None
        data = self.data[off:off + length]
        if _unpack(">h", data, 0, "glyf")[0] >= 0:
            return None
        out, at = [], 10
        while True:
            flags, child = _unpack(">HH", data, at, "glyf: component")
            at += 4
            if flags & _WORDS:
                a1, a2 = _unpack(">hh" if flags & _XY else ">HH", data, at, "glyf: component arguments")
                at += 4
            else:
                a1, a2 = _unpack(">bb" if flags & _XY else ">BB", data, at, "glyf: component arguments")
                at += 2
            if not flags & _XY:
                if not self._warned_matching:
                    self._warned_matching = True
                    warnings.warn(f"truetype: {self.family}: components placed by point matching get the offset (0, 0)")
                a1 = a2 = 0
            c00, c01, c10, c11 = 1.0, 0.0, 0.0, 1.0
            if flags & _SCALE:
                c00 = c11 = _unpack(">h", data, at, "glyf: component scale")[0] / 16384.0
                at += 2
            elif flags & _XY_SCALE:
                c00, c11 = (v / 16384.0 for v in _unpack(">hh", data, at, "glyf: component scale"))
                at += 4
            elif flags & _TWO_BY_TWO:
                c00, c01, c10, c11 = (v / 16384.0 for v in _unpack(">hhhh", data, at, "glyf: component scale"))
                at += 8
            out.append((child, (c00, c01, c10, c11, float(a1), float(a2))))
            if not flags & _MORE:
                return out

    def _flatten(self, gid: int, above: tuple, count: list) -> list:
        if gid in above:
            raise _TooDeep("a composite glyph that contains itself")
        if len(above) > MAX_DEPTH:
            raise _TooDeep(f"composite glyphs nested deeper than {MAX_DEPTH}")
        count[0] += 1   # (every glyph visited counts, composites too: the walk itself is bounded, not only its result)
        if count[0] > MAX_PARTS:
            raise _TooDeep(f"more than {MAX_PARTS} parts")
        components = self._placed_components(gid)
        if components is None:
            return [(gid, *_IDENTITY)] if len(self.simple_glyph(gid).on) else []
        out = []
        for child, (p00, p01, p10, p11, pdx, pdy) in components:
            for simple, c00, c01, c10, c11, cdx, cdy in self._flatten(child, above + (gid,), count):
                out.append((simple, c00 * p00 + c01 * p10, c00 * p01 + c01 * p11, c10 * p00 + c11 * p10, c10 * p01 + c11 * p11,
                            (cdx * p00 + cdy * p10) + pdx, (cdx * p01 + cdy * p11) + pdy))
        return out

    def __repr__(self) -> str:
        return f'TrueTypeFont(family="{self.family}", weight={self.weight}, style={self.style}, glyphs_count={self.n_glyphs})'


class _TooDeep(Exception):
    pass


# ----------------------------------------------------------------------------------------------------------------------
# tables
# ----------------------------------------------------------------------------------------------------------------------
def _directory(data: bytes, cff: bool = False) -> dict:
    """``{tag: (offset, length)}`` of an sfnt with TrueType outlines -- with `cff`, of an ``OTTO`` one, whose outline tables the
    caller asks for itself --, every table inside the data."""
    if len(data) < 4:
        raise ValueError("truetype: the data is shorter than an sfnt version")
    version = data[:4]
    if cff:
        if version != SFNT_CFF:
            raise ValueError(f"opentype: not an OpenType font with CFF outlines (the data begins with {version!r}, not b'OTTO')")
    elif version in REFUSED:
        raise ValueError(f"truetype: {REFUSED[version]}")
    elif version not in SFNT_TRUETYPE:
        raise ValueError(f"truetype: not a TrueType font (the data begins with {version!r})")
    n_tables, = _unpack(">H", data, 4, "table directory")
    _need(data, 12, 16 * n_tables, "table directory")
    tables = {}
    for i in range(n_tables):
        tag, _checksum, off, length = struct.unpack_from(">4sIII", data, 12 + 16 * i)
        _need(data, off, length, f"table {tag!r}")
        tables.setdefault(tag.decode("latin-1"), (off, length))
    missing = [tag for tag in (REQUIRED_CFF if cff else REQUIRED) if tag not in tables]
    if missing:
        raise ValueError(f"truetype: the font has no {' / '.join(missing)} table")
    return tables


def _table(tables: dict, tag: str, size: int) -> int:
    """The offset of a table that holds at least `size` bytes."""
    off, length = tables[tag]
    if length < size:
        raise ValueError(f"truetype: {tag}: the table has {length} bytes where {size} are needed")
    return off


class _Cmap4:
    def __init__(self, data, off, end):
        seg_x2, = _unpack(">H", data, off + 6, "cmap 4")
        n = seg_x2 // 2
        if n < 1 or off + 16 + 8 * n > end:
            raise ValueError("cmap: a format 4 subtable without segments or longer than the table")
        self.end = _array(data, ">u2", off + 14, n, "cmap 4").astype(np.int64)
        self.start = _array(data, ">u2", off + 16 + 2 * n, n, "cmap 4").astype(np.int64)
        self.delta = _array(data, ">u2", off + 16 + 4 * n, n, "cmap 4").astype(np.int64)
        self.range_at = off + 16 + 6 * n
        self.range = _array(data, ">u2", self.range_at, n, "cmap 4").astype(np.int64)
        if (self.start > self.end).any() or (self.start[1:] <= self.end[:-1]).any():
            raise ValueError("cmap: the segments of a format 4 subtable are not in order")
        self.data, self.limit = data, end
        self.ends = self.end.tolist()

    def lookup(self, code: int) -> int:
        if not 0 <= code <= 0xFFFF:
            return 0
        i = bisect.bisect_left(self.ends, code)
        if i >= len(self.ends) or int(self.start[i]) > code:
            return 0
        if self.range[i] == 0:
            return (code + int(self.delta[i])) & 0xFFFF
        at = self.range_at + 2 * i + int(self.range[i]) + 2 * (code - int(self.start[i]))
        if at + 2 > self.limit:
            return 0
        gid, = struct.unpack_from(">H", self.data, at)
        return (gid + int(self.delta[i])) & 0xFFFF if gid else 0

    def codes(self):
        for start, end in zip(self.start.tolist(), self.end.tolist()):
            yield from range(start, min(end, 0xFFFE) + 1)


class _Cmap12:
    def __init__(self, data, off, end):
        n, = _unpack(">I", data, off + 12, "cmap 12")
        if off + 16 + 12 * n > end:
            raise ValueError("cmap: a format 12 subtable longer than the table")
        groups = _array(data, ">u4", off + 16, 3 * n, "cmap 12").astype(np.int64).reshape(n, 3)
        self.start, self.end, self.gid = groups[:, 0], groups[:, 1], groups[:, 2]
        if (self.start > self.end).any() or (self.start[1:] <= self.end[:-1]).any() or (n and int(self.end[-1]) > 0x10FFFF):
            raise ValueError("cmap: the groups of a format 12 subtable are not in order or leave Unicode")
        self.ends = self.end.tolist()

    def lookup(self, code: int) -> int:
        i = bisect.bisect_left(self.ends, code)
        if i >= len(self.ends) or int(self.start[i]) > code:
            return 0
        return int(self.gid[i]) + code - int(self.start[i])

    def codes(self):
        for start, end in zip(self.start.tolist(), self.end.tolist()):
            yield from range(start, end + 1)


def _read_cmap(data, off, length):
    """The best subtable of format 4 or 12: platform 3 encoding 10, then 3 / 1, then platform 0; the first in the file among equals."""
    end = off + length
    n, = _unpack(">H", data, off + 2, "cmap")
    if 4 + 8 * n > length:
        raise ValueError("cmap: the encoding records leave the table")
    best = None
    for i in range(n):
        platform, encoding, sub = struct.unpack_from(">HHI", data, off + 4 + 8 * i)
        rank = 0 if (platform, encoding) == (3, 10) else 1 if (platform, encoding) == (3, 1) else 2 if platform == 0 else None
        if rank is None or sub + 2 > length:
            continue
        fmt, = struct.unpack_from(">H", data, off + sub)
        if fmt in (4, 12) and (best is None or rank < best[0]):
            best = (rank, fmt, off + sub)
    if best is None:
        raise ValueError("truetype: cmap: no Unicode subtable of format 4 or 12")
    return (_Cmap4 if best[1] == 4 else _Cmap12)(data[:end], best[2], end)


def _read_family(data, off, length):
    """Name id 1: the first platform 3 record (UTF-16BE; a US English one first), else the first platform 1 record (Latin-1)."""
    n, strings = _unpack(">HH", data, off + 2, "name")
    if 6 + 12 * n > length:
        raise ValueError("truetype: name: the records leave the table")
    found = {}
    for i in range(n):
        platform, _enc, language, name_id, size, at = struct.unpack_from(">HHHHHH", data, off + 6 + 12 * i)
        if name_id != 1 or platform not in (1, 3):
            continue
        if strings + at + size > length:
            raise ValueError("truetype: name: a string leaves the table")
        raw = data[off + strings + at:off + strings + at + size]
        found.setdefault((platform, platform == 3 and language == 0x409), raw)
    for key, codec in (((3, True), "utf-16-be"), ((3, False), "utf-16-be"), ((1, False), "latin-1")):
        if key in found:
            return found[key].decode(codec, "replace").strip("\0 ") or None
    return None


def _read_kern(data, off, length) -> dict:
    """``{(left, right): value}`` summed over the format 0, horizontal, non-cross-stream subtables of a version 0 table."""
    end = off + length
    version, n = _unpack(">HH", data, off, "kern")
    pairs: dict = {}
    if version != 0:   # (Apple's version 1 layout is not read)
        return pairs
    at = off + 4
    for _ in range(n):
        if at + 6 > end:
            raise ValueError("truetype: kern: a subtable leaves the table")
        _version, size, coverage = struct.unpack_from(">HHH", data, at)
        if coverage >> 8 == 0 and coverage & 1 and not coverage & 4:
            if at + 14 > end:
                raise ValueError("truetype: kern: a subtable leaves the table")
            n_pairs, = struct.unpack_from(">H", data, at + 6)
            if at + 14 + 6 * n_pairs > end:
                raise ValueError("truetype: kern: the pairs leave the table")
            rec = np.frombuffer(data, dtype=">u2", count=3 * n_pairs, offset=at + 14).reshape(n_pairs, 3)
            for left, right, value in zip(rec[:, 0].tolist(), rec[:, 1].tolist(), rec[:, 2].astype(np.int16).tolist()):
                pairs[(left, right)] = value if coverage & 8 else pairs.get((left, right), 0) + value
            size = max(size, 14 + 6 * n_pairs)   # (a 16-bit length cannot say what a large subtable takes)
        if size < 6:
            raise ValueError("truetype: kern: a subtable shorter than its header")
        at += size
    return pairs


def read_ttf(data: bytes, family: "str | None" = None) -> TrueTypeFont:
    """Parse a TrueType font (the module's docstring says what is read).  `family` replaces the family of the ``name`` table;
    a font that has none needs it."""
    font = TrueTypeFont(data, family)
    if font.family is None:
        raise ValueError("truetype: the font names no family (name id 1): pass family=")
    return font


def read_ttf_file(path: str, family: "str | None" = None) -> TrueTypeFont:
    """`read_ttf` of a file; a font that names no family takes the file's name without its extension."""
    with open(path, "rb") as f:
        data = f.read()
    font = TrueTypeFont(data, family)
    if font.family is None:
        font.family = os.path.splitext(os.path.basename(path))[0]
    return font
