"""Fonts: glyph tables -> text outlines (reference ``Glyph`` / ``Font`` / ``FontsDB``, S:2563-2718).

Host code in front of the hot path: a string becomes one ``Path`` of glyph outlines, which is then filled / stroked like
any other path.  ``Font`` is an SVG font (``<font>`` elements inside a document, or whole documents of them registered with
``FontsDB.register_file`` and loaded on first use) -- the only kind the reference has.  Beyond it, ``truetype.TrueTypeFont``
is a ``Font`` read from a ``.ttf`` (``FontsDB.register_file`` of such a file, ``FontsDB.register_ttf``) and
``opentype_cff.CFFFont`` one read from an ``.otf`` with CFF outlines (``OTTO``; ``register_file``, ``FontsDB.register_font``); other
font formats (collections, WOFF, CFF2) are refused.  Nothing looks for fonts on its own: no system directory is
scanned and nothing is fetched, the caller says which files.
"""
from __future__ import annotations

import os
import warnings

import numpy as np

from . import _abi
from .geometry import FLATNESS, PATH_ARC, Path
from .sdf import SdfAtlas, font_sdf_atlas

FONT_STYLE_NORMAL = "normal"
# generic families the well-known names fall back to (S:2653-2655)
_GENERIC = (
    ("sans", {"arial", "verdana"}),
    ("serif", {"times new roman", "times", "georgia"}),
    ("mono", {"iosevka", "courier", "pragmatapro"}),
)


def _ranges(begin, end):
    """The concatenation of ``arange(begin[k], end[k])`` over k."""
    begin, end = np.asarray(begin, dtype=np.int64), np.asarray(end, dtype=np.int64)
    count = end - begin
    total = int(count.sum())
    if total == 0:
        return np.zeros(0, dtype=np.int64)
    first = np.cumsum(count) - count   # where each range begins in the result
    return np.arange(total, dtype=np.int64) - np.repeat(first - begin, count)


class Glyph:
    """One glyph: its outline is kept as path data and parsed on first use."""

    __slots__ = ["unicode", "advance", "name", "path_source", "_path", "_arrays"]

    def __init__(self, unicode, advance: float, path_source: str, name=None):
        self.unicode = unicode
        self.advance = advance
        self.name = name
        self.path_source = path_source
        self._path = None
        self._arrays = None

    @property
    def path(self) -> Path:
        if self._path is None:
            self._path = Path.from_svg(self.path_source)
        return self._path

    @property
    def arrays(self):
        """The outline in the stroker's array form, in glyph units: ``(types int32, params (n, 8), sizes int32)``, converted once."""
        if self._arrays is None:
            types, params, sizes = self.path._segment_arrays()
            self._arrays = (np.array(types, dtype=np.int32), np.array(params, dtype=np.float64).reshape(-1, 8),
                            np.array(sizes, dtype=np.int32))
        return self._arrays

    def __repr__(self) -> str:
        return f"Glyph(unicode={self.unicode}, name={self.name})"


class Font:
    """Glyph table of one face.  Glyph space is y-up with ``units_per_em`` units per em."""

    __slots__ = ["family", "weight", "style", "ascent", "descent", "units_per_em", "glyphs", "missing_glyph", "hkern"]

    def __init__(self, family, weight, style, ascent, descent, units_per_em, glyphs=None, missing_glyph=None, hkern=None):
        self.family, self.weight, self.style = family, weight, style
        self.ascent, self.descent, self.units_per_em = ascent, descent, units_per_em
        self.glyphs = {} if glyphs is None else glyphs
        self.missing_glyph = missing_glyph
        self.hkern = {} if hkern is None else hkern

    def str_to_glyphs(self, string: str):
        """``([(pen x, glyph)], total advance)`` in glyph units (S:2602-2634).

        Ligatures: the key is grown one character at a time while it keeps naming a glyph; a single unknown character
        maps to the missing glyph.  Kerning is subtracted from the pen before the right glyph of a pair is placed.
        """
        placed, pen, prev = [], 0.0, None
        i, n = 0, len(string)
        while i < n:
            j = i + 1
            glyph = self.glyphs.get(string[i:j])
            if glyph is None:
                glyph = self.missing_glyph
            else:
                while j < n:
                    longer = self.glyphs.get(string[i:j + 1])
                    if longer is None:
                        break
                    glyph, j = longer, j + 1
            assert glyph is not None, "font has no missing-glyph"
            i = j
            if prev is not None:
                kern = self.hkern.get((prev, glyph.unicode))
                if kern is not None:
                    pen -= kern
            placed.append((pen, glyph))
            pen += glyph.advance
            prev = glyph.unicode
        return placed, pen

    def str_to_path(self, size: float, string: str):
        """Outline of ``string`` at ``size`` user units per em, y flipped to the SVG's y-down: ``(Path, advance)``
        (S:2636-2650; ``(x + pen) * scale``, ``-y * scale`` in that order of operations)."""
        scale = size / self.units_per_em
        placed, advance = self.str_to_glyphs(string)
        subpaths = []
        for pen, glyph in placed:
            for outline in glyph.path:
                sub = []
                for kind, pts in outline:
                    assert kind != PATH_ARC
                    sub.append((kind, [[(x + pen) * scale, -y * scale] for x, y in pts]))
                subpaths.append(sub)
        return Path(subpaths), advance * scale

    def str_on_path(self, path: Path, size: float, string: str, offset: float = 0.0, dy: float = 0.0):
        """Outline of ``string`` set along `path` (beyond the reference; ``<textPath>``, SVG 1.1 10.13): ``(Path, advance)``.
        Pen positions, ligatures and kerning are `str_to_glyphs`'; a glyph is anchored where the middle of its advance,
        ``offset + (pen + advance / 2) * scale``, falls on the path, turned into the path's direction there and moved by `dy` across
        it; scaling and y flip are `str_to_path`'s.  A glyph whose anchor lies off the path is left out.  Eager, on the device
        (svgr_path_place_glyphs)."""
        scale = size / self.units_per_em
        placed, advance = self.str_to_glyphs(string)
        types, params, sizes = path._segment_arrays()
        if not placed or not types:
            return Path([]), advance * scale
        index, atlas = {}, []
        for _pen, glyph in placed:
            if id(glyph) not in index:
                index[id(glyph)] = len(atlas)
                atlas.append(glyph)
        inst_glyph = np.array([index[id(g)] for _pen, g in placed], dtype=np.int32)
        pens = np.array([pen for pen, _g in placed], dtype=np.float64)
        advances = np.array([g.advance for g in atlas], dtype=np.float64)[inst_glyph]
        a_types = np.concatenate([g.arrays[0] for g in atlas])
        a_params = np.concatenate([g.arrays[1] for g in atlas])
        a_sizes = np.concatenate([g.arrays[2] for g in atlas])
        seg_off = np.concatenate([[0], np.cumsum([len(g.arrays[0]) for g in atlas])]).astype(np.int32)
        sub_off = np.concatenate([[0], np.cumsum([len(g.arrays[2]) for g in atlas])]).astype(np.int64)
        scaled = np.empty_like(a_params)
        scaled[:, 0::2] = a_params[:, 0::2] * scale
        scaled[:, 1::2] = -a_params[:, 1::2] * scale
        out, visible, _length = _abi.path_place_glyphs(types, np.array(params), sizes, a_types, scaled, seg_off, inst_glyph,
                                                       offset + (pens + advances / 2) * scale, advances * scale / 2,
                                                       np.full(len(placed), float(dy)))
        # types and subpath sizes of the result: gathers of the atlas' tables over the visible instances
        shown = inst_glyph[visible]
        seg_rows = _ranges(seg_off[shown], seg_off[shown + 1])
        seg_count = np.diff(seg_off.astype(np.int64))[inst_glyph]
        keep = np.repeat(visible, seg_count)
        return Path.from_segments(a_types[seg_rows], out[keep], a_sizes[_ranges(sub_off[shown], sub_off[shown + 1])]), advance * scale

    def sdf_atlas(self, string: str, size: float, spread: float, dtype=np.uint8, max_cols: int = 1024, flatness: float = FLATNESS) -> SdfAtlas:
        """An SDF atlas of the distinct glyphs of `string` (beyond the reference), ligatures and the missing glyph as
        `str_to_glyphs` resolves them: every glyph scaled by ``size / units_per_em`` and y-flipped, in a cell of its own -- the
        integer box around its control points grown by ``ceil(spread)`` pixels on every side --, the cells shelf-packed into an
        image at most `max_cols` wide.  ``dtype`` uint8 / float32: ``0.5 - d / (2 * spread)``, 0.5 on the outline and larger inside
        (times 255 and rounded for uint8); float64: the signed distance in pixels clamped to ``+-spread``, negative inside.  A glyph
        without an outline (a space) gets a cell of zero size and its advance; a string without glyphs a 0 x 0 image.  One batch,
        a path per glyph, and one union grid query on the device (svgr_batch_distance); see sdf.py."""
        return font_sdf_atlas(self, string, size, spread, dtype, max_cols, flatness)

    def msdf_atlas(self, string: str, size: float, spread: float, dtype=np.uint8, max_cols: int = 1024, angle: float = 3.0,
                   flatness: float = FLATNESS) -> SdfAtlas:
        """`sdf_atlas` with four channels (beyond the reference): the same cells, keys and layout, ``image`` of shape ``(rows, cols,
        4)``: R, G, B whose median (``sdf.median``) keeps the glyphs' corners sharp, and in A the field of `sdf_atlas` itself.  One
        batch, one group per glyph, and one query on the device (svgr_batch_msdf); see msdf.py."""
        from .msdf import font_msdf_atlas

        return font_msdf_atlas(self, string, size, spread, dtype, max_cols, angle, flatness)

    def names(self) -> dict:
        return {g.name: g.unicode for g in self.glyphs.values()}

    def __repr__(self) -> str:
        return f'Font(family="{self.family}", weight={self.weight}, style={self.style}, glyphs_count={len(self.glyphs)})'


class FontsDB:
    """Fonts by lower-cased family name, with the reference's resolution order (S:2661-2718)."""

    __slots__ = ["fonts", "fonts_files"]

    def __init__(self):
        self.fonts: dict = {}
        self.fonts_files: list = []

    def register(self, font: Font, alias=None) -> None:
        self.fonts.setdefault(font.family.lower(), []).append(font)
        if alias is not None and alias != font.family:
            self.fonts.setdefault(alias.lower(), []).append(font)

    def register_file(self, path: str) -> None:
        """A font file, told by its first four bytes: a TrueType font (``truetype.read_ttf``) or an ``OTTO`` font with CFF outlines
        (``opentype_cff.read_otf``) is read now and registered under the family of its ``name`` table (without one: the file's
        name); ``ttcf`` / ``wOFF`` / ``wOF2`` and a TrueType or ``OTTO`` file that is malformed or lacks a required table warn with the
        reason and are skipped (nothing is raised); anything else is an SVG document of ``<font>`` elements, remembered and loaded
        by the first ``resolve``."""
        from . import opentype_cff, truetype  # noqa: PLC0415  (both import this module)

        try:
            with open(path, "rb") as f:
                head = f.read(4)
        except OSError:
            head = b""   # (the first `resolve` warns about a file that is not there)
        if opentype_cff.is_cff(head):
            try:
                self.register(opentype_cff.read_otf_file(path))
            except ValueError as why:   # (a malformed file, or an OTTO one without a CFF table)
                warnings.warn(f"font file skipped: {path}: {why}")
        elif head in truetype.REFUSED:
            warnings.warn(f"font file skipped: {path}: {truetype.REFUSED[head]}")
        elif truetype.is_truetype(head):
            try:
                self.register(truetype.read_ttf_file(path))
            except ValueError as why:   # (a malformed file, or one without a required table)
                warnings.warn(f"font file skipped: {path}: {why}")
        else:
            self.fonts_files.append(path)

    def register_font(self, data_or_path, family=None):
        """Register a TrueType or an OpenType / CFF font, told by its first four bytes, from bytes in memory or from a file's
        path, under `family` when given (an alias: the font's own family stays registered too), and return it."""
        from . import opentype_cff  # noqa: PLC0415

        if isinstance(data_or_path, (bytes, bytearray, memoryview)):
            data = bytes(data_or_path)
            if not opentype_cff.is_cff(data):
                return self.register_ttf(data, family)
            font = opentype_cff.CFFFont(data)
            if font.family is None:   # (a font that names no family takes the caller's)
                if family is None:
                    raise ValueError("opentype: the font names no family (name id 1): pass family=")
                font.family = family
        else:
            path = os.fspath(data_or_path)
            with open(path, "rb") as f:
                head = f.read(4)
            if not opentype_cff.is_cff(head):
                return self.register_ttf(path, family)
            font = opentype_cff.read_otf_file(path)
        self.register(font, alias=family)
        return font

    def register_ttf(self, data_or_path, family=None):
        """Register a TrueType font from bytes in memory or from a file's path, under `family` when given (an alias: the font's
        own family stays registered too), and return it."""
        from . import truetype  # noqa: PLC0415

        if isinstance(data_or_path, (bytes, bytearray, memoryview)):
            font = truetype.TrueTypeFont(bytes(data_or_path))
            if font.family is None:   # (a font that names no family takes the caller's)
                if family is None:
                    raise ValueError("truetype: the font names no family (name id 1): pass family=")
                font.family = family
        else:
            font = truetype.read_ttf_file(os.fspath(data_or_path))
        self.register(font, alias=family)
        return font

    def _load_pending(self) -> None:
        from .svg import svg_scene_from_filepath  # the loader registers every <font> it meets
        while self.fonts_files:
            source = self.fonts_files.pop()
            if not os.path.isfile(source):
                warnings.warn(f"failed to find fonts file: {source}")
                continue
            svg_scene_from_filepath(source, fonts=self)

    def resolve(self, family, weight=None, style=None, variations=None):
        """Best face for ``family`` or None: exact family, else its generic family (unknown names count as serif);
        then the requested style (else normal); then the nearest weight (first registered wins ties).  A variable TrueType
        face with a ``wght`` axis is as near as the weight is to the axis' range (0 inside it) and comes back as its instance at
        that weight and at `variations`, ``{axis tag: value}``, of which the tags the face lacks are left out."""
        self._load_pending()
        family = "serif" if family is None else family.lower()
        faces = self.fonts.get(family)
        if faces is None:
            generic = "serif"
            for key, members in _GENERIC:
                if key in family or family in members:
                    generic = "monospace" if key == "mono" else key
                    break
            # the second lookup name is the reference's (S:2699); it only matters when the generic family is absent
            faces = self.fonts.get(generic, self.fonts.get("seif"))
        if faces is None:
            return None
        style = style or FONT_STYLE_NORMAL
        styled = [f for f in faces if f.style == style] or [f for f in faces if f.style == FONT_STYLE_NORMAL]
        if not styled:
            return None
        weight = weight or 400

        def distance(face):
            axis = next((a for a in getattr(face, "axes", ()) if a.tag == "wght"), None)
            if axis is None:
                return abs(face.weight - weight)
            return 0 if axis.minimum <= weight <= axis.maximum else min(abs(weight - axis.minimum), abs(weight - axis.maximum))

        face = min(styled, key=distance)
        tags = [a.tag for a in getattr(face, "axes", ())]
        if not tags:
            return face
        wanted = {"wght": weight, **(variations or {})}
        return face.instance({tag: value for tag, value in wanted.items() if tag in tags})
