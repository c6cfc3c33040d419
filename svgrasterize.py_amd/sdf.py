"""Glyph SDF atlases (beyond the reference): the distinct glyphs of a string, each in a cell of its own, as one signed distance
field image -- what GPU text renderers and differentiable-text pipelines sample.  ``Font.sdf_atlas`` (fonts.py) is the entry; the
cell geometry and the shelf packer here are plain host functions, the field itself is ONE batch with a path per glyph and ONE union
grid query (svgr_batch_distance, gfx950).

Why the union is enough: a glyph's control points, and so its outline, lie at least ``ceil(spread)`` inside its own cell, and cells
are disjoint.  A pixel centre of a cell is therefore farther than `spread` from every other glyph and outside it: the others
saturate at ``+spread``, the largest value there is, and the minimum over the paths is the cell's own glyph's field.
"""
from __future__ import annotations

import math

import numpy as np

from . import _abi
from .geometry import _SDF_DTYPES, FLATNESS, _sdf_dtype


class SdfCell(tuple):
    """One glyph's place in an ``SdfAtlas``: the cell ``image[row0:row0 + rows, col0:col0 + cols]``; ``(origin_row, origin_col)``,
    where the glyph's pen origin falls inside the cell (the baseline runs through ``row0 + origin_row``); ``advance`` in pixels.  A
    glyph without an outline has ``rows == cols == 0``."""
    __slots__ = []
    _fields = ("row0", "col0", "rows", "cols", "origin_row", "origin_col", "advance")

    def __new__(cls, row0, col0, rows, cols, origin_row, origin_col, advance):
        return tuple.__new__(cls, (row0, col0, rows, cols, origin_row, origin_col, advance))

    row0 = property(lambda self: self[0])
    col0 = property(lambda self: self[1])
    rows = property(lambda self: self[2])
    cols = property(lambda self: self[3])
    origin_row = property(lambda self: self[4])
    origin_col = property(lambda self: self[5])
    advance = property(lambda self: self[6])

    def __repr__(self) -> str:
        return "SdfCell(" + ", ".join(f"{k}={v}" for k, v in zip(self._fields, self)) + ")"


class SdfAtlas:
    """``image`` (rows, cols) -- (rows, cols, 4) from ``Font.msdf_atlas`` -- in the dtype asked for, ``size`` (pixels per em), ``spread`` (pixels) and ``cells``: per glyph --
    keyed by ``glyph.unicode``, or by the glyph id (a name for an SVG font) where it has none -- its ``SdfCell``."""
    __slots__ = ["image", "size", "spread", "cells"]

    def __init__(self, image, size, spread, cells):
        self.image, self.size, self.spread, self.cells = image, size, spread, cells

    def __repr__(self) -> str:
        return f"SdfAtlas(image={self.image.shape} {self.image.dtype}, size={self.size}, spread={self.spread}, cells={len(self.cells)})"

    def write_png(self, output=None, **kw):
        """The atlas image as a PNG into ``output`` (a binary file object; default a new BytesIO), which is returned: a
        ``(rows, cols)`` field as grey, a ``(rows, cols, 4)`` MSDF image as RGBA.  A uint8 image is written at depth 8 as it is; a
        float32 image (codes in [0, 1]) is quantised on the device, at depth 16 unless ``depth=8`` is given.  A float64 atlas holds
        signed pixel distances, not codes: TypeError.  ``kw``: ``canvas_to_png``'s ``level``, ``threads``, ``encoder``,
        ``filter``, ``huffman`` and ``depth``."""
        from . import png  # noqa: PLC0415
        from .layer import canvas_to_png  # noqa: PLC0415

        unknown = set(kw) - {"level", "threads", "encoder", "filter", "huffman", "depth"}
        if unknown:
            raise TypeError(f"SdfAtlas.write_png: unexpected arguments {sorted(unknown)}")
        image = np.asarray(self.image)
        if image.dtype not in (np.uint8, np.float32):
            raise TypeError(f"SdfAtlas.write_png writes a uint8 or float32 atlas, not {image.dtype} (signed distances are no sample codes)")
        if not (image.ndim == 2 or (image.ndim == 3 and image.shape[2] == 4)):
            raise ValueError(f"SdfAtlas.write_png: the image is (rows, cols) or (rows, cols, 4), not {image.shape}")
        color = "grey" if image.ndim == 2 else "rgba"
        depth = kw.pop("depth", None)
        if image.dtype == np.uint8:
            return canvas_to_png(image, output, color=color, depth=8 if depth is None else depth, **kw)
        if image.ndim == 3:
            return canvas_to_png(image, output, color=color, depth=16 if depth is None else depth, **kw)
        # a float field: one channel, which canvas_to_png has no form for -- the mask source of the same device stage
        args = png.encoder_arguments(kw.get("encoder", "host"), kw.get("level"), kw.get("threads"), kw.get("filter"), kw.get("huffman"))
        fmt = png.format_arguments(color, 16 if depth is None else depth)
        rows, cols = image.shape
        if rows == 0 or cols == 0:
            raise ValueError(f"a PNG image has at least one pixel, not {cols} x {rows}")
        samples = png.samples_device(image.astype(np.float64), _abi.PNG_SRC_MASK_F64, rows, cols, fmt[0], fmt[1])
        return png.encode_samples(samples, rows, cols, fmt[0], fmt[1], output, args)


def glyph_key(glyph):
    return glyph.unicode if glyph.unicode is not None else getattr(glyph, "gid", glyph.name)


def cell_geometry(box, scale: float, pad: int):
    """``(rows, cols, origin_row, origin_col)`` of a glyph's cell.  `box` is (x0, y0, x1, y1) of its control points in glyph units
    (y up) or None (no outline: a cell of zero size); the glyph is scaled by `scale` and y-flipped, the cell is the integer box
    around that, grown by `pad` on every side."""
    if box is None:
        return 0, 0, 0, 0
    x0, y0, x1, y1 = box
    r_lo, r_hi = math.floor(-y1 * scale), math.ceil(-y0 * scale)
    c_lo, c_hi = math.floor(x0 * scale), math.ceil(x1 * scale)
    return r_hi - r_lo + 2 * pad, c_hi - c_lo + 2 * pad, pad - r_lo, pad - c_lo


def pack_cells(sizes, max_cols: int):
    """Shelf packing of cells ``[(rows, cols)]`` into an image at most `max_cols` wide: ``(positions [(row0, col0)], image rows,
    image cols)``, positions in the order given.  The cells are placed tallest first, left to right, a new shelf when the next one
    does not fit.  A cell of zero size takes no room (position (0, 0)); one wider than `max_cols` is a ValueError."""
    max_cols = int(max_cols)
    if max_cols < 1:
        raise ValueError("max_cols is at least 1")
    positions = [(0, 0)] * len(sizes)
    order = sorted((k for k, (r, c) in enumerate(sizes) if r > 0 and c > 0), key=lambda k: -sizes[k][0])   # (stable)
    shelf_row = shelf_rows = cursor = width = 0
    for k in order:
        rows, cols = sizes[k]
        if cols > max_cols:
            raise ValueError(f"a cell of {cols} columns does not fit max_cols = {max_cols}")
        if cursor + cols > max_cols:
            shelf_row, shelf_rows, cursor = shelf_row + shelf_rows, 0, 0
        positions[k] = (shelf_row, cursor)
        cursor += cols
        shelf_rows = max(shelf_rows, rows)
        width = max(width, cursor)
    return positions, shelf_row + shelf_rows, width


def atlas_layout(glyphs, boxes, advances, size: float, units_per_em: float, spread: float, max_cols: int):
    """``(cells {key: SdfCell}, image rows, image cols)`` for glyph keys, control-point boxes (glyph units, or None) and advances
    (glyph units): no device, no font object."""
    scale, pad = size / units_per_em, int(math.ceil(spread))
    geo = [cell_geometry(box, scale, pad) for box in boxes]
    positions, rows, cols = pack_cells([(g[0], g[1]) for g in geo], max_cols)
    cells = {key: SdfCell(pos[0], pos[1], g[0], g[1], g[2], g[3], adv * scale) for key, pos, g, adv in zip(glyphs, positions, geo, advances)}
    return cells, rows, cols


def atlas_arguments(size, spread, dtype, max_cols):
    """The checked arguments of ``Font.sdf_atlas``: (size, spread, encoding); TypeError / ValueError before any device work."""
    enc = _SDF_DTYPES.get(_sdf_dtype(dtype))
    if enc is None:
        raise TypeError(f"an SDF atlas is float64, float32 or uint8, not {dtype!r}")
    spread = _abi.sdf_spread(spread, finite=True)
    if math.isinf(spread):
        raise ValueError("an SDF atlas needs a finite spread")
    size = float(size)
    if not (size > 0.0 and math.isfinite(size)):
        raise ValueError(f"a size is finite and > 0, not {size!r}")
    if int(max_cols) < 1:
        raise ValueError("max_cols is at least 1")
    return size, spread, enc


def font_sdf_atlas(font, string: str, size: float, spread: float, dtype=np.uint8, max_cols: int = 1024, flatness: float = FLATNESS) -> SdfAtlas:
    """``Font.sdf_atlas``: the distinct glyphs of `string`, in the order of their first appearance."""
    atlas_arguments(size, spread, dtype, max_cols)
    placed, _advance = font.str_to_glyphs(string)
    glyphs, seen = [], set()
    for _pen, glyph in placed:
        if id(glyph) not in seen:
            seen.add(id(glyph))
            glyphs.append(glyph)
    return glyphs_sdf_atlas(glyphs, [glyph_key(g) for g in glyphs], font.units_per_em, size, spread, dtype, max_cols, flatness)


def glyphs_sdf_atlas(glyphs, keys, units_per_em: float, size: float, spread: float, dtype=np.uint8, max_cols: int = 1024,
                     flatness: float = FLATNESS) -> SdfAtlas:
    """The atlas of a list of glyphs (of one face, or of several with the same ``units_per_em``: the instances of a variable font)
    under the keys given: one batch, a path per glyph with an outline, each with its own six numbers, and one union grid query."""
    size, spread, enc = atlas_arguments(size, spread, dtype, max_cols)
    paths = [g.path for g in glyphs]
    cells, rows, cols = atlas_layout(keys, [p.user_box() for p in paths], [g.advance for g in glyphs], size, units_per_em, spread, max_cols)
    if rows * cols == 0:
        return SdfAtlas(np.zeros((0, 0), dtype=_abi.SDF_OUT[enc][1]), size, spread, cells)
    scale = size / units_per_em
    packs, m6s = [], []
    for key, path in zip(keys, paths):
        cell = cells[key]
        if cell.rows:
            packs.append(path.packed())
            m6s.append(cell_m6(cell, scale))
    n = len(packs)
    offs = np.concatenate([[0], np.cumsum([len(pk[0]) for pk in packs])]).astype(np.int64)
    batch = _abi.Batch(_abi.Context.get(), np.concatenate([pk[0] for pk in packs]), np.concatenate([pk[1] for pk in packs]), offs,
                       np.array(m6s, dtype=np.float64), np.zeros(n, dtype=np.uint8), np.zeros((n, 4)), viewport=None, flatness=flatness)
    try:
        image = batch.distance(grid=(0, 0, rows, cols), spread=spread, out=enc, union=True).reshape(rows, cols)
    finally:
        batch.destroy()
    return SdfAtlas(image, size, spread, cells)


def median(image) -> np.ndarray:
    """The median of the first three channels of an MSDF image ``(..., 3 or 4)`` (``Path.msdf``, ``Font.msdf_atlas``): what a shader
    computes from a sample before it thresholds."""
    image = np.asarray(image)
    r, g, b = image[..., 0], image[..., 1], image[..., 2]
    return np.maximum(np.minimum(r, g), np.minimum(np.maximum(r, g), b))


def cell_m6(cell: SdfCell, scale: float) -> list:
    """The six numbers that take a glyph (glyph units, y up) into its cell of the atlas: row = origin - y * scale, col = origin + x *
    scale."""
    return [0.0, -scale, float(cell.row0 + cell.origin_row), scale, 0.0, float(cell.col0 + cell.origin_col)]
