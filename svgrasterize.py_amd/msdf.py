"""Multi-channel distance fields (beyond the reference): ``Path.msdf`` and ``Font.msdf_atlas``.  A single-channel field rounds every
corner at the scale of a texel; here the segments of an outline are dealt out to three colour channels so that the two sides of a
corner never share all their channels, each channel follows the nearest edge of its colour and reports the signed distance to that
edge's LINE, and the median of the three is sharp at the corner.  The fourth channel is the true signed distance of ``Path.sdf``.

The colouring (`colour_edges`) and the orientation (`orientation`) are plain host functions; the field itself is ONE batch -- up to
four paths per shape, one per colour, that share the shape's six numbers -- and ONE query (svgr_batch_msdf, gfx950; the arithmetic:
csrc/svgr_msdf.h).
"""
from __future__ import annotations

import math

import numpy as np

from . import _abi
from .geometry import _RULES, _SDF_DTYPES, FLATNESS, PATH_ARC, PATH_CUBIC, PATH_LINES, PATH_QUAD, Transform, _sdf_dtype, arc_to_cubics, quad_to_cubic
from .sdf import SdfAtlas, atlas_arguments, atlas_layout, cell_m6, glyph_key, median  # noqa: F401

WHITE, CYAN, MAGENTA, YELLOW = 7, 6, 5, 3           # bit 0 R, bit 1 G, bit 2 B
_TURN = (CYAN, MAGENTA, YELLOW)


def _pieces(sub):
    """A subpath's segments as control-point arrays in the order drawn: (2, 2) for a line (its closing line is one), (4, 2) for a
    cubic; a quadratic and an arc go through the cubics of ``Path.packed()``."""
    out = []
    for seg in sub:
        t = seg[0]
        if t in PATH_LINES:
            out.append(np.asarray(seg[1], dtype=np.float64).reshape(2, 2))
        elif t == PATH_CUBIC:
            out.append(np.asarray(seg[1], dtype=np.float64).reshape(4, 2))
        elif t == PATH_QUAD:
            out.append(quad_to_cubic(seg[1]).reshape(4, 2))
        elif t == PATH_ARC:
            out.extend(c.reshape(4, 2) for c in arc_to_cubics(*seg[1]))
        else:
            raise ValueError(f"unsupported path type: `{t}`")
    return out


def _tangents(piece):
    """(unit start tangent, unit end tangent) from the control points, skipping coincident ones; None for a piece that is a point.
    (Plain floats: a piece has two or four points, and an atlas has thousands of pieces.)"""
    pts = piece.tolist()
    p0, p1 = pts[0], pts[-1]
    first = next(((q[0] - p0[0], q[1] - p0[1]) for q in pts[1:] if q != p0), None)
    if first is None:
        return None
    last = next((p1[0] - q[0], p1[1] - q[1]) for q in pts[-2::-1] if q != p1)
    lf, ll = math.hypot(*first), math.hypot(*last)
    return (first[0] / lf, first[1] / lf), (last[0] / ll, last[1] / ll)


def _thirds(piece):
    """A piece cut at t = 1/3 and 2/3 (de Casteljau): three pieces of the same kind."""
    def cut(p, t):
        left, right = [p[0]], [p[-1]]
        while len(p) > 1:
            p = p[:-1] + (p[1:] - p[:-1]) * t
            left.append(p[0])
            right.append(p[-1])
        return np.array(left), np.array(right[::-1])

    a, rest = cut(piece, 1.0 / 3.0)
    b, c = cut(rest, 0.5)
    return [a, b, c]


def colour_subpath(pieces, angle: float = 3.0):
    """``(pieces, masks)`` of one closed subpath.  A corner lies between two consecutive pieces with unit end and start tangents u,
    v when ``dot(u, v) <= 0`` or ``|cross(u, v)| > sin(angle)``.  No corner: every piece is white (7).  Two or more: the spans
    between corners take cyan (6), magenta (5), yellow (3) in turn, the last span magenta when the span count is 1 modulo 3 (so
    that it differs from both neighbours).  Exactly one: three spans by piece index from the corner on, after cutting every piece
    in three when there are fewer than three.  A piece that is a point has no tangent: it is white and is passed over."""
    tan = [_tangents(p) for p in pieces]
    real = [k for k, t in enumerate(tan) if t is not None]
    masks = [WHITE] * len(pieces)
    if not real:
        return pieces, masks
    limit = math.sin(angle)
    corners = []           # (positions in `real` of the pieces that BEGIN at a corner)
    for j, k in enumerate(real):
        u, v = tan[real[j - 1]][1], tan[k][0]
        if u[0] * v[0] + u[1] * v[1] <= 0.0 or abs(u[0] * v[1] - u[1] * v[0]) > limit:
            corners.append(j)
    if not corners:
        return pieces, masks
    if len(corners) == 1:
        order = real[corners[0]:] + real[:corners[0]]
        if len(order) < 3:
            cut = {k: _thirds(pieces[k]) for k in order}
            place, new_pieces = {}, []
            for k, p in enumerate(pieces):
                for part in cut.get(k, [p]):
                    place.setdefault(k, []).append(len(new_pieces))
                    new_pieces.append(part)
            order = [i for k in order for i in place[k]]
            pieces, masks = new_pieces, [WHITE] * len(new_pieces)
        for i, k in enumerate(order):
            masks[k] = _TURN[3 * i // len(order)]
        return pieces, masks
    spans = len(corners)
    for s, j0 in enumerate(corners):
        j1 = corners[s + 1] if s + 1 < spans else corners[0] + len(real)
        mask = MAGENTA if (s == spans - 1 and spans % 3 == 1) else _TURN[s % 3]
        for j in range(j0, j1):
            masks[real[j % len(real)]] = mask
    return pieces, masks


def _chord_area(pieces) -> float:
    """Twice the signed area of the polygon through the pieces' start points."""
    pts = [p[0].tolist() for p in pieces]
    return sum(a[0] * b[1] - b[0] * a[1] for a, b in zip(pts, pts[1:] + pts[:1]))


def _coloured(path, angle: float):
    """(`colour_edges`' soups, the summed chord-polygon area) of `path`: one pass over its pieces."""
    lines, cubics, area = {}, {}, 0.0
    for sub in path.subpaths:
        pieces = _pieces(sub)
        area += _chord_area(pieces)
        pieces, masks = colour_subpath(pieces, angle)
        for piece, mask in zip(pieces, masks):
            (lines if len(piece) == 2 else cubics).setdefault(mask, []).append(piece.reshape(-1))
    out = []
    for mask in (WHITE, CYAN, MAGENTA, YELLOW):
        ls, cs = lines.get(mask, []), cubics.get(mask, [])
        if not ls and not cs:
            continue
        segs = np.zeros((len(ls) + len(cs), 8))
        if ls:
            segs[:len(ls), :4] = np.array(ls)
        if cs:
            segs[len(ls):] = np.array(cs)
        kinds = np.zeros(len(segs), dtype=np.uint8)
        kinds[len(ls):] = _abi.SEG_CUBIC
        out.append((mask, segs, kinds))
    return out, area


def colour_edges(path, angle: float = 3.0):
    """The segments of `path` dealt out by colour: up to four ``(mask, segs (n, 8), kinds (n,))`` soups in the layout of
    ``Path.packed()`` (lines first, then cubics), in the order white, cyan, magenta, yellow, only those that hold a segment.  They
    become up to four paths of a batch that share one transform and form one group of svgr_batch_msdf.  Every subpath is coloured
    on its own (`colour_subpath`); its closing line is a segment like any other."""
    return _coloured(path, angle)[0]


def _sigma(area: float, m6) -> int:
    det = 1.0 if m6 is None else float(m6[0]) * float(m6[4]) - float(m6[1]) * float(m6[3])
    return -1 if ((area > 0.0) - (area < 0.0)) * ((det > 0.0) - (det < 0.0)) < 0 else 1


def orientation(path, m6=None) -> int:
    """sigma of svgr_batch_msdf for `path` under the six numbers `m6`: the sign of the summed area of the subpaths' chord polygons
    (through the segments' start points) in user space, times the sign of the transform's determinant; +1 when that is 0."""
    return _sigma(sum(_chord_area(_pieces(sub)) for sub in path.subpaths), m6)


def shapes_batch(shapes, angle: float = 3.0, flatness: float = FLATNESS):
    """``(batch, colour, group_off, orient)`` of `shapes`, ``(path, m6, fill rule code)`` each: up to four paths per shape, one per
    colour, and one group per shape that has a segment; None when none has."""
    segs, kinds, counts, m6s, rules, colours, group_off, orient = [], [], [], [], [], [], [0], []
    for path, m6, rule in shapes:
        soups, area = _coloured(path, angle)
        for mask, s, k in soups:
            segs.append(s)
            kinds.append(k)
            counts.append(len(s))
            m6s.append(m6)
            rules.append(rule)
            colours.append(mask)
        if soups:
            group_off.append(len(colours))
            orient.append(_sigma(area, m6))
    if not colours:
        return None
    n = len(colours)
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    batch = _abi.Batch(_abi.Context.get(), np.concatenate(segs), np.concatenate(kinds), offs, np.array(m6s, dtype=np.float64),
                       np.array(rules, dtype=np.uint8), np.zeros((n, 4)), viewport=None, flatness=flatness)
    return batch, np.array(colours, dtype=np.uint8), np.array(group_off, dtype=np.int32), np.array(orient, dtype=np.int8)


def shapes_msdf(shapes, rows: int, cols: int, origin, spread: float, enc: str, angle: float = 3.0, flatness: float = FLATNESS) -> np.ndarray:
    """The ``(rows, cols, 4)`` field of `shapes` over the grid at `origin` = (row0, col0): one batch, one query."""
    built = shapes_batch(shapes, angle, flatness) if rows * cols else None
    if built is None:
        return _abi.sdf_encode(np.full((rows, cols, 4), spread), spread, enc)
    batch, colours, group_off, orient = built
    try:
        return batch.msdf(colours, group_off, orient, grid=(origin[0], origin[1], rows, cols), spread=spread, out=enc).reshape(rows, cols, 4)
    finally:
        batch.destroy()


def msdf_angle(angle) -> float:
    """The corner threshold as a float: 0 <= angle <= pi (ValueError before any device work)."""
    try:
        a = float(angle)
    except (TypeError, ValueError):
        raise ValueError(f"an angle is a number, not {angle!r}") from None
    if not 0.0 <= a <= math.pi:
        raise ValueError(f"an angle lies in [0, pi], not {angle!r}")
    return a


def path_msdf(path, transform, viewport, spread: float = 8.0, dtype=np.float32, fill_rule=None, angle: float = 3.0,
              flatness: float = FLATNESS) -> np.ndarray:
    """``Path.msdf``: the argument checks of ``Path.sdf``, then one shape."""
    enc = _SDF_DTYPES.get(_sdf_dtype(dtype))
    if enc is None:
        raise TypeError(f"an MSDF is float64, float32 or uint8, not {dtype!r}")
    if fill_rule not in _RULES:
        raise ValueError(f"Invalid fill rule: {fill_rule}")
    row0, col0, rows, cols = (int(v) for v in viewport)
    if rows < 0 or cols < 0:
        raise ValueError("a viewport has rows >= 0 and cols >= 0")
    spread = _abi.sdf_spread(spread, finite=enc != "f64")
    angle = msdf_angle(angle)
    m6 = (transform if transform is not None else Transform()).m6()
    return shapes_msdf([(path, m6, _RULES[fill_rule])], rows, cols, (row0, col0), spread, enc, angle, flatness)


def font_msdf_atlas(font, string: str, size: float, spread: float, dtype=np.uint8, max_cols: int = 1024, angle: float = 3.0,
                    flatness: float = FLATNESS) -> SdfAtlas:
    """``Font.msdf_atlas``: the distinct glyphs of `string`, in the order of their first appearance."""
    atlas_arguments(size, spread, dtype, max_cols)
    msdf_angle(angle)
    placed, _advance = font.str_to_glyphs(string)
    glyphs, seen = [], set()
    for _pen, glyph in placed:
        if id(glyph) not in seen:
            seen.add(id(glyph))
            glyphs.append(glyph)
    return glyphs_msdf_atlas(glyphs, [glyph_key(g) for g in glyphs], font.units_per_em, size, spread, dtype, max_cols, angle, flatness)


def glyphs_msdf_atlas(glyphs, keys, units_per_em: float, size: float, spread: float, dtype=np.uint8, max_cols: int = 1024, angle: float = 3.0,
                      flatness: float = FLATNESS) -> SdfAtlas:
    """The MSDF atlas of a list of glyphs under the keys given: the cells of ``glyphs_sdf_atlas`` exactly (`atlas_layout`,
    `cell_m6`), one batch, one group per glyph with an outline, one query.  Cells are disjoint and a glyph lies at least
    ``ceil(spread)`` inside its own, so in a cell every other glyph is +spread in all four channels and the minimum over the groups
    is the cell's own glyph's field, as in sdf.py."""
    size, spread, enc = atlas_arguments(size, spread, dtype, max_cols)
    angle = msdf_angle(angle)
    paths = [g.path for g in glyphs]
    cells, rows, cols = atlas_layout(keys, [p.user_box() for p in paths], [g.advance for g in glyphs], size, units_per_em, spread, max_cols)
    if rows * cols == 0:
        return SdfAtlas(np.zeros((0, 0, 4), dtype=_abi.SDF_OUT[enc][1]), size, spread, cells)
    scale = size / units_per_em
    shapes = [(path, cell_m6(cells[key], scale), 0) for key, path in zip(keys, paths) if cells[key].rows]
    return SdfAtlas(shapes_msdf(shapes, rows, cols, (0, 0), spread, enc, angle, flatness), size, spread, cells)
