"""Directed cases for the tile kernel's per-path layer outputs -- SVGR_OUT_MASK_F64 / FILL_F64 (one path) and MASKS_F64 / FILLS_F64
(every path of a batch, back to back) --, the `OUT > 1` branch of `process`: where a layer starts and ends relative to the 16 x 64
tile grid, the 8-row halves of the two waves and the 8-pixel chunk of a lane, class-1 tiles, tiles of the bbox the path never
touches, layers the viewport cuts, the `mask < 1e-6` cut, and layers of several paths that share tiles.  Host only.

Positions are in PIXELS from the viewport's origin (`lbox`, pathbuild_cases.poly) or in tile units (canvas_cases.Geo); like the
cases of tests/canvas_cases.py every case is built at both ORIGINS.  A path's layer is oracle.bbox: floor(min) - 1 .. ceil(max) + 1
(exclusive) per axis, cut to the viewport -- so a layer inside the viewport is at least two pixels high and wide: the layers of one
row, of one column and of 1 x 1 pixel are cut out by a viewport of that size.

A case (`LCase`) is its paths (path data, rule, premultiplied paint) in batch order, a viewport (None: the layer is the path's own
bbox and the tile grid starts there), the tiles it is about and what it claims of itself (`want`, `classes`, `exact`, `items`);
tests/test_layer_out_cases_host.py proves the claims from the reference.  The reference of a path's mask is canvas_ref.mask_layer
(oracle.path_mask), of its fill `mask[..., None] * paint`; `reference` computes both once per case and hands them out read-only.

`shift` (rows, cols): the same geometry translated by whole pixels, as svgr_batch_set_transforms moves it: the reference adds the
shift to the path's points (y + 3.0 is one rounding on the device and here) and asks the oracle for the mask of those."""
from __future__ import annotations

from types import MappingProxyType
from typing import NamedTuple

import numpy as np

from oracle import oracle as orc
from tests import canvas_cases as cc
from tests import canvas_ref as cr
from tests.canvas_cases import ORIGINS, PAINTS, TC, TR, VIEW, Geo, cell_class, tile_box   # noqa: F401  (the cases' vocabulary)
from tests.pathbuild_cases import PAGE_ITEMS, filler, layer_of, poly   # noqa: F401

HALF = TR // 2
ZERO = {None: 0.0, "evenodd": 0.0}   # a tile that holds only a layer's margin row / column, or nothing of the path: exactly 0.0
SHIFT = (3, -5)                       # the translation of the set_transforms route: (rows, cols)
DEEP_COUNTS = (23, 24, 25, 26)        # on either side of PAGE_ITEMS
SLIVER_BELOW, SLIVER_KEPT = 5e-7, 2e-6   # raw coverages on either side of the cut
SLIVER_ROWS = (20, 26)                # the pixel rows (from the viewport's origin) the two slivers lie in
SLIVER_COLS = (70, 140)               # ... and their first / last column


class LCase(NamedTuple):
    name: str
    paths: tuple              # ((path data, rule, paint), ...) in batch order
    viewport: tuple           # (r0, c0, rows, cols) or None
    tiles: tuple = ()         # (band, column tile) the case is about -- of the grid that starts at the viewport (or at the layer)
    what: str = ""            # the seam the case is named for
    want: dict = MappingProxyType({})   # what the (first path's) layer must be: see test_layer_out_cases_host.py
    classes: tuple = ()       # (path, band, column tile, class): from the geometry (the class of a cell does not ask the rule)
    exact: tuple = ()         # (path, band, column tile, value): the reference holds exactly that value in all of the tile's layer pixels
    items: tuple = ()         # ((band, column tile), count): paths with a cell there
    empty: tuple = ()         # paths without a layer
    named: tuple = ()         # multi-path: the paths the case is about


# --------------------------------------------------------------------------------------------------------------------------------
# the reference
# --------------------------------------------------------------------------------------------------------------------------------
def mask_ref(d, rule, viewport, shift=(0, 0)):
    """(mask (rows, cols), (r0, c0, rows, cols)) of the path's layer, or (None, None) when it has none."""
    if tuple(shift) == (0, 0) and viewport is not None:
        m, bb = cr.mask_layer(d, rule, viewport)
        if bb is None:
            return None, None
        r, c = bb[0] - viewport[0], bb[1] - viewport[1]
        return np.ascontiguousarray(m[r:r + bb[2], c:c + bb[3]]), bb
    lines, cubics = cr.segments(d)
    s = np.array(shift, dtype=np.float64)
    res = orc.path_mask(lines + s, cubics + s, None, rule, viewport)
    if res is None:
        return None, None
    m, (r0, c0), _e = res
    return m, (int(r0), int(c0), m.shape[0], m.shape[1])


def raw_coverage(d, rule, viewport, shift=(0, 0)):
    """canvas_ref.raw_coverage; of the translated points with a `shift`."""
    if tuple(shift) == (0, 0):
        return cr.raw_coverage(d, rule, viewport)
    lines, cubics = cr.segments(d)
    s = np.array(shift, dtype=np.float64)
    edges = orc.path_edges(lines + s, cubics + s)
    bb = orc.bbox(edges, viewport) if len(edges) else None
    if bb is None:
        return None
    trace = np.zeros((bb[2], bb[3]))
    for e in edges - np.array([bb[0], bb[1]], dtype=np.float64):
        orc.line_coverage(trace, e)
    s = np.cumsum(trace, axis=1)
    return np.fabs(s).clip(0, 1) if rule is None else np.fabs(np.remainder(s + 1.0, 2.0) - 1.0)


_REFS = {}


def reference(case, shift=(0, 0)):
    """[(mask, fill, bbox)] per path of the case -- (None, None, None) for a path without a layer --, computed once, read-only."""
    key = (case.name, tuple(shift))
    if key not in _REFS:
        out = []
        for d, rule, paint in case.paths:
            m, bb = mask_ref(d, rule, case.viewport, shift)
            if m is None:
                out.append((None, None, None))
                continue
            f = m[..., None] * np.asarray(paint, dtype=np.float64)
            m.flags.writeable = f.flags.writeable = False
            out.append((m, f, bb))
        _REFS[key] = out
    return _REFS[key]


def grid(case, shift=(0, 0)):
    """The viewport whose first pixel the tile grid starts at: the case's, or -- without one -- the path's own layer."""
    if case.viewport is not None:
        return case.viewport
    return reference(case, shift)[0][2]


# --------------------------------------------------------------------------------------------------------------------------------
# path data
# --------------------------------------------------------------------------------------------------------------------------------
def lbox(g, r0, c0, r1, c1):
    """A convex quadrilateral without an axis-aligned edge whose layer is exactly rows r0 .. r1 and columns c0 .. c1 (inclusive,
    pixels from the origin; at least three each): the layer reaches from floor(min) - 1 to ceil(max)."""
    assert r1 - r0 >= 2 and c1 - c0 >= 2
    x0, x1, y0, y1 = c0 + 1.3, c1 - 0.4, r0 + 1.3, r1 - 0.4
    w, h = x1 - x0, y1 - y0
    return poly(g, [(x0, y0 + 0.25 * h), (x0 + 0.8 * w, y0), (x1, y0 + 0.7 * h), (x0 + 0.15 * w, y1)])


def hbar(g, y, height, x0, x1):
    """A rectangle `height` high from row coordinate y: a sliver whose coverage is `height` in every whole pixel of its run."""
    return poly(g, [(x0, y), (x1, y), (x1, y + height), (x0, y + height)])


def c_shape(g):
    """A "C" open to the right over 4 bands x 4 column tiles: tiles (1 .. 2, 1 .. 3) lie in its bbox, and the
    path never touches them."""
    x0, x1, xa = 0.2 * TC, 3.7 * TC, 0.8 * TC
    y0, y1, ya, yb = 0.3 * TR, 3.4 * TR, 0.9 * TR, 3.05 * TR
    return poly(g, [(x0, y0), (x1, y0 + 0.4), (x1 - 0.3, ya), (xa, ya + 0.2), (xa + 0.4, yb), (x1 - 0.2, yb + 0.3), (x1, y1), (x0 + 0.3, y1 - 0.2)])


UNTOUCHED = ((1, 1), (1, 2), (1, 3), (2, 1), (2, 2), (2, 3))


# --------------------------------------------------------------------------------------------------------------------------------
# single-path cases
# --------------------------------------------------------------------------------------------------------------------------------
def _single(g):
    """(name, path data, viewport size or None, keywords) -- every one of them is built for both fill rules."""
    b1 = TR   # the first row of band 1
    # row starts: the first row of the layer at tile row 0, 7, 8, 15 (wrow0 and the skip test of the two waves)
    yield "row_start_0", lbox(g, b1 + 0, 70, b1 + 20, 150), VIEW, dict(tiles=((1, 1), (1, 2), (2, 1)), want=dict(row0=0), what="first row at tile row 0, into the next band")
    yield "row_start_7", lbox(g, b1 + 7, 70, b1 + 12, 150), VIEW, dict(tiles=((1, 1), (1, 2)), want=dict(row0=7), what="first row at tile row 7: one row of the first wave")
    yield "row_start_8", lbox(g, b1 + 8, 70, b1 + 13, 150), VIEW, dict(tiles=((1, 1), (1, 2)), want=dict(row0=8, half=1), what="first row at tile row 8: the second wave alone")
    yield "row_start_15", lbox(g, b1 + 15, 70, b1 + 20, 150), VIEW, dict(tiles=((1, 1), (2, 1)), want=dict(row0=15), exact_by_rule=ZERO, exact_tiles=((1, 1),), what="first row at tile row 15: one row in this band")
    yield "row_first_half", lbox(g, b1 + 0, 70, b1 + 7, 150), VIEW, dict(tiles=((1, 1), (1, 2)), want=dict(row0=0, row_last=7, half=0), what="rows 0 .. 7 of one tile: the first wave alone")
    yield "row_second_half", lbox(g, b1 + 8, 70, b1 + 15, 150), VIEW, dict(tiles=((1, 1), (1, 2)), want=dict(row0=8, row_last=15, half=1), what="rows 8 .. 15 of one tile: the second wave alone")
    # row ends: on, one before, one past a band border
    yield "row_end_on_border", lbox(g, b1 + 4, 70, b1 + 15, 150), VIEW, dict(tiles=((1, 1),), want=dict(row_last=15), what="last row = last row of the band")
    yield "row_end_before_border", lbox(g, b1 + 4, 70, b1 + 14, 150), VIEW, dict(tiles=((1, 1),), want=dict(row_last=14), what="last row one before the band border")
    yield "row_end_past_border", lbox(g, b1 + 4, 70, b1 + 16, 150), VIEW, dict(tiles=((1, 1), (2, 1)), want=dict(row_last=0), exact_by_rule=ZERO, exact_tiles=((2, 1),), what="last row = first row of the next band")
    yield "one_row", lbox(g, -3, 50, 4, 230), (1, VIEW[1]), dict(tiles=((0, 0), (0, 3)), want=dict(rows=1, cut="tb"), what="a layer of one row")
    # column starts / ends: either side of a lane's 8-pixel chunk, the tile's first and last column
    for k in (0, 7, 8, 9, 63):
        yield f"col_start_{k}", lbox(g, 18, TC + k, 28, TC + k + 30), VIEW, dict(tiles=((1, 1),) + (((1, 2),) if k == 63 else ()), want=dict(col0=k), exact_by_rule=ZERO, exact_tiles=((1, 1),) if k == 63 else (), what=f"first column at tile column {k}")
    for k in (0, 7, 8, 63):
        c1 = 2 * TC + k
        yield f"col_end_{k}", lbox(g, 18, c1 - (20 if k == 63 else 30), 28, c1), VIEW, dict(tiles=((1, 2),) + (((1, 1),) if k == 0 else ()), want=dict(col_last=k), exact_by_rule=ZERO, exact_tiles=((1, 2),) if k == 0 else (), what=f"last column at tile column {k}")
    yield "one_col", lbox(g, 5, -3, 50, 4), (VIEW[0], 1), dict(tiles=((0, 0), (2, 0)), want=dict(cols=1, cut="lr"), what="a layer of one column")
    yield "one_pixel", lbox(g, -1, -1, 2, 5), (1, 1), dict(tiles=((0, 0),), want=dict(rows=1, cols=1, cut="tblr"), what="a layer of 1 x 1")
    # class 1: a rectangle inside a rectangle, wound the same way -- winding 2 inside: 1 under nonzero, 0 under even-odd.  The layer
    # starts inside column tile 0 and ends inside column tile 3; tiles (1 .. 2, 1 .. 2) see carry-ins only
    ring = g.ring(0.3, 0.4, 3.4, 3.55, 0.6, 0.7, 3.1, 3.2)
    inner = tuple((b, t) for b in (1, 2) for t in (1, 2))
    yield "class1_interior", ring, VIEW, dict(
        tiles=inner + ((0, 0), (3, 3), (1, 0), (1, 3)), want=dict(col0=int(0.4 * TC) - 1, col_last=int(np.ceil(3.55 * TC)) - 3 * TC, bands=4, ctiles=4),
        classes=tuple((0, b, t, 1) for b, t in inner) + ((0, 1, 0, 2), (0, 1, 3, 2)), exact_by_rule={None: 1.0, "evenodd": 0.0}, exact_tiles=inner,
        what="3 x 3 tiles and more, the inner ones class 1, winding 2")
    # ... and class 1 in a column tile the layer does NOT fill: the viewport cuts the shape (whose right edges lie outside), so the
    # layer ends with the viewport inside column tile 3 and the carry-in runs up to there; the top edge lies inside row 3 of band 1:
    # the layer starts in row 2 of the band, which gets nothing, row 3 a fraction.  (A class-1 cell in a layer's FIRST column tile that starts inside the
    # tile does not exist: nothing of a path lies left of its layer, so no row there has a carry-in.)
    cut = poly(g, [(0.45 * TC, TR + 3.3), (4.5 * TC, TR + 3.3), (4.6 * TC, 2 * TR + 9.6), (0.5 * TC, 2 * TR + 9.6)])
    yield "class1_cut_right", cut, VIEW, dict(tiles=((1, 1), (1, 2), (1, 3), (2, 3)), want=dict(col0=int(0.45 * TC) - 1, cut="r"),
                                             classes=((0, 1, 0, 2), (0, 1, 1, 1), (0, 1, 2, 1), (0, 1, 3, 1), (0, 2, 3, 1)),
                                             what="class 1 up to a layer end inside the tile")
    # tiles of the bbox the path never touches: the memset alone writes them
    yield "untouched_tiles", c_shape(g), VIEW, dict(tiles=((0, 0), (3, 3), (1, 0)) + UNTOUCHED, classes=tuple((0, b, t, 0) for b, t in UNTOUCHED),
                                                     exact_by_rule=ZERO, exact_tiles=UNTOUCHED, what="tiles inside the bbox without a cell")
    # the viewport cuts the bbox
    bv, tv = VIEW[0] / TR, VIEW[1] / TC
    yield "cut_top", g.blob(0.1, 1.6, 0.7, 0.9), VIEW, dict(tiles=((0, 1), (0, 2)), want=dict(cut="t"), what="the bbox cut above")
    yield "cut_bottom", g.blob(bv - 0.1, 1.6, 0.7, 0.9), VIEW, dict(tiles=((3, 1), (3, 2)), want=dict(cut="b"), what="the bbox cut below")
    yield "cut_left", g.blob(1.6, 0.1, 0.9, 0.6), VIEW, dict(tiles=((1, 0), (2, 0)), want=dict(cut="l"), what="the bbox cut on the left")
    yield "cut_right", g.blob(1.6, tv - 0.1, 0.9, 0.6), VIEW, dict(tiles=((1, 3), (2, 3)), want=dict(cut="r"), what="the bbox cut on the right")
    small = (37, 150)
    yield "cut_all_sides", g.blob(small[0] / TR / 2, small[1] / TC / 2, 1.3, 1.3), small, dict(
        tiles=((0, 0), (0, 2), (2, 0), (2, 2)), want=dict(cut="tblr"), what="the bbox cut on all four sides: the layer is the viewport")
    yield "outside", g.rect(-3.0, -3.0, -2.0, -2.0), VIEW, dict(empty=(0,), what="wholly outside: no layer, nothing written")
    # the cut: a sliver below it over a run of pixels (exactly 0.0) and one above it (kept), in one path
    (ra, rb), (ca, cb) = SLIVER_ROWS, SLIVER_COLS
    yield "slivers_at_the_cut", hbar(g, ra + 0.3, SLIVER_BELOW, ca + 0.1, cb + 0.9) + " " + hbar(g, rb + 0.3, SLIVER_KEPT, ca + 0.1, cb + 0.9), VIEW, dict(
        tiles=((1, 1), (1, 2)), what="raw coverage 5e-7 (dropped) and 2e-6 (kept)")
    # no viewport: the layer is the path's own bbox and the tile grid starts at it
    yield "no_viewport", g.blob(1.4, 1.3, 1.2, 1.1), None, dict(tiles=((0, 0), (1, 1), (2, 2)), want=dict(bands=3, ctiles=3, row0=0, col0=0), what="viewport=None")


def _single_cases(g, tag):
    out = []
    for n, (name, d, view, kw) in enumerate(_single(g)):
        for rule in (None, "evenodd"):
            k = dict(kw)
            by_rule, tiles = k.pop("exact_by_rule", None), k.pop("exact_tiles", ())
            if by_rule is not None:
                k["exact"] = tuple((0, b, t, by_rule[rule]) for b, t in tiles)
            vp = None if view is None else (g.r, g.c, *view)
            out.append(LCase(f"{name}_{'evenodd' if rule else 'nonzero'}-{tag}", ((d, rule, PAINTS[n % 8]),), vp, **k))
    return out


# --------------------------------------------------------------------------------------------------------------------------------
# multi-path cases
# --------------------------------------------------------------------------------------------------------------------------------
SHARED_TILE = (1, 1)


def _neighbours(g):
    """Eight paths around tile (1, 1): an empty one (outside the viewport) first, in the middle and last, the others with layers of
    different sizes that all have a cell in the tile; every third path even-odd."""
    shapes = [g.rect(-3.0, -3.0, -2.0, -2.0),
              lbox(g, 10, 30, 40, 140),
              g.ring(0.7, 0.9, 2.6, 2.4, 1.2, 1.3, 2.1, 1.95),
              g.rect(5.0, 5.0, 6.0, 6.0),
              g.blob(1.5, 1.9, 0.8, 0.9),
              lbox(g, 20, 100, 33, 200),
              g.blob(1.2, 2.2, 0.5, 0.45),
              g.rect(-2.5, 1.0, -1.5, 2.0)]
    return tuple((d, "evenodd" if i % 3 == 2 else None, PAINTS[i % 8]) for i, d in enumerate(shapes))


NEIGHBOUR_EMPTY = (0, 3, 7)


def _multi_cases(g, tag):
    out = []
    vp = (g.r, g.c, *VIEW)
    nb = _neighbours(g)
    live = tuple(i for i in range(len(nb)) if i not in NEIGHBOUR_EMPTY)
    out.append(LCase(f"neighbours-{tag}", nb, vp, tiles=(SHARED_TILE, (1, 2), (0, 1), (2, 1)), empty=NEIGHBOUR_EMPTY, named=live,
                     items=((SHARED_TILE, len(live)),), what="layers of different widths that share tiles, empty paths between them"))
    for n in DEEP_COUNTS:
        entries, _groups, kw = cc._deep(g, "plain", n)
        out.append(LCase(f"deep_{n}-{tag}", tuple((e.d, e.rule, e.paint) for e in entries), (g.r, g.c, *cc.DEEP_VIEW), tiles=(cc.DEEP_TILE,),
                         named=tuple(range(n)), items=kw["items"], what=f"{n} layers with a cell in one tile (a page holds {PAGE_ITEMS})"))
    # beyond 4096 segments: the plan orders slabs, the replays run under the plan's places
    big = nb[:7] + ((filler(g, VIEW), None, PAINTS[7]),) + nb[7:]
    out.append(LCase(f"big_neighbours-{tag}", big, vp, tiles=(SHARED_TILE, (1, 2), (0, 3)), empty=(0, 3, 8), named=live + (7,),
                     items=((SHARED_TILE, len(live)),), what="the neighbours in a batch of more than 4096 segments"))
    return out


def _all():
    single, multi = [], []
    for origin in ORIGINS:
        g, tag = Geo(origin), "o%d_%d" % origin
        single += _single_cases(g, tag)
        multi += _multi_cases(g, tag)
    return single, multi


SINGLE, MULTI = _all()
CASES = SINGLE + MULTI
SINGLE_IDS, MULTI_IDS, IDS = [c.name for c in SINGLE], [c.name for c in MULTI], [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}
BIG = [c for c in MULTI if c.name.startswith("big_")]
SMALL_MULTI = [c for c in MULTI if not c.name.startswith("big_")]


def base_name(case):
    return case.name.split("-", 1)[0]


def n_segments(case):
    from svgrasterize_amd import Path

    return sum(len(Path.from_svg(d).packed()[0]) for d, _r, _p in case.paths)
