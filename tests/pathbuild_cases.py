"""Directed cases for the three geometry kernels between the flatten and the tile kernel -- k_path_build<0|1|2> (with the slab
cutting of k_path_bbox), k_band_entries and k_tile_lists -- at the sizes where their code takes another path, and the integer
rules those sizes follow from, restated in plain Python.

The constants are the ones of svgrasterize.py_amd/csrc/svgr_hip.hip.  The restatements:

  layer_of      the path's layer: oracle.bbox (floor - 1 / ceil + 1, cut to the viewport), as tests/test_path_box_host.py pins it
  path_ctiles   the column tiles a layer spans, from the viewport's first column
  slab_shape    how a path of nb bands x nct column tiles is cut: bands per slab, column-tile runs per band row
  slabs_of      the slab list k_path_bbox writes for a path: (first band, bands, k0, nk), band rows outside, column runs inside
  stage         what k_path_build's stage() makes of a slab's edges: per batch of PB_BATCH edges the kept (live) edges and the
                (edge, row) tasks -- an edge's rows [y_begin, y_end) cut to the slab's rows.  y_begin / y_end and the rule by which
                an edge is dropped come from the host build of csrc/svgr_core.h (edge_setup through tests/host_harness.cpp): the
                rounding rules are not written a second time.

Every path here is a solid fill made of straight lines, every vertex inside the viewport's rows or -- the slab shapes -- below its
last row (the flatten keeps every line that meets the viewport's rows: the path's edge range is then the reference's edge list,
edge for edge, and so are the batches).  Positions are in pixels from the viewport's origin; like tests/canvas_cases.py every case
is built at both ORIGINS, so that the tile grid starts on no multiple of 16 / 64 in one of them.

A case (`PB`) is a canvas_cases.Case -- its `tiles` under test, its `layout` rows ("entry", path, band, column tile, class) --
plus the slab list of every path under test (`slabs`) and, where the case is about them, the live edges and task totals of every
batch (`batches`).  tests/test_pathbuild_cases_host.py checks all of it from the reference and these restatements."""
from __future__ import annotations

import ctypes as C
import functools
from typing import NamedTuple

import numpy as np

from oracle import oracle as orc
from tests.canvas_cases import FAINT, ORIGINS, PAINTS, TC, TR, Case, Geo
from tests.canvas_ref import Entry, edges_of
from tests.util import host_build

PB_THREADS, PB_CELLS, PB_BANDS, PB_BATCH = 256, 80, 16, 256   # k_path_build
DET_LANES = 64                 # lanes that take the rows under SVGR_RENDER_DETERMINISTIC
BE_BLOCK, BE_KEEP = 1024, 4    # k_band_entries
TL_BLOCK, PAGE_ITEMS = 1024, 24   # k_tile_lists
WEIGHT_MAX = 63                # weight_of saturates here


class PB(NamedTuple):
    case: Case
    slabs: tuple = ()      # ((path, ((band0, nb, k0, nk), ...)), ...): the slab list of every path under test
    batches: tuple = ()    # ((path, slab index, ((live edges, tasks), ...)), ...): per batch of PB_BATCH edges
    what: str = ""         # the seam the case is named for

    @property
    def name(self):
        return self.case.name


# --------------------------------------------------------------------------------------------------------------------------------
# the restatements
# --------------------------------------------------------------------------------------------------------------------------------
def layer_of(d, viewport):
    """(r0, c0, rows, cols) of the path's layer, or None."""
    edges = edges_of(d)
    return orc.bbox(edges, tuple(int(v) for v in viewport)) if len(edges) else None


def path_ctiles(c0, cols, vc0):
    ct0 = (c0 - vc0) // TC
    return ct0, (c0 + cols - 1 - vc0) // TC - ct0 + 1


def path_bands(r0, rows, vr0):
    b0 = (r0 - vr0) // TR
    return b0, (r0 + rows - 1 - vr0) // TR - b0 + 1


def slab_shape(nb, nct):
    """(bands per slab, column-tile runs per band row)"""
    if nct <= PB_CELLS:
        return min(PB_CELLS // nct, PB_BANDS), 1
    return 1, -(-nct // PB_CELLS)


def owns_band(band, rank=0, world=1, strip=1):
    return world <= 1 or (band // strip) % world == rank


def slabs_of(d, viewport, rank=0, world=1, strip=1):
    """[(band0, nb, k0, nk)]: the path's slabs in k_path_bbox's order; band runs without a band of this rank are left out."""
    layer = layer_of(d, viewport)
    if layer is None:
        return []
    r0, c0, rows, cols = layer
    b0, nb = path_bands(r0, rows, viewport[0])
    _ct0, nct = path_ctiles(c0, cols, viewport[1])
    bands_per, col_runs = slab_shape(nb, nct)
    out = []
    for bb in range(0, nb, bands_per):
        be = min(bb + bands_per, nb)
        if not any(owns_band(b0 + b, rank, world, strip) for b in range(bb, be)):
            continue
        for c in range(col_runs):
            out.append((b0 + bb, be - bb, c * PB_CELLS, min(nct - c * PB_CELLS, PB_CELLS)))
    return out


@functools.lru_cache(maxsize=None)
def _harness():
    lib = host_build("host_harness")
    lib.hh_edge_rows.argtypes = [np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS"), C.c_long, C.c_int, C.c_int, C.c_int, C.c_int,
                                 np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")]
    lib.hh_edge_rows.restype = None
    return lib


def edge_rows(d, viewport):
    """Per edge of the path, in edge order: (y_begin, y_end, kept) in layer rows -- edge_setup of csrc/svgr_core.h and stage()'s
    `cmin >= cols + 2` rule, against the path's layer."""
    r0, c0, rows, cols = layer_of(d, viewport)
    e = np.ascontiguousarray(edges_of(d).reshape(-1, 4))
    out = np.zeros((len(e), 3), dtype=np.int32)
    _harness().hh_edge_rows(e, len(e), r0, c0, rows, cols, out)
    return out


def stage(d, viewport, slab):
    """[(live edges, tasks)] per batch of PB_BATCH edges of the path, for one slab (band0, nb, k0, nk)."""
    r0 = layer_of(d, viewport)[0]
    sr0 = viewport[0] + slab[0] * TR - r0
    sr1 = sr0 + slab[1] * TR
    er = edge_rows(d, viewport)
    cnt = np.where(er[:, 2] != 0, np.clip(np.minimum(er[:, 1], sr1) - np.maximum(er[:, 0], sr0), 0, None), 0)
    return [(int((cnt[i:i + PB_BATCH] > 0).sum()), int(cnt[i:i + PB_BATCH].sum())) for i in range(0, len(cnt), PB_BATCH)]


def tasks_per_lane(total, lanes):
    return -(-total // lanes)


def band_groups(n_paths):
    """(groups of 64 paths per wave, paths per wave) of k_band_entries"""
    groups = -(-n_paths // BE_BLOCK)
    return groups, groups * 64


# --------------------------------------------------------------------------------------------------------------------------------
# path data
# --------------------------------------------------------------------------------------------------------------------------------
def poly(g, pts):
    """A closed polygon through `pts` ((x, y) in pixels from the origin)."""
    f = lambda p: f"{float(g.c + p[0])!r},{float(g.r + p[1])!r}"
    return f"M{f(pts[0])} " + " ".join(f"L{f(p)}" for p in pts[1:]) + " Z"


def _view(nb, nct, extra_cols=40):
    """A viewport of nb bands (the last cut to 9 rows) and, by default, one more column tile than the shapes use (cut to 40)."""
    return ((nb - 1) * TR + 9, nct * TC + extra_cols)


def slab_shape_path(g, nb, nct, right="mid"):
    """Two quadrilaterals, wound the same way, over nb bands x nct column tiles; both run out below the viewport, so that their
    bottom edges never show and every band but the first has cells without an edge.

      main   top edge inside pixel row 3, from column tile 0 to the last one: ONE row whose middle run crosses every tile border
             (at nct > 80 the border between tiles 79 and 80: the run border cuts the row's middle run); left edge slanted over
             the first two or three column tiles and across every band border; right edge steep across every band border
      inner  over the last four column tiles: its inside is covered twice (0 under even-odd, 1 under nonzero)

    `right`: "mid" the layer ends inside the last tile; "border" exactly on a tile border (no sentinels); "cut" the viewport cuts
    the shape: the right edges lie wholly right of the layer, the first vertex hangs out left of the viewport."""
    w, below = nct * TC, nb * TR
    slant = min(2.6, 0.45 * nct) * TC
    if right == "cut":
        main = [(-0.4 * TC, 3.2), (w + 0.2 * TC, 3.8), (w + 0.5 * TC, below + 9.6), (slant, below + 11.2)]
        inner = [(w - 3.65 * TC, 8.0), (w + 0.3 * TC, 8.8), (w + 0.4 * TC, below + 9.6), (w - 3.6 * TC, below + 10.4)]
    else:
        x_end = w - 1.5 if right == "border" else w - 0.3 * TC   # (the layer ends at ceil(x_end) + 1)
        main = [(0.3 * TC, 3.2), (x_end - 9.6, 3.8), (x_end, below + 9.6), (slant, below + 11.2)]
        inner = [(w - 3.65 * TC, 8.0), (w - 0.7 * TC, 8.8), (w - 0.65 * TC, below + 9.6), (w - 3.6 * TC, below + 10.4)]
    return poly(g, main) + " " + poly(g, inner)


def zigzag(g, n_edges, x0=19.3, y_top=5.3, y_mid=27.6, y_bot=41.7, width=270.0):
    """A comb of exactly `n_edges` edges, none of them horizontal: n_edges - 3 teeth edges between y_top and y_mid, a right side,
    a shallow bottom and the closing left side."""
    m = n_edges - 3
    pts = [(x0 + width * i / m, y_top if i % 2 == 0 else y_mid + 3.1 * ((i * 7) % 5) / 5.0) for i in range(m + 1)]
    pts += [(x0 + width - 2.3, y_bot), (x0 + 1.9, y_bot - 0.7)]
    return poly(g, pts)


def tall_zigzag(g, rows_a, rows_b):
    """About 600 edges over 17 bands x 5 column tiles: 256 edges down the left side inside the first 16 bands (the first batch: no
    live edge in the last band's slab), 200 more that end in the last band (a batch that is live in both slabs, in part), and the
    way back up on the right."""
    pts = []
    for i in range(257):   # edges 0 .. 255
        pts.append((21.4 + (9.7 if i % 2 else 0.0) + 0.11 * i, 3.3 + (rows_a - 12.0) * i / 256.0))
    y = pts[-1][1]
    for i in range(1, 201):   # edges 256 .. 455: the last 60 or so inside the last band
        pts.append((49.8 + (7.9 if i % 2 else 0.0) + 0.2 * i, y + (rows_b - 4.6 - y) * i / 200.0))
    for i in range(1, 141):   # edges 456 ..: up again
        pts.append((232.3 + (11.3 if i % 2 else 0.0) + 0.3 * i, rows_b - 4.6 - (rows_b - 9.1) * i / 140.0))
    return poly(g, pts)


SLIVER_X0, SLIVER_Y0, SLIVER_DX = 14.3, 3.5, 23.7


def slivers(g, heights):
    """One path of thin triangles side by side, apex up: a triangle of height h has two long edges of h rows each and a base of one
    row: 2 h + 1 tasks."""
    d = []
    for j, h in enumerate(heights):
        x = SLIVER_X0 + SLIVER_DX * j
        d.append(poly(g, [(x + 4.2, SLIVER_Y0), (x + 9.9, SLIVER_Y0 + h - 1), (x + 1.1, SLIVER_Y0 + h - 1 - 0.25)]))
    return " ".join(d)


def sliver_slab(heights):
    """the one slab of slivers(): the layer reaches one row / column past ceil() of the largest coordinate"""
    last_row = int(np.ceil(SLIVER_Y0 + max(heights) - 1))
    last_col = int(np.ceil(SLIVER_X0 + SLIVER_DX * (len(heights) - 1) + 9.9))
    return (0, last_row // TR + 1, 0, last_col // TC + 1)


def single_edge(g, rows, view_cols):
    """One long edge inside the viewport; the rest of the outline is horizontal (no rows) or wholly right of the layer (dropped)."""
    xr = view_cols + 37.5
    return poly(g, [(33.4, 3.5), (45.1, 3.5 + rows - 1), (xr, 3.5 + rows - 1), (xr, 3.5)])


def one_row_edges(g, n, y_top=4.5, row=157):
    """A long left edge first, then `n` edges of one row each along the bottom (all inside pixel row `row`), the right side and the
    closing top edge: the first batch is one edge of many rows and 255 of one -- lanes whose runs hold several edges."""
    pts = [(12.3, y_top), (15.8, row + 0.2)]
    for i in range(1, n + 1):
        pts.append((15.8 + 0.8 * i, row + (0.8 if i % 2 else 0.2)))
    pts.append((15.8 + 0.8 * n + 4.4, y_top + 0.6))
    return poly(g, pts)


def filler(g, view, n=4100):
    """A path of `n` short segments in the viewport's last tile of its first band: it takes the batch beyond the 4096 segments up to
    which the single-pass plan is tried."""
    x0 = ((view[1] - 1) // TC) * TC + 1.7
    m = n - 3
    pts = [(x0 + 0.0097 * i, 5.2 + (0.57 if i % 2 else 0.0)) for i in range(m + 1)]
    pts += [(x0 + 0.0097 * m - 0.4, 11.6), (x0 + 0.6, 11.1)]
    return poly(g, pts)


# --------------------------------------------------------------------------------------------------------------------------------
# the cases
# --------------------------------------------------------------------------------------------------------------------------------
SLAB_SHAPES = ((5, 17, 16), (6, 14, 13), (27, 3, 2), (40, 3, 2), (41, 2, 1), (80, 2, 1), (81, 2, 1), (161, 2, 1))   # (nct, nb, bands per slab)
MULTI_BAND = ("slab_5x17", "slab_6x14", "slab_27x3")     # the slabs of several bands: the sharded route
RIGHT_ENDS = ("border", "mid", "cut")
BATCH_EDGES = (255, 256, 257, 512, 513)
TASKS_256 = {255: (127,), 256: (100, 27), 257: (128,), 511: (100, 100, 54), 513: (100, 100, 55)}   # tasks: the slivers' heights
TASKS_64 = {63: (31,), 64: (20, 11), 65: (32,), 129: (64,)}
TWO_PASS = ("slab_161x2_nonzero", "slab_5x17_evenodd")


def _expect_slabs(nb, nct, per):
    runs = -(-nct // PB_CELLS) if nct > PB_CELLS else 1
    return tuple((b, min(per, nb - b), c * PB_CELLS, min(nct - c * PB_CELLS, PB_CELLS)) for b in range(0, nb, per) for c in range(runs))


def _slab_case(g, tag, nct, nb, per, rule, right="mid"):
    d = slab_shape_path(g, nb, nct, right)
    view = _view(nb, nct, -23 if right == "cut" else 40)
    vp = (g.r, g.c, *view)
    ev = rule == "evenodd"
    last = nct - 1
    x0, x1, y1 = (-0.4 if right == "cut" else 0.3) * TC, min(2.6, 0.45 * nct) * TC, nb * TR + 11.2
    slant_at = lambda band: int((x0 + (x1 - x0) * (band * TR + 4 - 3.2) / (y1 - 3.2)) // TC)   # the tile the slanted left edge crosses the band in
    # band 0: the one-row top edge runs through every tile; below: the slanted left edge, and the steep right one unless it is cut off
    # (under nonzero the part the inner quadrilateral covers as well is plainly 1: the slanted edge shows only left of it)
    tiles = [(0, 0), (0, min(79, last)), (0, last)] + [(b, slant_at(b)) for b in (1, nb - 1) if ev or slant_at(b) < nct - 4]
    tiles += [] if right == "cut" else [(nb - 1, last)]
    layout = [("entry", 0, 0, min(79, last), 2), ("entry", 0, nb - 1, nct - 2, 0 if ev else 1)]   # covered twice, no edge
    if nct > PB_CELLS:
        tiles.append((0, 80))
        layout.append(("entry", 0, 0, 80, 2))          # (right of the run border: a class-2 cell with carry-in adds)
    if nct > 2 * PB_CELLS:
        layout += [("entry", 0, 1, 80, 1), ("entry", 0, 1, 120, 1)]   # class 1, the carry-in from s_left
    if right == "cut":
        layout.append(("entry", 0, nb - 1, last, 0 if ev else 1))    # the viewport cuts the shape: the last tile has no edge either
    name = f"slab_{nct}x{nb}" + ("" if right == "mid" else f"_{right}") + f"_{'evenodd' if ev else 'nonzero'}-{tag}"
    case = Case(name, (Entry(d, rule, PAINTS[(nct + nb) % 8]),), (), vp, tuple(dict.fromkeys(tiles)), tuple(layout))
    return PB(case, ((0, _expect_slabs(nb, nct, per)),), (), f"{nct} column tiles x {nb} bands: {per} bands per slab")


def _batches_case(g, tag, name, d, view, slabs, batches, what, tiles, rule=None, paint=2):
    case = Case(f"{name}-{tag}", (Entry(d, rule, PAINTS[paint]),), (), (g.r, g.c, *view), tuple(tiles))
    return PB(case, ((0, tuple(slabs)),), tuple((0, i, None if b is None else tuple(b)) for i, b in batches), what)


def _per_origin(g, tag):
    out = []
    for nct, nb, per in SLAB_SHAPES:
        for rule in (None, "evenodd"):
            out.append(_slab_case(g, tag, nct, nb, per, rule))
    for k, right in enumerate(RIGHT_ENDS):
        if right != "mid":   # ("mid" is what every case above is)
            out.append(_slab_case(g, tag, 81, 2, 1, None if k else "evenodd", right))
            out.append(_slab_case(g, tag, 27, 3, 2, "evenodd" if k else None, right))
    # edge batches: 3 bands x 5 column tiles, one slab
    view3 = (2 * TR + 13, 4 * TC + 41)
    for n in BATCH_EDGES:
        d = zigzag(g, n)
        split = [(min(PB_BATCH, n - i), None) for i in range(0, n, PB_BATCH)]
        out.append(_batches_case(g, tag, f"batch_{n}_edges", d, view3, [(0, 3, 0, 5)], [(0, split)], f"{n} edges: {len(split)} batches",
                                 [(0, 0), (1, 2), (2, 4)], rule="evenodd" if n % 2 else None))
    view17 = (16 * TR + 9, 4 * TC + 41)
    out.append(_batches_case(g, tag, "batch_tall_two_slabs", tall_zigzag(g, 16 * TR, view17[0]), view17, [(0, 16, 0, 5), (16, 1, 0, 5)],
                             [(0, None), (1, None)], "597 edges over two slabs: compaction, a batch without a live edge", [(3, 0), (15, 1), (16, 1), (16, 3)]))
    # task runs: 9 bands x 5 column tiles, one slab, one batch
    view9 = (8 * TR + 9, 4 * TC + 41)
    for lanes, table in ((PB_THREADS, TASKS_256), (DET_LANES, TASKS_64)):
        for total, heights in table.items():
            d = slivers(g, heights)
            out.append(_batches_case(g, tag, f"tasks_{total}_of_{lanes}_lanes", d, view9, [sliver_slab(heights)], [(0, [(None, total)])],
                                     f"{total} tasks for {lanes} lanes", [(0, 0), ((heights[0] + 2) // TR, 0)], paint=4))
    view14 = (13 * TR + 9, 4 * TC + 41)
    out.append(_batches_case(g, tag, "tasks_single_long_edge", single_edge(g, 212, view14[1]), view14, [(0, 14, 0, 5)], [(0, [(1, 212)])],
                             "one live edge of 212 rows: every lane starts inside it", [(0, 0), (6, 0), (13, 0)], paint=5))
    view11 = (10 * TR + 9, 4 * TC + 41)
    out.append(_batches_case(g, tag, "tasks_one_row_edges", one_row_edges(g, 320), view11, [(0, 10, 0, 5)], [(0, None)],
                             "320 edges of one row behind one of 154: runs that hold several edges", [(9, 0), (9, 2), (9, 4), (3, 0)], paint=6))
    return out


def _closing_one_row(g):
    """257 edges whose last -- the closing edge, alone in the second batch -- has exactly one row."""
    m = 255
    pts = [(30.2, 20.3)] + [(30.2 + 250.0 * i / m, 9.3 + (i % 2) * 16.4) for i in range(1, m + 1)]
    pts += [(275.0, 20.9)]   # ... and Z: from (275.0, 20.9) back to (30.2, 20.3), inside pixel row 20
    return poly(g, pts)


def _all():
    out = []
    for origin in ORIGINS:
        g, tag = Geo(origin), "o%d_%d" % origin
        cases = _per_origin(g, tag)
        view3 = (2 * TR + 13, 4 * TC + 41)
        cases.append(_batches_case(g, tag, "tasks_1_of_256_lanes", _closing_one_row(g), view3, [(0, 2, 0, 5)], [(0, [(256, None), (1, 1)])],
                                   "a second batch of one task", [(1, 0), (1, 2), (1, 4)], rule="evenodd", paint=1))
        # the two-pass plan: a wide and a tall case again, with a filler of 4100 segments
        for pb in list(cases):
            if pb.name.split("-", 1)[0] in TWO_PASS:
                c = pb.case
                fill = Entry(filler(g, c.viewport[2:]), None, PAINTS[7])
                cases.append(PB(c._replace(name="twopass_" + c.name, entries=c.entries + (fill,)), pb.slabs, pb.batches, pb.what + ", in a batch of more than 4096 segments"))
        out += cases
    return out


CASES = _all()
IDS = [pb.name for pb in CASES]
BY_NAME = {pb.name: pb for pb in CASES}


def base_name(pb):
    return pb.name.split("-", 1)[0]


def is_two_pass(pb):
    return pb.name.startswith("twopass_")


# --------------------------------------------------------------------------------------------------------------------------------
# band lists (k_band_entries) and tile lists (k_tile_lists)
# --------------------------------------------------------------------------------------------------------------------------------
BAND_COUNTS = (1023, 1024, 1025, 4096, 4097, 5121, 8193)
BAND_VIEW = (2 * TR + 16, 3 * TC + 38)     # 3 bands x 4 column tiles
PAIR_ROWS = (37, 45)                       # rows kept for the overlapping pairs (band 2): no other path reaches them


def pair_indices(n_paths):
    """The second path of every overlapping pair: where k_band_entries puts two pieces of its list together -- the first path of a
    wave (w * chunk) for several waves, and inside a wave the first path of groups 4 and 8 (the 64-path groups 3|4 and 7|8: the
    register-kept groups end at 4, the quads loaded later at 8)."""
    groups, chunk = band_groups(n_paths)
    at = [w * chunk for w in (1, 2, 3, 9, 15)]
    for w in (0, 1, 11):
        at += [w * chunk + gi * 64 for gi in (4, 8) if gi < groups]
    return sorted({i for i in at if 0 < i < n_paths})


def _quad(g, x, y, w, h, skew):
    return poly(g, [(x, y), (x + w, y + 0.3 * skew), (x + w - 0.4 * skew, y + h), (x + 0.5 * skew, y + h - 0.2 * skew)])


def band_list_case(origin, n_paths):
    """`n_paths` small translucent quadrilaterals in paint order; every pair of pair_indices() overlaps in rows no other path reaches."""
    g, tag = Geo(origin), "o%d_%d" % origin
    rows, cols = BAND_VIEW
    second = pair_indices(n_paths)
    spot = {}
    for k, i in enumerate(second):
        spot[i] = spot[i - 1] = (6.3 + 17.0 * k, PAIR_ROWS[0] + 1.3)
    rng = np.random.default_rng(2026 + n_paths)
    xs, ys = rng.uniform(1.5, cols - 12.0, n_paths), rng.uniform(1.5, 27.0, n_paths)   # bands 0, 1, 0|1 and 1|2: down to row 35
    ws, hs, sk = rng.uniform(2.5, 9.0, n_paths), rng.uniform(2.0, 7.5, n_paths), rng.uniform(-1.0, 1.0, n_paths)
    entries = []
    for i in range(n_paths):
        if i in spot:
            x, y = spot[i]
            first = i + 1 in spot and spot[i + 1] == spot[i] and i not in second
            entries.append(Entry(_quad(g, x + (0.0 if first else 2.6), y + (0.0 if first else 1.2), 8.4, 4.9, 0.7), None, PAINTS[i % 8]))
        else:
            entries.append(Entry(_quad(g, xs[i], ys[i], ws[i], hs[i], sk[i]), None, PAINTS[i % 8]))
    case = Case(f"bands_{n_paths}-{tag}", tuple(entries), (), (g.r, g.c, rows, cols), ((0, 0), (1, 1), (2, 0), (1, 3)))
    return case, second


def weights_case(origin):
    """One band (band 1) whose tiles have weights 62, 63, 64 and 70: small rectangles, 2 each (class 2), and one faint rectangle
    over all of tile 2 (class 1 there: 1; its sides lie in tiles 1 and 3: 2 there)."""
    g, tag = Geo(origin), "o%d_%d" % origin

    def small(t, i):
        b0, t0 = 1 + 0.05 + (i * 0.37) % 0.55, t + 0.03 + (i * 0.53) % 0.6
        return Entry(g.rect(b0, t0, b0 + 0.3 + (i % 3) * 0.04, t0 + 0.2 + (i % 5) * 0.03), None, PAINTS[(i + t) % 8])

    ent = [small(0, i) for i in range(3)] + [small(1, i) for i in range(30)] + [small(2, i) for i in range(31)]
    ent.append(Entry(g.rect(0.6, 1.7, 2.4, 3.3), None, FAINT))
    ent += [small(3, i) for i in range(31)] + [small(4, i) for i in range(35)]
    case = Case(f"weights-{tag}", tuple(ent), (), (g.r, g.c, 2 * TR + 11, 4 * TC + 52), ((1, 1), (1, 2), (1, 3), (1, 4)),
                items=(((1, 1), 31), ((1, 2), 32), ((1, 3), 32), ((1, 4), 35)))
    return case, {0: 6, 1: 62, 2: 63, 3: 64, 4: 70}


WIDE_COLS = (65536, 65537, 65600)   # 1024 column tiles (one chunk of k_tile_lists), 1025 and 1025
WIDE_ROWS = 20
WIDE_DEEP = 25                      # items of the deep tile at column tile 1024: one more than a page


def wide_case(origin, cols):
    """20 rows x `cols` columns: one path over the whole width, cut by the viewport on the right and below (13 column runs per band
    at 1025 column tiles; band 1 has no edge of it beyond the first tiles: class 1 up to the last tile); small paths in tiles 0,
    1022, 1023, 1024 and the last one; 25 paths in tile 1024 of band 0 (outside the viewport at 65 536 columns: empty paths)."""
    g, tag = Geo(origin), "o%d_%d" % origin
    n_ct = -(-cols // TC)
    ent = [Entry(poly(g, [(0.3 * TC, 3.2), (cols + 30.0, 3.8), (cols + 50.0, 30.4), (1.6 * TC, 31.2)]), None, PAINTS[3])]
    for k, t in enumerate((0, 1022, 1023, 1024, n_ct - 1)):
        ent.append(Entry(_quad(g, t * TC + 9.3 + 3.1 * k, 5.4 + 0.7 * k, 17.9, 11.3, 0.9), "evenodd" if k % 2 else None, PAINTS[k]))
    ent.append(Entry(poly(g, [(1023 * TC - 20.4, 9.2), (1024 * TC + 23.3, 9.7), (1024 * TC + 20.1, 18.3), (1023 * TC - 17.7, 17.1)]), None, PAINTS[6]))
    have = sum(1 for t in (1024, n_ct - 1) if t == 1024) + 2   # in tile 1024: the wide path, the small one(s), the one across the border
    for i in range(WIDE_DEEP - have):
        x, y = 1024 * TC + 0.7 + (i * 5.3) % 14.0, 1.4 + (i * 3.7) % 9.0   # (tile 1024 is 1, 64 or 64 columns wide)
        ent.append(Entry(_quad(g, x, y, 3.9 + (i % 3), 3.3 + (i % 4) * 0.6, 0.4), None, PAINTS[(i + 2) % 8]))
    tiles = ((0, 0), (0, 1022), (0, 1023)) + (((0, 1024),) if n_ct > 1024 else ())
    layout = (("entry", 0, 1, 1023, 1),) + ((("entry", 0, 1, 1024, 1),) if n_ct > 1024 else ())
    items = (((0, 1024), WIDE_DEEP),) if cols >= 1024 * TC + 20 else ()
    return Case(f"wide_{cols}-{tag}", tuple(ent), (), (g.r, g.c, WIDE_ROWS, cols), tiles, layout, items=items)


@functools.lru_cache(maxsize=None)
def list_cases():
    """The band-list, weight and wide cases, by name (built on demand: 8193 paths are 8193 strings)."""
    out = {}
    for origin in ORIGINS:
        for n in BAND_COUNTS:
            c, second = band_list_case(origin, n)
            out[c.name] = (c, second)
        c, w = weights_case(origin)
        out[c.name] = (c, w)
        for cols in WIDE_COLS:
            c = wide_case(origin, cols)
            out[c.name] = (c, None)
    return out


BAND_IDS = ["bands_%d-o%d_%d" % (n, *o) for o in ORIGINS for n in BAND_COUNTS]
WEIGHT_IDS = ["weights-o%d_%d" % o for o in ORIGINS]
WIDE_IDS = ["wide_%d-o%d_%d" % (c, *o) for o in ORIGINS for c in WIDE_COLS]


# --------------------------------------------------------------------------------------------------------------------------------
# the references: computed once per case and process, shared read-only
# --------------------------------------------------------------------------------------------------------------------------------
_REFS = {}


def reference(case):
    """canvas_ref.render of a case (a canvas_cases.Case), not clamped; non-trivial in every tile under test."""
    from tests import canvas_cases as cc
    from tests import canvas_ref as cr

    if case.name not in _REFS:
        ref = cr.render(case.entries, case.groups, case.viewport)
        for band, ct in case.tiles:
            assert cc.nontrivial(case, ref, band, ct), f"{case.name}: the reference is trivial in tile ({band}, {ct})"
        ref.flags.writeable = False
        _REFS[case.name] = ref
    return _REFS[case.name]
