"""The flatten in curve order, restated in numpy over the oracle's pinned primitives, and the cases the flatten tests share.

`flatten_in_order` is what k_flatten promises in every one of its launch forms: one dense block of edges in (path, segment,
curve) order.  It is built from `oracle.transform_points` (the reference's fma form), `oracle.flatness` and `oracle.split`
only -- level by level on whole arrays, every node carrying its place on the curve as the exact binary fraction k / 2^depth --
with the flat test and the threshold of `orc_flatten` (oracle/svgr_oracle.c: a node whose flatness is `< (tol * tol) * 16` is
emitted, any other is split).  Nothing of the HIP code goes in.

The case builders make drawings (the batch arrays of `_abi.Batch` plus a viewport) whose segment counts sit on the seams of the
flatten's launches, for a GPU comparison of every launch form with this reference; tests/test_flatten_ref_host.py shows, from
the reference's `info` alone, that they cross what they are meant to cross.  TEST INFRASTRUCTURE ONLY.
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import oracle as orc

FL_ENDS = 4          # pieces a lane remembers from its counting traversal: k_flatten's `FL_ENDS` (svgr_hip.hip)
SUBS = (5, 6)        # log2 of the lanes a segment is cut over: k_flatten's `SUB` (32 lanes, or 64 when the launch does not fill the chip)
FL_BLOCK = 256       # threads of a k_flatten workgroup: 256 >> SUB segments per workgroup (8 at 32 lanes, 4 at 64)
SCAN_WINDOW = 64     # predecessors one step of the look-back reads
SCAN_CHUNK = 8192    # segments per step of k_seg_scan (1024 lanes x 8 counts)
MI355X_CUS = 256     # compute units of an MI355X (what the CPU-side checks size the large group by)
EDGE_BUDGET = 300_000
MAX_LEVELS = 40      # (no case comes near it: the deepest piece of any builder is at depth 11)

SEG_LINE, SEG_CUBIC = 0, 1


# ---------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------
def _seg_path(path_seg_off, n_segs):
    off = np.asarray(path_seg_off, dtype=np.int64).reshape(-1)
    assert off[0] == 0 and off[-1] == n_segs and (np.diff(off) >= 0).all(), "path_seg_off does not tile the segments"
    return np.repeat(np.arange(len(off) - 1, dtype=np.int64), np.diff(off))


def transformed_points(segs, path_seg_off, path_m6):
    """The four points of every segment in presentation space (a line uses the first two): oracle.transform_points, one call
    per distinct transform (distinct by BITS: -0.0 is not 0.0 here)."""
    pts = np.ascontiguousarray(segs, dtype=np.float64).reshape(-1, 4, 2)
    seg_path = _seg_path(path_seg_off, len(pts))
    m6 = np.ascontiguousarray(path_m6, dtype=np.float64).reshape(-1, 6)
    out = np.empty_like(pts)
    if len(pts):
        per_seg = np.ascontiguousarray(m6[seg_path])
        uniq, inv = np.unique(per_seg.view(np.uint64), axis=0, return_inverse=True)
        inv = np.asarray(inv).reshape(-1)
        for k in range(len(uniq)):
            sel = inv == k
            out[sel] = orc.transform_points(uniq[k].view(np.float64).reshape(2, 3), pts[sel])
    return out, seg_path


def flatten_in_order(segs, seg_kind, path_seg_off, path_m6, tol=0.1):
    """-> (edges (E, 2, 2) float64, edge_path (E,) int32, info): every piece of every segment, ordered by (path, segment,
    place on the curve).  A line is one edge from its first point to its second.  `info`, per piece: `seg`, `depth` (the level
    at which subdivision stopped; 0 for a line), `k` (the piece covers [k, k + 1) / 2^depth of its curve), and `lane[SUB]` for
    SUB 5 and 6: the depth-SUB node it lies under, or -- for a piece that went flat above that level -- the first of the
    depth-SUB places it covers (the lane that emits it)."""
    pts, seg_path = transformed_points(segs, path_seg_off, path_m6)
    kind = np.asarray(seg_kind).reshape(-1)
    assert len(kind) == len(pts)
    thr = (tol * tol) * 16.0   # orc_flatten: `double thr = (flatness * flatness) * 16.0`, emitted when `cubic_flatness(c) < thr`
    lines = np.flatnonzero(kind == SEG_LINE)
    e_out = [np.stack([pts[lines, 0], pts[lines, 1]], axis=1)]
    s_out, k_out, d_out = [lines], [np.zeros(len(lines), np.int64)], [np.zeros(len(lines), np.int64)]
    seg = np.flatnonzero(kind != SEG_LINE)
    cur = np.ascontiguousarray(pts[seg])
    k = np.zeros(len(seg), np.int64)
    depth = 0
    while len(cur):
        if depth >= MAX_LEVELS:
            raise ValueError("flatten_in_order: a curve does not go flat (non-finite or absurd control points)")
        flat = orc.flatness(cur) < thr
        e_out.append(np.stack([cur[flat, 0], cur[flat, 3]], axis=1))
        s_out.append(seg[flat]); k_out.append(k[flat]); d_out.append(np.full(int(flat.sum()), depth, np.int64))
        keep = ~flat
        cur = orc.split(cur[keep])          # (2M, 4, 2): left half, right half of each, in that order
        seg = np.repeat(seg[keep], 2)
        k = np.repeat(k[keep] << 1, 2)
        k[1::2] |= 1
        depth += 1
    edges = np.concatenate(e_out).reshape(-1, 2, 2)
    seg, k, d = np.concatenate(s_out), np.concatenate(k_out), np.concatenate(d_out)
    top = int(d.max(initial=0))
    order = np.lexsort((k << (top - d), seg))   # k / 2^depth as an integer over the common denominator 2^top
    edges, seg, k, d = np.ascontiguousarray(edges[order]), seg[order], k[order], d[order]
    lane = {sub: np.where(d >= sub, k >> np.maximum(d - sub, 0), k << np.maximum(sub - d, 0)) for sub in SUBS}
    info = dict(seg=seg, depth=d, k=k, lane=lane, thr=thr, is_cubic=kind[seg] != SEG_LINE, n_segs=len(pts), pts=pts)
    return edges, seg_path[seg].astype(np.int32), info


# ---------------------------------------------------------------------------------------------------------------------
# what the tests ask of a result
# ---------------------------------------------------------------------------------------------------------------------
def lane_counts(info, sub):
    """Pieces per (cubic segment, lane) at 2^sub lanes per segment: the counts of the lanes that own any."""
    c = info["is_cubic"]
    _, n = np.unique((info["seg"][c] << sub) | info["lane"][sub][c], return_counts=True)
    return n


def path_extents(edges, edge_path, n_paths):
    """(n_paths, 4) {min row, min col, max row, max col} over the points of every path's edges; no edge: {+inf, +inf, -inf, -inf}."""
    ext = np.empty((n_paths, 4))
    ext[:, :2], ext[:, 2:] = np.inf, -np.inf
    e = np.asarray(edges).reshape(-1, 2, 2)
    for ax in (0, 1):
        np.minimum.at(ext[:, ax], edge_path, e[:, :, ax].min(axis=1))
        np.maximum.at(ext[:, 2 + ax], edge_path, e[:, :, ax].max(axis=1))
    return ext


def meets_rows(edges, row_lo, row_hi):
    """Pieces whose closed row range [min, max] meets the rows [row_lo, row_hi)."""
    r = np.asarray(edges).reshape(-1, 2, 2)[:, :, 0]
    return (r.max(axis=1) >= row_lo) & (r.min(axis=1) < row_hi)


def owned_bands(rank, world, strip, n_bands):
    """The bands rank `rank` of `world` keeps: interleaved strips of `strip` bands (include/svgr.h: svgr_batch_set_bands)."""
    b = np.arange(n_bands)
    return b[(b // strip) % world == rank]


def meets_bands(edges, viewport, band_rows, bands):
    """Pieces whose closed row range meets one of `bands` (band b = rows [b, b + 1) * band_rows from the viewport's first row,
    cut at the viewport's last)."""
    out = np.zeros(len(np.asarray(edges).reshape(-1, 4)), bool)
    for b in bands:
        lo = viewport[0] + int(b) * band_rows
        out |= meets_rows(edges, lo, min(lo + band_rows, viewport[0] + viewport[2]))
    return out


def path_row_reach(info, seg_kind, path_seg_off):
    """(n_paths, 2) integer rows [lo, hi] a path can reach at all: the rows of its transformed control points (a cubic and its
    halves stay inside their hull), widened by the bbox's own margin (floor - 1, ceil + 1) and one more row of slack -- what
    include/svgr.h means by "a path none of whose rows can reach an owned band".  A path without segments: lo > hi."""
    off = np.asarray(path_seg_off, dtype=np.int64)
    r = info["pts"][:, :, 0].copy()
    line = np.asarray(seg_kind).reshape(-1) == SEG_LINE
    r[line, 2:] = r[line, :2]
    out = np.empty((len(off) - 1, 2), np.int64)
    for p in range(len(off) - 1):
        seg = r[off[p]:off[p + 1]]
        out[p] = (int(np.floor(seg.min())) - 2, int(np.ceil(seg.max())) + 2) if seg.size else (1, 0)
    return out


def reach_meets_bands(reach, viewport, band_rows, bands):
    """Per path: whether its rows [lo, hi] meet one of `bands`.  "Cannot reach" stays on the safe side: the last band is not cut
    at the viewport's end, and the band's worth of rows just ABOVE the viewport counts to band 0 -- the kernels find a row's
    band by a division that rounds toward zero, so a path that ends less than a band above the viewport is listed for the rank
    that owns band 0 (it leaves no pixel there; documented here as the limit of what svgr.h promises)."""
    out = np.zeros(len(reach), bool)
    for b in bands:
        lo = viewport[0] + int(b) * band_rows
        out |= (reach[:, 1] >= (lo - band_rows if b == 0 else lo)) & (reach[:, 0] < lo + band_rows) & (reach[:, 0] <= reach[:, 1])
    return out


def _rows_of(edges, edge_path):
    e = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1, 4).view(np.uint64)
    return np.concatenate([e, np.asarray(edge_path, dtype=np.int64).reshape(-1, 1).view(np.uint64)], axis=1)


def place_in_reference(ref_edges, ref_path, got_edges, got_path):
    """The indices at which `got` (edges and their paths, by bits) is a subsequence of the reference, in order -- or None when it
    is not one.  The reference's rows must be distinct (the builders' are; asserted on the host)."""
    ref, got = _rows_of(ref_edges, ref_path), _rows_of(got_edges, got_path)
    _, inv = np.unique(np.concatenate([ref, got]), axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    ref_id, got_id = inv[:len(ref)], inv[len(ref):]
    at = np.full(int(inv.max(initial=-1)) + 1, -1, np.int64)
    at[ref_id] = np.arange(len(ref))
    assert len(np.unique(ref_id)) == len(ref), "the reference holds a piece twice"
    idx = at[got_id]
    if (idx < 0).any() or (np.diff(idx) <= 0).any():
        return None
    return idx


def sorted_rows(edges, edge_path):
    """(path, edge) rows sorted by path, then by the edge's bytes: a multiset's canonical form."""
    rows = _rows_of(edges, edge_path)
    return rows[np.lexsort((rows[:, 3], rows[:, 2], rows[:, 1], rows[:, 0], rows[:, 4]))]


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
VIEWPORT = (0, 0, 1024, 2048)       # contains every row of every case with room to spare; the deep cubics hang out of its columns
ROW_LO, ROW_HI = 64.0, 960.0        # the rows the geometry lies in (presentation space)
SMALL_SIZES = (1, 3, 4, 5, 256, 257, 261, 513, 517, 521)
LAYOUTS = ("one", "mixed", "singles")
# a viewport that cuts the geometry (a band of rows through the middle, first row not on a band of VIEWPORT's), one far below
# everything and one far above everything
CUT_VIEWPORTS = {"middle": (404, 0, 208, 2048), "below": (6000, 0, 256, 2048), "above": (-6000, 0, 256, 2048)}


def lane_switch_sub(n_items, n_cu):
    """choose_fl_sub (svgr_hip.hip) restated: 64 lanes per segment (6) while the launch at 32 would not fill six waves per SIMD."""
    waves32 = (max(int(n_items), 1) << 5) // 64
    return 6 if waves32 * 2 <= int(n_cu) * 4 * 6 else 5


def large_sizes(n_cu):
    """With T = 24 * n_cu: T and T + 1 (the last launches at 64 lanes -- the switch compares whole waves, so an odd T + 1 still
    takes 64), T + 2 (the first at 32), then k_seg_scan's chunk: a multiple of 8192 above the switch, + 1 (a scalar tail of
    one), + 8 (a tail of one vector step), and twice that + 1 (three steps)."""
    t = 24 * int(n_cu)
    base = SCAN_CHUNK * ((t + 2) // SCAN_CHUNK + 1)
    return (t, t + 1, t + 2, base, base + 1, base + 8, 2 * base + 1)


def _transforms():
    c, s = np.cos(0.5), np.sin(0.5)
    return np.array([
        [1.0, 0.0, 0.0, 0.0, 1.0, 0.0],                      # identity
        [0.0, 1.0, 0.0, 1.0, 0.0, 0.0],                      # the x / y swap
        [c, -s, 300.0, s, c, -150.0],                        # a rotation
        [1.0, 0.0, 0.0, 0.0, -1.0, 1900.0],                  # a reflection (determinant -1)
        [1.75, 0.0, 0.0, 0.0, 0.6, 0.0],                     # a non-uniform scale
        [1.0, 0.0, 0.3125, 0.0, 1.0, 0.7],                   # a sub-pixel translation
    ])


def _layout(n, name):
    if name == "one":
        return np.array([0, n], np.int64)
    if name == "singles":
        return np.arange(n + 1, dtype=np.int64)
    if n < 3:
        return None
    if n < 64:
        return np.array([0, 1, 1, n], np.int64)       # a path with no segments between two others
    # a boundary inside a workgroup (2), one on a workgroup boundary at both widths (8), a path with no segments, one path over
    # at least three workgroups at either width with others on both sides ([11, 40)), then runs of mixed lengths
    off = [0, 2, 8, 8, 11, 40]
    runs, i = (3, 5, 8, 1, 16, 0, 7, 33, 4, 64), 0
    while off[-1] < n:
        off.append(min(off[-1] + runs[i % len(runs)], n))
        i += 1
    return np.array(off, np.int64)


def _segments(n, rich, rng):
    """(n, 4, 2) presentation-space points and kinds.  `rich`: lines, cubics flat at the root and cubics of graded size in equal
    parts; else mostly lines.  Three large, strongly curved cubics (first, middle and last segment) reach depth 9 to 11."""
    i = np.arange(n)
    u = rng.uniform(size=(n, 6))
    r0, c0 = ROW_LO + u[:, 0] * (ROW_HI - 48.0 - ROW_LO), 16.0 + u[:, 1] * 1384.0
    zero = np.zeros(n)

    def four(*p):   # eight (n,) coordinate arrays -> (n, 4, 2)
        return np.stack(p, axis=1).reshape(n, 4, 2)

    # (mostly lines: a graded and a flat cubic every 53 segments, and every other one of the last twelve -- the scan's tail)
    what = i % 3 if rich else np.where((i % 53 == 0) | ((i >= n - 12) & (i % 2 == 0)), 0, np.where(i % 53 == 1, 2, 1))
    # graded: the sizes sweep a factor of 4^9.5, i.e. every maximal depth from 0 to 9
    d = 0.03 * 4.0 ** (((i // (3 if rich else 53)) * 0.6180339887498949) % 1.0 * (9.5 if rich else 8.5))
    h, w = 4.0 + 36.0 * u[:, 2], -10.0 + 20.0 * u[:, 3]
    graded = four(r0, c0, r0 + h / 3, c0 + (0.4 + 0.6 * u[:, 4]) * d, r0 + 2 * h / 3, c0 + (0.2 + 0.8 * u[:, 5]) * d, r0 + h, c0 + w)
    line = four(r0, c0, r0 - 6.0 + 12.0 * u[:, 2], c0 - 6.0 + 12.0 * u[:, 3], zero, zero, zero, zero)
    # flat at the root: the control points a hundredth of a pixel off the chord
    dr, dc = -20.0 + 40.0 * u[:, 2], -20.0 + 40.0 * u[:, 3]
    flat = four(r0, c0, r0 + dr / 3 + 0.01, c0 + dc / 3, r0 + 2 * dr / 3, c0 + 2 * dc / 3 - 0.01, r0 + dr, c0 + dc)
    pts = np.where((what == 0)[:, None, None], graded, np.where((what == 1)[:, None, None], line, flat))
    kind = np.where(what == 1, SEG_LINE, SEG_CUBIC).astype(np.uint8)
    for at, size in {0: 6.0e4, n // 2: 2.4e4, n - 1: 3.6e4}.items():
        # tall, so that the lanes of one cubic straddle a band of rows; the bulge goes to the right, out of the viewport
        ra, hh = ROW_LO + 60.0 * u[at, 0], 700.0 + 120.0 * u[at, 2]
        pts[at] = [[ra, c0[at]], [ra + 0.2 * hh, c0[at] + size], [ra + 0.9 * hh, c0[at] + 0.35 * size], [ra + hh, c0[at] + 8.0]]
        kind[at] = SEG_CUBIC
    return pts, kind


@functools.lru_cache(maxsize=None)
def make_case(n, layout, rich):
    """dict(segs, seg_kind, path_seg_off, path_m6, path_rule, path_paint, viewport) -- or None when `layout` does not fit `n`
    segments.  Deterministic: seeded by its arguments.  The geometry is laid out in presentation space and taken back through
    each path's transform, so every path lands in VIEWPORT's rows whatever its transform is."""
    off = _layout(n, layout)
    if off is None:
        return None
    rng = np.random.default_rng([n, LAYOUTS.index(layout), int(rich)])
    pres, kind = _segments(n, bool(rich), rng)
    n_paths = len(off) - 1
    tr = _transforms()
    which = (np.arange(n_paths) + n) % len(tr)       # (a one-path case takes the transform its size selects)
    m6 = tr[which]
    seg_path = _seg_path(off, n)
    segs = np.empty_like(pres)
    for t in range(len(tr)):
        sel = which[seg_path] == t
        a, b = tr[t].reshape(2, 3)[:, :2], tr[t].reshape(2, 3)[:, 2]
        segs[sel] = (pres[sel] - b) @ np.linalg.inv(a).T
    segs[kind == SEG_LINE, 2:] = 0.0
    paint = np.tile(np.array([[0.2, 0.3, 0.1, 0.5], [0.1, 0.05, 0.3, 0.4]]), ((n_paths + 1) // 2, 1))[:n_paths]
    return dict(segs=np.ascontiguousarray(segs.reshape(n, 8)), seg_kind=kind, path_seg_off=off, path_m6=np.ascontiguousarray(m6),
                path_rule=(np.arange(n_paths) % 2).astype(np.uint8), path_paint=np.ascontiguousarray(paint), viewport=VIEWPORT)


def case_ids(n_cu):
    """(n, layout, rich) of every case: the small group (64 lanes per segment) in rich geometry, the large group mostly lines."""
    out = [(n, lay, True) for n in SMALL_SIZES for lay in LAYOUTS if _layout(n, lay) is not None]
    out += [(n, lay, False) for n in large_sizes(n_cu) for lay in LAYOUTS]
    return out


def cull_case_ids(n_cu):
    """The cases the culling viewports are laid over: one of the small group, the first launch at 32 lanes, and a scalar scan tail."""
    big = large_sizes(n_cu)
    return [(521, "mixed", True), (big[2], "mixed", False), (big[4], "singles", False)]


SHARD_CASE = (521, "mixed", True)           # under CUT_VIEWPORTS["middle"]
SHARDINGS = ((2, 1), (3, 2))                # (world, strip_bands)


def moved(m6, which):
    """Three other sets of transforms for one batch: scaled about the origin and shifted (the piece counts change with the
    scale), all of them inside VIEWPORT's rows with the all-kept margin."""
    s, dr, dc = ((0.985, 3.375, -2.5), (1.0, -5.25, 0.0625), (1.0125, 1.0, 7.75))[which]
    out = np.array(m6, dtype=np.float64, copy=True).reshape(-1, 6) * s
    out[:, 2] += dr
    out[:, 5] += dc
    return out


@functools.lru_cache(maxsize=64)
def reference(n, layout, rich, which=-1):
    """flatten_in_order of a case (under its own transforms, or under `moved(.., which)`), computed once and shared: callers leave
    the arrays unchanged."""
    sc = make_case(n, layout, rich)
    m6 = sc["path_m6"] if which < 0 else moved(sc["path_m6"], which)
    edges, edge_path, info = flatten_in_order(sc["segs"], sc["seg_kind"], sc["path_seg_off"], m6)
    for a in (edges, edge_path):
        a.setflags(write=False)
    return edges, edge_path, info
