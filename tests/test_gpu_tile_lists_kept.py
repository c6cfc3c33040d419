"""A placed replay keeps the tile lists (`items`, `pages`, `tile_info`) of the replay before it: k_tile_lists compares every band's mask
words with the copy its last full run saved (`tile_mask_kept`) and lists again only the bands that differ.  Here: every seam of
that shortcut -- a grid of bands and tiles, lists longer than a page, two mask words, empty tiles and bands, one band listed again
beside kept ones (SVGR_DBG_STALE_BAND), everything that must void the kept lists -- with every picture against a FRESH batch of
the same inputs, bit for bit (deterministic renders: the order of the adds is fixed).  A picture does not say whether the
shortcut ran at all: one more test repeats the scenarios in a fresh interpreter under SVGR_DBG_PLAN and reads, pass by pass, what
the library asked k_tile_lists for.

The small scenes are planned with SVGR_NO_SPECULATIVE_PLAN: the two-pass plan orders the slabs of a batch of any size, and only
a batch with a slab order replays under the plan's places (as shipped: more than 4096 segments)."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.util import ROOT

pytestmark = pytest.mark.gpu

TR, TC = 16, 64            # the tile (asserted against the library's)
PAGE_ITEMS = 24            # items a tile's page holds (k_tile_lists): longer lists continue in `items`
CHILD = "SVGR_TLK_CHILD"   # set in the child interpreter: the scenarios announce themselves on stderr


@pytest.fixture(scope="module")
def S():
    import svgrasterize_amd as S
    from svgrasterize_amd import _abi

    S.Context.get()
    assert (_abi.tile_rows(), _abi.tile_cols()) == (TR, TC)
    return S


@contextlib.contextmanager
def _env(**kv):
    before = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in before.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _mark(name):
    if os.environ.get(CHILD):
        print(f"[case] {name}", file=sys.stderr, flush=True)


# ---------------------------------------------------------------------------------------------------------------------- scenes
def _scene(rows, cols, polys):
    """polygons [(row, col), ...] -> a batch's arrays: closed runs of line segments in user space (x = col, y = row) under the
    x / y swap, paints that differ from path to path (a list in another order is another picture), every third path evenodd"""
    from svgrasterize_amd import synth

    segs, offs = [], [0]
    for poly in polys:
        for (r0, c0), (r1, c1) in zip(poly, poly[1:] + poly[:1]):
            segs.append([c0, r0, c1, r1, 0.0, 0.0, 0.0, 0.0])
        offs.append(len(segs))
    n = len(polys)
    k = np.arange(n, dtype=np.float64)
    alpha = 0.35 + 0.5 * ((k * 7) % 5) / 5.0
    rgb = np.stack([((k * 3) % 7) / 7.0, ((k * 5) % 11) / 11.0, ((k * 2) % 3) / 3.0], axis=1)
    return dict(segs=np.array(segs, dtype=np.float64).reshape(-1, 8), seg_kind=np.zeros(len(segs), dtype=np.uint8),
                path_seg_off=np.array(offs, dtype=np.int64), path_m6=np.tile(synth.SWAP_M6, (n, 1)),
                path_rule=(np.arange(n) % 3 == 2).astype(np.uint8), path_paint=np.concatenate([rgb * alpha[:, None], alpha[:, None]], axis=1),
                viewport=(0, 0, rows, cols))


def _box(r0, c0, r1, c1, skew=0.0):
    return [(r0, c0), (r0 + skew, c1), (r1, c1 - skew), (r1 - skew, c0)]


def grid_scene():
    """64 x 192 = 4 bands x 3 column tiles, 6 paths: one over every tile (cells of class 1 inside it), one per corner region, one
    that crosses a band and a tile border, one sliver inside a single tile"""
    return _scene(64, 192, [_box(1.5, 2.25, 62.5, 189.75, 0.5), _box(3.25, 5.5, 20.75, 70.5, 1.25), _box(40.5, 120.25, 61.0, 188.5),
                            _box(14.25, 60.5, 34.75, 130.25, 2.0), _box(50.25, 3.5, 60.5, 40.25), _box(22.5, 150.25, 25.75, 170.5, 0.75)])


def page_scene(n=PAGE_ITEMS + 6):
    """32 x 128, `n` > PAGE_ITEMS paths that all lie inside tile (band 1, column tile 1): its list continues behind its page"""
    return _scene(32, 128, [_box(16.5 + 0.25 * (i % 9), 64.75 + 1.5 * i, 30.25 - 0.125 * (i % 5), 80.5 + 1.5 * i, 0.25 * (i % 3)) for i in range(n)])


def two_word_scene(n=70):
    """48 x 192, `n` > 64 paths in band 1's list (two mask words): the first 64 in column tiles 0 and 1, entry 64 -- bit 0 of the
    second word -- with all its cells in column tile 2, the rest over tiles 1 and 2"""
    polys = [_box(17.25 + 0.125 * (i % 7), 2.5 + 1.75 * i, 30.5, 12.25 + 1.75 * i, 0.5) for i in range(64)]
    polys.append(_box(18.5, 140.25, 29.75, 180.5, 1.0))
    polys += [_box(20.25, 100.5 + 3.0 * i, 28.5, 150.25 + 3.0 * i) for i in range(n - 65)]
    return _scene(48, 192, polys)


def hole_scene():
    """64 x 192 with paths in bands 0 and 3 only (bands 1 and 2 have no path at all) and, there, in column tiles 0 and 2 only"""
    return _scene(64, 192, [_box(2.5, 3.25, 13.5, 50.5, 0.5), _box(1.25, 140.5, 14.75, 185.25), _box(50.5, 5.25, 62.25, 60.5, 1.0),
                            _box(49.25, 130.5, 61.5, 190.25, 0.25), _box(4.5, 150.25, 10.25, 170.5)])


# --------------------------------------------------------------------------------------------------------------------- helpers
def _flags():
    from svgrasterize_amd import _abi

    return _abi.RENDER_CLIP01 | _abi.RENDER_DETERMINISTIC


class _Run:
    """a scene's batch with a float32 canvas; `small`: planned in two passes (a slab order for a batch of any size)"""

    def __init__(self, S, sc, small=True, m6=None):
        from svgrasterize_amd import _abi

        self.abi, self.sc, self.small = _abi, sc, small
        self.ctx = S.Context.get()
        self.rows, self.cols = sc["viewport"][2:]
        self.b = _abi.Batch(self.ctx, sc["segs"], sc["seg_kind"], sc["path_seg_off"], sc["path_m6"] if m6 is None else m6, sc["path_rule"],
                            sc["path_paint"], viewport=list(sc["viewport"]))
        self.out = self.ctx.alloc(self.rows * self.cols * 16)
        self.out64 = None

    def _planning(self):
        return _env(SVGR_NO_SPECULATIVE_PLAN="1") if self.small else contextlib.nullcontext()

    def plan(self):
        with self._planning():
            self.b.plan()

    def draw(self):
        with self._planning():
            self.b.draw(self.out, self.abi.OUT_CANVAS_F32, _flags())
        return self.out.download((self.rows, self.cols, 4), np.float32)

    def render(self, rows=None):
        self.b.render(self.out, self.abi.OUT_CANVAS_F32, _flags())
        return self.out.download((self.rows if rows is None else rows, self.cols, 4), np.float32)

    def render64(self):
        if self.out64 is None:
            self.out64 = self.ctx.alloc(self.rows * self.cols * 32)
        self.b.render(self.out64, self.abi.OUT_CANVAS_F64, _flags())
        return self.out64.download((self.rows, self.cols, 4), np.float64)

    def launches(self, fn):
        n0 = self.ctx.launches()
        got = fn()
        return got, self.ctx.launches() - n0

    def close(self):
        self.b.destroy()
        self.out.free()
        if self.out64 is not None:
            self.out64.free()


def _fresh(S, sc, small=True, m6=None, f64=False):
    """the picture of a new batch of the same inputs: plan + one deterministic render (a full k_tile_lists by construction)"""
    r = _Run(S, sc, small, m6)
    r.plan()
    want = r.render64() if f64 else r.render()
    r.close()
    assert want.any()
    return want


def _replays(r, want, n, what):
    for k in range(n):
        assert np.array_equal(r.render(), want), f"{what}: replay {k}"


# ------------------------------------------------------------------------------------------------------------------- scenarios
def test_grid_of_bands_and_tiles(S):
    """seam: more than one workgroup (4 bands) and more than one lane with items (3 column tiles), lists of one to three items.
    Plan, five replays: each the fresh batch's picture; five launches at most, then four (the launch stays, its work shrinks)."""
    sc = grid_scene()
    want = _fresh(S, sc)
    _mark("grid")
    r = _Run(S, sc)
    r.plan()
    counts = []
    for k in range(5):
        got, n = r.launches(r.render)
        counts.append(n)
        assert np.array_equal(got, want), f"replay {k}"
    assert counts[0] <= 5 and counts[1:] == [4, 4, 4, 4], counts
    r.close()


def test_a_list_longer_than_its_page(S):
    """seam: PAGE_ITEMS.  A tile with more items than its page holds draws the rest from `items`: a kept replay must find them
    there (nothing writes them again), in paint order (every path has another paint)."""
    sc = page_scene()
    assert len(sc["path_rule"]) > PAGE_ITEMS
    want = _fresh(S, sc)
    _mark("page")
    r = _Run(S, sc)
    r.plan()
    _replays(r, want, 3, "30 items in one tile")
    r.close()


def test_two_mask_words(S):
    """seam: mask_words = 2 (the compare and the clearing loop over a tile's 2 x W words instead of the one 16-byte load), an entry
    whose only cells are bit 0 of the second word."""
    sc = two_word_scene()
    assert len(sc["path_rule"]) > 64
    want = _fresh(S, sc)
    assert want[18:30, 165:180].any()   # (where entry 64 alone paints)
    _mark("two words")
    r = _Run(S, sc)
    r.plan()
    _replays(r, want, 3, "70 entries in one band")
    r.close()


def test_empty_tiles_and_bands(S):
    """seam: words that are zero in both arrays -- bands without a path (their workgroups compare, clear nothing, leave), tiles
    without an item between tiles with some."""
    sc = hole_scene()
    want = _fresh(S, sc)
    assert not want[16:48].any() and not want[:, 64:128].any()
    _mark("holes")
    r = _Run(S, sc)
    r.plan()
    _replays(r, want, 3, "bands 1, 2 and column tile 1 empty")
    r.close()


def test_one_band_rebuilt_beside_kept_bands(S):
    """seam: the fall-through.  SVGR_DBG_STALE_BAND flips a bit of band 1's saved words in front of a kept launch: band 1's workgroup
    lists its band again (as if entered fresh) between neighbours that keep theirs, the picture is the fresh one, the saved words
    are right again for the replay behind it."""
    sc = grid_scene()
    want = _fresh(S, sc)
    _mark("stale band")
    r = _Run(S, sc)
    r.plan()
    _replays(r, want, 3, "before")
    for band in (1, 2):
        with _env(SVGR_DBG_STALE_BAND=str(band)):
            got, n = r.launches(r.render)
        assert n == 4 and np.array_equal(got, want), f"band {band} listed again"
        _replays(r, want, 1, f"behind band {band}")
    r.close()


def _moved(sc, d_rows, d_cols):
    m6 = np.array(sc["path_m6"], dtype=np.float64, copy=True).reshape(-1, 6)
    m6[:, 2] += d_rows
    m6[:, 5] += d_cols
    return m6


def test_new_transforms_void_the_kept_lists(S):
    """replays, set_transforms + draw, replays: the moved drawing has other cells in other tiles -- a list of the old plan must
    never be drawn."""
    sc = grid_scene()
    m6 = _moved(sc, 1.0 * TR + 0.375, -TC + 2.25)
    want0, want1 = _fresh(S, sc), _fresh(S, sc, m6=m6)
    assert not np.array_equal(want0, want1)
    _mark("transforms")
    r = _Run(S, sc)
    r.plan()
    _replays(r, want0, 3, "before")
    r.b.set_transforms(m6)
    assert np.array_equal(r.draw(), want1), "draw after set_transforms"
    _replays(r, want1, 3, "after set_transforms + draw")
    r.close()


def test_set_bands_voids_the_kept_lists(S):
    """replays, set_bands(0, 2, 1) (this rank owns bands 0 and 2: another page layout, never kept), and back."""
    sc = grid_scene()
    want = _fresh(S, sc)
    _mark("bands")
    r = _Run(S, sc)
    r.plan()
    _replays(r, want, 3, "before")
    r.b.set_bands(0, 2, 1)
    r.plan()
    mine = np.concatenate([want[0:TR], want[2 * TR:3 * TR]])
    for k in range(2):
        assert np.array_equal(r.render(rows=2 * TR), mine), f"rank 0 of 2, render {k}"
    r.b.set_bands(0, 1, 1)
    r.plan()
    _replays(r, want, 3, "every band again")
    r.close()


def test_a_window_render_between_replays(S):
    """replays, render_window, replays: the window reads the lists in place and leaves them valid."""
    sc = grid_scene()
    want = _fresh(S, sc)
    _mark("window")
    r = _Run(S, sc)
    r.plan()
    _replays(r, want, 3, "before")
    win = (TR, TC, 2 * TR, 2 * TC)
    wout = r.ctx.alloc(win[2] * win[3] * 16)
    r.b.render(wout, r.abi.OUT_CANVAS_F32, _flags(), window=win)
    part = wout.download((win[2], win[3], 4), np.float32)
    wout.free()
    assert np.array_equal(part, want[win[0]:win[0] + win[2], win[1]:win[1] + win[3]])
    _replays(r, want, 2, "after the window")
    r.close()


def test_a_float64_canvas_between_float32_ones(S):
    """replays to OUT_CANVAS_F64 between float32 ones: another tile kernel over the same lists."""
    sc = grid_scene()
    want, want64 = _fresh(S, sc), _fresh(S, sc, f64=True)
    _mark("float64")
    r = _Run(S, sc)
    r.plan()
    _replays(r, want, 3, "before")
    assert np.array_equal(r.render64(), want64)
    _replays(r, want, 1, "between")
    assert np.array_equal(r.render64(), want64)
    _replays(r, want, 2, "after")
    r.close()


BIG = (512, 900)   # (canvas, paths): more than 4096 segments -- a destroyed batch leaves its work arrays to the context


def test_a_new_batch_on_inherited_arrays_starts_without_kept_lists(S):
    """destroy, then a batch of ANOTHER drawing for the same viewport: it inherits the arrays -- the lists and the saved words of the
    old drawing among them -- and must list every band itself before it keeps anything."""
    from svgrasterize_amd import synth

    sc_a, sc_b = synth.make_scene(*BIG), synth.make_scene(*BIG, seed=0x2545F491)
    assert len(sc_a["seg_kind"]) > 4096 and len(sc_b["seg_kind"]) > 4096
    with _env(SVGR_NO_SPARE="1"):
        want_a, want_b = _fresh(S, sc_a, small=False), _fresh(S, sc_b, small=False)
    assert not np.array_equal(want_a, want_b)
    _mark("inherited a")
    r = _Run(S, sc_a, small=False)
    r.plan()
    _replays(r, want_a, 3, "first drawing")
    r.close()
    _mark("inherited b")
    r = _Run(S, sc_b, small=False)
    r.plan()
    _replays(r, want_b, 3, "second drawing on the first one's arrays")
    r.close()


def test_edges_after_replays_are_the_plans(S):
    """a placed replay's flatten no longer stores `edge_path` (the plan's pass has): Batch.edges() after three replays returns what
    it returned right after the plan -- the edges, and for every one of them its path."""
    sc = grid_scene()
    want = _fresh(S, sc)
    _mark("edges")
    r = _Run(S, sc)
    r.plan()
    e0, p0 = r.b.edges()
    # (line segments inside the viewport: an edge each, in path order)
    assert np.array_equal(p0, np.repeat(np.arange(len(sc["path_rule"])), np.diff(sc["path_seg_off"])))
    _replays(r, want, 3, "replays")
    e1, p1 = r.b.edges()
    assert np.array_equal(p1, p0) and np.array_equal(e1, e0)
    r.close()


# ----------------------------------------------------------------------------------------------------------- what was asked for
# Per scenario, the placed passes (k_path_build<1>) in order: "r" = `tile lists rebuilt` (the full kernel), "k" = `tile lists kept`.
# Every first placed replay after a plan is "r" -- it saves the words --, the one behind it "k"; a render on a rank's share of the bands
# is never kept; a fresh batch inside a scenario is made before its mark.
WANT = {
    "grid": "rkkkk",
    "page": "rkk",
    "two words": "rkk",
    "holes": "rkk",
    "stale band": "rkk" + "kk" * 2,        # (asked for as kept: the band's own workgroup decides on the device)
    "transforms": "rkk" + "rkkk",          # (draw: plan, then the first placed replay)
    "bands": "rkk" + "rr" + "rkk",
    "window": "rkk" + "k" + "kk",
    "float64": "rkk" + "kkkkk",
    "inherited a": "rkk",
    "inherited b": "rkk",
    "edges": "rkk",
}
SCENARIOS = (test_grid_of_bands_and_tiles, test_a_list_longer_than_its_page, test_two_mask_words, test_empty_tiles_and_bands,
             test_one_band_rebuilt_beside_kept_bands, test_new_transforms_void_the_kept_lists, test_set_bands_voids_the_kept_lists,
             test_a_window_render_between_replays, test_a_float64_canvas_between_float32_ones,
             test_a_new_batch_on_inherited_arrays_starts_without_kept_lists, test_edges_after_replays_are_the_plans)


def _child():
    """(in the child interpreter) every scenario once, each announcing itself on stderr"""
    import svgrasterize_amd as S
    from svgrasterize_amd import _abi

    S.Context.get()
    assert (_abi.tile_rows(), _abi.tile_cols()) == (TR, TC)
    for fn in SCENARIOS:
        print("[case] -", file=sys.stderr, flush=True)   # (the scenario's fresh batches, in front of its own mark)
        fn(S)
    print("[case] end", file=sys.stderr, flush=True)


def test_kept_is_asked_for_from_the_second_placed_replay_on():
    """SVGR_DBG_PLAN in a fresh child (one child, under a time limit): a shortcut that never triggered would pass every picture."""
    env = dict(os.environ, SVGR_DBG_PLAN="1")
    env[CHILD] = "1"
    for k in ("SVGR_NO_SPECULATIVE_PLAN", "SVGR_NO_TWO_PASS_PLAN", "SVGR_SAFE_PATH", "SVGR_NO_SPARE", "SVGR_DBG_STALE_BAND"):
        env.pop(k, None)
    code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests import test_gpu_tile_lists_kept as T; T._child()"
    res = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert res.returncode == 0, res.stderr[-3000:]
    got, key = {}, None
    for line in res.stderr.splitlines():
        if line.startswith("[case] "):
            key = line[7:].strip()
            got.setdefault(key, "")
        elif key is not None and line.startswith("[geometry] k_path_build<1>"):
            assert ("tile lists kept" in line) != ("tile lists rebuilt" in line), line
            got[key] += "k" if "tile lists kept" in line else "r"
    assert got.pop("end", None) == "" and set(got.pop("-", "")) <= {"r"}   # (a fresh batch never keeps anything)
    for k in WANT:
        print(f"{k:14s} {got.get(k, '-')}")
    assert got == WANT
