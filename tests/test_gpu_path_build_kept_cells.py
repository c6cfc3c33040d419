"""What the lean placed path build (k_path_build<1, LEAN>) leaves standing between kept replays: the headers of the class-2 cells, the
layer-edge sentinels of their add lists and their two mask bits (k_tile_lists takes those from the words it saved).  All three are
the same bytes in every placed pass of one plan with one set of paints, so the lean form writes none of them -- and the host runs it
only behind a placed pass that did (PlanState::cells, csrc/svgr_plan_state.h).

The cases are those of tests/pathbuild_cases.py, put into batches of more than 4096 segments exactly as
tests/test_gpu_path_build_lean.py does (only a batch with a slab order replays under the plan's places), at both origins:

  ends_1, ends_63      a layer whose last column lies inside a tile (t_end < TC: sentinels exist), cols % 64 = 1 and 63
  ends_border          a layer that ends exactly on a tile border: no sentinel
  slab_5x17            a path of two slabs (17 bands);  slab_81x2, slab_161x2: more than 80 cells in a band row, slabs with k0 > 0
  slab_161x2_nonzero   class-1 cells (covered, no edge) beside class-2 cells in one band

Per case: plan, the placed render that writes the slab table (the full form), four lean replays; float64 and float32 canvases against
the plain float64 reference of tests/canvas_ref.py with the tolerances of tests/test_gpu_path_build.py (1e-10 absolute; 1 ULP of
float32), the device's error word clear.  Then the sequences that must void what a lean pass relies on, or leave it valid, each step
also against a FRESH batch of the same inputs (deterministic renders bit for bit; the others, whose adds land in another order, within
the float64 tolerance): new paints, new transforms + draw, a window and a float64 canvas between float32 replays, a deterministic
render between replays, a second plan between replays, the same bands set again (set_bands(0, 1, 1)) in front of a plan and in front
of a draw, another drawing on the arrays a destroyed batch left, one band's saved words made wrong
(SVGR_DBG_STALE_BAND) where the flipped bit is a class-2 cell's and where it is not.  A fresh interpreter under SVGR_DBG_PLAN reports
the form of every pass: the pass behind set_paints is `full`, the one behind it `lean` again.

Every comparison prints its worst error before it asserts.  No test provokes an error path on the device."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import canvas_cases as cc
from tests import pathbuild_cases as pc
from tests.canvas_cases import Case
from tests.canvas_ref import Entry, mask_layer
from tests.test_gpu_path_build import _check, _env
from tests.test_gpu_path_build_lean import _large
from tests.util import ROOT

pytestmark = pytest.mark.gpu

TR, TC = cc.TR, cc.TC
ENDS = {"ends_1": 127.5, "ends_63": 189.5, "ends_border": 190.5}   # x of the right edge's lower end -> cols = 129, 191, 192
ENDS_VIEW = (2 * TR + 9, 4 * TC + 40)
SLABS = ("slab_5x17_evenodd", "slab_81x2_evenodd", "slab_161x2_nonzero", "slab_81x2_border_evenodd", "slab_27x3_cut_evenodd")
CHILD = "SVGR_KEPT_CELLS_CHILD"   # set in the child interpreter: the scenarios announce themselves on stderr


def _tag(origin):
    return "o%d_%d" % origin


def _ends_shape(g, x_end):
    """A quadrilateral over three bands from column 1 on: a one-row top edge through every tile, a left edge that slants to the right (at
    x_end = 189.5 from column tile 0 in band 0 into column tile 1 in band 2), a steep right edge that ends at `x_end`."""
    below = 3 * TR
    return pc.poly(g, [(1.5, 3.2), (x_end - 9.6, 3.8), (x_end, below + 9.6), (x_end - 20.0, below + 11.2)])


def _ends_case(name, origin):
    g = cc.Geo(origin)
    d = _ends_shape(g, ENDS[name])
    case = Case(f"{name}-{_tag(origin)}", (Entry(d, None, cc.PAINTS[3]),), (), (g.r, g.c, *ENDS_VIEW), ((0, 0), (0, 1), (2, 1)))
    return pc.PB(case, ((0, tuple(pc.slabs_of(d, case.viewport))),), (), "the layer's right end")


CASES = {f"{n}-{_tag(o)}": _ends_case(n, o) for o in cc.ORIGINS for n in ENDS}
CASES.update({pb.name: pb for pb in pc.CASES if pc.base_name(pb) in SLABS})
NAMES = sorted(CASES)
SEQ = ("ends_63-o-7_83", "slab_161x2_nonzero-o0_0")       # the sequences: sentinels + one slab; column runs + class-1 cells
CHILD_CASES = ("ends_1-o0_0", "slab_81x2_evenodd-o-7_83")


def test_the_cases_cover_the_seams():
    assert len(NAMES) == 2 * (len(ENDS) + len(SLABS))
    ends = {}
    for name, pb in CASES.items():
        if name.startswith("ends_"):
            _r0, c0, _rows, cols = pc.layer_of(pb.case.entries[0].d, pb.case.viewport)
            ends[name.split("-")[0]] = (cols % TC, (c0 - pb.case.viewport[1] + cols) % TC)
    # (cols % 64, tile column one past the layer's last column: 0 = on the border, no sentinel)
    assert ends == {"ends_1": (1, 1), "ends_63": (63, 63), "ends_border": (0, 0)}, ends
    shapes = [s for pb in CASES.values() for _p, s in pb.slabs]
    assert any(len({b for b, _nb, _k0, _nk in s}) > 1 and any(nb == pc.PB_BANDS for _b, nb, _k0, _nk in s) for s in shapes), "no path of two slabs"
    assert any(any(k0 > 0 for _b, _nb, k0, _nk in s) for s in shapes) and any(any(nk == pc.PB_CELLS for _b, _nb, _k0, nk in s) for s in shapes)
    # class-1 cells beside class-2 cells in one band (the layout of tests/pathbuild_cases.py: band 1 of the 161-tile shape)
    lay = CASES["slab_161x2_nonzero-o0_0"].case.layout
    assert {c for _k, _i, b, _t, c in lay if b == 1} >= {1} and {c for _k, _i, b, _t, c in lay if b == 0} >= {2}


@pytest.fixture(scope="module")
def S():
    import svgrasterize_amd as S

    S.Context.get()
    return S


def _mark(text):
    if os.environ.get(CHILD):
        print(text, file=sys.stderr, flush=True)


def _close64(got, want, what):
    err = np.abs(got - want).max(initial=0.0)
    print(f"{what}: against the fresh batch, max abs diff {err:.3e}")
    assert err <= 2e-10, what   # (both within 1e-10 of the reference)


class _Run:
    """The large batch of a case, its reference and its output buffers."""

    def __init__(self, S, pb, paints=None):
        from svgrasterize_amd import _abi

        self.S, self.abi = S, _abi
        case = _large(pb)
        if paints is not None:
            case = case._replace(name=case.name + "_recoloured", entries=tuple(e._replace(paint=p) for e, p in zip(case.entries, paints)))
        self.case = case
        self.ctx = S.Context.get()
        self.batch = cc.build_batch(S, case, self.ctx)
        self.rows, self.cols = case.viewport[2:]
        self.ref = pc.reference(case)
        self.out = {dt: self.ctx.alloc(self.rows * self.cols * (32 if dt is np.float64 else 16)) for dt in (np.float64, np.float32)}

    def plan(self):
        _mark("[pass] plan")
        self.batch.plan()

    def render(self, what, dt=np.float64, det=False, draw=False, ref=None):
        kind = self.abi.OUT_CANVAS_F64 if dt is np.float64 else self.abi.OUT_CANVAS_F32
        _mark(f"[pass] {'det' if det else 'draw' if draw else 'plain'} {what}")
        (self.batch.draw if draw else self.batch.render)(self.out[dt], kind, self.abi.RENDER_DETERMINISTIC if det else 0)
        got = self.out[dt].download((self.rows, self.cols, 4), dt)
        _check(got, self.ref if ref is None else ref, f"{self.case.name} [{what}]")
        return got

    def window(self, what, win):
        out = self.ctx.alloc(win[2] * win[3] * 32)
        _mark(f"[pass] plain {what}")
        self.batch.render(out, self.abi.OUT_CANVAS_F64, 0, window=(self.case.viewport[0] + win[0], self.case.viewport[1] + win[1], win[2], win[3]))
        got = out.download((win[2], win[3], 4), np.float64)
        out.free()
        _check(got, self.ref[win[0]:win[0] + win[2], win[1]:win[1] + win[3]], f"{self.case.name} [{what}]")
        return got

    def warm(self):
        """plan, the render that finds the plan's last pass in place, the placed render that writes the slab table (full), one lean replay"""
        self.plan()
        for nth in (1, 2, 3):
            self.render(f"render {nth}")

    def close(self):
        self.batch.timings()    # (waits for the stream and raises on the device's sticky error word)
        for o in self.out.values():
            o.free()
        self.batch.destroy()


def _fresh(S, pb, paints=None, dt=np.float64):
    """the deterministic picture of a new batch of the same inputs"""
    r = _Run(S, pb, paints)
    r.plan()
    want = r.render("fresh batch", dt, det=True)
    r.close()
    return want


def replays(S, name):
    _mark(f"[case] replays {name}")
    with _env():
        r = _Run(S, CASES[name])
        r.plan()
        r.render("render 1: the plan's pass in place")
        r.render("render 2: the full placed pass")
        for nth in (1, 2):
            r.render(f"lean replay {nth}")
        for nth in (3, 4):
            r.render(f"lean replay {nth}, float32", np.float32)
        r.close()


@pytest.mark.parametrize("name", NAMES)
def test_lean_replays_equal_the_reference(S, name):
    replays(S, name)


def new_paints(S, name):
    """new colours, same geometry: the headers carry the paint, so the pass behind set_paints is the full form"""
    _mark(f"[case] paints {name}")
    with _env():
        pb = CASES[name]
        r = _Run(S, pb)
        paints = [cc.PAINTS[(k + 5) % 8] * 0.75 for k in range(len(r.case.entries))]
        want = _fresh(S, pb, paints)
        ref = pc.reference(r.case._replace(name=r.case.name + "_recoloured", entries=tuple(e._replace(paint=p) for e, p in zip(r.case.entries, paints))))
        r.warm()
        r.batch.set_paints(np.array(paints))
        for nth in (1, 2, 3):
            _close64(r.render(f"replay {nth} after set_paints", ref=ref), want, f"{name}: replay {nth} after set_paints")
        r.render("float32 after set_paints", np.float32, ref=ref)
        r.close()


def new_transforms(S, name):
    _mark(f"[case] transforms {name}")
    with _env():
        pb = CASES[name]
        want = _fresh(S, pb)
        r = _Run(S, pb)
        r.warm()
        swap = S.Transform().matrix(0, 1, 0, 1, 0, 0)
        r.batch.set_transforms(np.tile(swap.m6(), (len(r.case.entries), 1)))
        _close64(r.render("draw after set_transforms", draw=True), want, f"{name}: draw")
        for nth in (1, 2, 3, 4):
            _close64(r.render(f"replay {nth} after the draw"), want, f"{name}: replay {nth} after the draw")
        r.close()


def other_outputs_between(S, name):
    """a window and a float64 canvas between float32 replays; a deterministic render between replays"""
    _mark(f"[case] between {name}")
    with _env():
        pb = CASES[name]
        want = _fresh(S, pb)
        want32 = _fresh(S, pb, dt=np.float32)
        r = _Run(S, pb)
        r.warm()
        r.render("float32 replay", np.float32)
        win = (TR, TC, min(TR + 5, r.rows - TR), TC + 9)
        _close64(r.window("window between replays", win), want[win[0]:win[0] + win[2], win[1]:win[1] + win[3]], f"{name}: window")
        r.render("float32 replay after the window", np.float32)
        _close64(r.render("float64 canvas between float32 replays"), want, f"{name}: float64 canvas")
        r.render("float32 replay after the float64 canvas", np.float32)
        a = r.render("deterministic between replays", det=True)
        assert np.array_equal(a, want), f"{name}: the deterministic render is not the fresh batch's"
        a32 = r.render("deterministic float32", np.float32, det=True)
        assert np.array_equal(a32, want32), f"{name}: the deterministic float32 render is not the fresh batch's"
        for nth in (1, 2):
            _close64(r.render(f"replay {nth} after the deterministic renders"), want, f"{name}: replay {nth} after the deterministic renders")
        r.close()


def _cut(text):
    """(in the child interpreter) a transition: no pass behind it may be lean before a full placed pass has run"""
    _mark(f"[transition] {text}")


def plan_again(S, name):
    """svgr_batch_plan between kept replays: the planner's own passes are unplanned ones and write the cells at other places"""
    _mark(f"[case] plan again {name}")
    with _env():
        pb = CASES[name]
        want = _fresh(S, pb)
        r = _Run(S, pb)
        r.warm()
        r.render("lean replay before the second plan")
        _cut("plan")
        r.plan()
        for nth in (1, 2, 3, 4):
            _close64(r.render(f"replay {nth} after the second plan"), want, f"{name}: replay {nth} after the second plan")
        r.render("float32 after the second plan", np.float32)
        r.close()


def same_bands(S, name):
    """set_bands(0, 1, 1) on a batch that has all the bands already: nothing moves, and the plan is void all the same -- a new plan
    and replays, then the same in front of a draw"""
    _mark(f"[case] same bands {name}")
    with _env():
        pb = CASES[name]
        want = _fresh(S, pb)
        r = _Run(S, pb)
        r.warm()
        r.render("lean replay before set_bands")
        _cut("set_bands, plan")
        r.batch.set_bands(0, 1, 1)
        r.plan()
        for nth in (1, 2, 3, 4):
            _close64(r.render(f"replay {nth} after set_bands and a plan"), want, f"{name}: replay {nth} after set_bands and a plan")
        _cut("set_bands, draw")
        r.batch.set_bands(0, 1, 1)
        _close64(r.render("draw after set_bands", draw=True), want, f"{name}: draw after set_bands")
        for nth in (1, 2, 3, 4):
            _close64(r.render(f"replay {nth} after set_bands and a draw"), want, f"{name}: replay {nth} after set_bands and a draw")
        r.render("float32 after set_bands", np.float32)
        r.close()


def inherited(S, first, second):
    """destroy, then a batch of another drawing (same viewport) on the arrays the first one left"""
    _mark(f"[case] inherited {second}")
    with _env():
        r = _Run(S, CASES[first])
        r.warm()
        r.render("replay before destroy")
        r.close()
        want = _fresh(S, CASES[second])
        r = _Run(S, CASES[second])
        r.warm()
        for nth in (1, 2):
            _close64(r.render(f"replay {nth} on inherited arrays"), want, f"{second}: replay {nth} on inherited arrays")
        r.render("float32 on inherited arrays", np.float32)
        r.close()


def stale_band(S, name, bands):
    """the saved words of one band made wrong in front of a kept launch: still four launches, still the fresh picture -- whether the
    flipped bit (entry 0 of the band's list in column tile 0) is a class-2 cell's, which the lean pass does not set, or not"""
    _mark(f"[case] stale {name}")
    pb = CASES[name]
    with _env():
        want = _fresh(S, pb)
        r = _Run(S, pb)
        r.warm()
    for band in bands:
        with _env():
            os.environ["SVGR_DBG_STALE_BAND"] = str(band)
            try:
                n0 = r.ctx.launches()
                got = r.render(f"band {band} made stale")
                n = r.ctx.launches() - n0
            finally:
                os.environ.pop("SVGR_DBG_STALE_BAND", None)
            assert n == 4, (band, n)
            _close64(got, want, f"{name}: band {band} made stale")
            _close64(r.render(f"replay behind band {band}"), want, f"{name}: replay behind band {band}")
    with _env():
        r.close()


@pytest.mark.parametrize("name", SEQ)
def test_new_paints_force_one_full_pass(S, name):
    new_paints(S, name)


@pytest.mark.parametrize("name", SEQ)
def test_new_transforms_and_a_draw(S, name):
    new_transforms(S, name)


@pytest.mark.parametrize("name", SEQ)
def test_other_outputs_and_deterministic_renders_between_replays(S, name):
    other_outputs_between(S, name)


@pytest.mark.parametrize("name", SEQ)
def test_a_second_plan_between_replays(S, name):
    plan_again(S, name)


@pytest.mark.parametrize("name", SEQ)
def test_the_same_bands_set_again(S, name):
    same_bands(S, name)


def test_another_drawing_on_inherited_arrays(S):
    inherited(S, "ends_1-o-7_83", "ends_63-o-7_83")


def test_a_stale_band_is_listed_again_from_its_full_words(S):
    name = "ends_63-o0_0"
    case = CASES[name].case
    d = case.entries[0].d
    # band 0: entry 0 has its top edge in column tile 0 -- partly covered pixels, pieces, class 2; band 2: the slanted left edge has
    # left column tile 0 -- no coverage, no piece in any row of the band, class 0: the bit is clear in both rows of the saved words
    m, _bb = mask_layer(d, None, case.viewport)
    assert ((m[:TR, :TC] > 0) & (m[:TR, :TC] < 1)).any() and not m[2 * TR:, :TC].any() and m[2 * TR:, TC:2 * TC].any()
    stale_band(S, name, (0, 2))


# ----------------------------------------------------------------------------------------------------------------- who ran
def _child():
    """(in the child interpreter) replay cases and the sequences, each pass announced on stderr"""
    import svgrasterize_amd as S

    S.Context.get()
    for name in CHILD_CASES:
        replays(S, name)
    new_paints(S, SEQ[0])
    other_outputs_between(S, SEQ[0])
    for name in SEQ:
        plan_again(S, name)
        same_bands(S, name)
    print("[case] end", file=sys.stderr, flush=True)


def test_the_pass_behind_set_paints_is_full():
    """SVGR_DBG_PLAN in a fresh child (one child, under a time limit): which form every pass ran, and whether it found the cells current."""
    env = dict(os.environ, SVGR_DBG_PLAN="1", SVGR_NO_SPARE="1")
    env[CHILD] = "1"
    for k in ("SVGR_NO_SPECULATIVE_PLAN", "SVGR_NO_TWO_PASS_PLAN", "SVGR_SAFE_PATH", "SVGR_DBG_STALE_BAND"):
        env.pop(k, None)
    code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests import test_gpu_path_build_kept_cells as T; T._child()"
    res = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert res.returncode == 0, res.stderr[-3000:]
    got, key, what, form, cells = {}, None, None, None, None
    cuts = {}   # per case: (what happened, the passes reported before it)
    for line in res.stderr.splitlines():
        if line.startswith("[case] "):
            key = line[7:].strip()
            got[key] = []
        elif line.startswith("[transition] "):
            cuts.setdefault(key, []).append((line[13:].strip(), len(got[key])))
        elif line.startswith("[pass] "):
            what = line[7:].strip()
        elif line.startswith("[geometry] path build form "):
            form = line[len("[geometry] path build form "):]
            assert form in ("lean", "full"), line
        elif line.startswith("[geometry] cells "):
            cells = line[len("[geometry] cells "):]
            assert cells in ("current", "stale"), line
        elif line.startswith("[geometry] k_path_build<"):
            assert form is not None and cells is not None, line
            assert form != "lean" or cells == "current", (key, what, line)   # (the lean form never runs over cells it would have to write)
            got[key].append((what, form, cells, int(line[len("[geometry] k_path_build<")])))   # (<1>: a placed pass)
            form = cells = None
    assert got.pop("end", None) == []
    for k, v in got.items():
        print(k, "".join("L" if f == "lean" else "f" for _w, f, _c, _m in v))
    for n in CHILD_CASES:
        forms = "".join("L" if f == "lean" else "f" for _w, f, _c, _m in got[f"replays {n}"])
        assert re.fullmatch(r"f{2,}L{4}", forms), (n, forms)
    # the fresh batch's passes come first; then: plan, the full placed pass, a lean replay -- set_paints -- full, lean, lean, lean
    tail = [(w, f) for w, f, _c, _m in got[f"paints {SEQ[0]}"]][-5:]
    assert tail[0][1] == "lean" and "render 3" in tail[0][0], tail
    assert tail[1][1] == "full" and "replay 1 after set_paints" in tail[1][0], tail
    assert [f for _w, f in tail[2:]] == ["lean"] * 3, tail
    # a window, a float64 canvas and the deterministic renders (themselves full) leave the cells valid: lean right behind them
    seq = got[f"between {SEQ[0]}"]
    by = {w.partition(" ")[2]: f for w, f, _c, _m in seq}
    assert by["float32 replay after the window"] == "lean" and by["float32 replay after the float64 canvas"] == "lean", seq
    assert by["deterministic between replays"] == "full" and by["replay 1 after the deterministic renders"] == "lean", seq
    # a second plan, and the same bands set again (in front of a plan, in front of a draw): lean right before each, behind it no lean
    # pass until a full placed pass (k_path_build<1>) has written the cells again, and the lean form comes back
    for name in SEQ:
        for key, n_cuts in ((f"plan again {name}", 1), (f"same bands {name}", 2)):
            seq, ends = got[key], [at for _t, at in cuts[key]] + [len(got[key])]
            assert len(ends) == n_cuts + 1, (key, cuts[key])
            for (text, at), end in zip(cuts[key], ends[1:]):
                assert seq[at - 1][1] == "lean", (key, text, seq[at - 1])
                behind = [(f, m) for _w, f, _c, m in seq[at:end]]
                assert ("full", 1) in behind and behind[-1][0] == "lean", (key, text, behind)
                assert "lean" not in [f for f, _m in behind[:behind.index(("full", 1))]], (key, text, behind)
