"""The lean placed path build (k_path_build<1, LEAN>): a kept replay behind the lean flatten, on one GPU, not deterministic, without
groups or gradients, launches the planned pass with its options compiled in.  Here the directed cases of tests/pathbuild_cases.py --
slab shapes with and without a column run (k0 > 0), edge batches around PB_BATCH, the three right ends, slivers, the closing edge of
one row, both fill rules, both origins -- are put into batches of more than 4096 segments with pathbuild_cases.filler (the recipe of
its `twopass_` cases: only a batch with a slab order replays under the plan's places), planned and rendered six times; every picture
is compared with the plain float64 reference of tests/canvas_ref.py, never with another render, and the device's error word must
be clear.  A second scenario leaves the lean form and comes back: new transforms + draw, a deterministic render between replays, a
render window, other bands (set_bands(0, 2, 1): the full form), one rank again.  In a fresh interpreter under SVGR_DBG_PLAN the
library reports the form of every pass: `lean` exactly where the conditions hold, `full` everywhere else, each at least once.

Tolerances are the project's (tests/test_gpu_path_build.py): 1e-10 absolute on the float64 canvas, 1 ULP(float32) on the float32
canvas.  Each comparison prints its worst error before it asserts.  No test provokes an error path on the device."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import canvas_cases as cc
from tests import pathbuild_cases as pc
from tests.canvas_ref import Entry
from tests.test_gpu_path_build import _check, _env
from tests.util import ROOT

pytestmark = pytest.mark.gpu

BASES = ("slab_5x17_evenodd", "slab_80x2_nonzero", "slab_81x2_evenodd", "slab_161x2_nonzero",            # one slab of 16 bands + 1; nk = 80; k0 = 80; two column runs
         "slab_81x2_border_evenodd", "slab_81x2_cut_nonzero", "slab_27x3_border_nonzero", "slab_27x3_cut_evenodd",   # (mid: every case above)
         "batch_255_edges", "batch_256_edges", "batch_257_edges", "batch_512_edges", "batch_513_edges",
         "tasks_255_of_256_lanes", "tasks_256_of_256_lanes", "tasks_513_of_256_lanes", "tasks_1_of_256_lanes")
ROUND_TRIP = ("slab_5x17_evenodd-o-7_83", "slab_161x2_nonzero-o0_0")
CHILD_CASES = ("slab_81x2_evenodd-o-7_83", "batch_513_edges-o0_0", "tasks_1_of_256_lanes-o-7_83")
CHILD = "SVGR_PBLEAN_CHILD"   # set in the child interpreter: the scenarios announce themselves on stderr


def _origin(name):
    m = re.search(r"-o(-?\d+)_(-?\d+)$", name)
    return int(m.group(1)), int(m.group(2))


def _large(pb):
    """the case in a batch of more than 4096 segments: pathbuild_cases._all's recipe for its `twopass_` cases"""
    c = pb.case
    fill = Entry(pc.filler(cc.Geo(_origin(c.name)), c.viewport[2:]), None, cc.PAINTS[7])
    return c._replace(name="lean_" + c.name, entries=c.entries + (fill,))


NAMES = [pb.name for pb in pc.CASES if pc.base_name(pb) in BASES]


def test_the_cases_cover_the_seams():
    assert len(NAMES) == 2 * len(BASES), sorted(set(BASES) - {n.split("-", 1)[0] for n in NAMES})
    assert set(ROUND_TRIP) | set(CHILD_CASES) <= set(NAMES)
    shapes = {pc.BY_NAME[n].slabs[0][1] for n in NAMES}
    assert any(any(k0 > 0 for _b, _nb, k0, _nk in s) for s in shapes), "no slab behind a column run"
    assert any(any(nb == pc.PB_BANDS for _b, nb, _k0, _nk in s) for s in shapes) and any(any(nk == pc.PB_CELLS for _b, _nb, _k0, nk in s) for s in shapes)
    assert {pc.BY_NAME[n].case.entries[0].rule for n in NAMES} == {None, "evenodd"}


@pytest.fixture(scope="module")
def S():
    import svgrasterize_amd as S

    S.Context.get()
    return S


def _mark(text):
    if os.environ.get(CHILD):
        print(text, file=sys.stderr, flush=True)


class _Run:
    """The large batch of a case, its reference and its output buffers."""

    def __init__(self, S, name):
        from svgrasterize_amd import _abi

        self.S, self.abi, self.case = S, _abi, _large(pc.BY_NAME[name])
        self.ctx = S.Context.get()
        self.batch = cc.build_batch(S, self.case, self.ctx)
        self.rows, self.cols = self.case.viewport[2:]
        self.ref = pc.reference(self.case)
        self.out = {dt: self.ctx.alloc(self.rows * self.cols * (32 if dt is np.float64 else 16)) for dt in (np.float64, np.float32)}

    def plan(self):
        _mark("[pass] plan")
        self.batch.plan()

    def render(self, what, dt=np.float64, det=False, draw=False):
        kind = self.abi.OUT_CANVAS_F64 if dt is np.float64 else self.abi.OUT_CANVAS_F32
        _mark("[pass] det" if det else "[pass] draw" if draw else "[pass] plain")
        (self.batch.draw if draw else self.batch.render)(self.out[dt], kind, self.abi.RENDER_DETERMINISTIC if det else 0)
        got = self.out[dt].download((self.rows, self.cols, 4), dt)
        _check(got, self.ref, f"{self.case.name} [{what}]")
        return got

    def window(self, what, win):
        """`win` (row0, col0, rows, cols) from the viewport's origin"""
        out = self.ctx.alloc(win[2] * win[3] * 32)
        _mark("[pass] plain")
        self.batch.render(out, self.abi.OUT_CANVAS_F64, 0, window=(self.case.viewport[0] + win[0], self.case.viewport[1] + win[1], win[2], win[3]))
        got = out.download((win[2], win[3], 4), np.float64)
        out.free()
        _check(got, self.ref[win[0]:win[0] + win[2], win[1]:win[1] + win[3]], f"{self.case.name} [{what}]")

    def rank0_of_2(self, what):
        """rank 0 of two draws bands 0, 2, ... packed one under the other (tests/test_gpu_path_build.py: route_sharded)"""
        bands = list(range(0, -(-self.rows // cc.TR), 2))
        assert self.batch.owned_rows() == len(bands) * cc.TR
        out = self.ctx.alloc(len(bands) * cc.TR * self.cols * 32)
        for nth in (1, 2, 3):
            _mark("[pass] plain")
            self.batch.render(out, self.abi.OUT_CANVAS_F64, 0)
            got = out.download((len(bands) * cc.TR, self.cols, 4), np.float64)
            for k, b in enumerate(bands):
                n = min(cc.TR, self.rows - b * cc.TR)
                _check(got[k * cc.TR: k * cc.TR + n], self.ref[b * cc.TR: b * cc.TR + n], f"{self.case.name} [{what}, render {nth}, band {b}]")
        out.free()

    def close(self):
        self.batch.timings()    # (waits for the stream and raises on the device's sticky error word)
        for o in self.out.values():
            o.free()
        self.batch.destroy()


def replays(S, name):
    """plan, six renders into the float64 canvas, two into the float32 one: the plan's own pass, the placed pass that writes the slab
    table, then kept replays -- the lean form"""
    _mark(f"[case] replays {name}")
    with _env():
        r = _Run(S, name)
        r.plan()
        for nth in range(1, 7):
            r.render(f"render {nth}")
        for nth in (1, 2):
            r.render(f"float32 render {nth}", np.float32)
        r.close()


def round_trip(S, name):
    """out of the lean form and back: new transforms + draw, a deterministic render between replays, a window, other bands"""
    _mark(f"[case] round trip {name}")
    with _env():
        r = _Run(S, name)
        r.plan()
        for nth in range(1, 5):
            r.render(f"render {nth}")
        swap = S.Transform().matrix(0, 1, 0, 1, 0, 0)
        r.batch.set_transforms(np.tile(swap.m6(), (len(r.case.entries), 1)))
        r.render("draw after set_transforms", draw=True)
        for nth in range(1, 5):
            r.render(f"replay {nth} after the draw")
        a = r.render("deterministic between replays", det=True)
        b = r.render("deterministic again", det=True)
        assert np.array_equal(a, b), f"{name}: two deterministic renders differ"
        for nth in (1, 2):
            r.render(f"replay {nth} after the deterministic renders")
        r.window("window", (cc.TR, cc.TC, min(3 * cc.TR, r.rows - cc.TR), 2 * cc.TC))
        r.render("replay after the window")
        r.batch.set_bands(0, 2, 1)
        r.plan()
        r.rank0_of_2("rank 0 of 2")
        r.batch.set_bands(0, 1, 1)
        r.plan()
        for nth in range(1, 5):
            r.render(f"replay {nth}, one rank again")
        r.close()


@pytest.mark.parametrize("name", NAMES)
def test_kept_replays_equal_the_reference(S, name):
    replays(S, name)


@pytest.mark.parametrize("name", ROUND_TRIP)
def test_leaving_and_reentering_the_lean_form(S, name):
    round_trip(S, name)


# ----------------------------------------------------------------------------------------------------------------- who ran
def _child():
    """(in the child interpreter) a few replay cases and the round trips, each pass announced on stderr"""
    import svgrasterize_amd as S

    S.Context.get()
    for name in CHILD_CASES:
        replays(S, name)
    for name in ROUND_TRIP:
        round_trip(S, name)
    print("[case] end", file=sys.stderr, flush=True)


def test_the_lean_form_runs_exactly_where_its_conditions_hold():
    """SVGR_DBG_PLAN in a fresh child (one child, under a time limit): pass by pass, `[geometry] path build form lean` exactly when
    the pass is k_path_build<1> on a kept slab table behind a lean flatten and the render is not deterministic -- one GPU, no group
    and no gradient in any case here --, `full` on every other pass: the plans, the first renders behind them, the deterministic
    renders, everything under set_bands(0, 2, 1).  Both forms ran in every scenario."""
    env = dict(os.environ, SVGR_DBG_PLAN="1", SVGR_NO_SPARE="1")   # (no work arrays inherited from an earlier batch: every large batch plans in two passes)
    env[CHILD] = "1"
    for k in ("SVGR_NO_SPECULATIVE_PLAN", "SVGR_NO_TWO_PASS_PLAN", "SVGR_SAFE_PATH", "SVGR_DBG_STALE_BAND"):
        env.pop(k, None)
    code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests import test_gpu_path_build_lean as T; T._child()"
    res = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert res.returncode == 0, res.stderr[-3000:]
    got, key, kind, fl, form = {}, None, None, None, None
    for line in res.stderr.splitlines():
        if line.startswith("[case] "):
            key = line[7:].strip()
            got[key] = ""
        elif line.startswith("[pass] "):
            kind = line[7:].strip()
        elif line.startswith("[geometry] k_flatten<"):
            fl = line.rsplit(" ", 1)[1]
            assert fl in ("lean", "full"), line
        elif line.startswith("[geometry] path build form "):
            form = line[len("[geometry] path build form "):]
            assert form in ("lean", "full"), line
        elif line.startswith("[geometry] k_path_build<"):
            assert form is not None and kind is not None, f"no form line in front of: {line}"
            kept = line.endswith("slab table kept")
            assert kept or line.endswith("slab table written"), line
            want = kind == "plain" and fl == "lean" and kept and line[24] == "1"
            assert (form == "lean") == want, (key, kind, fl, form, line)
            got[key] += "L" if form == "lean" else "f"
            fl = form = None
    assert got.pop("end", None) == ""
    for k, v in got.items():
        print(f"{k:50s} {v}")
    assert set(got) == {f"replays {n}" for n in CHILD_CASES} | {f"round trip {n}" for n in ROUND_TRIP}
    for k, v in got.items():
        assert "L" in v and "f" in v, (k, v)
    # the plan's passes (as many as its route takes; the first render finds the last of them in place), the render that writes the slab
    # table, then the six kept replays (tests/test_gpu_path_build.py: the two-pass route)
    for n in CHILD_CASES:
        assert re.fullmatch(r"f{2,}L{6}", got[f"replays {n}"]), got[f"replays {n}"]
    # the round trip re-enters the lean form after the draw, after the deterministic renders (themselves full), after the window
    # (a kept replay like any other) and after the second set_bands; nothing under two ranks is lean
    for n in ROUND_TRIP:
        assert len(re.findall("L+", got[f"round trip {n}"])) == 4, got[f"round trip {n}"]
