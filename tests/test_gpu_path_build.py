"""k_path_build<0|1|2> and the slab cutting of k_path_bbox against the plain float64 reference of tests/canvas_ref.py, on the directed
cases of tests/pathbuild_cases.py: slab shapes on either side of every step of slab_shape, column runs with k0 > 0, edge batches
around PB_BATCH, task totals around the lane counts, layers that end on / inside / beyond a tile.  Every case goes through every
route that launches another instantiation -- the plan as shipped and its replays, the staged plan, SVGR_SAFE_PATH, a re-plan of
either kind of batch, the two-pass plan, deterministic renders, band sharding -- and every picture is compared with the
reference's pixels, never with another render.  One more test runs the routes in a fresh interpreter under SVGR_DBG_PLAN and
asserts, from what the library reports there, which instantiation every pass launched: a picture that equals the reference does
not say who drew it.

Tolerances are the project's (tests/test_gpu_tile_variants.py): 1e-10 absolute on the float64 canvas, 1 ULP(float32) on the float32
canvas; tests/test_pathbuild_cases_host.py keeps every coverage 1e-9 away from the `mask < 1e-6` cut and shows the wide references
good to 1e-11.  Each comparison prints its worst error before it asserts."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import canvas_cases as cc
from tests import pathbuild_cases as pc
from tests.util import ROOT, assert_close64, assert_f32_1ulp, ulp_f32

pytestmark = pytest.mark.gpu

SWITCHES = ("SVGR_NO_SPECULATIVE_PLAN", "SVGR_NO_TWO_PASS_PLAN", "SVGR_SAFE_PATH")


@pytest.fixture(scope="module")
def S():
    import svgrasterize_amd as S

    S.Context.get()
    return S


@contextlib.contextmanager
def _env(*names):
    """the named switches set, every other one of SWITCHES unset; the environment as it was afterwards"""
    before = {k: os.environ.get(k) for k in SWITCHES}
    for k in SWITCHES:
        os.environ.pop(k, None)
    for k in names:
        os.environ[k] = "1"
    try:
        yield
    finally:
        for k, v in before.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _check(got, ref, what):
    """float64: within 1e-10 of the reference; float32: within 1 ULP of float32(reference).  The worst error is printed first."""
    if got.dtype == np.float64:
        print(f"{what}: f64 max abs err {np.abs(got - ref).max(initial=0.0):.3e}")
        assert_close64(got, ref, atol=1e-10, what=what)
    else:
        err = np.abs(got.astype(np.float64) - ref.astype(np.float32).astype(np.float64))
        print(f"{what}: f32 max abs err {err.max(initial=0.0):.3e}, {(err / np.maximum(ulp_f32(ref), 2.0 ** -24)).max(initial=0.0):.2f} ulp")
        assert_f32_1ulp(got, ref, what=what)


class _Run:
    """One batch of a case with its output buffers: render / draw into the float64 canvas (or the float32 one) and compare."""

    def __init__(self, S, pb):
        from svgrasterize_amd import _abi

        self.S, self.abi, self.pb, self.case = S, _abi, pb, pb.case
        self.ctx = S.Context.get()
        self.batch = cc.build_batch(S, pb.case, self.ctx)
        self.rows, self.cols = pb.case.viewport[2:]
        self.ref = pc.reference(pb.case)
        self.out = {}

    def _buf(self, dt, k=0):
        if (dt, k) not in self.out:
            self.out[dt, k] = self.ctx.alloc(self.rows * self.cols * (32 if dt is np.float64 else 16))
        return self.out[dt, k]

    def render(self, what, dt=np.float64, flags=0, k=0, draw=False):
        kind = self.abi.OUT_CANVAS_F64 if dt is np.float64 else self.abi.OUT_CANVAS_F32
        (self.batch.draw if draw else self.batch.render)(self._buf(dt, k), kind, flags)
        got = self._buf(dt, k).download((self.rows, self.cols, 4), dt)
        _check(got, self.ref, f"{self.pb.name} [{what}]")
        return got

    def same_transforms(self):
        swap = self.S.Transform().matrix(0, 1, 0, 1, 0, 0)
        self.batch.set_transforms(np.tile(swap.m6(), (len(self.case.entries), 1)))

    def close(self):
        for o in self.out.values():
            o.free()
        self.batch.destroy()


def route_as_shipped(S, pb):
    """plan(), then three renders (the first finds the plan's own pass in place), then the float32 canvas.  Up to 4096 segments the
    single-pass plan runs k_path_build<2> and, as it leaves no slab order, so does every render; beyond, the two-pass plan runs <2>
    and the renders <1> -- the second of them on the slab table the first one left (the guard)."""
    with _env():
        r = _Run(S, pb)
        r.batch.plan()
        for nth in (1, 2, 3):
            r.render(f"as shipped, render {nth}")
        r.render("as shipped, float32", np.float32)
        r.render("as shipped, float32 again", np.float32)
        r.close()


def route_staged(S, pb):
    """the staged plan (k_path_build<0> measuring, then <0> in full) and three renders: its own pass, <1>, <1> on the kept slab table"""
    with _env("SVGR_NO_SPECULATIVE_PLAN", "SVGR_NO_TWO_PASS_PLAN"):
        r = _Run(S, pb)
        r.batch.plan()
    with _env():
        for nth in (1, 2, 3):
            r.render(f"staged, render {nth}")
        r.close()


def route_safe(S, pb):
    """SVGR_SAFE_PATH: the renders take no place from the plan -- k_path_build<0> with its second pass over the rows, every time"""
    with _env("SVGR_SAFE_PATH"):
        r = _Run(S, pb)
        r.batch.plan()
        for nth in (1, 2, 3):
            r.render(f"safe, render {nth}")
        r.close()


def route_replan(S, pb):
    """set_transforms with the same matrices, then draw(): the single pass on the sizes of the batch's last plan -- <2> on a batch the
    shipped plan made (its add lists have room), <0> on one the staged plan made (its add lists are dense)"""
    for staged in (False, True):
        with _env(*(("SVGR_NO_SPECULATIVE_PLAN", "SVGR_NO_TWO_PASS_PLAN") if staged else ())):
            r = _Run(S, pb)
            r.batch.plan()
        tag = "staged" if staged else "as shipped"
        with _env():
            r.render(f"re-plan of a batch planned {tag}, before")
            r.same_transforms()
            r.render(f"re-plan of a batch planned {tag}, draw", draw=True)
            r.render(f"re-plan of a batch planned {tag}, render")
            r.render(f"re-plan of a batch planned {tag}, render again")
            r.close()


def route_deterministic(S, pb):
    """two renders under SVGR_RENDER_DETERMINISTIC (the first wave alone takes the rows: 64 lanes): the same bits, the reference's values"""
    with _env():
        r = _Run(S, pb)
        r.batch.plan()
        a = r.render("deterministic, first", flags=r.abi.RENDER_DETERMINISTIC, k=0)
        b = r.render("deterministic, second", flags=r.abi.RENDER_DETERMINISTIC, k=1)
        assert np.array_equal(a, b), f"{pb.name}: two deterministic renders differ"
        r.close()


def route_sharded(S, pb, world):
    """svgr_batch_set_bands(rank, world, 1): the staged plan (<0>), renders with <1>; owns_band inside slabs of several bands.  The
    rows as tests/test_gpu_tile_variants.py compares them: rank r draws bands r, r + world, ... packed one under the other."""
    from svgrasterize_amd import _abi

    with _env():
        ctx = S.Context.get()
        case = pb.case
        batch = cc.build_batch(S, case, ctx)
        _r0, _c0, rows, cols = case.viewport
        n_bands = -(-rows // cc.TR)
        ref = pc.reference(case)
        for rank in range(world):
            bands = [b for b in range(n_bands) if b % world == rank]
            batch.set_bands(rank, world, 1)
            batch.plan()
            assert batch.owned_rows() == len(bands) * cc.TR
            out = ctx.alloc(len(bands) * cc.TR * cols * 32)
            for nth in (1, 2):
                batch.render(out, _abi.OUT_CANVAS_F64, 0)
                got = out.download((len(bands) * cc.TR, cols, 4), np.float64)
                for k, b in enumerate(bands):
                    n = min(cc.TR, rows - b * cc.TR)   # (the viewport's last band is cut: the rows behind it are not drawn)
                    _check(got[k * cc.TR: k * cc.TR + n], ref[b * cc.TR: b * cc.TR + n], f"{pb.name} [sharded {world}, rank {rank}, render {nth}, band {b}]")
            out.free()
        batch.destroy()


@pytest.mark.parametrize("pb", pc.CASES, ids=pc.IDS)
def test_as_shipped_plan_and_replays_equal_the_reference(S, pb):
    route_as_shipped(S, pb)


@pytest.mark.parametrize("pb", pc.CASES, ids=pc.IDS)
def test_staged_plan_and_replays_equal_the_reference(S, pb):
    route_staged(S, pb)


@pytest.mark.parametrize("pb", pc.CASES, ids=pc.IDS)
def test_safe_path_renders_equal_the_reference(S, pb):
    route_safe(S, pb)


@pytest.mark.parametrize("pb", pc.CASES, ids=pc.IDS)
def test_replans_equal_the_reference(S, pb):
    route_replan(S, pb)


@pytest.mark.parametrize("pb", pc.CASES, ids=pc.IDS)
def test_deterministic_renders_are_identical_and_equal_the_reference(S, pb):
    route_deterministic(S, pb)


SHARDED = [pb for pb in pc.CASES if pc.base_name(pb).rsplit("_", 1)[0] in pc.MULTI_BAND]


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("pb", SHARDED, ids=[pb.name for pb in SHARDED])
def test_every_rank_of_a_sharded_canvas_equals_the_references_rows(S, pb, world):
    route_sharded(S, pb, world)


def test_the_sharded_cases_are_the_slabs_of_several_bands():
    assert len(SHARDED) == 2 * 2 * len(pc.MULTI_BAND)
    for pb in SHARDED:
        assert all(nb > 1 for _b, nb, _k0, _nk in pb.slabs[0][1][:-1])


# ------------------------------------------------------------------------------------------------------------------ who drew it
# What every route must report under SVGR_DBG_PLAN, pass by pass: "2w" = `[geometry] k_path_build<2>, ... slab table written`,
# "1k" = <1> on the kept table (the guard), "0m" = the staged plan's measuring run of <0>; "single" / "two" = the plan's own
# report (`[plan] single pass: err 0`, `[plan] two passes: capacity bits 0`), in the order the library prints them (a plan reports
# after its pass; draw() after its render).
ROUTES = {
    "as shipped": (route_as_shipped, ["2w", "single", "2w", "2w", "2w", "2w"]),     # plan | render 1 finds the plan's pass | 2, 3 | float32: 1, 2
    "two-pass": (route_as_shipped, ["2w", "two", "1w", "1k", "1k", "1k"]),
    "staged": (route_staged, ["0m", "0w", "1w", "1k"]),
    "safe": (route_safe, ["0w", "single", "0w", "0w"]),
    "re-plan": (route_replan, ["2w", "single", "2w", "single", "2w", "2w",            # planned as shipped: plan | draw | two renders
                               "0m", "0w", "0w", "single", "0w", "0w"]),                # planned staged (dense lists: <0>, no slab order kept by draw)
    "deterministic": (route_deterministic, ["2w", "single", "2w", "2w"]),
    "sharded": (lambda S, pb: route_sharded(S, pb, 2), ["0m", "0w", "1w"] * 2),
}
ROUTE_CASES = [("slab_81x2_nonzero-o0_0", ("as shipped", "staged", "safe", "re-plan", "deterministic")),
               ("batch_513_edges-o-7_83", ("as shipped", "staged", "safe", "re-plan", "deterministic")),
               ("slab_5x17_evenodd-o-7_83", ("as shipped", "staged", "sharded")),
               ("twopass_slab_161x2_nonzero-o0_0", ("two-pass",)),
               ("twopass_slab_5x17_evenodd-o-7_83", ("two-pass",))]


def _route_child():
    """(in the child interpreter) the named cases through their routes, one after the other, each announced on stderr."""
    import svgrasterize_amd as S

    S.Context.get()
    for name, routes in ROUTE_CASES:
        for route in routes:
            print(f"[case] {name} | {route}", file=sys.stderr, flush=True)
            ROUTES[route][0](S, pc.BY_NAME[name])
    print("[case] end", file=sys.stderr, flush=True)


def _events(lines):
    out = []
    for line in lines:
        if line.startswith("[geometry] k_path_build<"):
            out.append(line[24] + ("m" if " measuring" in line else "k" if line.rstrip().endswith("kept") else "w"))
        elif line.startswith("[plan] single pass: err "):
            out.append("single" if line.startswith("[plan] single pass: err 0 ") else "single FAILED: " + line)
        elif line.startswith("[plan] two passes: capacity bits "):
            out.append("two" if line.startswith("[plan] two passes: capacity bits 0 ") else "two FAILED: " + line)
    return out


def test_each_route_launches_the_instantiation_it_is_named_for():
    """SVGR_DBG_PLAN in a fresh child (one child, under a time limit): per case and route, the passes the library reports are the
    table's -- the speculative plans without a fall-back (`err 0`, `capacity bits 0`), the staged route without either plan's
    report, every instantiation of k_path_build where the table says, the guard on the replays that keep the slab table."""
    env = dict(os.environ, SVGR_DBG_PLAN="1", SVGR_NO_SPARE="1")   # (no work arrays inherited from an earlier batch: every large batch plans in two passes)
    for k in SWITCHES:
        env.pop(k, None)
    code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests import test_gpu_path_build as T; T._route_child()"
    res = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert res.returncode == 0, res.stderr[-3000:]
    taken, key = {}, None
    for line in res.stderr.splitlines():
        if line.startswith("[case] "):
            key = line[7:].strip()
            taken[key] = []
        elif key is not None:
            taken[key].append(line)
    assert taken.pop("end", None) == []
    want = {f"{name} | {route}": ROUTES[route][1] for name, routes in ROUTE_CASES for route in routes}
    got = {k: _events(v) for k, v in taken.items()}
    for k in want:
        print(f"{k:60s} {' '.join(got.get(k, ['-']))}")
    assert got == want
    # the staged route printed neither plan's report
    assert not any(e in ("single", "two") for k, ev in got.items() if k.endswith("| staged") or k.endswith("| sharded") for e in ev)
