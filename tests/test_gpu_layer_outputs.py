"""The tile kernel's per-path layer outputs -- SVGR_OUT_MASK_F64 / FILL_F64 of a single path, MASKS_F64 / FILLS_F64 of every path
of a batch back to back: k_tile_render<2> / <3>, the `OUT > 1` branch of `process` -- against the plain float64 reference
(canvas_ref.mask_layer = oracle.path_mask; a fill is `mask * paint`), on the directed cases of tests/layer_out_cases.py: layers
that start and end at every seam of the 16 x 64 tile grid, class-1 and untouched tiles, layers the viewport cuts, slivers on either
side of the `mask < 1e-6` cut, layers of several paths that share tiles, a tile of 23 .. 26 layers, a batch beyond 4096 segments.

The discipline of tests/test_gpu_layer_kernels.py: the test allocates the output itself and sizes it from batch.bboxes(); the
library is handed a buffer of exactly that size, which lies in front of a guard of one layer row plus one pixel (at the output's
value size); output and guard hold NaN before every call; after it the guard is still NaN and the output holds none (the memset and
the stores cover every pixel).  Every comparison is with the reference, never with another render: the bboxes exactly, masks and
fills within 1e-11 (the mask tolerance of tests/test_gpu_fuzz.py) in ONE sweep of the whole buffer against the concatenated
references -- a store into a neighbour's layer shows there --, and where the reference is exactly 0 the device's value is +0.0 bit
for bit.  tests/test_layer_out_cases_host.py keeps every coverage 1e-9 away from the cut: no pixel is excluded.  Each comparison
prints its worst error before it asserts; the last test prints the worst per route."""
import numpy as np
import pytest

from tests import canvas_cases as cc
from tests import layer_out_cases as lc
from tests.test_gpu_path_build import _env
from tests.util import assert_close64

pytestmark = pytest.mark.gpu

TOL = 1e-11
WORST = {}   # route -> {"mask": worst error, "fill": worst error}


@pytest.fixture(scope="module")
def S():
    import svgrasterize_amd as S

    S.Context.get()
    return S


def _m6(S, shift=(0, 0)):
    """path data (x = column, y = row) -> (row, col), moved by `shift` (rows, cols)"""
    return S.Transform().matrix(0, 1, shift[0], 1, 0, shift[1]).m6()


class _Run:
    """One batch of a case.  `check` poisons a buffer, lets `call` write the layer output `what` ("mask" / "fill") into it and
    compares everything: bboxes, guard, coverage of the output, values, zeros."""

    def __init__(self, S, case, plan=True):
        from svgrasterize_amd import _abi

        self.S, self.abi, self.case = S, _abi, case
        self.ctx = S.Context.get()
        self.single = len(case.paths) == 1
        packs = [S.Path.from_svg(d).packed() for d, _r, _p in case.paths]
        offs = np.concatenate([[0], np.cumsum([len(p[0]) for p in packs])]).astype(np.int64)
        self.batch = _abi.Batch(self.ctx, np.concatenate([p[0] for p in packs]), np.concatenate([p[1] for p in packs]), offs,
                                np.tile(_m6(S), (len(packs), 1)), [1 if r == "evenodd" else 0 for _d, r, _p in case.paths],
                                np.array([p for _d, _r, p in case.paths], dtype=np.float64),
                                viewport=None if case.viewport is None else list(case.viewport))
        self.shift = (0, 0)
        self.big = None
        if plan:
            self.batch.plan()

    def kind(self, what):
        a = self.abi
        return {("mask", True): a.OUT_MASK_F64, ("fill", True): a.OUT_FILL_F64, ("mask", False): a.OUT_MASKS_F64, ("fill", False): a.OUT_FILLS_F64}[what, self.single]

    def move(self, shift):
        self.batch.set_transforms(np.tile(_m6(self.S, shift), (len(self.case.paths), 1)))
        self.shift = tuple(shift)

    def layout(self):
        """(pixels of the output, pixels of the guard) from batch.bboxes(), which must be the reference's layers exactly."""
        bb = self.batch.bboxes()
        refs = lc.reference(self.case, self.shift)
        assert len(bb) == len(refs)
        for p, (_m, _f, want) in enumerate(refs):
            got = tuple(int(v) for v in bb[p])
            if want is None:
                assert got[2] <= 0 or got[3] <= 0, f"{self.case.name}: path {p} has the bbox {got}, the reference none"
            else:
                assert got == want, f"{self.case.name}: path {p} has the bbox {got}, the reference {want}"
        live = (bb[:, 2] > 0) & (bb[:, 3] > 0)
        n = int(np.where(live, bb[:, 2].astype(np.int64) * bb[:, 3], 0).sum())
        guard = int(bb[live, 3].max(initial=0)) + 1    # one row of the widest layer plus one pixel
        return n, guard

    def want(self, what):
        refs = lc.reference(self.case, self.shift)
        parts = [(m if what == "mask" else f).ravel() for m, f, bb in refs if bb is not None]
        return np.concatenate(parts) if parts else np.zeros(0)

    def buffers(self, what, short=0):
        """(the NaN-filled block, the view of exactly the output's size -- `short` bytes less -- the library gets, doubles of the output)"""
        n, guard = self.layout()
        v = 1 if what == "mask" else 4
        if self.big is not None:
            self.big.free()
        self.big = self.ctx.from_host(np.full((n + guard) * v, np.nan))
        return self.big, self.ctx.wrap(self.big.ptr, n * v * 8 - short), n * v

    def check(self, route, what, call, tag="", prepare=None):
        big, out, n = self.buffers(what)
        if prepare is not None:   # (what voids the plan comes after the buffers are sized from its bboxes)
            prepare()
        call(out, self.kind(what))
        got = big.download((big.nbytes // 8,), np.float64)
        out.free()
        body, tail = got[:n], got[n:]
        name = f"{self.case.name} [{route}{tag}] {what}"
        assert np.isnan(tail).all(), f"{name}: a store behind the output ({int((~np.isnan(tail)).sum())} values of the guard)"
        assert not np.isnan(body).any(), f"{name}: {int(np.isnan(body).sum())} values of the output were never written"
        want = self.want(what)
        err = float(np.abs(body - want).max(initial=0.0))
        w = WORST.setdefault(route, {"mask": 0.0, "fill": 0.0})
        w[what] = max(w[what], err)
        print(f"{name}: max abs err {err:.3e}")
        assert_close64(body, want, atol=TOL, what=name)
        zero = want == 0.0
        assert not body.view(np.uint64)[zero].any(), f"{name}: {int((body.view(np.uint64)[zero] != 0).sum())} values that are not +0.0 where the reference is 0"
        return body

    def close(self):
        if self.big is not None:
            self.big.free()
        self.batch.destroy()


def _render(r, flags=0):
    return lambda out, kind: r.batch.render(out, kind, flags)


def _draw(r):
    return lambda out, kind: r.batch.draw(out, kind, 0)


# ------------------------------------------------------------------------------------------------------------------ the routes
@pytest.mark.parametrize("case", lc.CASES, ids=lc.IDS)
def test_plan_render_and_a_second_render_equal_the_reference(S, case):
    """plan(), a render (which finds the plan's own geometry pass in place) and a second one (which runs the geometry again), for
    both outputs; on the batch beyond 4096 segments: the two-pass plan as shipped and its replays under the plan's places."""
    with _env():
        r = _Run(S, case)
        for what in ("mask", "fill"):
            for nth in (1, 2, 3) if case in lc.BIG else (1, 2):
                r.check("plan + render", what, _render(r), f", render {nth}")
        r.close()


@pytest.mark.parametrize("case", lc.CASES, ids=lc.IDS)
def test_deterministic_renders_are_identical_and_equal_the_reference(S, case):
    with _env():
        r = _Run(S, case)
        for what in ("mask", "fill"):
            a = r.check("deterministic", what, _render(r, r.abi.RENDER_DETERMINISTIC), ", first")
            b = r.check("deterministic", what, _render(r, r.abi.RENDER_DETERMINISTIC), ", second")
            assert a.tobytes() == b.tobytes(), f"{case.name}: two deterministic {what} renders differ"
        r.close()


@pytest.mark.parametrize("case", lc.CASES, ids=lc.IDS)
def test_draw_with_a_layer_output_equals_the_reference(S, case):
    """svgr_batch_draw: plan and render behind one wait.  (The first plan() is there to size the output from batch.bboxes(); the
    same transforms set again void it.)"""
    with _env():
        r = _Run(S, case)
        for what in ("mask", "fill"):
            r.check("draw", what, _draw(r), prepare=lambda: r.move((0, 0)))
            r.check("draw", what, _render(r), ", then render")
        r.close()


@pytest.mark.parametrize("case", lc.CASES, ids=lc.IDS)
def test_translated_geometry_equals_the_reference_of_the_translated_path(S, case):
    """set_transforms to the same geometry moved by (+3 rows, -5 columns): the layers' offsets move, their place in the tile grid
    changes (and so does what the viewport cuts off); the reference is the oracle's mask of the moved points."""
    with _env():
        r = _Run(S, case)
        r.check("translated", "mask", _render(r), ", before")
        r.move(lc.SHIFT)
        r.batch.plan()
        for what in ("mask", "fill"):
            r.check("translated", what, _render(r))
        r.check("translated", "fill", _draw(r), ", by draw", prepare=lambda: r.move(lc.SHIFT))
        r.close()


@pytest.mark.parametrize("case", lc.CASES, ids=lc.IDS)
def test_the_planner_switches_equal_the_reference(S, case):
    """SVGR_NO_SPECULATIVE_PLAN, SVGR_NO_TWO_PASS_PLAN and SVGR_SAFE_PATH, one at a time (the other two unset), around plan and renders"""
    for switch in ("SVGR_NO_SPECULATIVE_PLAN", "SVGR_NO_TWO_PASS_PLAN", "SVGR_SAFE_PATH"):
        with _env(switch):
            r = _Run(S, case)
            for what in ("mask", "fill"):
                for nth in (1, 2):
                    r.check(switch, what, _render(r), f", render {nth}")
            r.close()


# ------------------------------------------------------------------------------------------------------------------ the public API
API = [c for c in lc.SINGLE if lc.base_name(c).rsplit("_", 1)[0] in
       ("row_start_15", "col_start_63", "col_end_0", "one_pixel", "class1_interior", "class1_cut_right", "untouched_tiles", "cut_all_sides",
        "outside", "slivers_at_the_cut", "no_viewport")]


@pytest.mark.parametrize("case", API, ids=[c.name for c in API])
def test_path_mask_and_path_fill_equal_the_reference(S, case):
    d, rule, paint = case.paths[0]
    m, f, bb = lc.reference(case)[0]
    tr = S.Transform().matrix(0, 1, 0, 1, 0, 0)
    for what, res, want in (("mask", S.Path.from_svg(d).mask(tr, rule, case.viewport), m),
                            ("fill", S.Path.from_svg(d).fill(tr, np.array(paint, dtype=np.float64), rule, case.viewport), f)):
        if bb is None:
            assert res is None, f"{case.name}: a {what} of a path outside the viewport"
            continue
        assert res is not None, f"{case.name}: no {what}"
        layer, _hull = res
        assert (int(layer.offset[0]), int(layer.offset[1])) == bb[:2], f"{case.name}: {what} offset {layer.offset}"
        img = np.asarray(layer.image)
        assert img.shape[:2] == bb[2:] and img.size == want.size, f"{case.name}: {what} shape {img.shape}"
        err = float(np.abs(img.reshape(want.shape) - want).max(initial=0.0))
        w = WORST.setdefault("Path.mask / Path.fill", {"mask": 0.0, "fill": 0.0})
        w[what] = max(w[what], err)
        print(f"{case.name} [Path.{what}]: max abs err {err:.3e}")
        assert_close64(img.reshape(want.shape), want, atol=TOL, what=f"{case.name} Path.{what}")


# ------------------------------------------------------------------------------------------------------------------ refusals
def _refused(r, what, call, short=0):
    """`call` raises ValueError, launches nothing and leaves output and guard as they were: NaN"""
    big, out, _n = r.buffers(what, short)
    before = r.ctx.launches()
    with pytest.raises(ValueError):
        call(out)
    assert r.ctx.launches() == before, "a refused call launched a kernel"
    r.ctx.sync()
    assert np.isnan(big.download((big.nbytes // 8,), np.float64)).all(), "a refused call wrote to the output"
    out.free()


def test_layer_outputs_are_refused_where_they_do_not_exist(S):
    from svgrasterize_amd import _abi

    with _env():
        one = _Run(S, lc.BY_NAME["row_start_7_nonzero-o-7_83"])
        r0, c0, rows, cols = one.case.viewport
        for what, kind in (("mask", _abi.OUT_MASK_F64), ("fill", _abi.OUT_FILL_F64)):
            _refused(one, what, lambda out: one.batch.render(out, kind, 0, window=(r0 + 16, c0 + 64, 16, 64)))    # a window with a layer output
            _refused(one, what, lambda out: one.batch.render(out, kind), short=8)                                 # 8 bytes short
            one.check("after a refusal", what, _render(one))                                                      # (the batch still renders)
        one.close()
        many = _Run(S, lc.BY_NAME["neighbours-o-7_83"])
        for what, kind, kinds in (("mask", _abi.OUT_MASK_F64, _abi.OUT_MASKS_F64), ("fill", _abi.OUT_FILL_F64, _abi.OUT_FILLS_F64)):
            _refused(many, what, lambda out: many.batch.render(out, kind))                                        # a single-path output of 8 paths
            _refused(many, what, lambda out: many.batch.render(out, kinds), short=8)
            _refused(many, what, lambda out: many.batch.render(out, kinds, 0, window=(r0 + 16, c0 + 64, 16, 64)))
            many.check("after a refusal", what, _render(many))
        many.batch.set_bands(0, 2, 1)                                                                             # sharded: no per-path outputs
        many.batch.plan()
        for what, kinds in (("mask", _abi.OUT_MASKS_F64), ("fill", _abi.OUT_FILLS_F64)):
            _refused(many, what, lambda out: many.batch.render(out, kinds))
        many.close()
        # isolated groups and gradient paints exist in the canvas outputs only
        for name in ("group_opacity_or_clip-o0_0", "gradient_kinds-o0_0"):
            case = cc.CASES[cc.IDS.index(name)]
            ctx = S.Context.get()
            batch = cc.build_batch(S, case, ctx)
            batch.plan()
            assert len(cc.paths_of(case)) > 1
            big = ctx.from_host(np.full(case.viewport[2] * case.viewport[3] * len(cc.paths_of(case)) * 4, np.nan))
            for kind in (_abi.OUT_MASKS_F64, _abi.OUT_FILLS_F64):
                before = ctx.launches()
                with pytest.raises(ValueError):
                    batch.render(big, kind)
                assert ctx.launches() == before, f"{name}: a refused call launched a kernel"
            ctx.sync()
            assert np.isnan(big.download((big.nbytes // 8,), np.float64)).all(), f"{name}: a refused call wrote to the output"
            big.free()
            batch.destroy()


def test_zz_the_worst_error_of_every_route():
    """(a report, printed last: the worst mask and fill error of every route this process ran; every one of them was asserted)"""
    for route, w in WORST.items():
        print(f"worst error [{route}]: mask {w['mask']:.3e}, fill {w['fill']:.3e}")
        assert w["mask"] <= TOL and w["fill"] <= TOL
