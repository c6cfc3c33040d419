"""Differentiable coverage on the host: csrc/svgr_cover.h compiled by g++ (tests/cover_harness.cpp) against its numpy
restatement (tests/cover_ref.py), against the oracle's Path.mask, and against central differences of the oracle's mask
(tests/cover_cases.py).  No GPU."""
import os
import re

import numpy as np
import pytest

from oracle import oracle
from tests import cover_cases as K
from tests import cover_ref as R
from tests.util import ROOT, assert_close64

F64_TOL = 1e-11   # the mask KATs' tolerance (tests/test_gpu_parity.py)
CSRC = os.path.join(ROOT, "svgrasterize.py_amd", "csrc")


def _args(c):
    return c["segs"], c["kinds"], c["off"], c["m6"]


@pytest.mark.parametrize("name,rule,tname", K.ALL)
def test_harness_equals_reference(name, rule, tname):
    """Forward and backward of the header against cover_ref.py, within the rounding of the sums (the bounds come from the term
    counts and magnitudes the reference reports)."""
    c = K.case(name, rule, tname)
    cover, slope, _acc, st = K.harness_forward(*_args(c), c["rules"], c["viewport"])
    assert st == 0
    rcover, rslope, A, tol = R.forward(*_args(c), c["rules"], c["viewport"])
    # (|d cover / dA| <= 1 away from the zero cut, where both sides give 0 or a value that small)
    near_cut = R.kink_distance(A, rule) <= tol
    err = np.abs(cover - rcover)
    assert (err[~near_cut] <= tol[~near_cut] + R.U).all(), float((err - tol)[~near_cut].max())
    assert (err[near_cut] <= R.ZERO_CUT + tol[near_cut]).all()
    assert (slope[~near_cut] == rslope[~near_cut]).all()
    g = np.where(near_cut, 0.0, c["g"])   # (so that both sides walk the same W)
    gs, gm, st = K.harness_backward(*_args(c), c["viewport"], rslope, g)
    assert st == 0
    rgs, rgm, tol_s, tol_m = R.backward(*_args(c), c["viewport"], rslope, g)
    assert gs.shape == rgs.shape and (np.abs(gs - rgs) <= tol_s).all(), float((np.abs(gs - rgs) - tol_s).max(initial=0.0))
    assert (np.abs(gm - rgm) <= tol_m).all(), float((np.abs(gm - rgm) - tol_m).max(initial=0.0))
    lines = c["kinds"] == 0
    assert (gs[lines][:, 2:] == 0.0).all()   # a line's last two points stay 0
    if name not in ("empty", "outside"):
        assert np.abs(gs).max() > 0.0 or not np.abs(g * rslope).any()


@pytest.mark.parametrize("name,rule,tname", K.ALL)
def test_harness_cover_equals_oracle_mask(name, rule, tname):
    c = K.case(name, rule, tname)
    cover, _slope, _acc, st = K.harness_forward(*_args(c), c["rules"], c["viewport"])
    assert st == 0
    assert_close64(cover[0], K.oracle_cover(c["segs"], c["kinds"], c["m6"][0], rule), atol=F64_TOL, what=f"{name} {rule} {tname}")


@pytest.mark.parametrize("name,rule,tname", K.ALL)
def test_harness_edges_are_the_renderers(name, rule, tname):
    """The edge set is the one the oracle's flatten gives (level order there, curve order here), and t0 / t1 place every piece
    on its cubic."""
    c = K.case(name, rule, tname)
    edges, seg = K.harness_edges(*_args(c), c["viewport"])
    lines, cubics = K.lines_cubics(c["segs"], c["kinds"])
    want = oracle.path_edges(lines, cubics, R.m3(c["m6"][0])).reshape(-1, 4) - np.tile(np.array(c["viewport"][:2], dtype=np.float64), 2)
    key = lambda e: e[np.lexsort(e.T[::-1])]   # noqa: E731
    assert len(edges) == len(want) and (key(edges[:, :4]) == key(want)).all()
    ref = [(s, *e) for s, *e in R.path_edges(*_args(c), 0, c["viewport"])]
    assert [s for s, *_ in ref] == list(seg)
    assert all(t0 == e[4] and t1 == e[5] for (_s, _p0, _p1, t0, t1), e in zip(ref, edges))


@pytest.mark.parametrize("name,rule,tname", [k for k in K.ALL if K.CASES[k[0]][2]])
def test_gradients_equal_central_differences(name, rule, tname):
    """d sum(g * cover) / d(points, transform) of the header against central differences of sum(g * oracle mask), every copy of a
    shared point moved together; the tolerance is the differences' own (cover_cases._differences)."""
    c = K.case(name, rule, tname)
    if not c["checked"]:
        return   # (the empty path: nothing to differentiate)
    _cover, slope, _acc, _st = K.harness_forward(*_args(c), c["rules"], c["viewport"])
    gs, gm, st = K.harness_backward(*_args(c), c["viewport"], slope, c["g"])
    assert st == 0
    got = np.concatenate([K.point_gradients(c, gs), gm[0]])
    err = np.abs(got - c["fd"])
    print(f"{name} rule {rule} {tname}: max |grad| {np.abs(got).max():.3e}, worst err {err.max():.3e}, worst err / tol "
          f"{(err / np.maximum(c['fd_tol'], 1e-300)).max():.3f}")
    assert (err <= c["fd_tol"]).all(), (float(err.max()), float(c["fd_tol"][err.argmax()]))


def test_slope_is_the_rules_derivative():
    lib = K.harness()
    A = np.concatenate([np.linspace(-3.2, 3.2, 2001), [0.0, 1e-7, -1e-7, 2e-6, -2e-6, 1.0, -1.0, 1.0 - 1e-9, 2.0, 2.0 - 1e-7, 0.999999]])
    for rule in (0, 1):
        got = np.array([lib.ch_slope(float(a), rule) for a in A])
        assert (got == R.slope_of(A, rule)).all()
        assert (np.array([lib.ch_fill(float(a), rule) for a in A]) == R.cover_of(A, rule)).all()
        # away from the kinks it IS the derivative of the fill rule
        h = 1e-7
        ok = R.kink_distance(A, rule) > 1e-5
        fd = (R.cover_of(A + h, rule) - R.cover_of(A - h, rule)) / (2 * h)
        assert np.abs(fd[ok] - got[ok]).max() < 1e-6


def test_far_and_refused_geometry():
    """A point that is not finite or beyond +-1e9 sets status bit 1 and its segment adds nothing; nothing loops."""
    segs = np.zeros((3, 4, 2))
    segs[0, :2] = [[1.0, 1.0], [5.0, 2.0]]
    segs[1, :2] = [[5.0, 2.0], [3.0, np.nan]]
    segs[2, :2] = [[3.0, 4.0], [3.5, 1e10]]
    kinds = np.zeros(3, dtype=np.uint8)
    cover, slope, acc, st = K.harness_forward(segs, kinds, [0, 3], [K.IDENTITY], [0], (0, 0, 8, 8))
    assert st == 2 and np.isfinite(acc).all()
    only, _s, acc1, st1 = K.harness_forward(segs[:1], kinds[:1], [0, 1], [K.IDENTITY], [0], (0, 0, 8, 8))
    assert st1 == 0 and (acc == acc1).all()
    gs, gm, st = K.harness_backward(segs, kinds, [0, 3], [K.IDENTITY], (0, 0, 8, 8), np.ones((1, 8, 8), dtype=np.int8), np.ones((1, 8, 8)))
    assert st == 2 and np.isfinite(gs).all() and (gs[1] == 0.0).all()


def test_header_rules_and_exports():
    """The header's own rules (no fma, no contraction pragma, SVGR_HD throughout), the ABI additions and the Python surface."""
    text = open(os.path.join(CSRC, "svgr_cover.h")).read()
    assert "fma(" not in text and "fp contract" not in text.lower() and "SVGR_HD" in text
    hdr = open(os.path.join(ROOT, "include", "svgr.h")).read()
    assert "#define SVGR_ABI_VERSION 6" in hdr
    import svgrasterize_amd as S
    from svgrasterize_amd import _abi, diff

    for name in ("svgr_cover_forward", "svgr_cover_backward", "svgr_cover_block", "svgr_cover_scan"):
        assert name in _abi.EXPORTS and re.search(rf"\b{name}\s*\(", hdr)
    for name in ("coverage", "coverage_backward", "coverage_tensor"):
        assert callable(getattr(diff, name)) and name in S.__all__
    assert callable(S.Path.coverage) and callable(S.Path.coverage_vjp)


def test_python_checks_come_before_any_device_work():
    """Wrong shapes, rules, dtypes and non-finite geometry are refused without a context."""
    from svgrasterize_amd import _abi, diff

    c = K.case("polygon", 0, "identity")
    ok = dict(segs=c["segs"], kinds=c["kinds"], path_seg_off=c["off"], m6=c["m6"], rules=c["rules"], viewport=c["viewport"])
    before = dict(_abi.Context._by_device)

    def call(**kw):
        return diff.coverage(**{**ok, **kw})

    bad_segs = c["segs"].copy()
    bad_segs[1, 0, 0] = np.inf
    for kw, exc in ((dict(segs=bad_segs), ValueError), (dict(segs=c["segs"][:, :3]), ValueError), (dict(kinds=c["kinds"][:-1]), ValueError),
                    (dict(path_seg_off=[0, len(c["segs"]) + 1]), ValueError), (dict(path_seg_off=[1, len(c["segs"])]), ValueError),
                    (dict(m6=np.zeros((2, 6))), ValueError), (dict(m6=[[np.nan] * 6]), ValueError), (dict(rules=[2]), ValueError),
                    (dict(rules=[0, 1]), ValueError), (dict(viewport=(0, 0, 0, 5)), ValueError), (dict(viewport=(0, 0, 5)), ValueError),
                    (dict(dtype=np.float16), TypeError), (dict(kinds=np.full(len(c["kinds"]), 3)), ValueError)):
        with pytest.raises(exc):
            call(**kw)
    slope, g = np.zeros((1, 24, 21), dtype=np.int8), np.zeros((1, 24, 21))
    for kw, exc in ((dict(slope=slope[:, :5]), ValueError), (dict(grad_out=g[0]), ValueError), (dict(slope=slope.astype(np.float64)), TypeError),
                    (dict(grad_out=g.astype(np.float16)), TypeError)):
        with pytest.raises(exc):
            diff.coverage_backward(c["segs"], c["kinds"], c["off"], c["m6"], c["rules"], c["viewport"], **{**dict(slope=slope, grad_out=g), **kw})
    assert _abi.Context._by_device == before
