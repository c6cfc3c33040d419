"""Differentiable coverage on the device (svgr_cover_forward / svgr_cover_backward through svgrasterize_amd.diff): the forward
against the oracle's Path.mask, the backward bit for bit against the host build of the same header fed the DEVICE's slope plane,
both end to end against central differences of the oracle's mask, and the launch seams."""
import ctypes as C

import numpy as np
import pytest

from tests import cover_cases as K
from tests import cover_ref as R
from tests.util import assert_close64

pytestmark = pytest.mark.gpu

F64_TOL = 1e-11    # the mask KATs' tolerance (tests/test_gpu_parity.py)
ORDER_TOL = 1e-12  # device against harness: the same pieces added in another order


def _diff():
    from svgrasterize_amd import diff

    return diff


def _args(c):
    return c["segs"], c["kinds"], c["off"], c["m6"]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _forward_both(segs, kinds, off, m6, rules, vp, what):
    """Device forward against the harness: cover within the order of the additions, slope equal away from the kinks."""
    cover, slope = _diff().coverage(segs, kinds, off, m6, rules, vp)
    hcover, hslope, acc, st = K.harness_forward(segs, kinds, off, m6, rules, vp)
    assert st == 0 and cover.dtype == np.float64 and slope.dtype == np.int8
    assert_close64(cover, hcover, atol=ORDER_TOL, what=what)
    A = np.cumsum(acc, axis=2)
    for p in range(len(rules)):
        far = R.kink_distance(A[p], int(rules[p])) > 1e-9
        assert (slope[p][far] == hslope[p][far]).all(), what
    return cover, slope


def _backward_bitwise(segs, kinds, off, m6, rules, vp, slope, g, what):
    gs, gm = _diff().coverage_backward(segs, kinds, off, m6, rules, vp, slope, g)
    hgs, hgm, st = K.harness_backward(segs, kinds, off, m6, vp, slope, g.astype(np.float64))
    assert st == 0
    assert np.array_equal(_bits(gs), _bits(hgs)), f"{what}: grad_segs differs from the host build, max {np.abs(gs - hgs).max():.3e}"
    assert np.array_equal(_bits(gm), _bits(hgm)), f"{what}: grad_m6 differs from the host build, max {np.abs(gm - hgm).max():.3e}"
    return gs, gm


@pytest.mark.parametrize("name,rule,tname", K.ALL)
def test_cases_forward_backward(name, rule, tname):
    """Every case: cover against the oracle's mask, the backward from the device's own slope plane bit for bit against the
    harness, and the gradients against the differences."""
    c = K.case(name, rule, tname)
    cover, slope = _forward_both(*_args(c), c["rules"], c["viewport"], name)
    assert_close64(cover[0], K.oracle_cover(c["segs"], c["kinds"], c["m6"][0], rule), atol=F64_TOL, what=f"{name} {rule} {tname}")
    gs, gm = _backward_bitwise(*_args(c), c["rules"], c["viewport"], slope, c["g"], name)
    if c["checked"]:
        got = np.concatenate([K.point_gradients(c, gs), gm[0]])
        err = np.abs(got - c["fd"])
        print(f"{name} rule {rule} {tname}: max |grad| {np.abs(got).max():.3e}, worst err {err.max():.3e}")
        assert (err <= c["fd_tol"]).all(), (float(err.max()), float(c["fd_tol"][err.argmax()]))


def _scene(seed, n_paths, n_segs, vp, cubic_share=0.5):
    """n_paths closed outlines of n_segs segments in all (every path a ring of lines or a blob of cubics), rules mixed."""
    rng = np.random.default_rng(seed)
    counts = np.full(n_paths, n_segs // n_paths)
    counts[: n_segs - counts.sum()] += 1
    paths = []
    centre0 = np.array([vp[0] + vp[2] / 2.0, vp[1] + vp[3] / 2.0])
    radius = max(1.5, min(vp[2], vp[3]) / 2.2)
    for p, n in enumerate(counts):
        centre = centre0 + rng.uniform(-0.3, 0.3, 2) * [vp[2], vp[3]]
        if n == 0:
            paths.append((0, None))
        elif rng.uniform() < cubic_share:
            paths.append((1, K._blob(rng, int(n), radius * rng.uniform(0.5, 1.0), centre)[0]))
        else:
            paths.append((0, K._closed_lines(K._ring(rng, int(n), radius * rng.uniform(0.5, 1.0), 0.2, centre))[0]))
    # packed order inside a path does not matter here: a path is all lines or all cubics
    segs = np.concatenate([s for _k, s in paths if s is not None]) if n_segs else np.zeros((0, 4, 2))
    kinds = np.concatenate([np.full(len(s), k, dtype=np.uint8) for k, s in paths if s is not None]) if n_segs else np.zeros(0, dtype=np.uint8)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    m6 = np.tile(np.array(K.IDENTITY), (n_paths, 1)) + rng.normal(0, 0.02, (n_paths, 6))
    rules = (np.arange(n_paths) % 2).astype(np.uint8)
    g = rng.standard_normal((n_paths, vp[2], vp[3]))
    return segs, kinds, off, m6, rules, g


def _check_scene(seed, n_paths, n_segs, vp, oracle_paths=1):
    segs, kinds, off, m6, rules, g = _scene(seed, n_paths, n_segs, vp)
    what = f"{n_paths} paths, {n_segs} segments, viewport {vp}"
    cover, slope = _forward_both(segs, kinds, off, m6, rules, vp, what)
    for p in range(min(oracle_paths, n_paths)):
        s = slice(off[p], off[p + 1])
        assert_close64(cover[p], K.oracle_cover(segs[s], kinds[s], m6[p], int(rules[p]), vp), atol=F64_TOL, what=what)
    _backward_bitwise(segs, kinds, off, m6, rules, vp, slope, g, what)


def test_segment_count_seams():
    block = _diff().cover_block()
    for n in (block - 1, block, block + 1, 4 * block + 1):
        _check_scene(100 + n, 3, n, (0, 0, 33, 37))


def test_viewport_column_seams():
    scan = _diff().cover_scan()
    for cols in (1, scan - 1, scan, scan + 1, 2 * scan + 1):
        for rows in (1, 3):
            _check_scene(200 + cols + rows, 2, 11, (1, -2, rows, cols), oracle_paths=2)


def test_path_count_seams():
    for n_paths in (1, 2, 65):
        _check_scene(300 + n_paths, n_paths, 5 * n_paths + 3, (0, 0, 19, 23), oracle_paths=3)


def test_cubic_of_many_pieces():
    """One cubic scaled until it flattens to more than 256 pieces: the lane walks them all, forward and backward."""
    segs, kinds = K._blob(np.random.default_rng(5), 3, 9.0, np.array([20.0, 20.0]))
    m6 = np.array([[700.0, 0.0, 20.0 - 700.0 * segs[0, 0, 0], 0.0, 700.0, 22.0 - 700.0 * segs[0, 0, 1]]])   # an anchor lands in the viewport
    off, rules, vp = np.array([0, 3], dtype=np.int32), np.array([1], dtype=np.uint8), (0, 0, 40, 45)
    edges, seg = K.harness_edges(segs, kinds, off, m6, vp)
    assert np.bincount(seg).max() > 256
    cover, slope = _forward_both(segs, kinds, off, m6, rules, vp, "large cubic")
    assert_close64(cover[0], K.oracle_cover(segs, kinds, m6[0], 1, vp), atol=F64_TOL, what="large cubic")
    assert 0.0 < cover.mean() < 1.0
    _backward_bitwise(segs, kinds, off, m6, rules, vp, slope, np.random.default_rng(6).standard_normal((1, 40, 45)), "large cubic")


def test_negative_viewport_origin():
    _check_scene(400, 2, 12, (-7, -5, 16, 19), oracle_paths=2)


def test_float32_planes():
    """float32 planes are the float64 ones rounded (the two runs add in their own order: the double may differ in its last
    bits, so the float by one ulp where it sits on a tie); a float32 grad_out is widened exactly."""
    vp = (0, 0, 21, 26)
    segs, kinds, off, m6, rules, g = _scene(500, 3, 17, vp)
    c64, s64 = _diff().coverage(segs, kinds, off, m6, rules, vp)
    c32, s32 = _diff().coverage(segs, kinds, off, m6, rules, vp, dtype=np.float32)
    assert c32.dtype == np.float32 and s32.dtype == np.int8
    want = c64.astype(np.float32)
    ulp = np.maximum(np.nextafter(np.abs(want), np.float32(np.inf)) - np.abs(want), np.float32(2.0 ** -24))
    assert (np.abs(c32.astype(np.float64) - want.astype(np.float64)) <= ulp).all()
    assert (c32 == want).mean() > 0.99
    _backward_bitwise(segs, kinds, off, m6, rules, vp, s32, g.astype(np.float32), "float32")


def test_backward_is_deterministic():
    vp = (0, 0, 31, 29)
    segs, kinds, off, m6, rules, g = _scene(600, 5, 150, vp)
    _cover, slope = _diff().coverage(segs, kinds, off, m6, rules, vp)
    a = _diff().coverage_backward(segs, kinds, off, m6, rules, vp, slope, g)
    b = _diff().coverage_backward(segs, kinds, off, m6, rules, vp, slope, g)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))
    assert np.abs(a[0]).max() > 0.0


def test_single_path_forms():
    import svgrasterize_amd as S

    p = S.Path.from_svg("M3,4 C9,2 14,6 12,12 L4,15 Z")
    t = S.Transform().translate(1.5, 0.5).scale(1.2)
    vp = (0, 0, 22, 20)
    cover, slope = p.coverage(t, vp, fill_rule="evenodd")
    res = p.mask(t, "evenodd", viewport=list(vp))
    layer = res[0]
    placed = np.zeros((22, 20))
    r0, c0 = layer.offset
    img = np.array(layer.image)[..., 0]
    placed[r0:r0 + img.shape[0], c0:c0 + img.shape[1]] = img
    assert_close64(cover, placed, atol=F64_TOL, what="Path.coverage against Path.mask")
    g = np.random.default_rng(9).standard_normal((22, 20))
    gs, gm = p.coverage_vjp(t, vp, g, fill_rule="evenodd")
    segs, kinds = p.packed()
    hgs, hgm, _st = K.harness_backward(segs, kinds, [0, len(segs)], [t.m6()], vp, slope[None], g[None])
    assert np.array_equal(_bits(gs), _bits(hgs)) and np.array_equal(_bits(gm), _bits(hgm[0])) and gm.shape == (6,)


def test_errors_and_empty_inputs_launch_nothing():
    from svgrasterize_amd import _abi

    diff = _diff()
    ctx = _abi.Context.get()
    c = K.case("polygon", 0, "identity")
    vp = c["viewport"]
    n0 = ctx.launches()
    cover, slope = diff.coverage(np.zeros((0, 4, 2)), [], [0, 0, 0], np.tile(K.IDENTITY, (2, 1)), [0, 1], vp)
    assert cover.shape == (2, vp[2], vp[3]) and not cover.any() and not slope.any()
    gs, gm = diff.coverage_backward(np.zeros((0, 4, 2)), [], [0, 0, 0], np.tile(K.IDENTITY, (2, 1)), [0, 1], vp, slope, np.ones_like(cover))
    assert gs.shape == (0, 4, 2) and gm.shape == (2, 6) and not gm.any()
    assert ctx.launches() == n0

    d_segs, d_kinds, d_off, d_m6 = diff._upload(ctx, c["segs"], c["kinds"], c["off"], c["m6"])
    d_rules = ctx.from_host(c["rules"])
    n_px = vp[2] * vp[3]
    cover, slope, status, small = ctx.alloc(n_px * 8), ctx.alloc(n_px), ctx.alloc(4), ctx.alloc(n_px - 1)
    g_segs, g_m6 = ctx.alloc(len(c["segs"]) * 64), ctx.alloc(48)
    status.zero()

    def forward(desc, cover=cover, slope=slope, segs=d_segs):
        return ctx.lib.svgr_cover_forward(ctx.handle, C.byref(desc), segs.handle, d_kinds.handle, d_off.handle, d_m6.handle, d_rules.handle,
                                          cover.handle, slope.handle, status.handle)

    def backward(desc, grad=cover, g_segs=g_segs):
        return ctx.lib.svgr_cover_backward(ctx.handle, C.byref(desc), d_segs.handle, d_kinds.handle, d_off.handle, d_m6.handle, slope.handle,
                                           grad.handle, g_segs.handle, g_m6.handle, status.handle)

    def desc(n_segs=len(c["segs"]), n_paths=1, vp=vp, plane=_abi.COVER_F64, flatness=0.1):
        return diff._desc(n_segs, n_paths, vp, plane, flatness)

    n0 = ctx.launches()
    invalid, overflow = -1, -5
    for d in (desc(n_segs=-1), desc(n_paths=0), desc(vp=(0, 0, 0, 5)), desc(vp=(0, 0, 5, -1)), desc(plane=2), desc(flatness=0.0),
              desc(flatness=float("nan")), desc(n_paths=2), desc(n_segs=len(c["segs"]) + 1)):
        assert forward(d) == invalid and backward(d) == invalid
    assert forward(desc(), slope=small) == invalid and forward(desc(plane=_abi.COVER_F32), cover=small) == invalid
    assert backward(desc(), g_segs=ctx.alloc(len(c["segs"]) * 64 - 8)) == invalid
    for d in (desc(n_paths=3, vp=(0, 0, 1 << 15, 1 << 15)), desc(vp=(0, 0, 1 << 16, 1 << 15)), desc(vp=(0, 0, 1 << 31, 1))):
        assert forward(d) == overflow and backward(d) == overflow
    assert ctx.launches() == n0
    assert forward(desc()) == 0 and ctx.launches() == n0 + 2
    assert backward(desc()) == 0 and ctx.launches() == n0 + 4
    ctx.sync()
    assert int(status.download((1,), np.uint32)[0]) == 0


def test_status_word_reports_refused_geometry():
    from svgrasterize_amd import _abi

    diff = _diff()
    segs = np.zeros((3, 4, 2))
    segs[:, 0], segs[:, 1] = [[1, 1], [6, 2], [3, 7]], [[6, 2], [3, 7], [1, 1]]
    with pytest.raises(_abi.SvgrError):
        diff.coverage(segs, [0, 0, 0], [0, 3], [[1e9, 0, 0, 0, 1, 0]], [0], (0, 0, 8, 8))
    with pytest.raises(_abi.SvgrError):
        diff.coverage_backward(segs, [0, 0, 0], [0, 3], [[1e9, 0, 0, 0, 1, 0]], [0], (0, 0, 8, 8), np.ones((1, 8, 8), dtype=np.int8), np.ones((1, 8, 8)))
