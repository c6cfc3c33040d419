"""CPU-side checks of the path bbox rule (csrc/svgr_core.h: path_box, host build tests/pathbox_harness.cpp): the one function
k_path_bbox places a path by and a replay that keeps the plan's slab table checks the plan's records with.  Against the CPU
oracle's bbox (oracle.py: floor - 1 / ceil + 1, cut to the viewport) on random extents, and against the same rule in Python
integers where the oracle's 64-bit arithmetic does not reach (|x| > 1e9).  No GPU needed."""
import ctypes as C
import math

import numpy as np
import pytest

from tests.util import host_build

TR, TC = 16, 64   # rows per band, columns per tile (svgr_hip.hip)


@pytest.fixture(scope="module")
def L():
    lib = host_build("pathbox_harness")
    f64 = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
    i32 = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
    u8 = np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")
    lib.pbx_path_box.argtypes = [C.c_long, f64, u8, C.c_int, i32, C.c_int, C.c_int, i32]
    lib.pbx_path_box.restype = None
    lib.pbx_guard_ok.argtypes = [f64, C.c_int, i32, C.c_int, C.c_int, i32]
    lib.pbx_guard_ok.restype = C.c_int
    return lib


def _run(L, ext, vp, has_edge=None):
    ext = np.ascontiguousarray(ext, dtype=np.float64).reshape(-1, 4)
    n = len(ext)
    he = np.ones(n, dtype=np.uint8) if has_edge is None else np.ascontiguousarray(has_edge, dtype=np.uint8)
    out = np.zeros((n, 8), dtype=np.int32)
    L.pbx_path_box(n, ext, he, 0 if vp is None else 1, np.array(vp if vp is not None else [0, 0, 0, 0], dtype=np.int32), TR, TC, out)
    return out


def _rule(e, vp):
    """The rule in Python integers: (r0, c0, rows, cols), None when empty, "refused" when the kernel refuses the extent."""
    if not all(math.isfinite(v) for v in e):
        return "refused"
    if vp is None and not (e[0] > -1e9 and e[1] > -1e9 and e[2] < 1e9 and e[3] < 1e9):
        return "refused"
    lo = [math.floor(e[0]) - 1, math.floor(e[1]) - 1]
    hi = [math.ceil(e[2]) + 1, math.ceil(e[3]) + 1]
    if vp is not None:
        for ax in range(2):
            lo[ax] = max(lo[ax], vp[ax])
            hi[ax] = min(hi[ax], vp[ax] + vp[2 + ax])
    rows, cols = hi[0] - lo[0], hi[1] - lo[1]
    return (lo[0], lo[1], rows, cols) if rows > 0 and cols > 0 else None


def _check_bands(row, vp):
    r0, c0, rows, cols, b0, nb, nct = (int(v) for v in row[:7])
    base_r, base_c = (vp[0], vp[1]) if vp is not None else (r0, c0)
    assert b0 == (r0 - base_r) // TR and nb == (r0 + rows - 1 - base_r) // TR - b0 + 1
    ct0 = (c0 - base_c) // TC
    assert nct == (c0 + cols - 1 - base_c) // TC - ct0 + 1


@pytest.mark.parametrize("vp", [None, [0, 0, 4096, 4096], [-300, 170, 1000, 777], [5, 5, 1, 1]])
def test_path_box_is_the_oracles_bbox(L, vp):
    """4000 random extents per viewport -- inside, across the border, outside, a point, whole numbers -- against oracle.bbox of an
    edge from the extent's one corner to the other; the band and column-tile ranges against their definitions."""
    from oracle import oracle as orc

    rng = np.random.default_rng(20261016 + (0 if vp is None else sum(vp)))
    n = 4000
    c = rng.uniform(-1500.0, 5500.0, size=(n, 2))
    half = rng.uniform(0.0, 1.0, size=(n, 2)) ** 3 * rng.choice([2.0, 40.0, 900.0, 6000.0], size=(n, 1))
    ext = np.concatenate([c - half, c + half], axis=1)
    ext[::7] = np.round(ext[::7])              # whole numbers: floor == ceil
    ext[::11, 2:] = ext[::11, :2]              # a point
    got = _run(L, ext, vp)
    n_full = 0
    for e, g in zip(ext, got):
        want = orc.bbox(np.array([[e[0], e[1]], [e[2], e[3]]]), vp)
        assert want == _rule(e, vp)
        assert g[7] == 0
        if want is None:
            assert g[2] == 0 and g[3] == 0 and g[5] == 0 and g[6] == 0
        else:
            assert tuple(int(v) for v in g[:4]) == want
            _check_bands(g, vp)
            n_full += 1
    assert n_full > 50    # (the sample reaches every viewport, the one-pixel one too)


def test_path_box_degenerate_extents(L):
    """A path without an edge, one wholly outside the viewport on each side, extents beyond +-1e9 and beyond the 64-bit range (cut to
    the viewport with one, refused without), infinite and NaN coordinates (refused)."""
    vp = [0, 0, 4096, 4096]
    z = _run(L, [[1.0, 2.0, 3.0, 4.0]], vp, has_edge=[0])[0]
    assert not z.any()
    outside = [[-50.0, 10.0, -2.5, 90.0], [4100.0, 10.0, 4200.0, 90.0], [10.0, -90.0, 50.0, -1.5], [10.0, 4097.5, 50.0, 5000.0]]
    for g in _run(L, outside, vp):
        assert g[2] == 0 and g[3] == 0 and g[5] == 0 and g[6] == 0 and g[7] == 0
    rng = np.random.default_rng(7)
    big = []
    for _ in range(2000):
        e = rng.uniform(-100.0, 4200.0, size=4)
        e[2:] = np.maximum(e[2:], e[:2])
        k = rng.integers(0, 4)
        mag = 10.0 ** rng.uniform(9.0, 300.0)
        e[k] = -mag if k < 2 else mag
        big.append(e)
    big = np.array(big)
    for e, g in zip(big, _run(L, big, vp)):
        want = _rule(e, vp)
        assert g[7] == 0
        if want is None:
            assert g[2] == 0 and g[3] == 0 and g[5] == 0
        else:
            assert tuple(int(v) for v in g[:4]) == want
            _check_bands(g, vp)
    for g in _run(L, big, None):
        assert g[7] == 1 and not g[:7].any()
    bad = []
    for k in range(4):   # (a folded extent has min <= max: a minimum is -inf or a maximum +inf, or both ends are the same infinity)
        for v in ((-math.inf if k < 2 else math.inf), math.nan):
            e = [10.0, 20.0, 30.0, 40.0]
            e[k] = v
            bad.append(e)
    bad += [[math.inf, 20.0, math.inf, 40.0], [10.0, -math.inf, 30.0, -math.inf], [-math.inf, -math.inf, math.inf, math.inf]]
    for use_vp in (vp, None):
        for e, g in zip(bad, _run(L, bad, use_vp)):
            assert g[7] == 1 and not g[:7].any(), (e, g)


def test_guard_accepts_the_plans_record_and_nothing_else(L):
    """path_box_is: the record a plan kept passes for the extent it was made from; a shifted extent, or a record with another band
    count, does not."""
    vp = np.array([0, 0, 2048, 2048], dtype=np.int32)
    rng = np.random.default_rng(3)
    n_bad = 0
    for _ in range(2000):
        lo = rng.uniform(-40.0, 2000.0, size=2)
        e = np.concatenate([lo, lo + rng.uniform(0.5, 300.0, size=2)])
        g = _run(L, [e], list(vp))[0]
        rec = np.array([g[0], g[1], g[2], g[3], g[5]], dtype=np.int32)
        assert L.pbx_guard_ok(e, 1, vp, TR, TC, rec) == 1
        moved = e + np.array([3.0 * TR, 0.0, 3.0 * TR, 0.0])
        g2 = _run(L, [moved], list(vp))[0]
        if tuple(g2[:4]) != tuple(g[:4]):
            assert L.pbx_guard_ok(moved, 1, vp, TR, TC, rec) == 0
            n_bad += 1
        if g[5] > 0:
            rec2 = rec.copy(); rec2[4] += 1
            assert L.pbx_guard_ok(e, 1, vp, TR, TC, rec2) == 0
    assert n_bad > 1000
