"""The per-node layer kernels and the five blur-convolution kernels through the C ABI, each against the plain long-double
reference of its operation (tests/layer_ref.py, pinned on the host by test_layer_ref_host.py), at shapes that cross the
kernels' blocks: 256-thread workgroups, the 256-column block of k_convolve_cols, the 64-column block and the CONV_RB = 12 /
CONV_U = 6 row blocks of k_convolve_rows, the CONV_TAPS = 160 and 65535-row switches between the convolution routes, and the
OVER_SRCS = 24 tables of the compose kernels.  Outputs are poisoned with NaN before a call, inputs read back after it."""
import ctypes as C
import functools
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

from tests import layer_ref as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    import svgrasterize_amd as S

    return S.Context.get()


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _bb(b):
    return (C.c_int64 * 4)(*[int(v) for v in b])


def _lib(ctx):
    from svgrasterize_amd import _abi

    return ctx.lib, _abi._check


def _poisoned(ctx, shape, dtype=np.float64):
    """A device buffer of `shape` that holds NaNs (0xAB bytes for an integer type): what a kernel leaves unwritten shows."""
    fill = np.full(shape, 0xAB, dtype=dtype) if np.issubdtype(dtype, np.integer) else np.full(shape, np.nan, dtype=dtype)
    return ctx.from_host(fill)


# ====================================================================================== convolution
def _gauss(n, rng):
    x = np.arange(n) - (n - 1) / 2
    s = max(n / 5.0, 0.6) * rng.uniform(0.8, 1.2)
    g = np.exp(-x * x / (2 * s * s))
    return g / g.sum()


def _kernel(kind, kw, kh, rng):
    if kind == "gauss":      # a blur: a product of two normalised Gaussians
        return np.outer(_gauss(kw, rng), _gauss(kh, rng))
    if kind == "signed":     # rank 1 with negative weights and a total far from 1
        return np.outer(rng.uniform(-0.3, 1.0, kw), rng.uniform(-0.3, 1.0, kh)) * 3.7
    if kind == "rand":       # not rank 1
        return rng.uniform(-0.5, 1.0, (kw, kh))
    if kind == "zero":       # rank 1, total exactly 0: nothing to divide by, a direct route
        return np.outer(np.arange(1.0, kw + 1), np.linspace(-1.0, 1.0, kh))
    raise ValueError(kind)


# name: (rows, cols, kw, kh, kernel kind, route).  Output columns cols + kh - 1 sit at 63 / 64 / 65 (k_convolve_rows' block)
# and 255 / 256 / 257 / 513 (k_convolve_cols' block), rows at 1, 5, 6, 7, 11, 12, 13, 25 (CONV_RB, CONV_U).  The images of
# the 159- to 255-tap cases are just large enough to reach the seam they are there for (the long-double reference is
# rows * cols * kw * kh products).  A single tap on an axis can not take a two-pass route (the rank-1 rule wants two taps on
# both axes): those cases are direct.
CONV_CASES = {
    "b_n2": (1, 62, 2, 2, "gauss", "blocked"),
    "b_n6": (5, 59, 6, 6, "gauss", "blocked"),
    "b_n7": (6, 59, 7, 7, "signed", "blocked"),
    "b_n12": (7, 244, 12, 12, "gauss", "blocked"),
    "b_n13": (11, 244, 13, 13, "gauss", "blocked"),
    "b_n159": (4, 99, 159, 159, "gauss", "blocked"),
    "b_n160": (5, 97, 160, 160, "gauss", "blocked"),
    "b_513": (25, 501, 7, 13, "signed", "blocked"),
    "b_rows13": (13, 60, 13, 5, "signed", "blocked"),
    "b_160x3": (12, 62, 160, 3, "gauss", "blocked"),
    "b_3x160": (13, 98, 3, 160, "gauss", "blocked"),
    "b_src_smaller": (3, 4, 13, 13, "gauss", "blocked"),
    "b_src_fewer_rows": (2, 40, 7, 3, "gauss", "blocked"),
    "b_src_fewer_cols": (30, 2, 3, 7, "signed", "blocked"),
    "b_src_1x1": (1, 1, 5, 5, "gauss", "blocked"),
    "b_rows65535": (65535, 3, 5, 5, "gauss", "blocked"),
    "p_rows65536": (65536, 3, 5, 5, "gauss", "plain"),
    "p_n161": (3, 96, 161, 161, "gauss", "plain"),
    "p_n255": (2, 3, 255, 255, "gauss", "plain"),
    "p_3x161": (7, 96, 3, 161, "gauss", "plain"),
    "p_161x3": (5, 62, 161, 3, "signed", "plain"),
    "s_160": (9, 31, 10, 16, "rand", "small"),
    "s_1x1": (7, 40, 1, 1, "rand", "small"),
    "s_1x7": (5, 60, 1, 7, "gauss", "small"),
    "s_5x1": (60, 5, 5, 1, "gauss", "small"),
    "s_total0": (9, 31, 3, 5, "zero", "small"),
    "s_src_1x1": (1, 1, 3, 3, "rand", "small"),
    "u_161": (9, 31, 7, 23, "rand", "uploaded"),
    "u_1x161": (3, 100, 1, 161, "rand", "uploaded"),
    "u_161x1": (100, 3, 161, 1, "rand", "uploaded"),
    "u_45x45": (6, 40, 45, 45, "rand", "uploaded"),
}
TWO_PASS = [n for n, c in CONV_CASES.items() if c[5] in ("blocked", "plain")]


@functools.lru_cache(maxsize=None)
def _conv_case(name, ops=0):
    """(image, kernel, want, tol) of a named case, computed once; with `ops` the source is converted first (by the reference)."""
    rows, cols, kw, kh, kind, route = CONV_CASES[name]
    rng = _rng(name)
    img = rng.random((rows, cols, 4))
    k = np.ascontiguousarray(_kernel(kind, kw, kh, rng))
    assert L.is_rank1(k) == (route in ("blocked", "plain")), name
    assert (kw * kh <= 160) == (route == "small") or route in ("blocked", "plain"), name
    rank1 = route in ("blocked", "plain")
    if not ops:
        want, tol = L.convolve(img, k, rank1=rank1)
    else:
        conv, e = L.convert(img, ops)
        want, tol = L.convolve(conv, k, rank1=rank1)
        tol += float(np.abs(k).sum()) * float(np.max(e))   # (the conversion's own error, through the weights)
    for a in (img, k, want):
        a.setflags(write=False)
    return img, k, want, tol


def _run_conv(ctx, img, k, ops=None):
    lib, check = _lib(ctx)
    from svgrasterize_amd import _abi

    rows, cols = img.shape[:2]
    kw, kh = k.shape
    oshape = (rows + kw - 1, cols + kh - 1, 4)
    src = ctx.from_host(img)
    guard = oshape[1] + 1   # (pixels of NaN behind the documented output: a store one row or one pixel too far lands there, and shows)
    out = _poisoned(ctx, (oshape[0] * oshape[1] + guard, 4))
    k0 = k.copy()
    if ops is None:
        check(lib.svgr_layer_convolve(ctx.handle, out.handle, src.handle, rows, cols, _abi.ptr(k), kw, kh))
    else:
        check(lib.svgr_layer_convolve_ops(ctx.handle, out.handle, src.handle, rows, cols, _abi.ptr(k), kw, kh, ops))
    got = out.download(oshape, np.float64)
    assert np.isnan(out.download((guard, 4), np.float64, offset=oshape[0] * oshape[1] * 32)).all(), "a store behind the output"
    assert np.array_equal(src.download(img.shape, np.float64), img) and np.array_equal(k, k0)
    return got


@pytest.mark.parametrize("name", list(CONV_CASES))
def test_convolution_against_the_reference(ctx, name, monkeypatch):
    monkeypatch.delenv("SVGR_BLUR_DIRECT", raising=False)
    img, k, want, tol = _conv_case(name)
    got = _run_conv(ctx, img, k)
    print(f"{name}: max |err| {L.max_err(got, want):.3e}, bound {tol:.3e}")
    L.assert_within(got, want, tol, name)


@pytest.mark.parametrize("name", [n for n in TWO_PASS if "rows655" not in n])
def test_separable_kernels_on_the_direct_routes(ctx, name, monkeypatch):
    """SVGR_BLUR_DIRECT (read on every call) sends a rank-1 kernel through the direct stencils: the same reference."""
    img, k, want, tol = _conv_case(name)
    monkeypatch.setenv("SVGR_BLUR_DIRECT", "1")
    got = _run_conv(ctx, img, k)
    monkeypatch.delenv("SVGR_BLUR_DIRECT")
    print(f"{name} direct: max |err| {L.max_err(got, want):.3e}, bound {tol:.3e}")
    L.assert_within(got, want, tol, name)


@pytest.mark.parametrize("ops", [1 | 2, 8, 1 | 4 | 8])
@pytest.mark.parametrize("name", ["b_n13", "p_3x161", "s_160", "u_161"])
def test_convolution_of_a_source_that_still_needs_its_conversion(ctx, name, ops, monkeypatch):
    """svgr_layer_convolve_ops on one case of each route, against the reference's conversion followed by its convolution."""
    monkeypatch.delenv("SVGR_BLUR_DIRECT", raising=False)
    img, k, want, tol = _conv_case(name, ops)
    got = _run_conv(ctx, img, k, ops)
    print(f"{name} ops {ops}: max |err| {L.max_err(got, want):.3e}, bound {tol:.3e}")
    L.assert_within(got, want, tol, f"{name} ops {ops}")


def test_kernel_analysis_is_not_stale(ctx, monkeypatch):
    """The kept analysis of a kernel (by address, then by hash): weights rewritten in place at the same address, and the same
    bytes under a transposed shape, are analysed for what they are now."""
    monkeypatch.delenv("SVGR_BLUR_DIRECT", raising=False)
    rng = _rng("cache")
    img = rng.random((9, 70, 4))
    k = np.ascontiguousarray(_kernel("gauss", 5, 5, rng))
    for step, new in enumerate([k.copy(), _kernel("gauss", 5, 5, rng) * 2.5, _kernel("rand", 5, 5, rng), _kernel("signed", 5, 5, rng)]):
        k[...] = new   # (the same array object, the same address)
        want, tol = L.convolve(img, k, rank1=L.is_rank1(k))
        L.assert_within(_run_conv(ctx, img, k), want, tol, f"rewritten in place, step {step}")
    flat = np.ascontiguousarray(rng.uniform(-0.5, 1.0, 15))
    for shape in ((3, 5), (5, 3), (3, 5), (1, 15), (15, 1)):
        kk = flat.reshape(shape)   # (a view: the same 15 values at the same address)
        assert kk.__array_interface__["data"][0] == flat.__array_interface__["data"][0]
        want, tol = L.convolve(img, kk, rank1=False)
        L.assert_within(_run_conv(ctx, img, kk), want, tol, f"15 weights as {shape}")
    g = np.ascontiguousarray(np.outer(_gauss(3, rng), _gauss(5, rng)).ravel())   # rank 1 as 3 x 5, not as 5 x 3
    for shape in ((3, 5), (5, 3)):
        kk = g.reshape(shape)
        want, tol = L.convolve(img, kk, rank1=L.is_rank1(kk))
        L.assert_within(_run_conv(ctx, img, kk), want, tol, f"a 3 x 5 blur's weights as {shape}")


ROUTE_CASES = {"b_n13": "two blocked passes", "p_3x161": "two plain passes", "s_160": "direct", "u_161": "direct",
               "b_rows13": "two blocked passes", "p_161x3": "two plain passes", "s_total0": "direct", "s_1x7": "direct"}


def _route_child():
    """(in the child interpreter) the named cases, one after the other, each announced on stderr."""
    import svgrasterize_amd as S

    c = S.Context.get()
    for name in ROUTE_CASES:
        img, k, want, tol = _conv_case(name)
        print(f"[case] {name}", file=sys.stderr, flush=True)
        L.assert_within(_run_conv(c, img, k), want, tol, name)


def test_each_route_is_the_one_its_cases_were_written_for():
    """SVGR_DBG_CONV (read once per process, hence a fresh child) reports the route of every call: the named cases take the
    routes the table above says -- a later change of CONV_TAPS can not silently turn it into copies of one route."""
    env = dict(os.environ, SVGR_DBG_CONV="1")
    env.pop("SVGR_BLUR_DIRECT", None)
    code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests import test_gpu_layer_kernels as T; T._route_child()"
    res = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    taken, name = {}, None
    for line in res.stderr.splitlines():
        if line.startswith("[case] "):
            name = line[7:].strip()
        elif line.startswith("[convolve] ") and name is not None:
            taken.setdefault(name, []).append(line.rsplit(": ", 1)[1].strip())
    print(taken)
    assert taken == {n: [r] for n, r in ROUTE_CASES.items()}
    # ... and the two direct stencils are told apart by their weight count, on either side of the switch
    assert CONV_CASES["s_160"][2] * CONV_CASES["s_160"][3] == 160 and CONV_CASES["u_161"][2] * CONV_CASES["u_161"][3] == 161


# ====================================================================================== two layers
D_BIG, D_ROW = (-7, 11, 300, 517), (3, -5, 1, 1025)
PAIRS = [(D_BIG, (-50, 100, 100, 200)), (D_BIG, (250, 100, 100, 200)), (D_BIG, (50, -80, 100, 200)), (D_BIG, (50, 400, 100, 200)),
         (D_BIG, (400, 600, 20, 30)), (D_BIG, (-10, 5, 310, 530)), (D_BIG, (10, 20, 33, 300)), (D_BIG, D_BIG),
         (D_ROW, (3, -20, 1, 1100)), (D_ROW, (0, 500, 5, 700)), (D_ROW, (2, -100, 3, 300)), (D_ROW, (10, 0, 2, 50)), (D_ROW, D_ROW),
         (D_BIG, D_ROW), (D_ROW, D_BIG)]


@functools.lru_cache(maxsize=None)
def _layer(box, ch, seed):
    img = np.random.default_rng(seed).random((box[2], box[3], ch))
    if ch == 4:
        img[..., :3] *= img[..., 3:]
    img.setflags(write=False)
    return img


K4S = [(0.3, 0.5, 0.7, 0.1), (1.5, 1.0, 1.0, 0.4), (-0.5, -1.0, 0.25, 0.1)]   # (the second clips at 1, the third at 0)


@pytest.mark.parametrize("op", ["over", "over_first", "in", "crop4", "blend1", "blend3", "blend4", "blend5"])
def test_two_layer_ops_against_the_reference(ctx, op):
    lib, check = _lib(ctx)
    worst = 0.0
    for n, (db, sb) in enumerate(PAIRS):
        for ch in (1, 4):
            dst, src = _layer(db, 4, 1), _layer(sb, ch, 2 + ch)
            s_dev = ctx.from_host(src)
            d_dev = _poisoned(ctx, dst.shape) if op == "crop4" else ctx.from_host(dst)
            a = (ctx.handle, d_dev.handle, _bb(db), s_dev.handle, _bb(sb), ch)
            if op in ("over", "over_first"):
                check(lib.svgr_layer_over(*a, int(op == "over_first")))
                want, tol = L.over(dst, db, src, sb, first=op == "over_first")
                if op == "over_first":
                    tol = 0
            elif op == "in":
                check(lib.svgr_layer_in(*a))
                want, tol = L.in_(dst, db, src, sb)
            elif op == "crop4":
                check(lib.svgr_layer_crop4(*a))
                want, tol = L.crop4(db, src, sb)
            else:
                mode = int(op[-1])
                k4 = np.array(K4S[n % 3])
                check(lib.svgr_layer_blend(*a, mode, k4.ctypes.data_as(C.c_void_p)))
                want, tol = L.blend(dst, db, src, sb, mode, k4)
                if mode == 5 and n < 3:
                    assert (want == 0).any() or (want == 1).any()
            got = d_dev.download(dst.shape, np.float64)
            assert np.array_equal(s_dev.download(src.shape, np.float64), src)
            worst = max(worst, L.max_err(got, want))
            L.assert_within(got, np.asarray(want, dtype=np.float64) if np.all(np.asarray(tol) == 0) else want, tol, f"{op} pair {n} ch {ch}")
    print(f"{op}: max |err| {worst:.3e}")


def _compose_specs(n, rng, mode):
    """n layers of mixed channel counts and ops, offsets of both signs; OVER: a union wider than 256 columns."""
    specs = []
    for i in range(n):
        if mode == "over":
            rows, cols = int(rng.integers(3, 40)), int(rng.integers(5, 200))
            r0, c0 = int(rng.integers(-25, 25)), int(rng.integers(-160, 160))
        else:
            rows, cols = int(rng.integers(30, 50)), int(rng.integers(280, 330))
            r0, c0 = int(rng.integers(-8, 8)), int(rng.integers(-12, 12))
        ch = 1 if i % 5 == 3 else 4
        ops = 0 if ch == 1 else int(rng.choice([0, 0, 8, 1, 4 | 8, 1 | 2, 1 | 2 | 8, 1 | 4 | 8]))
        specs.append((rng.random((rows, cols, ch)), (r0, c0, rows, cols), ops))
    return specs


def _run_compose(ctx, specs, ob, mode):
    lib, check = _lib(ctx)
    from svgrasterize_amd import _abi

    n = len(specs)
    srcs = [ctx.from_host(s[0]) for s in specs]
    out = _poisoned(ctx, (ob[2], ob[3], 4))
    fn = lib.svgr_layer_compose_over if mode == "over" else lib.svgr_layer_compose_in
    check(fn(ctx.handle, out.handle, _bb(ob), n, (_abi._P * n)(*[b.handle for b in srcs]), (C.c_int64 * (4 * n))(*[v for s in specs for v in s[1]]),
             (C.c_int32 * n)(*[s[0].shape[2] for s in specs]), (C.c_uint32 * n)(*[s[2] for s in specs])))
    got = out.download((ob[2], ob[3], 4), np.float64)
    for b, s in zip(srcs, specs):
        assert np.array_equal(b.download(s[0].shape, np.float64), s[0])
    return got


@pytest.mark.parametrize("n", [1, 24, 25, 49])
@pytest.mark.parametrize("mode", ["over", "in"])
def test_compose_in_one_pass_against_the_reference(ctx, mode, n):
    """One, two and three tables of OVER_SRCS = 24 sources."""
    specs = _compose_specs(n, _rng(f"{mode}{n}"), mode)
    want, tol, ob = (L.compose_over if mode == "over" else L.compose_in)(specs)
    if mode == "over" and n > 1:
        assert ob[3] > 256
    got = _run_compose(ctx, specs, ob, mode)
    print(f"compose_{mode} of {n}: max |err| {L.max_err(got, want):.3e}, largest bound {float(np.max(tol)):.3e}")
    L.assert_within(got, want, tol, f"compose_{mode} of {n}")


def test_compose_in_on_a_single_pixel(ctx):
    rng = _rng("one pixel")
    specs = [(rng.random((40, 300, 4)), (0, 0, 40, 300), 8), (rng.random((20, 30, 1)), (39, 299, 20, 30), 0), (rng.random((50, 400, 4)), (-10, -100, 50, 400), 1 | 2 | 8)]
    want, tol, ob = L.compose_in(specs)
    assert tuple(ob) == (39, 299, 1, 1)
    L.assert_within(_run_compose(ctx, specs, ob, "in"), want, tol, "compose_in, one pixel")


# ====================================================================================== one layer
def _sprinkle_nan(img, rng, n):
    flat = img.reshape(-1)
    flat[rng.choice(flat.size, n, replace=False)] = np.nan


@pytest.mark.parametrize("is_max", [0, 1])
def test_morphology_against_the_reference(ctx, is_max):
    lib, check = _lib(ctx)
    rng = _rng("morph")
    cases = [((37, 41), (1, 1)), ((37, 41), (1, 9)), ((37, 41), (9, 1)), ((20, 23), (20, 23)), ((3, 700), (2, 300)), ((3, 700), (3, 1)), ((300, 5), (4, 5)),
             ((19, 300), (3, 4))]
    for (rows, cols), (ky, kx) in cases:
        img = rng.uniform(-1.0, 2.0, (rows, cols, 4))
        _sprinkle_nan(img, rng, img.size // 7)
        img[:ky, :kx, 1] = np.nan   # (one window of nothing but NaN in a channel)
        src = ctx.from_host(img)
        oshape = (rows - ky + 1, cols - kx + 1, 4)
        out = _poisoned(ctx, oshape)
        check(lib.svgr_layer_morphology(ctx.handle, out.handle, src.handle, rows, cols, ky, kx, is_max))
        want, tol = L.morphology(img, ky, kx, is_max)
        assert np.isnan(want[0, 0, 1]) and not np.isnan(want).all()
        L.assert_within(out.download(oshape, np.float64), want, tol, f"morphology {rows}x{cols} window {ky}x{kx}")
        got_src = src.download(img.shape, np.float64)
        assert np.array_equal(np.isnan(got_src), np.isnan(img)) and np.array_equal(got_src[~np.isnan(img)], img[~np.isnan(img)])


N_PX = [255, 256, 257, 300 * 517]


@pytest.mark.parametrize("n_px", N_PX)
def test_per_pixel_ops_against_the_reference(ctx, n_px):
    lib, check = _lib(ctx)
    rng = _rng(f"px{n_px}")
    img = rng.uniform(-0.25, 1.25, (n_px, 4))
    P = C.c_void_p
    # colour matrix: rows that push values below 0 and above 1
    m = np.array([[0.9, -0.7, 0.3, 0.1, -0.2], [1.4, 0.8, 0.6, 0.0, 0.3], [-0.2, -0.3, -0.4, 0.5, 0.1], [0.25, 0.25, 0.25, 0.5, -0.05]])
    buf = ctx.from_host(img)
    check(lib.svgr_layer_color_matrix(ctx.handle, buf.handle, n_px, m.ctypes.data_as(P)))
    want, tol = L.color_matrix(img, m)
    assert (want == 0).any() and (want == 1).any()
    L.assert_within(buf.download(img.shape, np.float64), want, tol, "color_matrix")
    # luminance
    src = ctx.from_host(img)
    out = _poisoned(ctx, (n_px,))
    check(lib.svgr_layer_luminance(ctx.handle, out.handle, src.handle, n_px))
    L.assert_within(out.download((n_px,), np.float64), *L.luminance(img), "luminance")
    assert np.array_equal(src.download(img.shape, np.float64), img)
    # background
    rgba = np.array([0.2, 0.4, 0.1, 0.8])
    buf = ctx.from_host(img)
    check(lib.svgr_layer_background(ctx.handle, buf.handle, n_px, rgba.ctypes.data_as(P)))
    L.assert_within(buf.download(img.shape, np.float64), *L.background(img, rgba), "background")
    # scale, in place and into another buffer: one product
    for f in (0.375, 1.0 / 3.0, -2.5e-3):
        buf = ctx.from_host(img)
        check(lib.svgr_layer_scale(ctx.handle, buf.handle, n_px * 4, f))
        L.assert_within(buf.download(img.shape, np.float64), *L.scale(img, f), f"scale by {f}")
        out = _poisoned(ctx, img.shape)
        check(lib.svgr_layer_scale_to(ctx.handle, out.handle, src.handle, n_px * 4, f))
        L.assert_within(out.download(img.shape, np.float64), *L.scale(img, f), f"scale_to by {f}")
    # clip01 with NaNs and a negative zero
    x = img.copy()
    x[::7, 2] = np.nan
    x[1, 0] = -0.0
    buf = ctx.from_host(x)
    check(lib.svgr_layer_clip01(ctx.handle, buf.handle, n_px * 4))
    L.assert_within(buf.download(x.shape, np.float64), *L.clip01(x), "clip01")
    # the four conversions, in place and into another buffer
    pix = rng.random((n_px, 4))
    pix[::5, 3] = rng.uniform(0.0, 2e-4, len(pix[::5]))   # (alphas on either side of the 1e-4 of "premultiplied -> straight")
    pix[::11, :3] *= 0.05                                   # (colours on either side of the sRGB curve's joint)
    psrc = ctx.from_host(pix)
    for ops in (1, 2, 4, 8, 1 | 2, 4 | 8, 1 | 2 | 8, 1 | 4 | 8):
        out = _poisoned(ctx, pix.shape)
        check(lib.svgr_layer_convert_to(ctx.handle, out.handle, psrc.handle, n_px, ops))
        want, tol = L.convert(pix, ops)
        L.assert_within(out.download(pix.shape, np.float64), want, tol, f"convert ops {ops}")
        out = _poisoned(ctx, pix.shape)
        check(lib.svgr_layer_convert_scale_to(ctx.handle, out.handle, psrc.handle, n_px, ops, 0.3125))
        # (the factor: one more rounding, on a value scaled by it)
        L.assert_within(out.download(pix.shape, np.float64), want * np.longdouble(0.3125), np.asarray(tol) * 0.3125 + L.U * np.abs(want).astype(np.float64) * 0.3125,
                        f"convert_scale ops {ops}")
    assert np.array_equal(psrc.download(pix.shape, np.float64), pix)


def test_to_float32_rounds_like_ieee(ctx):
    lib, check = _lib(ctx)
    rng = _rng("f32")
    f = rng.random(3000).astype(np.float32)
    up = np.nextafter(f, np.float32(2))
    ties = (f.astype(np.float64) + up.astype(np.float64)) / 2   # (exact in double: halfway between two float32 neighbours)
    assert ((ties - f) == (up - ties)).all()
    tiny = np.float64(2.0) ** -149
    x = np.concatenate([ties, -ties, rng.uniform(-1, 2, 3000), [np.nan, -0.0, 0.0, 1.0, 1.0 + 2.0 ** -24, 1.0 - 2.0 ** -25, -3.0, 2.0, 1e300, -1e300],
                        tiny * np.array([0.5, 0.5 + 2.0 ** -30, 1.0, 1.5, 2.5, 3.0, 1e3 + 0.5, 2.0 ** 22 + 0.5, 2.0 ** 23 - 0.5]), [1e-40, -1e-40, 1e-46, 1.17549435e-38]])
    x[5::97] = np.nan
    src = ctx.from_host(x)
    for clip in (0, 1):
        out = _poisoned(ctx, x.shape, np.float32)
        check(lib.svgr_layer_to_f32(ctx.handle, out.handle, src.handle, x.size, clip))
        got = out.download(x.shape, np.float32)
        want, tol = L.to_f32(x, clip)
        L.assert_within(got, want, tol, f"to_f32 clip {clip}")
    assert np.array_equal(np.isnan(src.download(x.shape, np.float64)), np.isnan(x))


def test_to_rgba8_rounds_half_to_even(ctx):
    lib, check = _lib(ctx)
    k = np.arange(256.0)
    x = np.concatenate([k / 255.0, (k[:255] + 0.5) / 255.0, [-0.0, -1e-300, 1.0 + 1e-16, 2.0, -3.0, np.nan],
                        _rng("u8").uniform(-0.2, 1.2, 4096 - 256 - 255 - 6 + 4 * 77)])
    x = x.reshape(-1, 4)
    halves = (x * 255.0) % 1.0 == 0.5
    assert halves.sum() > 100   # (ties that the product leaves exactly on k + 0.5: where half-to-even and half-up differ)
    src = ctx.from_host(x)
    out = _poisoned(ctx, x.shape, np.uint8)
    check(lib.svgr_layer_to_rgba8(ctx.handle, out.handle, src.handle, x.shape[0]))
    got = out.download(x.shape, np.uint8)
    want, _ = L.to_rgba8(x)
    assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ, first at {np.argwhere(got != want)[:3].tolist()}"
    assert np.array_equal(want.reshape(-1)[:256], np.arange(256, dtype=np.uint8))
    assert np.array_equal(np.isnan(src.download(x.shape, np.float64)), np.isnan(x))
