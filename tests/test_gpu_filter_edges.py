"""The filter primitives at the edges of their values, on the device: every case of tests/filter_edge_cases.py through the C ABI
and through ``Layer.*``, against the host build of csrc/svgr_core.h bit for bit (where ``pow`` is evaluated: within the
tolerance of the primitive's own tests, gamma 1e-14 and lighting 1e-13) and against the restatements; the refusals, which must
launch nothing; and the documents whose numbers are not finite, which must render without an exception and without a NaN.
Outputs of ABI calls are poisoned with NaN and end in a guard that must stay NaN (tests/test_gpu_filter_paint_seams.py's
discipline).  tests/test_filter_edges_host.py shows on the CPU that every case reaches its edge and is memory-safe."""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest

from tests import filter_edge_cases as E
from tests import filter_ref as F
from tests import lighting_ref as LR

pytestmark = pytest.mark.gpu

GAMMA_TOL, LIGHTING_TOL, TURBULENCE_TOL = 1e-14, 1e-13, 1e-15
GUARD = 5


@pytest.fixture(scope="module")
def ctx():
    import svgrasterize_amd as S

    return S.Context.get()


@functools.lru_cache(maxsize=None)
def _fh():
    return F.harness()


@functools.lru_cache(maxsize=None)
def _lh():
    return LR.harness()


def _bb(b):
    return (C.c_int64 * 4)(*[int(v) for v in b])


def _lib(ctx):
    from svgrasterize_amd import _abi

    return ctx.lib, _abi._check, _abi.ptr


def _poisoned(ctx, n_px):
    return ctx.from_host(np.full((n_px + GUARD, 4), np.nan))


def _output(buf, shape):
    n_px = int(np.prod(shape[:-1]))
    got = buf.download(shape, np.float64)
    assert np.isnan(buf.download((GUARD, 4), np.float64, offset=n_px * 32)).all(), "a store behind the output"
    return got


def _unit(values, what):
    assert not np.isnan(values).any() and (values >= 0.0).all() and (values <= 1.0).all(), what


def _names(cases):
    return [c["name"] for c in cases]


# ====================================================================================== feTurbulence
@pytest.fixture(scope="module")
def turbulence_hosts():
    """name -> (host build, restatement), each computed once."""
    from svgrasterize_amd.layer import turbulence_seed

    out = {}
    for case in E.TURBULENCE:
        px, py = E.turb_points(case)
        out[case["name"]] = (
            F.harness_turbulence(_fh(), turbulence_seed(case["seed"]), case["freq"], case["octaves"], case["fractal"], case["tile"], px, py),
            F.turbulence_exact(case["seed"], case["freq"], case["octaves"], case["fractal"], case["tile"], px, py))
    return out


@pytest.mark.parametrize("name", _names(E.TURBULENCE))
def test_turbulence(ctx, turbulence_hosts, name):
    from svgrasterize_amd import Layer
    from svgrasterize_amd.layer import turbulence_seed

    lib, check, ptr = _lib(ctx)
    case = next(c for c in E.TURBULENCE if c["name"] == name)
    host, want = turbulence_hosts[name]
    shape, tr = case["shape"], E.turb_transform(case)
    inv = np.ascontiguousarray(tr.invert.m6(), dtype=np.float64)
    tile4 = np.ascontiguousarray((0, 0, 0, 0) if case["tile"] is None else case["tile"], dtype=np.float64)
    out = _poisoned(ctx, shape[0] * shape[1])
    check(lib.svgr_layer_turbulence(ctx.handle, out.handle, _bb(case["offset"] + shape), ptr(inv), case["freq"][0], case["freq"][1],
                                    ptr(tile4), turbulence_seed(case["seed"]), case["octaves"], int(case["fractal"]),
                                    int(case["tile"] is not None)))
    got = _output(out, shape + (4,)).reshape(-1, 4)
    _unit(got, name)
    err = float(np.abs(got - want).max())
    print(f"{name}: device == host build: {np.array_equal(got, host)}, max |device - restatement| {err:.3e}, bound {TURBULENCE_TOL}")
    assert np.array_equal(got, host), np.argwhere(got != host)[:4].tolist()
    assert err <= TURBULENCE_TOL
    layer = Layer.turbulence(tr, case["offset"], shape, case["freq"], case["octaves"], case["seed"], case["tile"], case["fractal"])
    assert np.array_equal(layer.image.reshape(-1, 4), host)


# ====================================================================================== feComponentTransfer
@pytest.mark.parametrize("name", _names(E.TRANSFER))
def test_component_transfer(ctx, name):
    from svgrasterize_amd import Layer

    lib, check, ptr = _lib(ctx)
    case = next(c for c in E.TRANSFER if c["name"] == name)
    c, fn = case["c"], case["fn"]
    long_table = fn is not None and fn[0] in ("table", "discrete") and len(fn[1]) == 4096   # (4096 values in all: one channel only)
    funcs = [fn, None, ("linear", 0.5, 0.25), None if long_table else fn]
    img = np.ascontiguousarray(np.stack([c, c[::-1], c, c[::-1]], axis=1))
    host = np.stack([F.harness_transfer(_fh(), img[:, k], funcs[k]) for k in range(4)], axis=1)
    want = np.stack([F.transfer(img[:, k], funcs[k]) for k in range(4)], axis=1)
    types, params, counts, tables = np.zeros(4, dtype=np.int32), np.zeros((4, 5)), np.zeros(4, dtype=np.int64), [np.zeros(0)]
    for k, f in enumerate(funcs):
        types[k], params[k], values = F.transfer_abi(f)
        counts[k] = len(values)
        tables.append(values)
    values = np.ascontiguousarray(np.concatenate(tables) if counts.sum() else np.zeros(1))
    buf = ctx.from_host(np.concatenate([img, np.full((GUARD, 4), np.nan)]))
    check(lib.svgr_layer_component_transfer(ctx.handle, buf.handle, len(img), ptr(types), ptr(np.ascontiguousarray(params)), ptr(counts),
                                            ptr(values)))
    got = _output(buf, (len(img), 4))
    _unit(got, name)
    gamma = fn is not None and fn[0] == "gamma"
    err = float(np.abs(got - want).max())
    print(f"{name}: max |device - restatement| {err:.3e}, |device - host build| {float(np.abs(got - host).max()):.3e}")
    if gamma:
        assert np.array_equal(got[:, 1:3], host[:, 1:3]) and np.abs(got - host).max() <= GAMMA_TOL and err <= GAMMA_TOL
        assert np.array_equal(got == 0.0, host == 0.0)   # (what NaN and the clamp make 0 is 0 on both)
    else:
        assert np.array_equal(got, host) and np.array_equal(got, want)
    layer = Layer(img.reshape(1, -1, 4), (3, -2), pre_alpha=False, linear_rgb=True).component_transfer(funcs)
    assert np.array_equal(layer.image.reshape(-1, 4), got)


# ====================================================================================== feConvolveMatrix
@pytest.mark.parametrize("name", _names(E.CONVOLVE))
def test_convolve_matrix(ctx, name):
    from svgrasterize_amd import Layer

    lib, check, ptr = _lib(ctx)
    case = next(c for c in E.CONVOLVE if c["name"] == name)
    img, kernel, preserve = np.ascontiguousarray(case["image"]), case["kernel"], case["preserve"]
    args = (img, kernel, case["divisor"], case["bias"], case["target"], case["edge_mode"], preserve)
    host = F.harness_convolve_matrix(_fh(), *args)
    want = F.convolve_matrix(*args)
    rows, cols = img.shape[:2]
    src = ctx.from_host(img)
    out = _poisoned(ctx, rows * cols)
    check(lib.svgr_layer_convolve_matrix(ctx.handle, out.handle, src.handle, rows, cols, ptr(kernel), kernel.shape[1], kernel.shape[0],
                                         case["target"][0], case["target"][1], case["divisor"], case["bias"],
                                         F.EDGE_MODES[case["edge_mode"]], int(preserve)))
    got = _output(out, img.shape)
    _unit(got[..., :3] if preserve else got, name)
    assert np.array_equal(got, host) and np.array_equal(got, want)
    assert np.array_equal(src.download(img.shape, np.float64), img, equal_nan=True)
    layer = Layer(img, (4, -3), pre_alpha=not preserve, linear_rgb=True).convolve_matrix(
        kernel, case["divisor"], case["bias"], case["target"], case["edge_mode"], preserve)
    assert np.array_equal(layer.image, got)


# ====================================================================================== lighting
def _light(kind, light):
    from svgrasterize_amd.filters import DistantLight, PointLight, SpotLight

    return {LR.DISTANT: DistantLight, LR.POINT: PointLight, LR.SPOT: SpotLight}[kind](*light)


@pytest.mark.parametrize("name", _names(E.LIGHTING))
def test_lighting(ctx, name):
    from svgrasterize_amd import Layer

    lib, check, ptr = _lib(ctx)
    case = next(c for c in E.LIGHTING if c["name"] == name)
    A, params, offset, se = case["A"], np.ascontiguousarray(case["params"]), case["offset"], case["se"]
    color = np.ascontiguousarray(case["color"], dtype=np.float64)
    rows, cols = A.shape
    args = (A, offset, case["kind"], params, case["color"], case["ss"], case["constant"], se)
    host = LR.harness_layer(_lh(), *args)
    want = LR.lighting(*args)
    img = np.ascontiguousarray(np.stack([np.full(A.shape, 0.3), np.full(A.shape, 0.6), np.full(A.shape, 0.9), A], axis=-1))
    src = ctx.from_host(img)
    out = _poisoned(ctx, rows * cols)
    check(lib.svgr_layer_lighting(ctx.handle, out.handle, _bb(offset + A.shape), src.handle, _bb(offset + A.shape), case["kind"],
                                  ptr(params), ptr(color), case["ss"], case["constant"], 1.0 if se is None else se, int(se is not None)))
    got = _output(out, A.shape + (4,))
    _unit(got, name)
    to_host, to_ref = float(np.abs(got - host).max()), float(np.abs(got - want).max())
    print(f"{name}: max |device - host build| {to_host:.3e}, |device - restatement| {to_ref:.3e}, bound {LIGHTING_TOL}")
    if se is None and case["kind"] != LR.SPOT:
        assert np.array_equal(got, host)   # (no pow anywhere)
    assert to_host <= LIGHTING_TOL and to_ref <= LIGHTING_TOL
    assert np.array_equal(src.download(img.shape, np.float64), img, equal_nan=True)
    # Layer.lighting builds the device-frame light itself, from the light source (equal to `params` up to cos(90 degrees) = 6e-17)
    layer = Layer(img, offset, pre_alpha=False, linear_rgb=True).lighting(
        E._identity(), offset, A.shape, _light(case["kind"], case["light"]), case["color"], case["ss"], case["constant"], se)
    from_light = LR.lighting(A, offset, case["kind"], LR.light_frame(E._identity(), case["kind"], case["light"]), case["color"],
                             case["ss"], case["constant"], se)
    _unit(layer.image, name)
    assert np.abs(layer.image - from_light).max() <= LIGHTING_TOL


# ====================================================================================== refusals
def _refused(ctx, call):
    lib, _check, _ptr = _lib(ctx)
    before = ctx.launches()
    rc = call()
    assert rc == -1, rc                       # SVGR_E_INVALID
    assert ctx.launches() == before           # and nothing was launched
    assert lib.svgr_last_error()


def _abi_call(ctx, primitive, p, bufs):
    """The ABI call of one primitive with the parameters `p` (the form of E.refusal_base()); returns its status."""
    lib, _check, ptr = _lib(ctx)
    if primitive == "turbulence":
        return lib.svgr_layer_turbulence(ctx.handle, bufs["out"].handle, _bb(p["offset"] + p["shape"]), ptr(p["inv"]), p["freq"][0],
                                         p["freq"][1], ptr(p["tile"]), p["seed"], p["octaves"], p["fractal"], p["stitch"])
    if primitive == "transfer":
        return lib.svgr_layer_component_transfer(ctx.handle, bufs["out"].handle, p["n_px"], ptr(p["types"]),
                                                 ptr(np.ascontiguousarray(p["params"])), ptr(p["counts"]), ptr(p["values"]))
    if primitive == "convolve":
        return lib.svgr_layer_convolve_matrix(ctx.handle, bufs["out"].handle, bufs["src"].handle, p["shape"][0], p["shape"][1],
                                              ptr(np.ascontiguousarray(p["kernel"])), 3, 3, 1, 1, p["scalars"][0], p["scalars"][1], 0, 0)
    return lib.svgr_layer_lighting(ctx.handle, bufs["out"].handle, _bb(p["offset"] + p["shape"]), bufs["src"].handle,
                                   _bb(p["offset"] + p["shape"]), LR.SPOT, ptr(p["params"]), ptr(p["color"]), p["scalars"][0],
                                   p["scalars"][1], p["scalars"][2], 1)


@pytest.mark.parametrize("primitive", ["turbulence", "transfer", "convolve", "lighting"])
def test_refusals_launch_nothing(ctx, primitive):
    _lib_, check, _ptr = _lib(ctx)
    start = np.full((32, 4), 0.5)
    bufs = {"out": ctx.from_host(start), "src": ctx.from_host(start)}
    base = E.refusal_base()[primitive]
    check(_abi_call(ctx, primitive, base, bufs))      # the base is accepted: each refusal below is for the one number changed
    bufs["out"] = ctx.from_host(start)
    n = 0
    for prim, field, index, value in E.REFUSALS:
        if prim != primitive:
            continue
        p = dict(base)
        p[field] = np.array(base[field], dtype=np.float64)
        p[field].flat[index] = value
        _refused(ctx, lambda: _abi_call(ctx, primitive, p, bufs))
        n += 1
    assert n >= 33
    assert np.array_equal(bufs["out"].download(start.shape, np.float64), start)   # no refused call wrote anything


def test_layer_methods_raise_value_error(ctx):
    from svgrasterize_amd import Layer
    from svgrasterize_amd.filters import PointLight
    from svgrasterize_amd.geometry import Transform

    img = np.full((3, 4, 4), 0.5)
    layer = Layer(img, (0, 0), pre_alpha=False, linear_rgb=True)
    before = ctx.launches()
    for bad in E.NON_FINITE:
        calls = [
            lambda: Layer.turbulence(Transform(), (0, 0), (3, 4), (bad, 0.05), 2),
            lambda: Layer.turbulence(Transform(), (0, 0), (3, 4), (0.05, 0.05), 2, seed=bad),
            lambda: Layer.turbulence(Transform(), (0, 0), (3, 4), (0.05, 0.05), 2, stitch_tile=(0.0, bad, 10.0, 10.0)),
            lambda: Layer.turbulence(Transform().translate(bad if np.isnan(bad) else 0.0, bad), (0, 0), (3, 4), (0.05, 0.05), 2),
            lambda: layer.component_transfer([("linear", bad, 0.0), None, None, None]),
            lambda: layer.component_transfer([None, ("table", (0.0, bad, 1.0)), None, None]),
            lambda: layer.component_transfer([None, None, None, ("gamma", 1.0, bad, 0.0)]),
            lambda: layer.convolve_matrix(np.array([[1.0, bad], [0.0, 1.0]]), 2.0),
            lambda: layer.convolve_matrix(np.ones((3, 3)), bad),
            lambda: layer.convolve_matrix(np.ones((3, 3)), None, bad),
            lambda: layer.lighting(Transform(), (0, 0), (3, 4), PointLight(1.0, bad, 3.0), (1.0, 1.0, 1.0), 2.0, 1.0),
            lambda: layer.lighting(Transform(), (0, 0), (3, 4), PointLight(1.0, 2.0, 3.0), (1.0, bad, 1.0), 2.0, 1.0),
            lambda: layer.lighting(Transform(), (0, 0), (3, 4), PointLight(1.0, 2.0, 3.0), (1.0, 1.0, 1.0), bad, 1.0),
            lambda: layer.lighting(Transform(), (0, 0), (3, 4), PointLight(1.0, 2.0, 3.0), (1.0, 1.0, 1.0), 2.0, bad),
            lambda: layer.lighting(Transform(), (0, 0), (3, 4), PointLight(1.0, 2.0, 3.0), (1.0, 1.0, 1.0), 2.0, 1.0, bad),
        ]
        for k, call in enumerate(calls):
            with pytest.raises(ValueError):
                call()
                pytest.fail(f"call {k} with {bad} was accepted")
    for size in (0.0, -1.0):
        with pytest.raises(ValueError):
            Layer.turbulence(Transform(), (0, 0), (3, 4), (0.05, 0.05), 2, stitch_tile=(0.0, 0.0, size, 10.0))
        with pytest.raises(ValueError):
            Layer.turbulence(Transform(), (0, 0), (3, 4), (0.05, 0.05), 2, stitch_tile=(0.0, 0.0, 10.0, size))
    assert ctx.launches() == before


# ====================================================================================== documents
@pytest.mark.parametrize("name", [d[0] for d in E.DOCUMENTS])
def test_document_renders_without_nan(ctx, name):
    import svgrasterize_amd as S

    _, text, _attribute = next(d for d in E.DOCUMENTS if d[0] == name)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        scene, _ids, _size = S.svg_scene_from_str(text)
        assert scene is not None
        view = S.Transform().matrix(0, 1, 0, 1, 0, 0)
        out = scene.render(view, viewport=[0, 0, 16, 16], linear_rgb=True)
    assert out is not None
    image = out[0].image
    canvas = out[0].to_canvas_f32(16, 16)
    assert not np.isnan(image).any() and not np.isnan(canvas).any()
    assert canvas[..., 3].max() > 0.2   # (the flood that stays in the chain is what is drawn)
