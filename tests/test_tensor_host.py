"""Tensor output on the CPU: csrc/svgr_tensor.h, driven serially by tests/tensor_harness.cpp, against numpy's own conversions,
torch's bfloat16 and the restatement of tests/tensor_ref.py; the checks of the two ABI entries, which run before anything is
launched and so need no GPU; the keyword checks of the Python layer.  The device runs the same header (tests/test_gpu_tensor.py
holds its bytes against this harness), so what is pinned here is the device's too."""
import ctypes as C

import numpy as np
import pytest

import svgrasterize_amd as S
from svgrasterize_amd import _abi
from tests import tensor_ref as R


@pytest.fixture(scope="module")
def lib():
    return R.harness()


def _encode(lib, dtype, y):
    y = np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
    out = np.empty(y.size, dtype=np.uint32)
    lib.h_encode_many(dtype, y.ctypes.data, y.size, out.ctypes.data)
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# 1. element conversions
# ------------------------------------------------------------------------------------------------------------------------------
def _half_edge_values(dtype):
    """float64 values around everything the half conversions decide: ties, the top of the range, the subnormals, zeros."""
    if dtype == R.F16:
        bits = np.arange(0, 0x7C01, dtype=np.uint32)   # every non-negative float16 up to infinity
        h = bits.astype(np.uint16).view(np.float16).astype(np.float64)
        ulp_above = np.diff(h[:0x7C00])                 # (finite neighbours)
        mids = h[:0x7BFF] + ulp_above / 2               # exact ties between neighbours: round to even
        top = 65504.0
        special = [top, top + 16.0, np.nextafter(top + 16.0, 0), np.nextafter(top + 16.0, np.inf), 65536.0, 1e6,
                   2.0 ** -24, 2.0 ** -25, np.nextafter(2.0 ** -25, 1), np.nextafter(2.0 ** -25, 0), 2.0 ** -26, 2.0 ** -14,
                   np.nextafter(2.0 ** -14, 0), 1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24]
        v = np.concatenate([h[:0x7C00], mids, np.nextafter(mids, np.inf), np.nextafter(mids, -np.inf), special])
    else:
        rng = np.random.default_rng(8)
        hi = rng.integers(0, 0x7F80, 6000).astype(np.uint32)   # bfloat16 patterns below infinity, subnormals among them
        hi = np.concatenate([hi, np.arange(0, 260, dtype=np.uint32), [0x7F7F, 0x7F7E, 0x0080, 0x007F, 0x0001]])
        base = (hi << 16).view(np.float32).astype(np.float64)
        nxt = ((hi + 1) << 16).view(np.float32).astype(np.float64)
        with np.errstate(invalid="ignore"):
            mids = np.where(np.isfinite(nxt), base + (nxt - base) / 2, base + 2.0 ** 119)   # (7f7f's tie: the largest finite value plus half an ulp)
        v = np.concatenate([base, mids, np.nextafter(mids, np.inf), np.nextafter(mids, -np.inf),
                            [3.3895313892515355e38, 3.4028234663852886e38, 3.5e38, 1e39, 2.0 ** -133, 2.0 ** -134, 2.0 ** -135]])
    v = v[np.isfinite(v)]
    return np.concatenate([v, -v, [0.0, -0.0, np.inf, -np.inf]])


def test_f16_matches_numpys_astype_chain(lib):
    v = _half_edge_values(R.F16)
    with np.errstate(over="ignore"):
        want = v.astype(np.float32).astype(np.float16).view(np.uint16)
    got = _encode(lib, R.F16, v)
    assert np.array_equal(got, want), [(float(x), hex(g), hex(w)) for x, g, w in zip(v, got, want) if g != w][:5]
    # what the values were made for
    f32 = np.float32
    assert lib.h_encode(R.F16, 65504.0 + 16.0) == 0x7C00 and lib.h_encode(R.F16, float(np.nextafter(f32(65520.0), f32(0)))) == 0x7BFF
    assert lib.h_encode(R.F16, float(np.nextafter(65520.0, 0))) == 0x7C00, "two steps: the float32 is the tie, whatever the double was"
    assert lib.h_encode(R.F16, 2.0 ** -25) == 0 and lib.h_encode(R.F16, float(np.nextafter(f32(2.0 ** -25), f32(1)))) == 1
    assert lib.h_encode(R.F16, 1.5 * 2.0 ** -24) == 2 and lib.h_encode(R.F16, 2.5 * 2.0 ** -24) == 2   # ties to even
    assert lib.h_encode(R.F16, -0.0) == 0x8000 and lib.h_encode(R.F16, 0.0) == 0
    assert lib.h_encode(R.F16, float("inf")) == 0x7C00 and lib.h_encode(R.F16, float("-inf")) == 0xFC00
    # every float32 pattern of a stride through the whole range, against numpy
    bits = np.arange(0, 1 << 32, 65521, dtype=np.uint64).astype(np.uint32)
    f = bits.view(np.float32)
    keep = ~np.isnan(f)
    with np.errstate(over="ignore"):
        want = f[keep].astype(np.float16).view(np.uint16)
    assert [lib.h_f16_bits(int(b)) for b in bits[keep][::7]] == want[::7].tolist()


def test_bf16_matches_torch(lib):
    torch = pytest.importorskip("torch")
    v = _half_edge_values(R.BF16)
    with np.errstate(over="ignore"):
        f32 = v.astype(np.float32)
    want = torch.from_numpy(f32).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = _encode(lib, R.BF16, v)
    assert np.array_equal(got, want), [(float(x), hex(g), hex(w)) for x, g, w in zip(v, got, want) if g != w][:5]
    assert np.array_equal(R.bf16_bits_ref(f32), want)   # (the restatement the GPU tests use)
    assert lib.h_encode(R.BF16, 3.3895313892515355e38 + 2.0 ** 119) == 0x7F80, "the largest finite value plus half an ulp: a tie, to infinity"
    assert lib.h_encode(R.BF16, 3.3895313892515355e38) == 0x7F7F and lib.h_encode(R.BF16, -0.0) == 0x8000
    t16 = torch.from_numpy(f32).to(torch.float16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(_encode(lib, R.F16, v), t16), "tensor.float().half() is the same two steps"


def test_nan_leaves_as_the_quiet_nan_of_its_type(lib):
    nans = np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF, 0x7FF4000000000000], dtype=np.uint64).view(np.float64)
    for dtype in (R.F32, R.F16, R.BF16):
        assert (_encode(lib, dtype, nans) == R.QNAN[dtype]).all()
        assert np.isnan(R.decode_ref(dtype, _encode(lib, dtype, nans).astype(R.STORE[dtype]))).all()
    assert (_encode(lib, R.U8, nans) == 0).all()
    for b in (0x7FC00001, 0xFFC00000, 0x7F800001):
        assert lib.h_f16_bits(b) == 0x7E00 and lib.h_bf16_bits(b) == 0x7FC0


def test_f32_is_numpys_rounding(lib):
    rng = np.random.default_rng(2)
    v = np.concatenate([rng.normal(0, 1, 4000), rng.normal(0, 1e30, 200), [1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, 1e-46, 2.0 ** -150, 3.5e38, -3.5e38, 0.0, -0.0]])
    with np.errstate(over="ignore"):
        want = v.astype(np.float32).view(np.uint32)
    assert np.array_equal(_encode(lib, R.F32, v), want)


def test_u8(lib):
    k = np.arange(256, dtype=np.float64)
    assert np.array_equal(_encode(lib, R.U8, k / 255.0), k)
    ties = (k[:-1] + 0.5) / 255.0
    got = _encode(lib, R.U8, ties)
    assert np.array_equal(got, np.rint(ties * 255.0)), "whatever side of the tie the product falls, it is numpy's"
    exact = np.array([0.5, 1.5, 2.5, 3.5, 126.5, 127.5, 254.5]) / 255.0   # (the products that ARE ties go to the even byte)
    on_tie = (exact * 255.0) % 1 == 0.5
    assert on_tie.any() and (_encode(lib, R.U8, exact)[on_tie] % 2 == 0).all()
    odd = np.array([-1e-9, -0.3, -1e300, 1.0000001, 1.5, 256.0, 1e300, np.inf, -np.inf, np.nan, -0.0])
    assert _encode(lib, R.U8, odd).tolist() == [0, 0, 0, 255, 255, 255, 255, 255, 0, 0, 0]
    assert np.array_equal(_encode(lib, R.U8, odd), R.encode_ref(R.U8, odd))


def test_inverse_is_exact(lib):
    for b in range(256):
        assert lib.h_decode(R.U8, b) == b / 255.0
    bits = np.arange(0, 1 << 16, dtype=np.uint32)
    for dtype in (R.F16, R.BF16):
        got = np.array([lib.h_decode(dtype, int(b)) for b in bits])
        want = R.decode_ref(dtype, bits)
        assert np.array_equal(got.view(np.uint64)[~np.isnan(want)], want.view(np.uint64)[~np.isnan(want)])
        assert np.isnan(got[np.isnan(want)]).all()
        finite = np.isfinite(want)
        assert np.array_equal(_encode(lib, dtype, got[finite]), bits[finite]), "widened and rounded back: the same element"
    f = np.random.default_rng(4).normal(0, 100, 500).astype(np.float32)
    assert [lib.h_decode(R.F32, int(b)) for b in f.view(np.uint32)] == f.astype(np.float64).tolist()


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the pixel: background, channels, affine; where the elements go
# ------------------------------------------------------------------------------------------------------------------------------
BG = (0.25, 0.5, 0.125)
SCALE, BIAS = (1 / 0.229, 1 / 0.224, 1 / 0.225, 2.0), (-0.485 / 0.229, -0.456 / 0.224, -0.406 / 0.225, -1.0)


@pytest.mark.parametrize("dtype", list(R.DTYPES))
@pytest.mark.parametrize("channels", list(R.CHANNELS))
@pytest.mark.parametrize("variant", ["plain", "bg", "affine", "bg+affine"])
def test_pixels_against_the_restatement(lib, dtype, channels, variant):
    rng = np.random.default_rng(31)
    src = R.random_layer(rng, 5, 9)
    bg = BG if "bg" in variant else None
    scale, bias = (SCALE, BIAS) if "affine" in variant else (None, None)
    for layout in ("chw", "hwc"):
        d = R.desc(7, 11, R.DTYPES[dtype], R.CHANNELS[channels], layout, bg=bg, scale=scale, bias=bias)
        buf = np.full(R.n_elements(d) * 4, 0xA5, dtype=np.uint8)
        got = R.view_of(R.harness_pack(lib, d, src, (-1, 3, 5, 9), buf), d)
        want = R.pack_ref(src, (-1, 3, 5, 9), 7, 11, R.DTYPES[dtype], R.CHANNELS[channels], bg, scale, bias)
        assert np.array_equal(got, want)


def test_luma_is_the_luminance_kernels_sum(lib):
    rng = np.random.default_rng(12)
    src = rng.uniform(0, 1, (6, 6, 4))
    d = R.desc(6, 6, R.F32, R.LUMA)
    got = R.view_of(R.harness_pack(lib, d, src, (0, 0, 6, 6), np.zeros(6 * 6 * 4, dtype=np.uint8)), d)[..., 0].view(np.float32)
    fused = R.luma_ref(src[..., 0], src[..., 1], src[..., 2]).reshape(6, 6)
    plain = src[..., 0] * 0.2125 + src[..., 1] * 0.7154 + src[..., 2] * 0.072
    assert np.array_equal(got, fused.astype(np.float32))
    assert (fused != plain).any(), "the two fma round once each: not the plain sum"


def test_sources_and_placement(lib):
    rng = np.random.default_rng(5)
    for kind in (R.SRC_F64, R.SRC_F32, R.SRC_MASK):
        src = R.random_layer(rng, 4, 6, kind)
        for bbox in ((0, 0, 4, 6), (-2, 0, 4, 6), (0, -3, 4, 6), (3, 0, 4, 6), (0, 5, 4, 6), (-1, -1, 4, 6), (9, 9, 4, 6), (-4, 0, 4, 6)):
            d = R.desc(5, 8, R.F16, R.RGBA, "chw", source=kind)
            got = R.view_of(R.harness_pack(lib, d, src, bbox, np.zeros(R.n_elements(d) * 2, dtype=np.uint8)), d)
            assert np.array_equal(got, R.pack_ref(src, bbox, 5, 8, R.F16))
            if bbox[0] in (9, -4):
                assert not got.any(), "a box wholly outside the plane: all zeros"


def test_strided_destination_and_untouched_bytes(lib):
    rng = np.random.default_rng(6)
    src = R.random_layer(rng, 3, 5)
    for offset in range(4):
        d = R.desc(3, 5, R.F16, R.RGB, "chw", stride_h=11, stride_c=3 * 11 + 7, offset=offset)
        buf = rng.integers(0, 256, (R.n_elements(d) + 9) * 2, dtype=np.uint8)
        out = R.harness_pack(lib, d, src, (0, 0, 3, 5), buf)
        assert np.array_equal(R.view_of(out, d), R.pack_ref(src, (0, 0, 3, 5), 3, 5, R.F16, R.RGB))
        touched = np.zeros(buf.size // 2, dtype=bool)
        idx = d.offset + np.add.outer(np.add.outer(np.arange(3) * d.stride_h, np.arange(5) * d.stride_w), np.arange(3) * d.stride_c)
        touched[idx.reshape(-1)] = True
        assert np.array_equal(out.view(np.uint16)[~touched], buf.view(np.uint16)[~touched])


def test_u8_rgba_identity_is_the_rgba8_output(lib):
    # svgr_layer_to_rgba8 is documented for the straight sRGB values Layer.convert(pre_alpha=False) leaves, all in [0, 1]
    rng = np.random.default_rng(9)
    image = rng.uniform(0, 1, (8, 13, 4))
    image[rng.integers(0, 4, image.shape) == 0] = 0.0
    image[rng.integers(0, 4, image.shape) == 1] = 1.0
    image[0, :, 0] = (np.arange(13) + 0.5) / 255.0
    d = R.desc(8, 13, R.U8, R.RGBA, "hwc")
    got = R.view_of(R.harness_pack(lib, d, image, (0, 0, 8, 13), np.zeros(8 * 13 * 4, dtype=np.uint8)), d)
    assert np.array_equal(got, np.round(image * 255).astype(np.uint8))


def test_round_trip_through_the_inverse(lib):
    rng = np.random.default_rng(10)
    for dtype in R.DTYPES.values():
        for channels in R.CHANNELS.values():
            for layout in ("chw", "hwc"):
                n = R.N_CH[channels]
                bits = rng.integers(0, 1 << 16, (4, 7, n)).astype(R.STORE[dtype]) if dtype != R.F32 else rng.normal(0, 1, (4, 7, n)).astype(np.float32).view(np.uint32)
                d = R.desc(4, 7, dtype, channels, layout)
                buf = np.zeros(R.n_elements(d) * bits.itemsize, dtype=np.uint8)
                R.view_of(buf, d)[...] = bits
                back = R.harness_unpack(lib, d, buf)
                want = R.decode_ref(dtype, bits)
                if channels == R.RGB:
                    want = np.concatenate([want, np.ones((4, 7, 1))], axis=-1)
                assert back.shape == want.shape and np.array_equal(np.nan_to_num(back, nan=-7.0), np.nan_to_num(want, nan=-7.0))


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the ABI's checks (before anything is launched: no GPU needed)
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def abi():
    return _abi.load_library()


def _wrapped(abi, nbytes, keep):
    """A non-owning svgr_buf over host memory (never dereferenced: every call below fails its checks, or is empty).
    svgr_buf_wrap only files its context argument, so any non-NULL pointer does."""
    mem = np.zeros(max(nbytes, 64), dtype=np.uint8)
    h = _abi._P()
    assert abi.svgr_buf_wrap(_abi._P(mem.ctypes.data), _abi._P(mem.ctypes.data), nbytes, C.byref(h)) == 0
    keep.append(mem)
    return h


def _last_error(abi):
    return abi.svgr_last_error().decode()


INVALID = {
    "source": dict(source=3), "source-": dict(source=-1), "dtype": dict(dtype=4), "dtype-": dict(dtype=-1),
    "channels": dict(channels=4), "channels-": dict(channels=-1), "has_bg": dict(has_bg=2),
    "strides": dict(stride_w=2), "strides hwc": dict(stride_c=1, stride_w=3), "stride_c of hwc": dict(stride_c=2, stride_w=4),
    "negative stride_h": dict(stride_h=-8), "negative stride_c": dict(stride_c=-1), "negative stride_w": dict(stride_w=-1),
    "negative offset": dict(offset=-1), "negative rows": dict(rows=-1), "negative cols": dict(cols=-1),
    "stride_h below cols": dict(stride_h=7), "stride_h below cols * channels": dict(stride_c=1, stride_w=4, stride_h=31),
}


@pytest.mark.parametrize("entry", ["svgr_layer_to_tensor", "svgr_tensor_to_layer"])
def test_invalid_descriptions(abi, entry):
    keep = []
    big = _wrapped(abi, 1 << 20, keep)
    bbox = (C.c_int64 * 4)(0, 0, 4, 8)

    def call(d, tensor=big, layer=big, ctx=None):
        if entry == "svgr_layer_to_tensor":
            return abi.svgr_layer_to_tensor(ctx, C.byref(d), layer, bbox, tensor)
        return abi.svgr_tensor_to_layer(ctx, C.byref(d), tensor, layer)

    for name, fields in INVALID.items():
        d = R.desc(4, 8)
        for field, value in fields.items():
            setattr(d, field, value)
        assert call(d) == -1, name
        assert entry in _last_error(abi) and "ctx is NULL" not in _last_error(abi), (name, _last_error(abi))
    for field in ("scale", "bias", "bg"):
        for bad in (float("nan"), float("inf"), float("-inf")):
            d = R.desc(4, 8)
            getattr(d, field)[2] = bad
            assert call(d) == -1 and "finite" in _last_error(abi), (field, bad)
    # the largest element index against the tensor's bytes: exactly enough passes this check (and fails the next: no context)
    for layout, dtype, es in (("chw", R.F32, 4), ("hwc", R.F16, 2), ("chw", R.U8, 1)):
        d = R.desc(4, 8, dtype, R.RGBA, layout, stride_h=8 * (4 if layout == "hwc" else 1) + 3, offset=5)
        need = R.n_elements(d) * es
        assert call(d, tensor=_wrapped(abi, need - 1, keep)) == -1 and "reaches past" in _last_error(abi)
        assert call(d, tensor=_wrapped(abi, need, keep)) == -1 and "ctx is NULL" in _last_error(abi)
    d = R.desc(4, 8, R.F32, stride_c=1 << 40, stride_h=1 << 40)
    assert call(d) == -1 and "reaches past" in _last_error(abi), "no wrap-around in the index arithmetic"
    d = R.desc(4, 8, R.F16)
    odd = _abi._P()
    assert abi.svgr_buf_wrap(_abi._P(keep[0].ctypes.data), _abi._P(keep[0].ctypes.data + 1), 4096, C.byref(odd)) == 0
    assert call(d, tensor=odd) == -1 and "multiple of its element size" in _last_error(abi)
    small = _wrapped(abi, 4 * 8 * 32 - 1, keep)
    assert call(R.desc(4, 8), layer=small) == -1 and "too small" in _last_error(abi)
    assert call(R.desc(4, 8), tensor=None) == -1 and call(R.desc(4, 8), layer=None) == -1
    if entry == "svgr_layer_to_tensor":
        assert abi.svgr_layer_to_tensor(None, C.byref(R.desc(4, 8)), big, None, big) == -1
        assert abi.svgr_layer_to_tensor(None, None, big, bbox, big) == -1
    for h in (big, odd, small):
        abi.svgr_buf_free(None, h)


def test_empty_plane_succeeds_without_a_context(abi):
    bbox = (C.c_int64 * 4)(0, 0, 0, 0)
    for rows, cols in ((0, 8), (4, 0), (0, 0)):
        d = R.desc(rows, cols, stride_h=8)
        assert abi.svgr_layer_to_tensor(None, C.byref(d), None, bbox, None) == 0
        assert abi.svgr_tensor_to_layer(None, C.byref(d), None, None) == 0
    assert abi.svgr_layer_to_tensor(None, C.byref(R.desc(0, 8, dtype=9)), None, bbox, None) == -1, "an empty plane is still checked"


def test_block_and_run(abi):
    block, run = abi.svgr_tensor_block(), abi.svgr_tensor_run()
    assert run >= 4 and block % (64 * run) == 0 and abi.svgr_abi_version() == 6
    assert abi.svgr_stream_wait_for(None, None) == -1 and abi.svgr_stream_signal_to(None, None) == -1


# ------------------------------------------------------------------------------------------------------------------------------
# 4. the Python layer
# ------------------------------------------------------------------------------------------------------------------------------
def test_names_are_exported():
    assert all(name in S.__all__ for name in ("render_to_tensor", "render_svgs_to_tensor"))
    assert all(callable(getattr(S.Layer, name)) for name in ("to_array", "to_tensor", "from_tensor"))
    assert {"svgr_layer_to_tensor", "svgr_tensor_to_layer", "svgr_tensor_block", "svgr_tensor_run", "svgr_stream_wait_for",
            "svgr_stream_signal_to"} <= set(_abi.EXPORTS)
    assert C.sizeof(_abi.TensorDesc) == 16 + 8 * 11 + 8 * 6


def test_keywords_are_refused_before_any_device_work(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("device work before the arguments were checked")

    monkeypatch.setattr(_abi.Context, "get", classmethod(no_device))
    monkeypatch.setattr(S.Layer, "_device", no_device)
    layer = S.Layer(np.zeros((2, 3, 4)), (0, 0), True, False)
    bad = [dict(layout="nchw"), dict(channels="bgr"), dict(alpha="pre"), dict(bg=(1, 1, 1), alpha="straight"), dict(bg=(1, 1)),
           dict(bg=(1, float("nan"), 1)), dict(mean=(0.5, 0.5)), dict(std=(1, 1, 1)), dict(std=0.0), dict(mean=float("inf")),
           dict(std=(1, 1, 0, 1)), dict(channels="rgb", mean=(0, 0, 0, 0)), dict(size=(-1, 4))]
    for kw in bad:
        with pytest.raises(ValueError):
            layer.to_array(**kw)
        with pytest.raises(ValueError):
            layer.to_tensor(**kw)
    for dtype in (np.float64, np.int8, "bfloat16", "no such type"):
        with pytest.raises(ValueError, match="dtype"):
            layer.to_array(dtype=dtype)
    torch = pytest.importorskip("torch")
    for dtype in (torch.float64, np.float32, "float32"):
        with pytest.raises(TypeError, match="dtype"):
            layer.to_tensor(dtype=dtype)
    with pytest.raises(TypeError, match="torch.Tensor"):
        layer.to_tensor(out=np.zeros((4, 2, 3), dtype=np.float32))
    with pytest.raises(TypeError, match="float16"):
        layer.to_tensor(out=torch.zeros((4, 2, 3), dtype=torch.float32), dtype=torch.float16)
    with pytest.raises(ValueError, match="shape"):
        layer.to_tensor(out=torch.zeros((4, 3, 2)))
    with pytest.raises(ValueError, match="shape"):
        layer.to_tensor(out=torch.zeros((4, 2, 3)), layout="hwc")
    with pytest.raises(ValueError, match="device"):
        layer.to_tensor(out=torch.zeros((4, 2, 3)))   # (a CPU tensor)
    with pytest.raises(TypeError):
        S.Layer.from_tensor(torch.zeros((4, 2, 3), dtype=torch.float64))
    with pytest.raises(TypeError):
        S.Layer.from_tensor(np.zeros((4, 2, 3)))
    with pytest.raises(ValueError, match="device"):
        S.Layer.from_tensor(torch.zeros((4, 2, 3)))
    with pytest.raises(ValueError):
        S.Layer.from_tensor(np.zeros((5, 6, 7), dtype=np.float32))
    with pytest.raises(ValueError, match="channels"):
        S.Layer.from_tensor(np.zeros((3, 6, 7), dtype=np.float32), channels="rgba")
    with pytest.raises(ValueError):
        S.render_svgs_to_tensor(["<svg/>"], (8, 8), layout="nchw")


def test_mean_and_std_become_scale_and_bias():
    from svgrasterize_amd import tensor

    opt = tensor._options("chw", "rgb", "premultiplied", False, None, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    assert opt.scale == (1 / 0.229, 1 / 0.224, 1 / 0.225, 1.0) and opt.bias == (-0.485 / 0.229, -0.456 / 0.224, -0.406 / 0.225, 0.0)
    opt = tensor._options("hwc", "rgba", "premultiplied", True, (0.5, 0.25, 1.0), 0.5, None)
    assert opt.scale == (1.0,) * 4 and opt.bias == (-0.5,) * 4 and opt.bg == (0.5, 0.25, 1.0) and opt.linear_rgb
    fit = tensor.fit_transform((100, 50), (64, 64))   # xMidYMid meet: scaled by 0.64, centred vertically
    assert np.allclose(fit(np.array([0.0, 0.0])), (0.0, 16.0)) and np.allclose(fit(np.array([100.0, 50.0])), (64.0, 48.0))


def test_empty_size_needs_no_device():
    layer = S.Layer(np.zeros((2, 3, 4)), (0, 0), True, False)
    assert layer.to_array((0, 5)).shape == (4, 0, 5) and layer.to_array((3, 0), layout="hwc", channels="rgb", dtype=np.uint8).shape == (3, 0, 3)
