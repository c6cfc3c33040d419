"""Tensor output on the device: svgr_layer_to_tensor and svgr_tensor_to_layer against the host build of the same header
(tests/tensor_harness.cpp, itself held against numpy, torch and tests/tensor_ref.py by tests/test_tensor_host.py) bit for bit,
at the row lengths where the kernel's launch geometry changes -- a lane's run, a workgroup's block -- and at every element
alignment a row can begin at; the whole destination buffer is compared, so a byte written outside the addressed window shows.
No torch here: Layer.to_array and a raw svgr_layer_to_tensor into a buffer of the library's."""
import ctypes as C
import io

import numpy as np
import pytest

from tests import tensor_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import svgrasterize_amd as S

    S.Context.get()
    return S


@pytest.fixture(scope="module")
def lib():
    return R.harness()


@pytest.fixture(scope="module")
def geometry(S):
    abi = S.load_library()
    return abi.svgr_tensor_run(), abi.svgr_tensor_block()


def _device_pack(S, d, src, bbox, pattern):
    """The whole destination buffer (pre-filled with `pattern`) after svgr_layer_to_tensor."""
    from svgrasterize_amd import _abi

    ctx = S.Context.get()
    sbuf = ctx.from_host(np.ascontiguousarray(src))
    dbuf = ctx.from_host(pattern)
    _abi._check(ctx.lib.svgr_layer_to_tensor(ctx.handle, C.byref(d), sbuf.handle, (C.c_int64 * 4)(*bbox), dbuf.handle))
    return dbuf.download(pattern.shape, np.uint8)


def _check_pack(S, lib, d, src, bbox, rng, slack=37):
    es = np.dtype(R.STORE[d.dtype]).itemsize
    pattern = rng.integers(0, 256, (R.n_elements(d) + slack) * es, dtype=np.uint8)
    got = _device_pack(S, d, src, bbox, pattern)
    want = R.harness_pack(lib, d, src, bbox, pattern)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{bad.size} bytes differ, the first at {bad[0]} of {got.size} (element {bad[0] // es}): "
                             f"dtype {d.dtype} channels {d.channels} strides ({d.stride_c}, {d.stride_h}, {d.stride_w}) offset {d.offset} "
                             f"{d.rows} x {d.cols}")


VARIANTS = {"plain": {}, "bg": dict(bg=(0.25, 0.5, 0.125)), "affine": dict(scale=(1 / 0.229, 1 / 0.224, 1 / 0.225, 2.0), bias=(-2.1, -2.0, -1.8, -1.0))}
VARIANTS["bg+affine"] = {**VARIANTS["bg"], **VARIANTS["affine"]}


def _cols(geometry):
    run, block = geometry
    return [1, run - 1, run, run + 1, block - 1, block, block + 1, 2 * block + 3]


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("which", range(8))
def test_row_lengths_at_the_launch_seams(S, lib, geometry, which, rows):
    cols = _cols(geometry)[which]
    rng = np.random.default_rng(100 * which + rows)
    src = R.random_layer(rng, rows, cols)
    k = 0
    for dtype in R.DTYPES.values():
        for layout in ("chw", "hwc"):
            # (every dtype and layout at every length; the channel selections and variants take turns -- their full cross is below)
            channels = list(R.CHANNELS.values())[k % 4]
            variant = list(VARIANTS.values())[(k // 2 + which) % 4]
            k += 1
            n = R.N_CH[channels]
            stride_h = cols * (n if layout == "hwc" else 1) + 5   # (rows begin at every element alignment)
            d = R.desc(rows, cols, dtype, channels, layout, stride_h=stride_h, offset=which % 4, **variant)
            _check_pack(S, lib, d, src, (0, 0, rows, cols), rng)


@pytest.mark.parametrize("dtype", list(R.DTYPES))
@pytest.mark.parametrize("layout", ["chw", "hwc"])
def test_every_channel_selection_and_variant(S, lib, geometry, dtype, layout):
    run, block = geometry
    rows, cols = 3, block + run + 1
    rng = np.random.default_rng(7)
    src = R.random_layer(rng, rows, cols)
    for channels in R.CHANNELS.values():
        for variant in VARIANTS.values():
            d = R.desc(rows, cols, R.DTYPES[dtype], channels, layout, **variant)
            _check_pack(S, lib, d, src, (0, 0, rows, cols), rng)


@pytest.mark.parametrize("kind", [R.SRC_F64, R.SRC_F32, R.SRC_MASK], ids=["rgba64", "rgba32", "mask"])
def test_source_kinds_and_placement(S, lib, geometry, kind):
    run, block = geometry
    rng = np.random.default_rng(20 + kind)
    h, w = 5, block + 9
    src = R.random_layer(rng, h, w, kind)
    rows, cols = 6, block + 2 * run
    # the layer's box hanging over each edge of the plane, inside it, over a corner, and wholly outside (above, left, below, right)
    boxes = [(-2, 3, h, w), (3, 3, h, w), (1, -7, h, w), (1, 40, h, w), (0, 0, h, w), (-3, -(w - 4), h, w),
             (-h, 0, h, w), (0, -w, h, w), (rows, 0, h, w), (0, cols, h, w), (1000, -1000, h, w)]
    for i, bbox in enumerate(boxes):
        dtype = list(R.DTYPES.values())[i % 4]
        for layout, channels in (("chw", R.RGBA), ("hwc", R.RGB)):
            d = R.desc(rows, cols, dtype, channels, layout, source=kind, **(VARIANTS["bg"] if i % 3 == 2 else {}))
            _check_pack(S, lib, d, src, bbox, rng)
    outside = R.desc(rows, cols, R.F16, R.RGBA, "chw", source=kind)
    got = _device_pack(S, outside, src, (0, cols, h, w), np.full(R.n_elements(outside) * 2, 0xEE, dtype=np.uint8))
    assert not got.any(), "a box wholly outside the plane: all zeros"


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_element_offsets_and_odd_row_strides(S, lib, geometry, offset):
    run, block = geometry
    rng = np.random.default_rng(40 + offset)
    rows, cols = 4, block + 3 * run + 2
    src = R.random_layer(rng, rows, cols)
    for dtype in R.DTYPES.values():
        for extra in (1, run + 3, 2 * run - 1):   # stride_h is no multiple of the run, nor of 16 bytes: every row's head is different
            d = R.desc(rows, cols, dtype, R.RGBA, "chw", stride_h=cols + extra, stride_c=rows * (cols + extra) + 3, offset=offset)
            _check_pack(S, lib, d, src, (0, 0, rows, cols), rng)
            d = R.desc(rows, cols, dtype, R.RGB, "hwc", stride_h=3 * cols + extra, offset=offset)
            _check_pack(S, lib, d, src, (0, 0, rows, cols), rng)
    # a window of a larger picture, planes far apart, and a slice of a batch (the offset of slice 2)
    big_cols = cols + 40
    d = R.desc(rows, cols, R.F16, R.RGB, "chw", stride_h=big_cols, stride_c=(rows + 6) * big_cols, offset=big_cols + 3 + offset)
    _check_pack(S, lib, d, src, (0, 0, rows, cols), rng, slack=5 * big_cols)
    d = R.desc(rows, cols, R.U8, R.RGBA, "chw", offset=2 * 4 * rows * cols)
    _check_pack(S, lib, d, src, (0, 0, rows, cols), rng, slack=4 * rows * cols)


def test_many_rows_loop_over_the_grid(S, lib):
    # more rows than the launch has workgroup rows (65535): the kernel's row loop takes a second turn
    rng = np.random.default_rng(3)
    rows, cols = 65535 + 70, 3
    src = R.random_layer(rng, rows, cols)
    d = R.desc(rows, cols, R.F16, R.RGBA, "chw", stride_h=5)
    _check_pack(S, lib, d, src, (0, 0, rows, cols), rng)


def test_short_destination_is_refused_on_the_device_too(S):
    from svgrasterize_amd import _abi

    ctx = S.Context.get()
    src = ctx.alloc(4 * 8 * 32)
    d = R.desc(4, 8, R.F16)
    dst = ctx.alloc(R.n_elements(d) * 2 - 1)
    with pytest.raises(ValueError, match="reaches past"):
        _abi._check(ctx.lib.svgr_layer_to_tensor(ctx.handle, C.byref(d), src.handle, (C.c_int64 * 4)(0, 0, 4, 8), dst.handle))
    ctx.sync()


# ------------------------------------------------------------------------------------------------------------------------------
# the inverse
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(R.DTYPES))
def test_unpack_round_trips(S, lib, dtype):
    from svgrasterize_amd import _abi

    ctx = S.Context.get()
    rng = np.random.default_rng(50)
    code = R.DTYPES[dtype]
    rows, cols = 5, 300
    for channels in R.CHANNELS.values():
        for layout in ("chw", "hwc"):
            n = R.N_CH[channels]
            d = R.desc(rows, cols, code, channels, layout, stride_h=cols * (n if layout == "hwc" else 1) + 3, offset=2)
            store = np.dtype(R.STORE[code])
            buf = rng.integers(0, 256, (R.n_elements(d) + 8) * store.itemsize, dtype=np.uint8)
            out_ch = 4 if channels in (R.RGBA, R.RGB) else 1
            dst = ctx.alloc(rows * cols * out_ch * 8)
            tbuf = ctx.from_host(buf)
            _abi._check(ctx.lib.svgr_tensor_to_layer(ctx.handle, C.byref(d), tbuf.handle, dst.handle))
            got = dst.download((rows, cols, out_ch), np.float64)
            want = R.harness_unpack(lib, d, buf)
            assert np.array_equal(got.view(np.uint64)[~np.isnan(want)], want.view(np.uint64)[~np.isnan(want)])
            assert np.isnan(got[np.isnan(want)]).all()
            # packed again (no background, identity affine), the finite elements are the ones that came in
            elems = R.view_of(buf, d)
            layer = S.Layer._from_device(dst, (rows, cols, out_ch), (0, 0), True, False)
            if channels != R.LUMA:
                name = {R.RGBA: "rgba", R.RGB: "rgb", R.ALPHA: "alpha"}[channels]
                if code == R.BF16:
                    continue   # (numpy has no such type: the torch test packs it)
                again = layer.to_array(dtype={R.F32: np.float32, R.F16: np.float16, R.U8: np.uint8}[code], layout="hwc", channels=name)
                finite = ~np.isnan(R.decode_ref(code, elems))
                assert np.array_equal(again.view(store)[finite], elems[finite])


def test_png_of_a_round_trip_is_the_same_file(S):
    rng = np.random.default_rng(60)
    image = rng.uniform(0, 1, (37, 53, 4))
    image[..., :3] *= image[..., 3:]
    layer = S.Layer(image, (0, 0), True, False)
    packed = layer.to_array(dtype=np.uint8, layout="hwc", alpha="straight")
    assert np.array_equal(packed, layer.to_rgba8())
    back = S.Layer.from_tensor(packed, pre_alpha=False, linear_rgb=False)
    assert back.on_device and not back.pre_alpha
    assert back.write_png().getvalue() == layer.write_png().getvalue()


# ------------------------------------------------------------------------------------------------------------------------------
# a document
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def document(S):
    from tests.svg_cases import CASES

    text = dict((name, doc) for name, doc, _ in CASES)["basic_shapes"]
    scene, _ids, _size = S.svg_scene(io.StringIO(text))
    view = S.Transform().matrix(0, 1, 0, 1, 0, 0) @ S.Transform().scale(64 / 200)
    layer, _hull = scene.render(view, viewport=[0, 0, 64, 64], linear_rgb=False)
    return layer


def test_document_to_array(S, document):
    layer = document
    on_canvas = layer.convert(pre_alpha=True, linear_rgb=False).on_canvas(64, 64)
    assert np.array_equal(on_canvas.to_array(dtype=np.uint8, layout="hwc", alpha="straight"), on_canvas.to_rgba8())
    chw = layer.to_array((64, 64), dtype=np.float32, layout="chw", linear_rgb=layer.linear_rgb)
    want = layer.to_canvas_f32(64, 64, clip01=False)
    assert chw.shape == (4, 64, 64) and np.array_equal(chw.view(np.uint32), np.ascontiguousarray(want.transpose(2, 0, 1)).view(np.uint32))
    assert chw[3].max() > 0.9 and (chw[3] == 0).any()
    # the same picture as half the bytes, over white, normalised: against the restatement on the float64 pixels
    image = layer.convert(pre_alpha=True, linear_rgb=False).image
    got = layer.to_array((64, 64), dtype=np.float16, channels="rgb", bg=(1, 1, 1), mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
    scale, bias = 1.0 / np.array([0.229, 0.224, 0.225]), -np.array([0.485, 0.456, 0.406]) / np.array([0.229, 0.224, 0.225])
    ref = R.pack_ref(image, (*layer.offset, *image.shape[:2]), 64, 64, R.F16, R.RGB, (1.0, 1.0, 1.0), scale, bias)
    assert np.array_equal(got.view(np.uint16), ref.transpose(2, 0, 1))
    own = layer.to_array(dtype=np.float32, channels="alpha")
    assert own.shape == (1, layer.height, layer.width)
    assert np.array_equal(own[0], image[..., 3].astype(np.float32))
    luma = layer.to_array(dtype=np.float32, channels="luma", layout="hwc")
    assert np.array_equal(luma[..., 0], R.luma_ref(image[..., 0], image[..., 1], image[..., 2]).reshape(image.shape[:2]).astype(np.float32))
    mask = S.Layer(image[..., 3:].copy(), layer.offset, True, False)   # a 1-channel layer: broadcast like Layer.compose does
    m = mask.to_array((64, 64), dtype=np.uint8, layout="hwc")
    assert m.shape == (64, 64, 4) and (m[..., 0] == m[..., 3]).all() and np.array_equal(m[..., 3], np.round(R.plane_ref(image[..., 3:], (*layer.offset, *image.shape[:2]), 64, 64)[..., 3] * 255))
    with pytest.raises(ValueError, match="bfloat16"):
        layer.to_array(dtype="bfloat16")


# ------------------------------------------------------------------------------------------------------------------------------
# stream ordering
# ------------------------------------------------------------------------------------------------------------------------------
def _runtime(S):
    """The HIP runtime the library itself is bound to: a symbol looked up through the library's handle is searched in its
    dependencies, whichever copies of the runtime the process has loaded besides (torch brings one of its own)."""
    hip = S.load_library()
    hip.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    return hip


def test_ordering_against_a_second_stream(S, lib):
    from svgrasterize_amd import _abi

    hip = _runtime(S)
    ctx = S.Context.get()
    rng = np.random.default_rng(70)
    rows, cols = 16, 1000
    src = R.random_layer(rng, rows, cols)
    d = R.desc(rows, cols, R.F16, R.RGBA, "chw", offset=64)
    nbytes = 256 << 20   # (the fill takes a while: a pack that did not wait for it would be overwritten)
    dst, sbuf = ctx.alloc(nbytes), ctx.from_host(src)
    window = (R.n_elements(d) + 64) * 2
    ctx.sync()
    other = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(other), 1) == 0   # hipStreamNonBlocking
    try:
        got = np.empty(window, dtype=np.uint8)
        assert hip.hipMemsetAsync(dst.ptr, 0x5A, nbytes, other) == 0                     # a fill on the other stream
        _abi._check(ctx.lib.svgr_stream_wait_for(ctx.handle, other))
        _abi._check(ctx.lib.svgr_layer_to_tensor(ctx.handle, C.byref(d), sbuf.handle, (C.c_int64 * 4)(0, 0, rows, cols), dst.handle))
        _abi._check(ctx.lib.svgr_stream_signal_to(ctx.handle, other))
        assert hip.hipMemcpyAsync(got.ctypes.data, dst.ptr, window, 2, other) == 0       # a read on the other stream (device to host)
        assert hip.hipStreamSynchronize(other) == 0
        want = R.harness_pack(lib, d, src, (0, 0, rows, cols), np.full(window, 0x5A, dtype=np.uint8))
        assert np.array_equal(got, want), "fill, then pack, then read"
        # once more: the context's two events are used again
        _abi._check(ctx.lib.svgr_stream_wait_for(ctx.handle, other))
        _abi._check(ctx.lib.svgr_stream_signal_to(ctx.handle, other))
        ctx.sync()
    finally:
        hip.hipStreamSynchronize(other)
        hip.hipStreamDestroy(other)
