"""The colour quantiser on the device: svgr_quant_distinct, svgr_quant_bins and svgr_quant_index against the host build of the
same header (tests/quant_harness.cpp, itself held against numpy by tests/test_quant_host.py) and against tests/quant_ref.py, bit
for bit, at the smallest shapes where each kernel can go wrong; then the public route end to end through read_png."""
import re
import struct

import numpy as np
import pytest

from tests import quant_ref as R

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
def block(S, lib):
    from svgrasterize_amd import _abi

    assert _abi.quant_block() == 256 * lib.h_run()
    return _abi.quant_block()


def _colors(n, seed=0):
    rng = np.random.default_rng(seed)
    vals = rng.choice(1 << 24, size=n, replace=False).astype(np.uint32)
    alpha = np.where(np.arange(n) % 3 == 0, 255, 1 + (np.arange(n) * 37) % 254).astype(np.uint32)
    c = R.rgba(vals | alpha << 24).copy()
    c[0] = 0
    return c


def _image(rows, cols, n_colors, seed=1):
    """rows x cols pixels with exactly n_colors distinct canonical colours, every one used; transparent pixels carry stray colour."""
    c = _colors(n_colors, seed)
    rng = np.random.default_rng(seed + 100)
    pick = rng.integers(0, n_colors, rows * cols)
    pick[:min(n_colors, rows * cols)] = np.arange(min(n_colors, rows * cols))
    img = c[rng.permutation(pick)].reshape(rows, cols, 4).copy()
    img[img[..., 3] == 0, :3] = (9, 8, 7)
    return img


def _noise(rows, cols, seed):
    img = np.random.default_rng(seed).integers(0, 256, (rows, cols, 4), dtype=np.uint8)
    img[::3, ::2, 3] = 0
    return img


def _cases(block):
    yield "1x1", _image(1, 1, 1)
    yield "1x1 translucent", np.array([[[200, 100, 50, 77]]], dtype=np.uint8)
    clear = np.random.default_rng(2).integers(0, 256, (4, 5, 4), dtype=np.uint8)
    clear[..., 3] = 0
    yield "all transparent", clear
    yield "3x5 two colours", _image(3, 5, 2)
    yield "9x17 16 colours", _image(9, 17, 16)
    yield "9x17 17 colours", _image(9, 17, 17)
    yield "16x17 256 colours", _image(16, 17, 256)
    yield "16x17 257 colours", _image(16, 17, 257)
    yield "a block and a pixel, one row", _image(1, block + 1, 5)
    yield "a block and two pixels, two rows", _image(2, block // 2 + 1, 40)
    yield "noise across a block", _noise(3, block // 2 + 3, 7)


def test_stages_are_the_host_build(S, lib, block):
    from svgrasterize_amd import _abi, quant

    ctx = S.Context.get()
    for name, img in _cases(block):
        rows, cols = img.shape[:2]
        buf = ctx.from_host(img)
        n_distinct = len(np.unique(R.u32(R.canon(img))))
        for max_colors in sorted({1, 2, 256, min(max(n_distinct, 1), 256), min(max(n_distinct - 1, 1), 256)}):
            got, want = _abi.quant_distinct(ctx, buf, rows, cols, max_colors), R.harness_distinct(lib, img, max_colors)
            assert (got is None) == (want is None) == (n_distinct > max_colors), (name, max_colors)
            if want is not None:
                assert np.array_equal(got, want) and np.array_equal(got, R.distinct_ref(img, max_colors)), (name, max_colors)
        keys, bins = _abi.quant_bins(ctx, buf, rows, cols)
        hkeys, hbins = R.harness_bins(lib, img)
        assert np.array_equal(keys, hkeys) and np.array_equal(bins, hbins), name
        assert (np.diff(keys.astype(np.int64)) > 0).all() and int(bins[:, 0].sum()) == rows * cols, name
        idx, pal = S.quantize(img)
        assert np.array_equal(pal, R.palette_ref(img, 256)), name
        stream, plain = _abi.quant_index(ctx, buf, rows, cols, pal, stream=True, indices=True)
        hstream, hidx = R.harness_index(lib, img, pal)
        assert np.array_equal(plain.download((rows, cols), np.uint8), hidx) and np.array_equal(idx, hidx), name
        assert np.array_equal(stream.download(hstream.shape, np.uint8), hstream), name
        assert np.array_equal(hidx, R.indices_ref(img, pal)) and np.array_equal(hstream, R.pack_rows(hidx, quant.depth_of(len(pal)))), name
        if n_distinct <= 256:
            assert np.array_equal(pal[idx], R.canon(img)), name
        else:
            assert len(pal) <= 256 and not np.array_equal(pal[idx], R.canon(img)), name
        idx2, pal2 = S.quantize(img)
        assert np.array_equal(idx, idx2) and np.array_equal(pal, pal2), name


@pytest.mark.parametrize("n_pal", [1, 2, 3, 4, 5, 16, 17, 255, 256])
def test_index_at_every_depth_and_ragged_width(S, lib, block, n_pal):
    from svgrasterize_amd import _abi

    ctx = S.Context.get()
    pal = _colors(n_pal, seed=n_pal)
    for rows, cols in ((3, 5), (2, 9), (2, 17), (1, block + 1), (2, block + 7)):
        img = _noise(rows, cols, n_pal + cols)
        img[0, :min(cols, n_pal)] = pal[:min(cols, n_pal)]
        stream, plain = _abi.quant_index(ctx, ctx.from_host(img), rows, cols, pal, stream=True, indices=True)
        hstream, hidx = R.harness_index(lib, img, pal)
        assert np.array_equal(plain.download((rows, cols), np.uint8), hidx), (rows, cols)
        assert np.array_equal(stream.download(hstream.shape, np.uint8), hstream), (rows, cols)
    only_stream, none = _abi.quant_index(ctx, ctx.from_host(img), rows, cols, pal, stream=True, indices=False)
    assert none is None and np.array_equal(only_stream.download(hstream.shape, np.uint8), hstream)


def test_index_with_more_rows_than_the_grid_has(S, lib):
    # 2^16 rows, the most an image may have: the launch has 65535 workgroups along the rows, so one of them strides on to a second
    from svgrasterize_amd import _abi

    ctx = S.Context.get()
    rows, cols = 1 << 16, 3
    pal = _colors(5, seed=21)
    img = pal[np.random.default_rng(22).integers(0, 5, (rows, cols))]
    stream, plain = _abi.quant_index(ctx, ctx.from_host(img), rows, cols, pal, stream=True, indices=True)
    hstream, hidx = R.harness_index(lib, img, pal)
    assert np.array_equal(plain.download((rows, cols), np.uint8), hidx) and np.array_equal(pal[hidx], img)
    assert np.array_equal(stream.download(hstream.shape, np.uint8), hstream)


def test_ties_go_to_the_lowest_index(S, lib):
    from svgrasterize_amd import _abi

    ctx = S.Context.get()
    img = np.array([[[20, 0, 0, 255], [20, 0, 0, 255], [10, 0, 0, 255], [30, 0, 0, 255], [0, 0, 0, 0]]], dtype=np.uint8)
    for pal in ([(10, 0, 0, 255), (30, 0, 0, 255)], [(30, 0, 0, 255), (10, 0, 0, 255)], [(10, 0, 0, 255), (30, 0, 0, 255), (10, 0, 0, 255)]):
        pal = np.array(pal, dtype=np.uint8)
        assert R.dist(pal[0], img[0, 0]) == R.dist(pal[1], img[0, 0])
        _, plain = _abi.quant_index(ctx, ctx.from_host(img), 1, 5, pal, stream=False, indices=True)
        got = plain.download((1, 5), np.uint8)
        assert got[0, 0] == got[0, 1] == 0
        assert np.array_equal(got, R.harness_index(lib, img, pal)[1]) and np.array_equal(got, R.indices_ref(img, pal))


def test_colours_that_share_a_slot_or_a_bin(S, lib):
    from svgrasterize_amd import _abi

    ctx = S.Context.get()
    slots = lib.h_slots()
    by_slot = {}
    for v in range(1, 60000):
        px = 0xFF000000 | v
        by_slot.setdefault(lib.h_slot(px), []).append(px)
    crowded = max(by_slot, key=lambda s: len(by_slot[s]))
    assert len(by_slot[crowded]) >= 8
    # eight colours that begin their probe at one slot, four more at the slot behind it (which the eight have taken), and six at
    # the last slot, whose probes wrap around to the first
    chosen = by_slot[crowded][:8] + by_slot[(crowded + 1) % slots][:4] + by_slot[slots - 1][:6]
    assert len(set(chosen)) == 18 and len(by_slot[slots - 1]) >= 6
    img = R.rgba(np.array(chosen * 3, dtype=np.uint32)).reshape(3, 18, 4)
    got = _abi.quant_distinct(ctx, ctx.from_host(img), 3, 18, 18)
    assert np.array_equal(got, np.sort(np.array(chosen, dtype=np.uint32))) and np.array_equal(got, R.harness_distinct(lib, img, 18))
    assert _abi.quant_distinct(ctx, ctx.from_host(img), 3, 18, 17) is None
    # 64 colours of one bin (they differ in the low three bits of r and b) next to a neighbour bin
    one_bin = np.array([[8 + (i & 7), 40, 16 + (i >> 3), 200] for i in range(64)] + [[16, 40, 16, 200]], dtype=np.uint8).reshape(1, 65, 4)
    keys, bins = _abi.quant_bins(ctx, ctx.from_host(one_bin), 1, 65)
    hkeys, hbins = R.harness_bins(lib, one_bin)
    assert len(keys) == 2 and bins[0, 0] == 64 and np.array_equal(keys, hkeys) and np.array_equal(bins, hbins)
    assert np.array_equal(bins, R.bins_ref(one_bin)[1])


def test_flat_runs_and_waves_of_one_bin(S, lib, block):
    # whole waves of one colour (the bins kernel's wave-wide sum), a colour change inside a lane's run, and a ragged tail
    from svgrasterize_amd import _abi

    ctx = S.Context.get()
    cols = block + 64 * lib.h_run() + 3
    img = np.zeros((2, cols, 4), dtype=np.uint8)
    img[...] = (255, 255, 255, 255)
    img[0, 5:block // 2 + 3] = (10, 200, 30, 128)
    img[1, 100:103] = (1, 2, 3, 0)
    img[1, -2:] = (77, 66, 55, 44)
    buf = ctx.from_host(img)
    keys, bins = _abi.quant_bins(ctx, buf, 2, cols)
    hkeys, hbins = R.harness_bins(lib, img)
    assert np.array_equal(keys, hkeys) and np.array_equal(bins, hbins) and int(bins[:, 0].sum()) == 2 * cols
    assert np.array_equal(_abi.quant_distinct(ctx, buf, 2, cols, 4), R.harness_distinct(lib, img, 4))
    idx, pal = S.quantize(img, 4)
    assert len(pal) == 4 and np.array_equal(pal[idx], R.canon(img))


def test_bins_when_a_workgroup_takes_several_blocks(S, lib, block):
    # one block (and a pixel) more than the histogram kernel has workgroups: the first of them strides on to a second block, and
    # its table in LDS holds sums of both; flat bands with a sprinkling of noise, so that table and memory both take part
    from svgrasterize_amd import _abi

    ctx = S.Context.get()
    cols = 4099
    rows = ((_abi.quant_groups() + 1) * block + 1 + cols - 1) // cols
    y, x = np.mgrid[0:rows, 0:cols]
    img = _colors(6, seed=9)[(y // 7 + x // 301) % 6]
    rng = np.random.default_rng(12)
    spots = rng.integers(0, rows * cols, 3000)
    img.reshape(-1, 4)[spots] = rng.integers(0, 256, (3000, 4), dtype=np.uint8)
    keys, bins = _abi.quant_bins(ctx, ctx.from_host(img), rows, cols)
    hkeys, hbins = R.harness_bins(lib, img)
    assert len(keys) > 256 and np.array_equal(keys, hkeys) and np.array_equal(bins, hbins) and int(bins[:, 0].sum()) == rows * cols


def test_refused_before_any_launch(S):
    from svgrasterize_amd import _abi

    ctx = S.Context.get()
    buf = ctx.from_host(np.zeros((2, 2, 4), dtype=np.uint8))
    pal = np.zeros((2, 4), dtype=np.uint8)
    with pytest.raises(ValueError, match="buffer too small"):
        _abi.quant_bins(ctx, buf, 3, 2)
    with pytest.raises(ValueError, match="2\\^16"):
        _abi.quant_distinct(ctx, buf, 1, (1 << 16) + 1, 4)
    with pytest.raises(ValueError, match="max_colors"):
        _abi.quant_distinct(ctx, buf, 2, 2, 257)
    with pytest.raises(ValueError, match="buffer too small"):
        _abi.quant_index(ctx, buf, 2, 3, pal)
    with pytest.raises(ValueError, match="entries"):
        _abi.quant_index(ctx, buf, 2, 2, np.zeros((257, 4), dtype=np.uint8))
    with pytest.raises(ValueError):
        _abi.quant_index(ctx, buf, 2, 2, pal, stream=False, indices=False)


# ---------------------------------------------------------------------------------------------------------------------
# the public route
# ---------------------------------------------------------------------------------------------------------------------
def _layer(S, body, w=64, h=48):
    from svgrasterize_amd.geometry import Transform

    scene, _, _ = S.svg_scene_from_str(f'<svg xmlns="http://www.w3.org/2000/svg" width="{w}" height="{h}">{body}</svg>')
    return scene.render(Transform().matrix(0, 1, 0, 1, 0, 0), viewport=[0, 0, h, w])[0].on_canvas(h, w)


FLAT = ('<rect x="4" y="3" width="50" height="40" fill="#e02010"/><rect x="10" y="8" width="30" height="20" fill="#1040f0" fill-opacity="0.5"/>'
        '<rect x="20.5" y="30.25" width="20" height="10" fill="#20c040"/>')
SHADED = ('<defs><linearGradient id="g" x1="0" y1="0" x2="1" y2="1"><stop offset="0" stop-color="#e02010"/>'
          '<stop offset="1" stop-color="#1040f0"/></linearGradient></defs>'
          '<rect x="4" y="3" width="50" height="40" fill="url(#g)"/><circle cx="40" cy="26" r="17" fill="#20c040" fill-opacity="0.5"/>')


@pytest.mark.parametrize("which", ["flat", "shaded"])
def test_layer_write_png_palette(S, which):
    layer = _layer(S, FLAT if which == "flat" else SHADED)
    rgba = layer.to_rgba8()
    n_distinct = len(np.unique(R.u32(R.canon(rgba))))
    assert (n_distinct <= 256) == (which == "flat") and n_distinct > 2
    idx, pal = S.quantize(layer)
    idx_a, pal_a = S.quantize(rgba)
    assert np.array_equal(idx, idx_a) and np.array_equal(pal, pal_a)
    assert np.array_equal(pal, R.palette_ref(rgba, 256)) and np.array_equal(idx, R.indices_ref(rgba, pal))
    from svgrasterize_amd import quant

    want = R.canon(rgba) if which == "flat" else pal[idx]
    depth = quant.depth_of(len(pal))
    assert depth == (8 if which == "shaded" else R.depth_of(n_distinct))
    sizes = {}
    for encoder, kw in (("host", {}), ("host", dict(level=1, threads=2)), ("device", {}), ("device", dict(filter="none", huffman="fixed"))):
        data = layer.write_png(encoder=encoder, palette=True, **kw).getvalue()
        assert np.array_equal(S.read_png(data), want), (encoder, kw)
        assert struct.unpack(">IIBB", data[16:26]) == (64, 48, depth, 3)
        assert re.findall(rb"IHDR|PLTE|tRNS|IDAT|IEND", data) == [b"IHDR", b"PLTE", b"tRNS", b"IDAT", b"IEND"]
        assert data == S.canvas_to_png(rgba, encoder=encoder, palette=256, **kw).getvalue()
        sizes[encoder, tuple(kw)] = len(data)
    few = layer.write_png(palette=7).getvalue()
    idx7, pal7 = S.quantize(layer, 7)
    assert len(pal7) <= 7 and struct.unpack(">IIBB", few[16:26])[2] == quant.depth_of(len(pal7)) and np.array_equal(S.read_png(few), pal7[idx7])
    assert layer.write_png(palette=None).getvalue() == layer.write_png().getvalue() == layer.write_png(palette=False).getvalue()
    print(which, n_distinct, "colours; indexed file sizes", sizes, "RGBA host file", len(layer.write_png().getvalue()))
    with pytest.raises(ValueError, match="paeth"):
        layer.write_png(encoder="device", palette=True, filter="paeth")


def test_stray_colour_under_alpha_zero(S):
    img = _image(7, 11, 5, seed=4)
    img[2:4, 3:9] = (250, 1, 2, 0)
    img[5, :, :] = (3, 4, 5, 0)
    assert (img[img[..., 3] == 0, :3] != 0).any()
    for encoder in ("host", "device"):
        data = S.canvas_to_png(img, encoder=encoder, palette=True).getvalue()
        assert np.array_equal(S.read_png(data), R.canon(img))
        assert struct.unpack(">IIBB", data[16:26]) == (11, 7, 4, 3)


def test_render_svg_palette(S, tmp_path):
    import os

    from tests.util import GOLDEN

    doc = os.path.join(GOLDEN, "demo", "material-design.svgz")
    px = S.read_png(S.render_svg(doc, width=256))
    out = S.render_svg(doc, tmp_path / "out.png", width=256, palette=True)
    device = S.render_svg(doc, width=256, palette=True, encoder="device")
    idx, pal = S.quantize(px)
    assert (tmp_path / "out.png").read_bytes() == out
    assert np.array_equal(S.read_png(out), pal[idx]) and np.array_equal(S.read_png(device), pal[idx])
    print("material-design at width 256:", len(np.unique(R.u32(R.canon(px)))), "colours; indexed host", len(out), "device", len(device))
