"""Dithering on the device: svgr_quant_dither against the host build of the same header (tests/dither_harness.cpp, itself held
against numpy by tests/test_dither_host.py), bit for bit, indices and packed stream, at the launch seams of both kernels -- the
diffusion kernel's tiles (strips and blocks, taken from the getters) and the ordered kernel's blocks; then the public route
end to end through read_png."""
import os

import numpy as np
import pytest

from tests import dither_ref as R
from tests import quant_ref as Q

pytestmark = pytest.mark.gpu

MODES = ("ordered", "diffusion")


@pytest.fixture(scope="module")
def S():
    import svgrasterize_amd as S

    S.Context.get()
    return S


@pytest.fixture(scope="module")
def lib():
    return R.harness()


@pytest.fixture(scope="module")
def tile(S):
    from svgrasterize_amd import _abi

    return _abi.dither_tile()


def _colors(n, seed=0):
    rng = np.random.default_rng(seed)
    vals = rng.choice(1 << 24, size=n, replace=False).astype(np.uint32)
    alpha = np.where(np.arange(n) % 3 == 0, 255, 1 + (np.arange(n) * 37) % 254).astype(np.uint32)
    c = Q.rgba(vals | alpha << 24).copy()
    c[0] = 0
    return c


def _noise(rows, cols, seed):
    """Noise with transparent holes (stray colour under them), opaque and translucent pixels."""
    img = np.random.default_rng(seed).integers(0, 256, (rows, cols, 4), dtype=np.uint8)
    img[::3, ::2, 3] = 0
    img[1::2, 1::3, 3] = 255
    return img


def _gradient(rows, cols):
    y, x = np.mgrid[0:rows, 0:cols]
    img = np.empty((rows, cols, 4), dtype=np.uint8)
    img[..., 0] = 255 * x // max(cols - 1, 1)
    img[..., 1] = 255 * y // max(rows - 1, 1)
    img[..., 2] = (3 * x + 5 * y) % 256
    img[..., 3] = 255 - 100 * y // max(rows - 1, 1)
    return img


def _check(S, lib, img, pal, mode, what):
    from svgrasterize_amd import _abi, quant

    ctx = S.Context.get()
    rows, cols = img.shape[:2]
    amp = quant.ordered_amplitude(pal) if mode == "ordered" else 0
    hstream, hidx = R.harness_dither(lib, img, pal, mode, amp)
    stream, plain = _abi.quant_dither(ctx, ctx.from_host(img), rows, cols, pal, mode, amp, stream=True, indices=True)
    got = plain.download((rows, cols), np.uint8)
    assert np.array_equal(got, hidx), (what, mode, rows, cols, len(pal), int((got != hidx).sum()))
    assert np.array_equal(stream.download(hstream.shape, np.uint8), hstream), (what, mode, rows, cols, len(pal))
    return hstream, hidx


def _diffusion_shapes(tile):
    s, w = tile
    yield from ((1, 1), (1, w + 1), (s + 1, 1))
    yield from ((r, c) for r in (s - 1, s, s + 1) for c in (w - 1, w, w + 1))
    yield 2 * s + 1, 2 * w + 3     # three strips by three blocks: the (r-1, c+1) term crosses a strip seam and a block seam at once
    yield 2 * s, 3                 # narrower than the skew


@pytest.mark.parametrize("n_pal", [1, 2, 4, 16, 17, 256])
def test_diffusion_at_the_tile_seams(S, lib, tile, n_pal):
    pal = _colors(n_pal, seed=n_pal) if n_pal > 1 else np.array([[90, 80, 70, 200]], dtype=np.uint8)
    for rows, cols in _diffusion_shapes(tile):
        _check(S, lib, _noise(rows, cols, 31 * rows + cols), pal, "diffusion", "noise")
    rows, cols = 2 * tile[0] + 1, 2 * tile[1] + 3
    _check(S, lib, _gradient(rows, cols), pal, "diffusion", "gradient")


def test_diffusion_over_many_fronts(S, lib, tile):
    # more blocks than strips and more strips than blocks: every shape of a front (growing, full, shrinking)
    s, w = tile
    pal = _colors(9, seed=3)
    for rows, cols in ((3 * s + 2, 9 * w + 5), (9 * s + 5, 2 * w + 1)):
        _check(S, lib, _gradient(rows, cols), pal, "diffusion", "fronts")
        _check(S, lib, _noise(rows, cols, rows), pal, "diffusion", "fronts")


@pytest.mark.parametrize("n_pal", [2, 4, 16, 17, 256])
def test_ordered_at_every_depth(S, lib, n_pal):
    from svgrasterize_amd import _abi

    block = _abi.quant_block()
    pal = _colors(n_pal, seed=n_pal)
    for rows, cols in ((1, 1), (4, 5), (3, 5), (9, 17), (16, 17), (2, 9), (1, block + 1), (2, block // 2 + 1), (3, block // 2 + 3), (2, block + 7)):
        _check(S, lib, _noise(rows, cols, n_pal + cols), pal, "ordered", "noise")
    _check(S, lib, _gradient(9, 2 * 8 + 1), pal, "ordered", "gradient")
    flat = np.zeros((9, 40, 4), dtype=np.uint8)   # one colour: a lane's run repeats its pixel and still changes its target
    flat[...] = (120, 130, 140, 255)
    _check(S, lib, flat, pal, "ordered", "flat")


@pytest.mark.parametrize("mode", MODES)
def test_ties_go_to_the_lowest_index(S, lib, tile, mode):
    # every entry twice, and entries at equal distances on both sides of the image's greys: the lowest index wins, through the
    # lanes' reduction as in the sequential loop
    base = np.array([(10, 10, 10, 255), (30, 30, 30, 255), (50, 50, 50, 255), (30, 30, 30, 255), (10, 10, 10, 255), (50, 50, 50, 255)], dtype=np.uint8)
    pal = np.concatenate([base] * 6)[:34]   # (more entries than a pixel has lanes: ties inside a lane's slice and across lanes)
    rows, cols = tile[0] + 1, tile[1] + 1
    img = np.zeros((rows, cols, 4), dtype=np.uint8)
    img[..., :3] = (20 + 20 * ((np.arange(rows)[:, None] + np.arange(cols)[None, :]) % 2))[..., None]
    img[..., 3] = 255
    _, idx = _check(S, lib, img, pal, mode, "ties")
    assert idx.max() < 3
    one = np.array([[1, 2, 3, 255]], dtype=np.uint8)
    assert not _check(S, lib, _noise(rows, cols, 8), one, mode, "one entry")[1].any()


@pytest.mark.parametrize("mode", MODES)
def test_one_output_at_a_time_and_twice(S, lib, tile, mode):
    from svgrasterize_amd import _abi, quant

    ctx = S.Context.get()
    rows, cols = tile[0] + 3, tile[1] + 5
    img, pal = _noise(rows, cols, 77), _colors(5, seed=2)   # (depth 4: bytes of two pixels)
    amp = quant.ordered_amplitude(pal)
    hstream, hidx = _check(S, lib, img, pal, mode, "both")
    buf = ctx.from_host(img)
    for _ in range(2):
        stream, none = _abi.quant_dither(ctx, buf, rows, cols, pal, mode, amp, stream=True, indices=False)
        assert none is None and np.array_equal(stream.download(hstream.shape, np.uint8), hstream)
        none, plain = _abi.quant_dither(ctx, buf, rows, cols, pal, mode, amp, stream=False, indices=True)
        assert none is None and np.array_equal(plain.download((rows, cols), np.uint8), hidx)


def test_refused_before_any_launch(S):
    from svgrasterize_amd import _abi

    ctx = S.Context.get()
    buf = ctx.from_host(np.zeros((2, 2, 4), dtype=np.uint8))
    pal = np.zeros((2, 4), dtype=np.uint8)
    for mode in (0, 3, -1):
        with pytest.raises(ValueError, match="mode"):
            _abi.quant_dither(ctx, buf, 2, 2, pal, mode)
    for mode in MODES:
        with pytest.raises(ValueError, match="buffer too small"):
            _abi.quant_dither(ctx, buf, 2, 3, pal, mode)
        with pytest.raises(ValueError, match="entries"):
            _abi.quant_dither(ctx, buf, 2, 2, np.zeros((257, 4), dtype=np.uint8), mode)
        with pytest.raises(ValueError):
            _abi.quant_dither(ctx, buf, 2, 2, pal, mode, stream=False, indices=False)
        d_pal = ctx.from_host(pal)
        with pytest.raises(ValueError, match="must not be the source"):
            _abi._check(ctx.lib.svgr_quant_dither(ctx.handle, buf.handle, 2, 2, d_pal.handle, 2, _abi.DITHER_MODES[mode], 0, None, buf.handle))
        short = ctx.from_host(np.zeros(3, dtype=np.uint8))   # (four pixels: four indices, or two rows of two bytes)
        for outputs in ((short.handle, None), (None, short.handle)):
            with pytest.raises(ValueError, match="buffer too small"):
                _abi._check(ctx.lib.svgr_quant_dither(ctx.handle, buf.handle, 2, 2, d_pal.handle, 2, _abi.DITHER_MODES[mode], 0, *outputs))
    with pytest.raises(ValueError, match="amplitude"):
        _abi.quant_dither(ctx, buf, 2, 2, pal, "ordered", 65026)


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


@pytest.mark.parametrize("mode", MODES)
def test_shaded_document(S, mode):
    layer = _layer(S, SHADED)
    rgba = layer.to_rgba8()
    plain_idx, plain_pal = S.quantize(layer)
    idx, pal = S.quantize(layer, dither=mode)
    assert np.array_equal(pal, plain_pal) and np.array_equal(pal, Q.palette_ref(rgba, 256))
    assert np.array_equal(idx, R.dither_ref(rgba, pal, mode)) and not np.array_equal(idx, plain_idx)
    assert np.array_equal(S.quantize(rgba, dither=mode)[0], idx)
    for max_colors in (7, 16):   # (depth 4: the stream's bytes hold two pixels)
        few_idx, few_pal = S.quantize(layer, max_colors, dither=mode)
        assert np.array_equal(few_pal, S.quantize(layer, max_colors)[1]) and np.array_equal(few_idx, R.dither_ref(rgba, few_pal, mode))
        assert np.array_equal(S.read_png(layer.write_png(palette=max_colors, dither=mode).getvalue()), few_pal[few_idx])
    undithered = layer.write_png(palette=True).getvalue()
    for encoder, kw in (("host", {}), ("host", dict(level=1, threads=2)), ("device", {}), ("device", dict(filter="none", huffman="fixed"))):
        data = layer.write_png(encoder=encoder, palette=True, dither=mode, **kw).getvalue()
        assert np.array_equal(S.read_png(data), pal[idx]), (encoder, kw)
        assert data == S.canvas_to_png(rgba, encoder=encoder, palette=256, dither=mode, **kw).getvalue()
        assert data != layer.write_png(encoder=encoder, palette=True, **kw).getvalue()
        assert layer.write_png(encoder=encoder, palette=True, dither="none", **kw).getvalue() == layer.write_png(encoder=encoder, palette=True, **kw).getvalue()
        print(mode, encoder, kw, len(data), "bytes against", len(undithered), "undithered")


def test_flat_document_is_never_dithered(S):
    layer = _layer(S, FLAT)
    plain = layer.write_png(palette=True).getvalue()
    for encoder in ("host", "device"):
        files = {d: layer.write_png(encoder=encoder, palette=True, dither=d).getvalue() for d in (None, "none", "ordered", "diffusion")}
        assert len(set(files.values())) == 1 and (encoder == "device" or files[None] == plain)
    idx, pal = S.quantize(layer)
    for mode in MODES:
        got = S.quantize(layer, dither=mode)
        assert np.array_equal(got[0], idx) and np.array_equal(got[1], pal)


def test_render_svg_dither(S, tmp_path):
    from tests.util import GOLDEN

    doc = os.path.join(GOLDEN, "demo", "material-design.svgz")
    px = S.read_png(S.render_svg(doc, width=256))
    out = S.render_svg(doc, tmp_path / "out.png", width=256, palette=True, dither="diffusion")
    device = S.render_svg(doc, width=256, palette=True, dither="diffusion", encoder="device")
    idx, pal = S.quantize(px, dither="diffusion")
    assert (tmp_path / "out.png").read_bytes() == out
    assert np.array_equal(S.read_png(out), pal[idx]) and np.array_equal(S.read_png(device), pal[idx])
    few = S.render_svg(doc, width=256, palette=16, dither="ordered")
    idx16, pal16 = S.quantize(px, 16, dither="ordered")
    assert np.array_equal(S.read_png(few), pal16[idx16])   # (black icons: the offset moves colour only, and this file may equal the plain one)
