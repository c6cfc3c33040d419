"""The filter primitives beyond the reference on the device: Layer.turbulence / component_transfer / convolve_matrix /
displacement_map against the host build of svgr_core.h (tests/filter_harness.cpp) and the numpy restatement
(tests/filter_ref.py) on odd sizes under a rotated and an x/y-swapped transform; feFlood against a solid fill; and one
document whose chain uses them, rendered through the loader and against the same chain built from Layer calls."""
import warnings

import numpy as np
import pytest

from tests import filter_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import svgrasterize_amd as S

    S.Context.get()
    return S


@pytest.fixture(scope="module")
def fh():
    return R.harness()


def _transforms():
    from svgrasterize_amd.geometry import Transform

    return {
        "swap": Transform().matrix(0, 1, 0, 1, 0, 0).translate(3.5, -2.25).scale(1.5),
        "rotated": Transform().matrix(0, 1, 0, 1, 0, 0).translate(20, 10).rotate(0.7).scale(1.25, 0.8),
    }


TRANSFORMS = ["swap", "rotated"]


def _image(shape, seed, lo=0.0, hi=1.0):
    rng = np.random.default_rng(seed)
    return rng.uniform(lo, hi, shape + (4,))


def _premultiplied(shape, seed):
    img = _image(shape, seed)
    img[..., :3] *= img[..., 3:]
    return img


@pytest.mark.parametrize("name", TRANSFORMS)
@pytest.mark.parametrize("octaves, fractal, stitch, seed", [(1, False, False, 0), (4, True, True, -17), (8, False, True, 3.9),
                                                            (6, True, False, 2 ** 35)])
def test_turbulence(S, fh, name, octaves, fractal, stitch, seed):
    from svgrasterize_amd.layer import turbulence_seed

    tr = _transforms()[name]
    offset, shape = (-3, 5), (37, 53)
    tile = (-2.5, 1.75, 23.3, 31.9) if stitch else None
    freq = (0.061, 0.093)
    got = S.Layer.turbulence(tr, offset, shape, freq, octaves, seed, tile, fractal)
    assert (got.offset, got.pre_alpha, got.linear_rgb) == (offset, False, True)
    img = got.image
    host = R.harness_turbulence_layer(fh, tr, offset, shape, freq, octaves, turbulence_seed(seed), tile, fractal)
    assert np.array_equal(img, host)
    ref = R.turbulence_layer(tr, offset, shape, freq, octaves, seed, tile, fractal)
    assert np.abs(img - ref).max() <= 1e-15
    assert img.std() > 0.01


FUNCS = {
    "table": [("table", (0.0, 0.3, 0.2, 1.0)), ("table", (0.7,)), ("table", (1.0, 0.0)), None],
    "discrete": [("discrete", (0.1, 0.9, 0.4)), None, ("discrete", (0.25, 0.5, 0.75, 1.0, 0.0)), ("discrete", (0.5,))],
    "linear": [("linear", 1.7, -0.2), ("linear", -1.0, 1.0), None, ("linear", 0.5, 0.25)],
    "gamma": [("gamma", 1.1, 2.2, -0.05), ("gamma", 0.8, 0.45, 0.1), ("gamma", 1.0, 1.0, 0.0), None],
}


@pytest.mark.parametrize("kind", sorted(FUNCS))
def test_component_transfer(S, kind):
    img = _image((29, 41), 5, -0.1, 1.1)
    img[0, 0] = (0.0, 1.0, 0.5, 1.0)
    layer = S.Layer(img, (7, -4), pre_alpha=False, linear_rgb=True)
    got = layer.component_transfer(FUNCS[kind])
    assert (got.offset, got.pre_alpha, got.linear_rgb, got.image.shape) == ((7, -4), False, True, img.shape)
    ref = R.component_transfer(img, FUNCS[kind])
    if kind == "gamma":
        assert np.abs(got.image - ref).max() <= 1e-14
    else:
        assert np.array_equal(got.image, ref)


@pytest.mark.parametrize("edge_mode", ["duplicate", "wrap", "none"])
@pytest.mark.parametrize("preserve_alpha", [False, True])
@pytest.mark.parametrize("order", [(3, 4), (32, 5)])
def test_convolve_matrix(S, edge_mode, preserve_alpha, order):
    oy, ox = order
    rng = np.random.default_rng(oy * 7 + ox)
    kernel = rng.uniform(-1.0, 2.0, (oy, ox))
    target = (0, oy - 1)
    shape = (23, 37)
    img = _image(shape, 11) if preserve_alpha else _premultiplied(shape, 11)
    layer = S.Layer(img, (2, 9), pre_alpha=not preserve_alpha, linear_rgb=True)
    got = layer.convolve_matrix(kernel, 3.5, 0.05, target, edge_mode, preserve_alpha)
    assert (got.offset, got.pre_alpha, got.linear_rgb) == ((2, 9), not preserve_alpha, True)
    ref = R.convolve_matrix(img, kernel, 3.5, 0.05, target, edge_mode, preserve_alpha)
    assert np.array_equal(got.image, ref)


@pytest.mark.parametrize("name", TRANSFORMS)
def test_displacement_map(S, name):
    tr = _transforms()[name]
    lin = np.asarray(tr.m)[:2, :2]
    src = _premultiplied((31, 27), 3)
    disp = _image((25, 33), 4)
    a = S.Layer(src, (-5, 8), pre_alpha=True, linear_rgb=True)
    m = S.Layer(disp, (-2, 3), pre_alpha=False, linear_rgb=True)
    for xc in "RGBA":
        for yc in "RGBA":
            got = a.displacement_map(m, tr, 9.5, xc, yc)
            assert (got.offset, got.pre_alpha, got.image.shape) == ((-2, 3), True, disp.shape)
            ref = R.displacement_map(src, (-5, 8), disp, (-2, 3), lin, 9.5, "RGBA".index(xc), "RGBA".index(yc))
            assert np.array_equal(got.image, ref), (xc, yc)


def _render(S, text, tr=None):
    from svgrasterize_amd.geometry import Transform

    tr = Transform().matrix(0, 1, 0, 1, 0, 0) if tr is None else tr
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        scene, _, _ = S.svg_scene_from_str(text)
        layer, hull = scene.render(tr, linear_rgb=True)
    return layer, hull, [str(w.message) for w in caught]


SVG = '<svg xmlns="http://www.w3.org/2000/svg" width="64" height="48">{}</svg>'


def test_flood_equals_solid_fill(S):
    flood, _, w1 = _render(S, SVG.format('<filter id="f" filterUnits="userSpaceOnUse" x="10" y="20" width="30" height="15">'
                                         '<feFlood flood-color="#3080c0"/></filter><rect width="5" height="5" filter="url(#f)"/>'))
    fill, _, w2 = _render(S, SVG.format('<rect x="10" y="20" width="30" height="15" fill="#3080c0"/>'))
    assert not w1 and not w2
    assert (flood.offset, flood.width, flood.height) == ((20, 10), 30, 15)
    a = flood.on_canvas(48, 64).image
    b = fill.on_canvas(48, 64).image
    assert np.array_equal(a, b) and a[25, 20, 3] == 1.0


CHAIN = ('<filter id="f" filterUnits="userSpaceOnUse" x="2" y="3" width="58" height="40">'
         '<feTurbulence type="fractalNoise" baseFrequency="0.05 0.08" numOctaves="3" seed="7" result="noise"/>'
         '<feDisplacementMap in="SourceGraphic" in2="noise" scale="6" xChannelSelector="R" yChannelSelector="G"/>'
         '<feComponentTransfer><feFuncR type="table" tableValues="0 0.5 1"/><feFuncG type="discrete" tableValues="0.2 0.8"/>'
         '<feFuncB type="linear" slope="0.5" intercept="0.25"/></feComponentTransfer>'
         '<feDropShadow dx="3" dy="2" stdDeviation="1.5" flood-color="#102030" flood-opacity="0.6"/>'
         '</filter>')
SHAPES = '<rect x="8" y="6" width="40" height="30" fill="#3388cc"/><circle cx="40" cy="30" r="10" fill="#cc4400"/>'


def test_document_chain_matches_layer_calls(S):
    from svgrasterize_amd import filters as F
    from svgrasterize_amd.layer import COMPOSE_IN

    got, _, warned = _render(S, SVG.format(CHAIN + f'<g filter="url(#f)">{SHAPES}</g>'))
    assert not any("unsupported" in w for w in warned), warned
    source, _, _ = _render(S, SVG.format(f"<g>{SHAPES}</g>"))
    tr = S.Transform().matrix(0, 1, 0, 1, 0, 0)
    src = source.convert(pre_alpha=False, linear_rgb=True)
    offset, shape, _ = F.filter_region((False, 2.0, 3.0, 58.0, 40.0), tr, src)
    noise = S.Layer.turbulence(tr, offset, shape, (0.05, 0.08), 3, 7.0, None, True)
    moved = src.displacement_map(noise, tr, 6.0, "R", "G")
    tinted = moved.component_transfer([("table", (0.0, 0.5, 1.0)), ("discrete", (0.2, 0.8)), ("linear", 0.5, 0.25), None])
    alpha = tinted.color_matrix(F.COLOR_MATRIX_ALPHA)
    blurred = alpha.convolve(F.blur_kernel(tr, (1.5, 1.5)))
    x, y = blurred.offset
    tx, ty = tr(tr.invert([x, y]) + [3.0, 2.0])
    shifted = blurred.translate(int(tx) - x, int(ty) - y)
    color = np.array([0x10, 0x20, 0x30, 255], dtype=np.float64) / 255.0
    lin = np.where(color[:3] <= 0.04045, color[:3] / 12.92, ((color[:3] + 0.055) / 1.055) ** 2.4)
    flood = S.Layer.flood((*lin, 0.6), offset, shape)
    shadow = S.Layer.compose([shifted, flood], COMPOSE_IN, linear_rgb=True)
    want = S.Layer.compose([shadow, tinted], linear_rgb=True)
    a = got.on_canvas(48, 64).image
    b = want.on_canvas(48, 64).image
    assert np.array_equal(a, b)
    assert np.abs(a - source.on_canvas(48, 64).image).max() > 0.1   # (the chain did something)
