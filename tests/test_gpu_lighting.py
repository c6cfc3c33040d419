"""feDiffuseLighting / feSpecularLighting on the device: Layer.lighting against the numpy restatement (tests/lighting_ref.py) for
each light kind on odd regions under an x/y-swapped and a rotated transform, with the input partly outside the region; a
lighting document under the identity and the swap giving transposed canvases; and two documents (a bevel, a spot-lit diffuse
surface) through the loader against the same chains built from Layer calls."""
import warnings

import numpy as np
import pytest

from tests import lighting_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import svgrasterize_amd as S

    S.Context.get()
    return S


def _transforms():
    from svgrasterize_amd.geometry import Transform

    return {
        "swap": Transform().matrix(0, 1, 0, 1, 0, 0).translate(3.5, -2.25).scale(1.5),
        "rotated": Transform().matrix(0, 1, 0, 1, 0, 0).translate(20, 10).rotate(0.7).scale(1.25, 0.8),
    }


def _light(kind, tr, offset, shape):
    """A light of `kind` in user space that lights the device region (offset, shape) under `tr`."""
    from svgrasterize_amd import filters as F

    inv = tr.invert
    c = np.array([offset[0] + shape[0] / 2, offset[1] + shape[1] / 2])
    if kind == "distant":
        return R.DISTANT, F.DistantLight(-63.0, 41.0)
    x, y = inv(c + [2.5, -4.0])
    if kind == "point":
        return R.POINT, F.PointLight(x, y, 18.0)
    ax, ay = inv(c)
    return R.SPOT, F.SpotLight(x, y, 25.0, ax, ay, 0.0, 3.0, 55.0)


REGIONS = [((5, -3), (1, 17)), ((-2, 4), (2, 2)), ((1, 2), (17, 1)), ((-7, 3), (13, 21)), ((0, 0), (33, 19))]


@pytest.mark.parametrize("name", ["swap", "rotated"])
@pytest.mark.parametrize("kind", ["distant", "point", "spot"])
@pytest.mark.parametrize("specular", [False, True])
def test_layer_lighting_matches_restatement(S, name, kind, specular):
    tr = _transforms()[name]
    rng = np.random.default_rng(5)
    color = (0.95, 0.7, 0.35)
    se = 17.0 if specular else None
    for offset, shape in REGIONS:
        # the input: straight-alpha RGBA that covers the region's middle and reaches past its top-left corner
        src_offset = (offset[0] - 2, offset[1] - 3)
        src_shape = (max(shape[0] // 2 + 3, 2), max(shape[1] // 2 + 4, 2))
        img = rng.uniform(0.0, 1.0, src_shape + (4,))
        src = S.Layer(img, src_offset, pre_alpha=False, linear_rgb=True)
        code, light = _light(kind, tr, offset, shape)
        got = src.lighting(tr, offset, shape, light, color, 2.0, 0.9, se)
        assert (got.offset, got.pre_alpha, got.linear_rgb, got.image.shape) == (offset, specular, True, shape + (4,))
        A = R.region_alpha(img, src_offset, offset, shape)
        ref = R.lighting(A, offset, code, R.light_frame(tr, code, tuple(light)), color, 2.0, 0.9, se)
        assert np.abs(got.image - ref).max() <= 1e-13, (offset, shape)
        if shape[0] > 2 and shape[1] > 2:
            assert got.image[..., :3].max() > 0.01
        # a premultiplied view of the same input: alpha is the same, so is the result
        pre = src.convert(pre_alpha=True)
        assert np.array_equal(pre.lighting(tr, offset, shape, light, color, 2.0, 0.9, se).image, got.image)


def _render(S, text, tr=None):
    from svgrasterize_amd.geometry import Transform

    tr = Transform().matrix(0, 1, 0, 1, 0, 0) if tr is None else tr
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        scene, _, _ = S.svg_scene_from_str(text)
        layer, hull = scene.render(tr, linear_rgb=True)
    return layer, hull, [str(w.message) for w in caught]


SVG = '<svg xmlns="http://www.w3.org/2000/svg" width="64" height="48">{}</svg>'
LIT = ('<filter id="f" filterUnits="userSpaceOnUse" x="4" y="2" width="50" height="41">'
       '<feSpecularLighting in="SourceAlpha" surfaceScale="6" specularConstant="1.3" specularExponent="9" lighting-color="#ffeecc" result="s">'
       '<feSpotLight x="12" y="8" z="30" pointsAtX="30" pointsAtY="25" specularExponent="2" limitingConeAngle="40"/>'
       '</feSpecularLighting>'
       '<feDiffuseLighting in="SourceAlpha" surfaceScale="-3" diffuseConstant="0.8" result="d"><fePointLight x="50" y="10" z="20"/>'
       '</feDiffuseLighting>'
       '<feComposite in="d" in2="s" operator="arithmetic" k2="0.5" k3="0.5"/>'
       '</filter>'
       '<rect x="10" y="7" width="30" height="24" fill="#4080c0" filter="url(#f)"/>')


def test_document_transposes_with_the_transform(S):
    """x/y swapped between the two renders: the canvases are transposes of each other (the device-frame mapping)."""
    from svgrasterize_amd.geometry import Transform

    a, _, wa = _render(S, SVG.format(LIT), Transform())
    b, _, wb = _render(S, SVG.format(LIT), Transform().matrix(0, 1, 0, 1, 0, 0))
    assert not any("unsupported" in w for w in wa + wb), wa + wb
    ca = a.on_canvas(64, 48).image
    cb = b.on_canvas(48, 64).image
    assert np.abs(ca - cb.transpose(1, 0, 2)).max() <= 1e-13
    assert ca[..., 3].max() > 0.5 and ca[..., :3].std() > 0.05


BEVEL = ('<filter id="bevel" filterUnits="userSpaceOnUse" x="0" y="0" width="64" height="48">'
         '<feGaussianBlur in="SourceAlpha" stdDeviation="2" result="blur"/>'
         '<feSpecularLighting in="blur" surfaceScale="5" specularConstant="0.75" specularExponent="20" lighting-color="#bbbbbb" '
         'result="spec"><fePointLight x="-20" y="-30" z="80"/></feSpecularLighting>'
         '<feComposite in="spec" in2="SourceAlpha" operator="in" result="specOut"/>'
         '<feComposite in="SourceGraphic" in2="specOut" operator="arithmetic" k1="0" k2="1" k3="1" k4="0"/>'
         '</filter>')
SPOTLIT = ('<filter id="spot" filterUnits="userSpaceOnUse" x="2" y="3" width="58" height="40">'
           '<feDiffuseLighting in="SourceGraphic" surfaceScale="3" diffuseConstant="1.2" style="lighting-color: #ffe0a0">'
           '<feSpotLight x="10" y="5" z="40" pointsAtX="32" pointsAtY="24" pointsAtZ="0" specularExponent="3" limitingConeAngle="30"/>'
           '</feDiffuseLighting></filter>')
SHAPES = '<rect x="8" y="6" width="40" height="30" fill="#3388cc"/><circle cx="40" cy="30" r="10" fill="#cc4400"/>'


def _source(S):
    source, _, _ = _render(S, SVG.format(f"<g>{SHAPES}</g>"))
    return source


def test_bevel_document_matches_layer_calls(S):
    from svgrasterize_amd import filters as F
    from svgrasterize_amd.layer import COMPOSE_IN, Layer
    from svgrasterize_amd.svg import parse_color

    got, _, warned = _render(S, SVG.format(BEVEL + f'<g filter="url(#bevel)">{SHAPES}</g>'))
    assert not any("unsupported" in w for w in warned), warned
    source = _source(S)
    tr = S.Transform().matrix(0, 1, 0, 1, 0, 0)
    src = source.convert(pre_alpha=False, linear_rgb=True)
    alpha = Layer(source.image[..., -1:] * np.array([0, 0, 0, 1]), source.offset, pre_alpha=True, linear_rgb=True)
    blurred = alpha.convolve(F.blur_kernel(tr, (2.0, 2.0)))
    offset, shape, _ = F.filter_region((False, 0.0, 0.0, 64.0, 48.0), tr, src)
    spec = blurred.lighting(tr, offset, shape, F.PointLight(-20.0, -30.0, 80.0), parse_color("#bbbbbb")[:3], 5.0, 0.75, 20.0)
    spec_out = Layer.compose([alpha, spec], COMPOSE_IN, linear_rgb=True)
    want = Layer.compose([spec_out, src], (0.0, 1.0, 1.0, 0.0), linear_rgb=True)
    a = got.on_canvas(48, 64).image
    assert np.array_equal(a, want.on_canvas(48, 64).image)
    assert np.abs(a - source.on_canvas(48, 64).image).max() > 0.05   # (the highlight is there)


def test_spot_diffuse_document_matches_layer_calls(S):
    from svgrasterize_amd import filters as F
    from svgrasterize_amd.svg import parse_color

    got, _, warned = _render(S, SVG.format(SPOTLIT + f'<g filter="url(#spot)">{SHAPES}</g>'))
    assert not any("unsupported" in w for w in warned), warned
    source = _source(S)
    tr = S.Transform().matrix(0, 1, 0, 1, 0, 0)
    src = source.convert(pre_alpha=False, linear_rgb=True)
    offset, shape, _ = F.filter_region((False, 2.0, 3.0, 58.0, 40.0), tr, src)
    want = src.lighting(tr, offset, shape, F.SpotLight(10.0, 5.0, 40.0, 32.0, 24.0, 0.0, 3.0, 30.0), parse_color("#ffe0a0")[:3],
                        3.0, 1.2)
    assert (got.offset, got.width, got.height) == ((3, 2), 58, 40)
    a = got.on_canvas(48, 64).image
    assert np.array_equal(a, want.on_canvas(48, 64).image)
    assert (a[3:43, 2:60, 3] == 1.0).all()   # (diffuse output is opaque over the whole region)
    assert np.abs(a - source.on_canvas(48, 64).image).max() > 0.1
