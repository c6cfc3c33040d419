"""CPU-side checks of filter primitive subregions, primitiveUnits, feTile and feImage: what the loader makes of the attributes,
how the chain resolves subregions to device boxes (against tests/subregion_ref.py), and the tile index functions of
csrc/svgr_core.h (host build, tests/subregion_harness.cpp) against numpy's floor modulo.  No GPU needed."""
import base64
import warnings

import numpy as np
import pytest

from svgrasterize_amd import filters as F
from svgrasterize_amd.geometry import Transform
from svgrasterize_amd.layer import Layer, canvas_to_png
from svgrasterize_amd.svg import svg_scene_from_str
from tests import subregion_ref as R

DEFAULT_REGION = (True, None, None, None, None)


def _filter(body, attrs=""):
    text = (f'<svg xmlns="http://www.w3.org/2000/svg" xmlns:xlink="http://www.w3.org/1999/xlink" width="40" height="30">'
            f'<filter id="f" {attrs}>{body}</filter><rect id="r" width="10" height="10" filter="url(#f)"/></svg>')
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        _scene, ids, _size = svg_scene_from_str(text)
    return ids["f"], [str(w.message) for w in caught], ids


def _png_uri(pixels):
    return "data:image/png;base64," + base64.b64encode(canvas_to_png(pixels).getvalue()).decode()


# -- loader --------------------------------------------------------------------------------------------------------------------
def test_loader_subregion_reaches_the_filter():
    flt, warned, _ = _filter('<feFlood x="10" y="11.5" width="20" height="5" flood-color="red"/><feOffset dx="3" width="7"/>'
                             '<feGaussianBlur stdDeviation="2"/>')
    assert not warned
    assert flt.subregions == {0: (10.0, 11.5, 20.0, 5.0), 1: (None, None, 7.0, None)}
    assert flt.primitive_bbox is False and flt.region == DEFAULT_REGION
    assert [f[0] for f in flt.filters] == [F.FE_FLOOD, F.FE_OFFSET, F.FE_GAUSSIAN_BLUR]
    # the entries themselves are what they were without the attributes
    assert flt.filters[0] == (F.FE_FLOOD, ((1.0, 0.0, 0.0, 1.0), DEFAULT_REGION), [])
    assert flt.filters[1] == (F.FE_OFFSET, (3.0, 0.0), [2])


def test_loader_primitive_units():
    flt, warned, _ = _filter('<feFlood x="0.25" y="10%" width="0.5" height="50%"/>', 'primitiveUnits="objectBoundingBox"')
    assert not warned
    assert flt.primitive_bbox is True and flt.subregions == {0: (0.25, 0.1, 0.5, 0.5)}
    flt, warned, _ = _filter('<feFlood x="3"/>', 'primitiveUnits="userSpaceOnUse"')
    assert not warned and flt.primitive_bbox is False and flt.subregions == {0: (3.0, None, None, None)}
    flt, warned, _ = _filter('<feFlood x="3"/>', 'primitiveUnits="bogus"')
    assert len(warned) == 1 and "invalid primitive units: bogus" in warned[0]
    assert flt.primitive_bbox is False and flt.subregions == {0: (3.0, None, None, None)}


def test_loader_filter_without_the_attributes_is_todays():
    flt, warned, _ = _filter('<feFlood flood-color="red" result="a"/><feOffset dx="3" dy="1"/><feGaussianBlur stdDeviation="2 3"/>'
                             '<feDiffuseLighting><fePointLight x="1" y="2" z="3"/></feDiffuseLighting>'
                             '<feDropShadow/>')
    assert not warned
    want = (F.Filter.empty().flood((1.0, 0.0, 0.0, 1.0), DEFAULT_REGION, "a").offset(3.0, 1.0).blur(2.0, 3.0)
            .diffuse_lighting(None, F.PointLight(1.0, 2.0, 3.0), (1.0, 1.0, 1.0), 1.0, 1.0, DEFAULT_REGION)
            .drop_shadow(2.0, 2.0, 2.0, 2.0, (0.0, 0.0, 0.0, 1.0), DEFAULT_REGION))
    assert flt.names == want.names and flt.subregions == {} and flt.primitive_bbox is False and flt.region is None
    assert len(flt.filters) == len(want.filters)
    for (t0, a0, i0), (t1, a1, i1) in zip(flt.filters, want.filters):
        assert t0 == t1 and i0 == i1 and repr(a0) == repr(a1)
    assert tuple(F.Filter.empty()) == ({"SourceAlpha": 0, "SourceGraphic": 1}, [], {}, False, None)


def test_loader_percent_and_negative_warn():
    flt, warned, _ = _filter('<feFlood x="10%" y="4" width="50%"/>')
    assert len(warned) == 2 and all("needs the viewport" in w for w in warned)
    assert flt.subregions == {0: (None, 4.0, None, None)}
    flt, warned, _ = _filter('<feFlood x="10%"/>')   # (nothing is left: no subregion)
    assert len(warned) == 1 and flt.subregions == {}
    flt, warned, _ = _filter('<feFlood x="1" y="2" width="-5" height="3"/>')
    assert len(warned) == 1 and "negative subregion size" in warned[0]
    assert flt.subregions == {0: (None, None, None, None)}   # (the default subregion)
    with pytest.raises(ValueError):
        F.Filter.empty().offset(1, 1).subregion(width=-1)


def test_loader_tile_and_image_take_their_place_in_the_chain():
    pixels = np.zeros((3, 5, 4), dtype=np.uint8)
    pixels[..., 0], pixels[..., 3] = 200, 255
    flt, warned, ids = _filter(f'<feOffset dx="1" result="o"/><feTile x="0" width="30"/><feOffset dx="2"/>'
                               f'<feImage xlink:href="{_png_uri(pixels)}" preserveAspectRatio="none" x="2" y="3" width="10" height="6"/>'
                               f'<feOffset dx="4"/><feImage href="#later"/><feOffset dx="5"/>'
                               f'<feImage href="https://example.org/a.png"/><feOffset dx="6"/>')
    assert not any("unsupported filter type" in w for w in warned), warned
    assert len(warned) == 1 and "only data URIs and local files" in warned[0]   # (<image>'s rule: nothing is fetched)
    kinds = [f[0] for f in flt.filters]
    assert kinds == [F.FE_OFFSET, F.FE_TILE, F.FE_OFFSET, F.FE_IMAGE, F.FE_OFFSET, F.FE_IMAGE, F.FE_OFFSET, F.FE_IMAGE, F.FE_OFFSET]
    # every primitive without `in` reads the one in front of it, the new ones included
    assert [f[2] for f in flt.filters] == [[1], [2], [3], [], [5], [], [7], [], [9]]
    assert flt.subregions == {1: (0.0, None, 30.0, None), 3: (2.0, 3.0, 10.0, 6.0)}
    kind, got, par, smooth = flt.filters[3][1]
    assert kind == "raster" and np.array_equal(got, pixels) and par == "none" and smooth is True
    assert flt.filters[5][1][:2] == ("element", "later") and flt.filters[5][1][2]("r") is ids["r"]
    assert flt.filters[7][1] == ("none",)


def test_loader_object_bounding_box_warns_once_about_what_it_does_not_rescale():
    body = ('<feDiffuseLighting surfaceScale="2"><fePointLight x="1" y="2" z="3"/></feDiffuseLighting>'
            '<feDisplacementMap in2="SourceGraphic" scale="4"/><feSpecularLighting><feDistantLight/></feSpecularLighting>')
    _, warned, _ = _filter(body, 'primitiveUnits="objectBoundingBox"')
    assert len(warned) == 1 and "stay in user units" in warned[0]
    _, warned, _ = _filter(body)
    assert not warned


def test_drop_shadow_subregion_goes_to_the_merge_and_the_flood():
    flt, warned, _ = _filter('<feOffset dx="1"/><feDropShadow x="1" y="2" width="30" height="20"/>')
    assert not warned and len(flt.filters) == 7
    assert flt.subregions == {6: (1.0, 2.0, 30.0, 20.0, [2]), 4: 6}
    assert flt.filters[4][0] == F.FE_FLOOD and flt.filters[6][0] == F.FE_MERGE


# -- resolution ----------------------------------------------------------------------------------------------------------------
TRANSFORMS = {
    "swap": Transform().matrix(0, 1, 0, 1, 0, 0).translate(3.5, -2.25).scale(1.5),
    "rotated": Transform().matrix(0, 1, 0, 1, 0, 0).translate(20, 10).rotate(0.7).scale(1.25, 0.8),
}
REGION = (False, 2.0, 3.0, 58.0, 40.0)


def _source():
    return Layer(np.zeros((20, 30, 4)), (4, -6), pre_alpha=True, linear_rgb=True)


def _resolved(flt, tr):
    source = _source()
    f_off, f_shape, f_rect = F.filter_region(flt.region, tr, source)
    regions = flt._regions(tr, source, None, (f_rect, (*f_off, *f_shape)))
    return [regions(k + 2) for k in range(len(flt.filters))]


def _boxes(regions):
    return [None if r is None else tuple(int(v) for v in r[1]) for r in regions]


@pytest.mark.parametrize("name", sorted(TRANSFORMS))
def test_resolution_matches_the_restatement(name):
    tr = TRANSFORMS[name]
    flt = (F.Filter.empty(region=REGION)
           .offset(1, 1, "SourceGraphic", "a").subregion(10.3, 8.1, 20.0, 12.7)       # 0: standard input: defaults = filter region
           .offset(2, 2, "SourceGraphic", "b").subregion(y=20.2, height=30.0)         # 1: x / width from the region; cut by it
           .merge(["a", "b"], "m")                                                    # 2: no attributes: union of a and b
           .blur(1.0, None, "m").subregion(x=15.0)                                    # 3: missing ones from the union
           .merge(["m", "SourceGraphic"])                                             # 4: a standard input: none
           .flood((1, 0, 0, 1), REGION).subregion(-50.0, -50.0, 10.0, 10.0)           # 5: outside the region: empty
           .offset(0, 0, "a").subregion(width=0.0))                                   # 6: width 0: empty
    chain = [dict(inputs=[1], sub=(10.3, 8.1, 20.0, 12.7)), dict(inputs=[1], sub=(None, 20.2, None, 30.0)), dict(inputs=[2, 3]),
             dict(inputs=[4], sub=(15.0, None, None, None)), dict(inputs=[4, 1]), dict(inputs=[], sub=(-50.0, -50.0, 10.0, 10.0)),
             dict(inputs=[2], sub=(None, None, 0.0, None))]
    want, frame = R.resolve(chain, tr, REGION[1:])
    got = _resolved(flt, tr)
    assert _boxes(got) == [None if w is None else w[1] for w in want]
    for g, w in zip(got, want):
        assert (g is None) == (w is None)
        if g is not None:
            assert np.allclose(g[0], w[0], rtol=0, atol=1e-12)
    boxes = _boxes(got)
    assert boxes[4] is None and boxes[5][2:] == (0, 0) and boxes[6][2:] == (0, 0)
    assert boxes[2] == R.union_boxes([boxes[0], boxes[1]])
    f = frame[1]
    for b in boxes[:4]:   # inside the filter region's box
        assert b[0] >= f[0] and b[1] >= f[1] and b[0] + b[2] <= f[0] + f[2] and b[1] + b[3] <= f[1] + f[3] and b[2] * b[3] > 0
    assert boxes[1][0] + boxes[1][2] == f[0] + f[2] or boxes[1][1] + boxes[1][3] == f[1] + f[3]   # (it was cut by the region)


def test_resolution_known_boxes():
    """Under the plain x/y swap (row = y, column = x) the boxes can be read off."""
    tr = Transform().matrix(0, 1, 0, 1, 0, 0)
    flt = (F.Filter.empty(region=REGION).flood((1, 0, 0, 1), REGION).subregion(10.5, 8.0, 20.0, 12.25)
           .offset(1, 1, "SourceGraphic").subregion(x=50.0)
           .offset(1, 1, "SourceGraphic"))
    got = _resolved(flt, tr)
    assert _boxes(got) == [(8, 10, 13, 21), (3, 50, 40, 10), None]
    assert got[1][0] == (50.0, 3.0, 58.0, 40.0)   # (width from the filter region; the box is cut at the region's edge, x = 60)


def test_a_chain_without_attributes_has_no_subregions():
    flt = F.Filter.empty(region=REGION).offset(1, 1).blur(2.0).merge([None, "SourceGraphic"]).flood((1, 0, 0, 1), REGION)
    assert flt.subregions == {}
    assert all(r is None for r in _resolved(flt._replace(subregions={99: (0.0, 0.0, 1.0, 1.0)}), TRANSFORMS["swap"]))


def test_resolution_object_bounding_box():
    tr = TRANSFORMS["rotated"]
    source = _source()
    bbox = F._user_bbox(tr, source)
    flt = (F.Filter.empty(True, REGION).offset(0.1, 0.2, "SourceGraphic").subregion(0.25, 0.125, 0.5, 0.75)
           .blur(0.05, 0.1).morphology(0.02, 0.04, "max", None))
    got = _resolved(flt, tr)
    want, _ = R.resolve([dict(inputs=[1], sub=(0.25, 0.125, 0.5, 0.75)), dict(inputs=[2]), dict(inputs=[3])], tr, REGION[1:], bbox)
    assert _boxes(got) == [w[1] for w in want] and got[0][1][2] * got[0][1][3] > 0
    bx, by, bw, bh = bbox
    assert np.allclose(got[0][0], (bx + 0.25 * bw, by + 0.125 * bh, 0.5 * bw, 0.75 * bh), rtol=0, atol=1e-12)


def test_drop_shadow_resolution():
    tr = Transform().matrix(0, 1, 0, 1, 0, 0)
    flt = F.Filter.empty(region=REGION).drop_shadow(region=REGION, subregion=(10.0, 8.0, 20.0, 12.0))
    boxes = _boxes(_resolved(flt, tr))
    assert boxes == [None, None, None, (8, 10, 12, 20), None, (8, 10, 12, 20)]


# -- the tile index functions of svgr_core.h -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sh():
    return R.harness()


@pytest.mark.parametrize("o0, n, t0, tn, s0, sn", [
    (-37, 101, 5, 7, 5, 7),        # the output starts left of / above the tile
    (3, 11, -20, 64, -20, 64),     # the tile is larger than the output
    (-9, 40, 2, 1, 0, 5),          # a 1 x 1 tile
    (-15, 60, -4, 9, 0, 20),       # the tile starts outside the source layer
    (0, 50, 10, 13, 0, 17),        # the tile ends outside the source layer
    (-6, 30, 100, 5, 0, 10),       # the tile lies wholly outside the source layer
    (7, 23, 7, 23, -3, 40),        # tile = output: the window
    (2 ** 30 - 50, 49, -(2 ** 30) + 1, 2 ** 30 - 1, 0, 2 ** 30 - 1),   # the far corners of what the entry point admits
])
def test_tile_index_functions(sh, o0, n, t0, tn, s0, sn):
    want = R.axis_source(o0, n, t0, tn, s0, sn)
    assert np.array_equal(R.harness_axis(sh, o0, n, t0, tn, s0, sn, walk=False), want)
    assert np.array_equal(R.harness_axis(sh, o0, n, t0, tn, s0, sn, walk=True), want)
    # and the restatement of whole images agrees with the per-axis one
    if n <= 101 and sn <= 64:
        img = np.arange(sn * 3 * 4, dtype=np.float64).reshape(sn, 3, 4) + 1.0
        got = R.tile(img, (s0, 0), (o0, 0, n, 3), (t0, 0, tn, 3))
        rows = np.where(want[:, None, None] >= 0, img[np.maximum(want, 0)], 0.0)
        assert np.array_equal(got, rows)
