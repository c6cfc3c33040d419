"""Filter primitive subregions, primitiveUnits, feTile and feImage on the device: Layer.tile (svgr_layer_tile, k_layer_tile)
and Layer.window against the numpy restatement (tests/subregion_ref.py) bit for bit, and documents rendered through the loader
against (a) the same chain built from Filter calls and (b) the numpy chain evaluator, under the x/y-swapped and the rotated
transform of tests/test_gpu_filter_primitives.py.  Copies and floods compare with np.array_equal; a case that runs through the
blur takes the blur's tolerance of tests/test_gradient_blur.py (1e-14 against scipy's convolution), the feImage cases the image
fill's of tests/test_gpu_image.py (1e-6)."""
import base64
import ctypes as C
import warnings

import numpy as np
import pytest

from tests import subregion_ref as R

pytestmark = pytest.mark.gpu

BLUR_TOL = 1e-14    # tests/test_gradient_blur.py: the convolution against scipy's
IMAGE_TOL = 1e-6    # tests/test_gpu_image.py: TOL
COMPOSE_TOL = 1e-14  # tests/test_filters_compose.py: compose (SourceGraphic goes to straight alpha and back on its way through a merge)


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


TRANSFORMS = ["swap", "rotated"]


def _premultiplied(shape, seed):
    img = np.random.default_rng(seed).uniform(0.05, 1.0, shape + (4,))
    img[..., :3] *= img[..., 3:]
    return img


# -- Layer.tile / Layer.window ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_box, tile_box", [
    ((-11, -7, 53, 67), (2, 3, 7, 5)),          # the output starts above / left of the tile; odd sizes
    ((5, 9, 9, 13), (-3, 4, 31, 41)),           # the tile is larger than the output
    ((-5, -5, 33, 29), (6, 8, 1, 1)),           # a 1 x 1 tile
    ((-20, -30, 77, 131), (-9, -13, 17, 23)),   # the tile reaches beyond the layer (above / left)
    ((0, 0, 64, 300), (10, 20, 25, 37)),        # ... and below / right; a row of more than one workgroup (300 pixels)
    ((-4, 1, 3, 2), (100, 100, 5, 5)),          # the tile lies outside the layer: transparent
])
def test_layer_tile(S, out_box, tile_box):
    img, off = _premultiplied((23, 31), 11), (-2, -6)
    src = S.Layer(img, off, pre_alpha=True, linear_rgb=True)
    got = src.tile(out_box[:2], out_box[2:], tile_box[:2], tile_box[2:])
    assert (got.offset, got.height, got.width, got.pre_alpha, got.linear_rgb) == (out_box[:2], out_box[2], out_box[3], True, True)
    want = R.tile(img, off, out_box, tile_box)
    assert np.array_equal(got.image, want)
    assert (want != 0).any() == (tile_box[0] < 100)


@pytest.mark.parametrize("box", [(-7, -9, 41, 53), (3, 2, 5, 7), (10, 20, 30, 40), (-2, -6, 23, 31), (50, 50, 3, 3)])
def test_layer_window(S, box):
    img, off = _premultiplied((23, 31), 12), (-2, -6)
    for make in (lambda: S.Layer(img, off, pre_alpha=True, linear_rgb=True),
                 lambda: S.Layer(img, off, pre_alpha=True, linear_rgb=True).convert(pre_alpha=True, linear_rgb=True)):
        src = make()
        got = src.window(box[:2], box[2:])
        assert (got.offset, got.height, got.width) == (box[:2], box[2], box[3])
        want = R.window(img, off, box)
        assert np.array_equal(got.image, want)
        assert (want != 0).any() == (box[0] < 50)
        # the tile with tile = output is the same operation
        assert np.array_equal(src.tile(box[:2], box[2:], box[:2], box[2:]).image, want)
    # a conversion noted on a device-resident layer runs as the window reads it
    dev = S.Layer._from_device(S.Layer(img, off, True, True)._device(), img.shape, off, True, True).convert(pre_alpha=False)
    assert np.array_equal(dev.window(box[:2], box[2:]).image, R.window(dev.image, off, box))
    empty = S.Layer(img, off, True, True).window((4, 5), (0, 9))
    assert empty.offset == (4, 5) and not empty.image.any()


def test_layer_tile_bad_arguments(S):
    src = S.Layer(_premultiplied((4, 4), 1), (0, 0), True, True)
    with pytest.raises(ValueError):
        src.tile((0, 0), (4, 4), (0, 0), (0, 4))
    with pytest.raises(ValueError):
        src.tile((0, 0), (0, 4), (0, 0), (2, 2))
    ctx = S.Context.get()
    buf, out = src._device(), ctx.alloc(4 * 4 * 32)
    bb = lambda *v: (C.c_int64 * 4)(*v)   # noqa: E731
    tile = lambda *a: ctx.lib.svgr_layer_tile(ctx.handle, *a)   # noqa: E731
    assert tile(out.handle, bb(0, 0, 4, 4), buf.handle, bb(0, 0, 4, 4), bb(0, 0, 2, 2)) == 0
    assert tile(out.handle, bb(0, 0, 4, 4), buf.handle, bb(0, 0, 4, 4), bb(0, 0, 0, 2)) == -1    # an empty tile
    assert tile(out.handle, bb(0, 0, 0, 4), buf.handle, bb(0, 0, 4, 4), bb(0, 0, 2, 2)) == -1    # an empty output
    assert tile(out.handle, bb(0, 0, 4, 5), buf.handle, bb(0, 0, 4, 4), bb(0, 0, 2, 2)) == -1    # out too small
    assert tile(out.handle, bb(0, 0, 4, 4), buf.handle, bb(0, 0, 4, 5), bb(0, 0, 2, 2)) == -1    # src too small
    assert tile(buf.handle, bb(0, 0, 4, 4), buf.handle, bb(0, 0, 4, 4), bb(0, 0, 2, 2)) == -1    # out is src
    assert tile(out.handle, bb(2 ** 30 - 1, 0, 4, 4), buf.handle, bb(0, 0, 4, 4), bb(-(2 ** 30) + 1, 0, 2, 2)) == -1   # beyond 32 bits


# -- documents -------------------------------------------------------------------------------------------------------------------
SVG = ('<svg xmlns="http://www.w3.org/2000/svg" xmlns:xlink="http://www.w3.org/1999/xlink" width="64" height="48">{}</svg>')
REGION = (False, 2.0, 3.0, 58.0, 40.0)
FILTER = '<filter id="f" filterUnits="userSpaceOnUse" x="2" y="3" width="58" height="40" {}>{}</filter>'
SHAPES = '<rect x="8" y="6" width="40" height="30" fill="#3388cc"/><circle cx="40" cy="30" r="10" fill="#cc4400" fill-opacity="0.7"/>'


def _render(S, text, tr):
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        scene, ids, _ = S.svg_scene_from_str(text)
        layer, hull = scene.render(tr, linear_rgb=True)
    return layer, hull, [str(w.message) for w in caught], ids


def _filtered(S, body, tr, attrs=""):
    """The document's render, and the filtered group rendered alone: its layer, hull and straight-alpha linear pixels."""
    got, _, warned, _ = _render(S, SVG.format(FILTER.format(attrs, body) + f'<g filter="url(#f)">{SHAPES}</g>'), tr)
    source, hull, _, _ = _render(S, SVG.format(f"<g>{SHAPES}</g>"), tr)
    return got, warned, source, hull, source.convert(pre_alpha=False, linear_rgb=True).image


def _straight(layer):
    return layer.convert(pre_alpha=False, linear_rgb=True).image


def _check_box(layer, box):
    """The layer is exactly `box`, and something is drawn in it."""
    assert (int(layer.x), int(layer.y), layer.height, layer.width) == tuple(box)
    assert layer.image[..., 3].max() > 0.05


@pytest.mark.parametrize("name", TRANSFORMS)
def test_document_flood_subregion(S, name):
    from svgrasterize_amd import filters as F
    from svgrasterize_amd.svg import _flood_color

    tr = _transforms()[name]
    got, warned, source, hull, src = _filtered(S, '<feFlood x="10.5" y="8" width="20" height="12.25" flood-color="#3080c0" '
                                                  'flood-opacity="0.5"/>', tr)
    assert not warned
    color = _flood_color({"flood-color": "#3080c0", "flood-opacity": "0.5"})
    api = F.Filter.empty(region=REGION).flood(color, REGION).subregion(10.5, 8.0, 20.0, 12.25)(tr, source, hull)
    want, off = R.evaluate([dict(op="flood", color=color, inputs=[], sub=(10.5, 8.0, 20.0, 12.25))], tr, src, source.offset, REGION[1:])
    _check_box(got, (*off, *want.shape[:2]))
    assert np.array_equal(got.image, api.image) and api.offset == got.offset
    assert np.array_equal(got.image, want)
    # exactly the box is flooded: smaller than the filter region, which the flood used to fill
    frame = R.device_box(tr, REGION[1:])
    assert got.height < frame[2] and got.width < frame[3]
    canvas = got.on_canvas(120, 120).image
    inside = np.zeros((120, 120), dtype=bool)
    r0, c0 = max(off[0], 0), max(off[1], 0)
    inside[r0:off[0] + want.shape[0], c0:off[1] + want.shape[1]] = True
    assert (canvas[inside][:, 3] == 0.5).all() and inside.sum() > 100 and not canvas[~inside].any()


@pytest.mark.parametrize("name", TRANSFORMS)
def test_document_offset_cut_at_its_subregion(S, name):
    from svgrasterize_amd import filters as F

    tr = _transforms()[name]
    sub = (12.0, 9.5, 30.0, 22.0)
    got, warned, source, hull, src = _filtered(S, '<feOffset dx="7" dy="-4" x="12" y="9.5" width="30" height="22"/>', tr)
    assert not warned
    api = F.Filter.empty(region=REGION).offset(7.0, -4.0).subregion(*sub)(tr, source, hull)
    want, off = R.evaluate([dict(op="offset", dx=7.0, dy=-4.0, inputs=[1], sub=sub)], tr, src, source.offset, REGION[1:])
    _check_box(got, (*off, *want.shape[:2]))
    assert np.array_equal(got.image, api.image) and api.offset == got.offset
    assert np.array_equal(got.image, want)
    # the uncut offset reaches beyond the box
    whole = F.Filter.empty().offset(7.0, -4.0)(tr, source, hull)
    assert whole.height > got.height or whole.width > got.width


@pytest.mark.parametrize("name", TRANSFORMS)
def test_document_blur_of_a_cut_input(S, name):
    from svgrasterize_amd import filters as F

    tr = _transforms()[name]
    sub = (14.0, 10.0, 24.5, 18.0)
    body = '<feOffset dx="0" dy="0" x="14" y="10" width="24.5" height="18" result="cut"/><feGaussianBlur in="cut" stdDeviation="1.5 2"/>'
    got, warned, source, hull, src = _filtered(S, body, tr)
    assert not warned
    api = F.Filter.empty(region=REGION).offset(0.0, 0.0, None, "cut").subregion(*sub).blur(1.5, 2.0, "cut")(tr, source, hull)
    chain = [dict(op="offset", dx=0.0, dy=0.0, inputs=[1], sub=sub), dict(op="blur", std=(1.5, 2.0), inputs=[2])]
    want, off = R.evaluate(chain, tr, src, source.offset, REGION[1:])
    _check_box(got, (*off, *want.shape[:2]))   # (the blur has its input's subregion: the result is not re-extended)
    assert np.array_equal(got.image, api.image) and api.offset == got.offset
    assert np.abs(got.image - want).max() <= BLUR_TOL
    # the input was transparent outside its box: the blur's edge pixels are darker than those of the uncut source's blur
    uncut, uoff = R.evaluate([dict(op="blur", std=(1.5, 2.0), inputs=[1])], tr, src, source.offset, REGION[1:])
    same = R.window(uncut, uoff, (*off, *want.shape[:2]))
    assert (same[..., 3] - want[..., 3]).max() > 0.05


@pytest.mark.parametrize("name", TRANSFORMS)
def test_document_tile(S, name):
    """The classic: a small subregion of SourceGraphic, moved by feOffset, tiled over the filter region."""
    from svgrasterize_amd import filters as F

    tr = _transforms()[name]
    sub = (30.0, 20.0, 13.0, 11.0)
    body = '<feOffset in="SourceGraphic" dx="2" dy="1" x="30" y="20" width="13" height="11"/><feTile/>'
    got, warned, source, hull, src = _filtered(S, body, tr)
    assert not warned, warned
    api = F.Filter.empty(region=REGION).offset(2.0, 1.0, "SourceGraphic").subregion(*sub).tile()(tr, source, hull)
    chain = [dict(op="offset", dx=2.0, dy=1.0, inputs=[1], sub=sub), dict(op="tile", inputs=[2])]
    want, off = R.evaluate(chain, tr, src, source.offset, REGION[1:])
    frame = R.device_box(tr, REGION[1:])
    _check_box(got, frame)
    assert (tuple(off), want.shape[:2]) == (frame[:2], frame[2:])
    assert np.array_equal(got.image, api.image)
    assert np.array_equal(got.image, want)
    # it repeats: one tile further the same pixels
    (regions, _) = R.resolve(chain, tr, REGION[1:])
    t = regions[0][1]
    assert t[2] < frame[2] and t[3] < frame[3]
    assert np.array_equal(got.image[:-t[2]], got.image[t[2]:]) and np.array_equal(got.image[:, :-t[3]], got.image[:, t[3]:])
    assert len(np.unique(got.image.reshape(-1, 4), axis=0)) > 2   # (the tile holds the rectangle and a part of the circle)


@pytest.mark.parametrize("name", TRANSFORMS)
def test_document_tile_with_its_own_subregion(S, name):
    tr = _transforms()[name]
    body = ('<feFlood flood-color="#ff0000" x="20" y="12" width="4" height="3" result="a"/>'
            '<feFlood flood-color="#0000ff" flood-opacity="0.25" x="24" y="15" width="5" height="4" result="b"/>'
            '<feMerge result="m"><feMergeNode in="a"/><feMergeNode in="b"/></feMerge>'
            '<feOffset in="m" dx="0" dy="0"/><feTile x="5" y="6" width="41" height="33"/>')
    got, warned, source, hull, src = _filtered(S, body, tr)
    assert not warned, warned
    chain = [dict(inputs=[], sub=(20.0, 12.0, 4.0, 3.0)), dict(inputs=[], sub=(24.0, 15.0, 5.0, 4.0)), dict(inputs=[2, 3]),
             dict(inputs=[4]), dict(inputs=[5], sub=(5.0, 6.0, 41.0, 33.0))]
    regions, _ = R.resolve(chain, tr, REGION[1:])
    t, box = regions[3][1], regions[4][1]
    assert t == R.union_boxes([regions[0][1], regions[1][1]])   # (the tile: the union the merge and the offset inherit)
    _check_box(got, box)
    img = got.image
    # the output starts above / left of the tile, and the tile repeats with its own period
    assert box[0] < t[0] and box[1] < t[1]
    assert np.array_equal(img[:-t[2]], img[t[2]:]) and np.array_equal(img[:, :-t[3]], img[:, t[3]:])
    assert (img[..., 3] == 1.0).any() and (img[..., 3] == 0.0).any()


@pytest.mark.parametrize("name", TRANSFORMS)
def test_document_object_bounding_box_units(S, name):
    """primitiveUnits="objectBoundingBox" against the same filter written out in user units (the shapes' box: 8, 6, 42 x 34)."""
    tr = _transforms()[name]
    bx, by, bw, bh = 8.0, 6.0, 42.0, 34.0
    body = ('<feOffset dx="{}" dy="{}" x="{}" y="{}" width="{}" height="{}"/><feGaussianBlur stdDeviation="{} {}"/>'
            '<feMorphology operator="dilate" radius="{} {}"/>')
    frac = (0.05, -0.03, 0.3, 0.2, 0.55, 0.45, 0.03, 0.05, 0.02, 0.03)
    user = tuple(o + f * n for f, o, n in zip(frac, (0, 0, bx, by, 0, 0, 0, 0, 0, 0), (bw, bh, bw, bh, bw, bh, bw, bh, bw, bh)))
    got, warned, source, hull, _ = _filtered(S, body.format(*frac), tr, 'primitiveUnits="objectBoundingBox"')
    assert not warned
    assert np.allclose(hull.bbox(tr), (bx, by, bw, bh), rtol=0, atol=1e-9)
    want, warned, _, _, _ = _filtered(S, body.format(*(repr(u) for u in user)), tr)
    assert not warned
    assert (want.offset, want.height, want.width) == (got.offset, got.height, got.width)
    # (the lengths agree to rounding: the blur's weights and so its result to the blur's tolerance)
    assert np.abs(_straight(got) - _straight(want)).max() <= BLUR_TOL
    assert _straight(got)[..., 3].max() > 0.5
    plain, _, _, _, _ = _filtered(S, body.format(*frac), tr)   # (the same numbers as user units: another picture)
    assert (plain.offset, plain.height, plain.width) != (got.offset, got.height, got.width)


def _picture():
    """A 6 x 9 picture with a gradient, an opaque marker and a transparent corner (made here: no fixture file)."""
    px = np.zeros((6, 9, 4), dtype=np.uint8)
    px[..., 0] = np.linspace(20, 250, 9).astype(np.uint8)[None, :]
    px[..., 1] = np.linspace(240, 30, 6).astype(np.uint8)[:, None]
    px[..., 2], px[..., 3] = 90, 255
    px[1, 2] = (255, 255, 255, 255)
    px[4:, 6:, 3] = 0
    return px


@pytest.mark.parametrize("name", TRANSFORMS)
@pytest.mark.parametrize("par", ["xMidYMid meet", "none"])
@pytest.mark.parametrize("rendering", ["auto", "pixelated"])
def test_document_image_raster(S, name, par, rendering):
    tr = _transforms()[name]
    uri = "data:image/png;base64," + base64.b64encode(S.canvas_to_png(_picture()).getvalue()).decode()
    where = f'x="10" y="8" width="30" height="26" preserveAspectRatio="{par}" image-rendering="{rendering}"'
    got, warned, _, _, _ = _filtered(S, f'<feImage xlink:href="{uri}" {where}/>', tr)
    assert not warned, warned
    want, _, warned, _ = _render(S, SVG.format(f'<image xlink:href="{uri}" {where}/>'), tr)
    assert not warned
    box = R.intersect(R.device_box(tr, (10.0, 8.0, 30.0, 26.0)), R.device_box(tr, REGION[1:]))
    _check_box(got, box)
    a, b = got.on_canvas(120, 120).image, want.on_canvas(120, 120).image
    assert np.abs(a - b).max() <= IMAGE_TOL
    assert b[..., 3].max() > 0.9 and (b[..., 3] > 0.5).sum() > 200


@pytest.mark.parametrize("name", TRANSFORMS)
def test_document_image_element_defined_later(S, name):
    from svgrasterize_amd import filters as F

    tr = _transforms()[name]
    badge = '<g id="badge"><circle cx="30" cy="20" r="9" fill="#22aa44"/><rect x="26" y="10" width="30" height="5" fill="#aa2244"/></g>'
    text = SVG.format(FILTER.format("", '<feImage href="#badge" x="22" y="8" width="25" height="20"/>')
                      + f'<g filter="url(#f)">{SHAPES}</g><defs>{badge}</defs>')
    got, _, warned, ids = _render(S, text, tr)
    assert not warned, warned
    shape, _, _, _ = _render(S, SVG.format(badge), tr)
    source, hull, _, _ = _render(S, SVG.format(f"<g>{SHAPES}</g>"), tr)
    box = R.intersect(R.device_box(tr, (22.0, 8.0, 25.0, 20.0)), R.device_box(tr, REGION[1:]))
    _check_box(got, box)
    want = R.window(shape.image, shape.offset, box)
    assert np.array_equal(got.image, want)
    assert (shape.height > box[2] or shape.width > box[3]) and (want[..., 3] == 1.0).any()   # (it was cut)
    api = F.Filter.empty(region=REGION).image(element="badge", ids=ids).subregion(22.0, 8.0, 25.0, 20.0)(tr, source, hull)
    assert np.array_equal(api.image, got.image) and api.offset == got.offset
    # an unknown id and a non-drawable target: a warning, a transparent result, the chain goes on
    for ref, what in (("#nothing", "no drawable element"), ("#f", "no drawable element")):
        text = SVG.format(FILTER.format("", f'<feImage href="{ref}" result="i"/><feMerge><feMergeNode in="i"/>'
                                            f'<feMergeNode in="SourceGraphic"/></feMerge>') + f'<g filter="url(#f)">{SHAPES}</g>')
        got, _, warned, _ = _render(S, text, tr)
        assert len(warned) == 1 and what in warned[0]
        assert np.abs(got.on_canvas(120, 120).image - source.on_canvas(120, 120).image).max() <= COMPOSE_TOL
        assert source.image[..., 3].max() == 1.0


def test_document_image_of_itself_terminates(S):
    tr = _transforms()["swap"]
    text = SVG.format(FILTER.format("", '<feImage href="#me" result="i"/><feMerge><feMergeNode in="i"/>'
                                        '<feMergeNode in="SourceGraphic"/></feMerge>') + f'<g id="me" filter="url(#f)">{SHAPES}</g>')
    got, _, warned, _ = _render(S, text, tr)
    assert len(warned) == 1 and "this very feImage" in warned[0]
    source, _, _, _ = _render(S, SVG.format(f"<g>{SHAPES}</g>"), tr)
    # the inner feImage is transparent, so the inner render is the shapes; the outer one draws that under the shapes again
    twice = S.Layer.compose([source, source], linear_rgb=True)
    assert np.abs(got.on_canvas(120, 120).image - twice.on_canvas(120, 120).image).max() <= COMPOSE_TOL
    assert got.image[..., 3].max() == 1.0


def test_zero_size_subregion_is_transparent(S):
    tr = _transforms()["swap"]
    body = ('<feFlood flood-color="red" width="0" result="none"/><feMerge><feMergeNode in="none"/><feMergeNode in="SourceGraphic"/>'
            '</feMerge>')
    got, warned, source, _, _ = _filtered(S, body, tr)
    assert not warned
    assert np.abs(got.on_canvas(120, 120).image - source.on_canvas(120, 120).image).max() <= COMPOSE_TOL
    assert source.image[..., 3].max() == 1.0
