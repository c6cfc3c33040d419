"""mix-blend-mode on the device: Layer.mix_blend (svgr_layer_mix_blend, k_layer_mix_blend) against the host build of
csrc/svgr_core.h and the numpy restatement (tests/blend_ref.py) for every mode, on offset, overlapping, nested and disjoint
extents, 1- and 4-channel sources and both colour spaces, in place and out of place; and documents through the loader and
Scene.render against the same layers rendered without the blend and blended on the host."""
import ctypes as C
import warnings

import numpy as np
import pytest

from tests import blend_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import svgrasterize_amd as S

    S.Context.get()
    return S


@pytest.fixture(scope="module")
def bh():
    return R.harness()


def _premul(rng, shape, ch=4):
    img = rng.random(shape + (ch,))
    if ch == 4:
        img[..., 3] = np.where(rng.random(shape) < 0.15, 0.0, np.where(rng.random(shape) < 0.2, 1.0, img[..., 3]))
        img[..., :3] *= img[..., 3:4]
    return img


def _dev_layer(S, img, offset, linear_rgb=False, pre_alpha=True):
    ctx = S.Context.get()
    buf = ctx.from_host(np.ascontiguousarray(img, dtype=np.float64))
    return S.Layer._from_device(buf, img.shape, offset, pre_alpha, linear_rgb)


def _bytes(layer):
    return layer._dev.download(layer._shape, np.float64).tobytes()


# (backdrop offset, shape), (source offset, shape): offset, partly overlapping, source inside, backdrop inside, disjoint
PLACEMENTS = [
    (((0, 0), (23, 31)), ((0, 0), (23, 31))),
    (((3, -4), (19, 26)), ((-6, 9), (17, 21))),
    (((-5, 2), (40, 33)), ((4, 7), (9, 13))),
    (((8, 8), (5, 7)), ((0, 1), (29, 22))),
    (((0, 0), (11, 12)), ((20, -30), (6, 9))),
]


@pytest.mark.parametrize("name", R.MODES)
def test_layer_mix_blend_matches_host(S, bh, name):
    rng = np.random.default_rng(R.CODE[name] + 1)
    mode = S.BLEND_MODES[name]
    for (bo, bs), (so, ss) in PLACEMENTS:
        for sch in (4, 1):
            b_img, s_img = _premul(rng, bs), _premul(rng, ss, sch)
            b, s = _dev_layer(S, b_img, bo), _dev_layer(S, s_img, so)
            before = _bytes(b), _bytes(s)
            got = S.Layer.mix_blend(b, s, mode)
            assert (_bytes(b), _bytes(s)) == before   # the inputs are left as they are
            want, off = R.mix_blend_layers(name, b_img, bo, s_img, so)
            host, off_h = R.mix_blend_layers(name, b_img, bo, s_img, so, px=lambda m, d, x: R.harness_px(bh, m, d, x))
            assert got.offset == off == off_h and got.image.shape == want.shape   # the union of the extents
            assert got.pre_alpha and not got.linear_rgb
            assert np.array_equal(host, want)
            err = np.abs(got.image - want).max()
            assert err <= 1e-12, (name, bo, so, sch, err)


@pytest.mark.parametrize("name", ["multiply", "soft-light", "color-dodge", "hue", "luminosity"])
def test_layer_mix_blend_colour_spaces(S, name):
    """Straight-alpha sRGB inputs blended in linearRGB and in sRGB: each converted as compose converts it, then blended."""
    rng = np.random.default_rng(3)
    b_img, s_img = rng.random((17, 19, 4)), rng.random((13, 11, 4))
    for lin in (False, True):
        b = _dev_layer(S, b_img, (2, -3), linear_rgb=False, pre_alpha=False)
        s = _dev_layer(S, s_img, (5, 1), linear_rgb=False, pre_alpha=False)
        got = S.Layer.mix_blend(b, s, S.BLEND_MODES[name], linear_rgb=lin)
        assert got.linear_rgb == lin and got.pre_alpha
        bc = b.convert(pre_alpha=True, linear_rgb=lin).image
        sc = s.convert(pre_alpha=True, linear_rgb=lin).image
        want, off = R.mix_blend_layers(name, bc, (2, -3), sc, (5, 1))
        assert got.offset == off and np.abs(got.image - want).max() <= 1e-12, (name, lin)


@pytest.mark.parametrize("name", ["multiply", "overlay", "color-burn", "difference", "saturation", "color"])
def test_layer_mix_blend_in_place(S, bh, name):
    """A backdrop the caller owns and a source inside it: the blend runs over the source's rectangle in the backdrop's buffer;
    everything outside the source keeps its bytes."""
    rng = np.random.default_rng(8)
    b_img, s_img = _premul(rng, (37, 41)), _premul(rng, (12, 17))
    b = _dev_layer(S, b_img, (-4, 6))
    s = _dev_layer(S, s_img, (3, 10))
    s_before = _bytes(s)
    got = S.Layer.mix_blend(b, s, S.BLEND_MODES[name], reuse_backdrop=True)
    assert got._dev is b._dev and got.offset == (-4, 6) and got._shape == (37, 41, 4)
    want, off = R.mix_blend_layers(name, b_img, (-4, 6), s_img, (3, 10), px=lambda m, d, x: R.harness_px(bh, m, d, x))
    assert off == (-4, 6) and np.abs(got.image - want).max() <= 1e-12
    out = got.image
    mask = np.ones((37, 41), dtype=bool)
    mask[7:19, 4:21] = False
    assert np.array_equal(out[mask], b_img[mask]) and _bytes(s) == s_before
    # a source reaching outside the backdrop: a fresh layer over the union, the backdrop untouched
    b2 = _dev_layer(S, b_img, (-4, 6))
    s2 = _dev_layer(S, s_img, (30, 40))
    before = _bytes(b2)
    got2 = S.Layer.mix_blend(b2, s2, S.BLEND_MODES[name], reuse_backdrop=True)
    assert got2._dev is not b2._dev and _bytes(b2) == before
    want2, off2 = R.mix_blend_layers(name, b_img, (-4, 6), s_img, (30, 40))
    assert got2.offset == off2 and np.abs(got2.image - want2).max() <= 1e-12


def test_normal_is_compose_over_bit_for_bit(S):
    rng = np.random.default_rng(12)
    for (bo, bs), (so, ss) in PLACEMENTS:
        for sch in (4, 1):
            b_img, s_img = _premul(rng, bs), _premul(rng, ss, sch)
            b, s = _dev_layer(S, b_img, bo), _dev_layer(S, s_img, so)
            got = S.Layer.mix_blend(b, s, S.BLEND_MODES["normal"])
            over = S.Layer.compose([b, s], S.COMPOSE_OVER)
            assert got.offset == over.offset and np.array_equal(got.image, over.image)


def test_none_inputs_and_bad_modes(S):
    rng = np.random.default_rng(1)
    b = _dev_layer(S, _premul(rng, (4, 5)), (0, 0))
    assert S.Layer.mix_blend(None, b, 1) is b and S.Layer.mix_blend(b, None, 1) is b
    with pytest.raises(ValueError):
        S.Layer.mix_blend(b, b, 16)
    ctx = S.Context.get()
    bb = (C.c_int64 * 4)(0, 0, 4, 5)
    out = ctx.alloc(4 * 5 * 32)
    buf = b._device()
    for mode in (-1, 16):
        assert ctx.lib.svgr_layer_mix_blend(ctx.handle, out.handle, bb, buf.handle, bb, 4, buf.handle, bb, 4, mode) == -1
    bad = (C.c_int64 * 4)(0, 0, -1, 5)
    assert ctx.lib.svgr_layer_mix_blend(ctx.handle, out.handle, bb, buf.handle, bad, 4, buf.handle, bb, 4, 1) == -1
    assert ctx.lib.svgr_layer_mix_blend(ctx.handle, out.handle, bb, buf.handle, bb, 4, out.handle, bb, 4, 1) == -1   # src is out
    small = (C.c_int64 * 4)(0, 0, 3, 5)
    assert ctx.lib.svgr_layer_mix_blend(ctx.handle, out.handle, bb, out.handle, small, 4, buf.handle, bb, 4, 1) == -1   # in place, other box
    ctx.sync()


# -- documents -------------------------------------------------------------------------------------------------------------
W, H = 48, 40
DEFS = ('<defs><linearGradient id="grad" x1="0" y1="0" x2="1" y2="1"><stop offset="0" stop-color="#1040a0"/>'
        '<stop offset="0.6" stop-color="#f0c020"/><stop offset="1" stop-color="#30c070" stop-opacity="0.7"/></linearGradient></defs>')
BACKDROPS = {
    "gradient": '<rect x="2" y="3" width="40" height="33" fill="url(#grad)"/>',
    "solid": '<rect x="2" y="3" width="40" height="33" fill="#c04080" fill-opacity="0.8"/>',
}
SOURCE = '<circle cx="28" cy="20" r="14" fill="#3080ff" fill-opacity="0.85"{attr}/><rect x="5" y="25" width="30" height="12" fill="#ffe060"{attr}/>'


def _doc(body):
    return f'<svg xmlns="http://www.w3.org/2000/svg" width="{W}" height="{H}">{DEFS}{body}</svg>'


def _render(S, body, linear_rgb=False):
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        scene, _ids, _size = S.svg_scene_from_str(_doc(body))
    view = S.Transform().matrix(0, 1, 0, 1, 0, 0)
    res = scene.render(view, viewport=[0, 0, H, W], linear_rgb=linear_rgb)
    assert res is not None
    layer = res[0].convert(pre_alpha=True, linear_rgb=linear_rgb)
    return layer.image, layer.offset


def _canvas(img, off):
    out = np.zeros((H, W, 4))
    img = np.repeat(img, 4, axis=2) if img.shape[2] == 1 else img
    r0, c0 = max(off[0], 0), max(off[1], 0)
    r1, c1 = min(off[0] + img.shape[0], H), min(off[1] + img.shape[1], W)
    out[r0:r1, c0:c1] = img[r0 - off[0]:r1 - off[0], c0 - off[1]:c1 - off[1]]
    return out


def _host_chain(S, back, sources, linear_rgb=False):
    """`back` rendered alone, then each (body, mode) of `sources` rendered alone and blended on the host."""
    acc, off = _render(S, back, linear_rgb)
    for body, mode in sources:
        img, soff = _render(S, body, linear_rgb)
        acc, off = R.mix_blend_layers(mode, acc, off, img, soff)
    return _canvas(acc, off)


@pytest.mark.parametrize("backdrop", sorted(BACKDROPS))
@pytest.mark.parametrize("name", ["multiply", "screen", "difference", "color"])
def test_document_blend_matches_host(S, backdrop, name):
    back = BACKDROPS[backdrop]
    src = f'<g>{SOURCE.format(attr="")}</g>'
    got = _canvas(*_render(S, back + f'<g style="mix-blend-mode:{name}">{SOURCE.format(attr="")}</g>'))
    want = _host_chain(S, back, [(src, name)])
    assert np.abs(got - want).max() <= 1e-12, name
    over = _canvas(*_render(S, back + src))
    assert np.abs(got - over).max() > 0.05   # the blend is not source-over


def test_document_multiply_is_not_over(S):
    back = BACKDROPS["solid"]
    rect = '<rect x="10" y="10" width="20" height="20" fill="#4080c0"{attr}/>'
    got = _canvas(*_render(S, back + rect.format(attr=' mix-blend-mode="multiply"')))
    over = _canvas(*_render(S, back + rect.format(attr="")))
    # inside the square: multiply of #4080c0 with 0.8 * #c04080 over nothing, against the opaque square of source-over
    assert np.abs(got[20, 20] - over[20, 20]).max() > 0.2
    want = _host_chain(S, back, [(rect.format(attr=""), "multiply")])
    assert np.abs(got - want).max() <= 1e-12


def test_blend_inside_plain_group_sees_outside(S):
    back = BACKDROPS["gradient"]
    inner = SOURCE.format(attr=' style="mix-blend-mode:screen"')
    got = _canvas(*_render(S, back + f'<g><g>{inner}</g></g>'))
    # the two shapes blend one after the other with everything drawn before them, the backdrop outside the <g> included
    circle, rect = SOURCE.split("/>", 1)
    want = _host_chain(S, back, [(circle.format(attr="") + "/>", "screen"), (rect.format(attr=""), "screen")])
    assert np.abs(got - want).max() <= 1e-12


@pytest.mark.parametrize("wrapper", ['<g style="isolation:isolate">', '<g opacity=".9">'])
def test_blend_inside_isolated_group_does_not(S, wrapper):
    back = BACKDROPS["gradient"]
    blended = _canvas(*_render(S, back + wrapper + SOURCE.format(attr=' mix-blend-mode="multiply"') + "</g>"))
    plain = _canvas(*_render(S, back + wrapper + SOURCE.format(attr="") + "</g>"))
    # the circle blends with nothing (first in its group); the rect with the circle alone, inside the group
    circle, rect = SOURCE.split("/>", 1)
    inner = _host_chain(S, circle.format(attr="") + "/>", [(rect.format(attr=""), "multiply")])
    group_plain = _canvas(*_render(S, SOURCE.format(attr="")))
    assert np.abs(blended - plain).max() > 0.05   # the rect does blend with the circle
    # and nothing inside blends with the backdrop: the group over it is source-over
    base = _canvas(*_render(S, back))
    op = 0.9 if "opacity" in wrapper else 1.0
    want = inner * op + base * (1.0 - inner[..., 3:4] * op)
    assert np.abs(blended - want).max() <= 1e-12
    assert np.abs(plain - (group_plain * op + base * (1.0 - group_plain[..., 3:4] * op))).max() <= 1e-12


def test_several_blended_siblings(S):
    back = BACKDROPS["gradient"]
    shapes = [('<rect x="4" y="4" width="20" height="20" fill="#ff8040"{attr}/>', "multiply"),
              ('<circle cx="24" cy="22" r="12" fill="#40a0ff" fill-opacity="0.6"{attr}/>', "soft-light"),
              ('<rect x="18" y="8" width="26" height="10" fill="#80ff80"{attr}/>', "difference"),
              ('<rect x="1" y="1" width="46" height="38" fill="#602080" fill-opacity="0.5"{attr}/>', "hue"),
              ('<rect x="30" y="26" width="6" height="6" fill="#ffffff"{attr}/>', "exclusion")]
    body = back + "".join(s.format(attr=f' mix-blend-mode="{m}"') for s, m in shapes)
    got = _canvas(*_render(S, body))
    want = _host_chain(S, back, [(s.format(attr=""), m) for s, m in shapes])
    assert np.abs(got - want).max() <= 1e-12


def test_linear_rgb_document(S):
    back = BACKDROPS["gradient"]
    body = back + SOURCE.format(attr=' mix-blend-mode="overlay"')
    got = _canvas(*_render(S, body, linear_rgb=True))
    circle, rect = SOURCE.split("/>", 1)
    want = _host_chain(S, back, [(circle.format(attr="") + "/>", "overlay"), (rect.format(attr=""), "overlay")], linear_rgb=True)
    assert np.abs(got - want).max() <= 1e-12
    srgb = _canvas(*_render(S, body))
    assert np.abs(got - srgb).max() > 1e-3   # (blending in linearRGB is not blending in sRGB)


def test_row_strips_match_the_full_render(S):
    """Blending is per pixel: rendering the document's rows in strips (each render's viewport a band of rows) gives the rows of
    the one-viewport render."""
    body = BACKDROPS["gradient"] + SOURCE.format(attr=' mix-blend-mode="color-burn"') + \
        '<rect x="8" y="6" width="30" height="28" fill="#20c0a0" fill-opacity="0.6" mix-blend-mode="saturation"/>'
    scene, _ids, _size = S.svg_scene_from_str(_doc(body))
    view = S.Transform().matrix(0, 1, 0, 1, 0, 0)
    full = scene.render(view, viewport=[0, 0, H, W])[0].convert(pre_alpha=True, linear_rgb=False)
    full = _canvas(full.image, full.offset)
    for r0, r1 in ((0, 16), (16, 32), (32, H)):
        res = scene.render(view, viewport=[r0, 0, r1 - r0, W])
        part = res[0].convert(pre_alpha=True, linear_rgb=False)
        part = _canvas(part.image, part.offset)
        assert np.abs(part[r0:r1] - full[r0:r1]).max() <= 1e-12, (r0, r1)
