"""Stylesheets and document structure on the GPU: a dozen pairs of tests/css_cases.py -- one per construct -- rendered on the device,
the styled document against its plain twin, on the 64 x 64 canvas of the cases.  A scene that is batchable is rendered with
``render_canvas(deterministic=True)`` and must give equal bits; every scene is also drawn by ``Scene.render`` (node by node where
there is a filter, a clip or a gradient) and held to what tests/test_gpu_fullsize.py holds two renders of one scene to: where two
values differ they are neighbouring float32 numbers.  The two pairs whose scene dump needs the device (marker vertices, dashes) are dumped and compared here."""
import io
import struct
import warnings

import numpy as np
import pytest

from tests import css_cases

pytestmark = pytest.mark.gpu

SIZE = 64


@pytest.fixture(scope="module")
def S():
    import svgrasterize_amd as S

    S.Context.get()
    return S


def load(S, name, text, styled=True):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        scene, _ids, _size = S.svg_scene_from_str(text, **(css_cases.OPTIONS.get(name, {}) if styled else {}))
    assert scene is not None
    return scene


def canvases(S, scene):
    """``(batched, walked)``: the canvas of doubles of the deterministic batch (None when the scene is not batchable) and the
    float32 canvas of ``Scene.render``, which takes every node that is not a run of solid fills (filter, clip, gradient) by
    itself."""
    view = S.Transform().matrix(0, 1, 0, 1, 0, 0)   # (render_svg's: x along the columns)
    try:
        batched, _stats = S.render_canvas(scene, view, [0, 0, SIZE, SIZE], linear_rgb=True, out_f64=True, deterministic=True)
    except NotImplementedError:
        batched = None
    out = scene.render(view, viewport=[0, 0, SIZE, SIZE], linear_rgb=True)
    assert out is not None
    return batched, out[0].to_canvas_f32(SIZE, SIZE)


@pytest.fixture(scope="module")
def renders(S):
    """Every pair of the dozen (and the filter pair, which no batch takes), rendered once: name -> (styled, plain)."""
    S.clear_render_cache()
    return {name: (canvases(S, load(S, name, css_cases.BY_NAME[name][0])), canvases(S, load(S, name, css_cases.BY_NAME[name][1], False)))
            for name in css_cases.GPU_DOZEN}


@pytest.mark.parametrize("name", css_cases.GPU_DOZEN)
def test_styled_document_renders_like_its_plain_twin(renders, name):
    (got_batch, got), (want_batch, want) = renders[name]
    assert (got_batch is None) == (want_batch is None) and got.shape == want.shape == (SIZE, SIZE, 4)
    assert got[..., 3].max() > 0.4   # (something is drawn)
    if got_batch is not None:   # one deterministic batch each: equal bits
        assert got_batch.dtype == np.float64 and got_batch[..., 3].max() > 0.4 and np.array_equal(got_batch, want_batch)
    differs = got != want
    print(f"{name}: {'batchable' if got_batch is not None else 'not batchable'}; Scene.render: {int(differs.sum())} differing values")
    assert got.dtype == np.float32
    if differs.any():   # (tests/test_gpu_fullsize.py: neighbouring float32 numbers, never more)
        lo, hi = np.minimum(got[differs], want[differs]), np.maximum(got[differs], want[differs])
        assert (np.nextafter(lo, np.float32(np.inf)) == hi).all(), "the two renders differ by more than one float32 ULP somewhere"


def test_solid_fills_went_as_one_batch(renders):
    assert all(renders[name][0][0] is not None for name in ("important", "display_none_on_a_group", "a_around_a_shape"))


def test_hidden_and_clipped_pixels_are_exactly_zero(renders):
    shown = renders["display_none_on_a_group"][0][1]
    assert (shown[30:50, 30:50] == 0).all()            # the hidden rectangle's box: all four channels
    assert shown[4:24, 4:24, 3].min() > 0.99           # (the rectangle beside it is there)
    sliced = renders["symbol_sliced_xMinYMax"][0][1]   # the <use> viewport is x in [16, 32], y in [24, 32]
    outside = np.ones((SIZE, SIZE), dtype=bool)
    outside[24:32, 16:32] = False
    assert (sliced[outside] == 0).all() and sliced[24:30, 18:30, 3].min() > 0.99


@pytest.mark.parametrize("name", css_cases.NEEDS_DEVICE)
def test_pairs_whose_dump_needs_the_device(S, name):
    from svgrasterize_amd import scenedump

    styled, plain = css_cases.BY_NAME[name]
    got, want = load(S, name, styled), load(S, name, plain, False)
    assert scenedump.compare_dumps(*scenedump.dump_scene(got), *scenedump.dump_scene(want), tol=0.0) == []


def test_render_svg_of_a_symbol_by_id(S):
    """``render_svg(id=...)`` of a symbol: one instance at the origin, on the symbol's own viewport."""
    doc = ('<svg xmlns="http://www.w3.org/2000/svg" width="64" height="64"><symbol id="sym" viewBox="0 0 8 4" width="24" height="12">'
           '<rect x="-2" y="1" width="6" height="2" fill="#06c"/></symbol><rect width="1" height="1"/><g id="gone" display="none"><rect width="9" height="9"/></g></svg>')
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        png = S.render_svg(io.StringIO(doc), id="sym")
        assert S.render_svg(io.StringIO(doc), id="gone") is None
    assert png[:8] == b"\x89PNG\r\n\x1a\n" and struct.unpack(">II", png[16:24]) == (24, 12)
    pixels = S.read_png(png)
    assert pixels.shape == (12, 24, 4)
    # scale 3: the rectangle covers x in [-6, 12], y in [3, 9]; what hangs out on the left is clipped away with the canvas
    assert (pixels[3:9, 0:12, 3] == 255).all() and not pixels[:3].any() and not pixels[9:].any() and not pixels[:, 12:].any()
