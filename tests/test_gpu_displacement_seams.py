"""k_layer_displacement_map through the C ABI on the cases of tests/image_cases.py: maps of 255 / 256 / 257 / 300 pixels (one
block, its end, one lane more), map boxes entirely off each side of the source, a 1 x 1 source, no displacement (scale 0, map
values of exactly 0.5), displacements of 1e300 and infinity, NaN in the map, all sixteen channel pairs on the smallest case;
through Layer.displacement_map a premultiplied map with alpha 0 / 5e-5 / 1e-3 pixels; and one document.  The output is a copy
of source pixels: compared bit for bit with filter_ref.displacement_map_wide (long-double displaced points), which
tests/test_image_cases_host.py shows to keep IC.CLEARANCE from every pixel edge.  Outputs are poisoned with NaN and end in a
guard that must stay NaN."""
import warnings

import numpy as np
import pytest

from tests import filter_ref as F
from tests import image_cases as IC
from tests import layer_ref as LR
from tests.test_gpu_filter_paint_seams import _bb, _lib, _output, _poisoned

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import svgrasterize_amd as S

    return S.Context.get()


def _run(ctx, case, src, disp, xc, yc):
    lib, check, ptr = _lib(ctx)
    rows, cols = case.map_shape
    sbuf, dbuf = ctx.from_host(src), ctx.from_host(disp)
    guard = cols + 1
    out = _poisoned(ctx, rows * cols, guard)
    lin = np.ascontiguousarray(case.lin, dtype=np.float64).reshape(4)
    check(lib.svgr_layer_displacement_map(ctx.handle, out.handle, _bb(case.map_off + case.map_shape), dbuf.handle, sbuf.handle,
                                          _bb(case.src_off + case.src_shape), ptr(lin), float(case.scale), xc, yc))
    got = _output(out, (rows, cols, 4), guard)
    assert not np.isnan(got).any(), "map pixels never written"
    assert np.array_equal(sbuf.download(src.shape, np.float64), src)
    assert np.array_equal(dbuf.download(disp.shape, np.float64), disp, equal_nan=True)
    return got


@pytest.mark.parametrize("case", IC.DM_CASES, ids=lambda c: c.name)
def test_displacement_map_bit_for_bit(ctx, case):
    src, disp = IC.dm_inputs(case)
    xc, yc = IC.DM_CHANNELS
    got = _run(ctx, case, src, disp, xc, yc)
    want = F.displacement_map_wide(src, case.src_off, disp, case.map_off, case.lin, case.scale, xc, yc)
    assert np.array_equal(got, want), np.argwhere((got != want).any(axis=-1))[:3].tolist()
    assert want.any() == (case.route == "on")


def test_displacement_map_all_channel_pairs(ctx):
    case = IC.DM_CASES[0]
    assert case.name == "dm_smallest"
    src, disp = IC.dm_inputs(case)
    seen = set()
    for xc in range(4):
        for yc in range(4):
            got = _run(ctx, case, src, disp, xc, yc)
            args = (disp, case.map_off, case.lin, case.scale, xc, yc)
            assert F.displacement_clearance(case.src_shape, case.src_off, *args) >= IC.CLEARANCE
            want = F.displacement_map_wide(src, case.src_off, *args)
            assert np.array_equal(got, want), (xc, yc)
            seen.add(want.tobytes())
    assert len(seen) == 16   # (every pair moves the pixels its own way)


def _rotated():
    from svgrasterize_amd.geometry import Transform

    return Transform().matrix(0, 1, 0, 1, 0, 0).translate(20, 10).rotate(0.7).scale(1.25, 0.8)


def test_premultiplied_map_with_transparent_pixels(ctx):
    """Layer.displacement_map converts a premultiplied map to straight alpha first: a pixel of alpha <= 1e-4 keeps its colour
    as it is (alpha 0 and 5e-5 here), one of alpha 1e-3 is divided.  The expected map is layer_ref's convert rule."""
    import svgrasterize_amd as S

    tr = _rotated()
    lin = np.asarray(tr.m, dtype=np.float64)[:2, :2]
    rng = np.random.default_rng(9)
    src = rng.random((14, 50, 4))
    src[..., :3] *= src[..., 3:]
    pre = IC.dm_premultiplied_map()
    straight = LR.convert(pre, LR.PRE_TO_STRAIGHT)[0].astype(np.float64)
    a = S.Layer(src, (-6, 3), pre_alpha=True, linear_rgb=True)
    m = S.Layer(pre, (-5, 5), pre_alpha=True, linear_rgb=True)
    args = (straight, (-5, 5), lin, 9.5, 0, 1)   # (9.5 pixels a unit: a colour wrongly divided, or wrongly kept, moves by pixels)
    assert F.displacement_clearance(src.shape[:2], (-6, 3), *args) >= IC.CLEARANCE
    got = a.displacement_map(m, tr, 9.5, "R", "G")
    assert (got.offset, got.pre_alpha, got.image.shape) == ((-5, 5), True, pre.shape)
    want = F.displacement_map_wide(src, (-6, 3), *args)
    assert np.array_equal(got.image, want), np.argwhere((got.image != want).any(axis=-1))[:3].tolist()
    for alpha in (0.0, 5e-5, 1e-3):
        assert want[pre[..., 3] == alpha].any()
    # the rule matters: with every pixel divided, or none, other source pixels would be read
    wrong = pre.copy()
    wrong[..., :3] = np.clip(pre[..., :3] / np.maximum(pre[..., 3:], 1e-300), 0, 1)
    assert not np.array_equal(F.displacement_map_wide(src, (-6, 3), wrong, *args[1:]), want)
    assert not np.array_equal(F.displacement_map_wide(src, (-6, 3), np.clip(pre, 0, 1), *args[1:]), want)


DOC = ('<svg xmlns="http://www.w3.org/2000/svg" width="64" height="48">'
       '<filter id="f" filterUnits="userSpaceOnUse" x="2" y="3" width="58" height="40">'
       '<feTurbulence type="fractalNoise" baseFrequency="0.05 0.08" numOctaves="2" seed="3" result="noise"/>'
       '<feDisplacementMap in="noise" in2="SourceGraphic" scale="8" xChannelSelector="R" yChannelSelector="A"/></filter>'
       '{}</svg>')
SHAPE = '<circle cx="30" cy="22" r="12.3" fill="#cc4400" fill-opacity="0.5"/>'


def test_document_with_a_semi_transparent_map_over_nothing(ctx):
    """feDisplacementMap whose map (in2 = SourceGraphic) is a half-transparent circle over nothing: alpha 0 around it, small
    alphas on its anti-aliased edge.  The document against the same two Layer calls, and those against the references."""
    import svgrasterize_amd as S
    from svgrasterize_amd import filters as FL

    tr = S.Transform().matrix(0, 1, 0, 1, 0, 0)

    def render(text):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            scene, _, _ = S.svg_scene_from_str(text)
            return scene.render(tr, linear_rgb=True)[0]

    got = render(DOC.format(f'<g filter="url(#f)">{SHAPE}</g>'))
    source = render(DOC.format(f"<g>{SHAPE}</g>"))
    offset, shape, _ = FL.filter_region((False, 2.0, 3.0, 58.0, 40.0), tr, source)
    noise = S.Layer.turbulence(tr, offset, shape, (0.05, 0.08), 2, 3.0, None, True)
    moved = noise.displacement_map(source.convert(pre_alpha=False, linear_rgb=True), tr, 8.0, "R", "A")
    a, b = got.on_canvas(48, 64).image, moved.on_canvas(48, 64).image
    assert np.array_equal(a, b) and a[..., 3].max() > 0.1
    # the Layer call against the references: the map made straight by layer_ref's rule, the noise premultiplied by it
    pre = source.convert(pre_alpha=True, linear_rgb=True)
    straight = LR.convert(pre.image, LR.PRE_TO_STRAIGHT)[0].astype(np.float64)
    assert (straight[..., 3] == 0).any() and ((straight[..., 3] > 0) & (straight[..., 3] < 0.4)).any()
    src_wide, tol = LR.convert(noise.image, LR.STRAIGHT_TO_PRE)
    lin = np.asarray(tr.m, dtype=np.float64)[:2, :2]
    args = (straight, pre.offset, lin, 8.0, 0, 3)
    assert F.displacement_clearance(noise.image.shape[:2], noise.offset, *args) >= IC.CLEARANCE
    want = F.displacement_map_wide(src_wide.astype(np.float64), noise.offset, *args)
    bound = float(np.max(tol))   # (a copy of premultiplied noise: layer_ref's tolerance of that product)
    err = float(np.abs(moved.image - want).max())
    print(f"document, displacement by a half-transparent map: max |err| {err:.3e}, bound {bound:.3e}")
    assert moved.offset == pre.offset and err <= bound and want.any()
