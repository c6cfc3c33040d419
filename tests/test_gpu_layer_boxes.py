"""The windows of the layer kernels (csrc/svgr_box.h: box_find, box_meet; layer_px of svgr_hip.hip) through the C ABI where no other
suite puts them: svgr_layer_mix_blend in place with a source that reaches outside `out` (a clipped window) or lies wholly outside
it (no launch), and out of place over a 1-channel backdrop; svgr_layer_lighting and svgr_layer_displacement_map with a source that
covers part of a region wider than one 16 x 16 tile and than 256 pixels.  Each against the restatement its own suite uses."""
import ctypes as C
import zlib

import numpy as np
import pytest

from tests import blend_ref as R
from tests import filter_ref as F
from tests import lighting_ref as LR

pytestmark = pytest.mark.gpu

MODES = ["multiply", "color-burn", "hue"]
B_BOX = (-4, 6, 37, 301)   # (wider than a 256-lane workgroup)


@pytest.fixture(scope="module")
def ctx():
    import svgrasterize_amd as S

    return S.Context.get()


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _bb(b):
    return (C.c_int64 * 4)(*[int(v) for v in b])


def _lib(ctx):
    from svgrasterize_amd import _abi

    return ctx.lib, _abi._check, _abi.ptr


def _poisoned(ctx, n_px, guard):
    """A device buffer of n_px + guard RGBA pixels of NaN: the output of a call and the guard behind it."""
    return ctx.from_host(np.full((n_px + guard, 4), np.nan))


def _output(buf, shape, guard):
    """The output a call left in a `_poisoned` buffer; the guard behind it must be untouched."""
    n_px = int(np.prod(shape[:-1]))
    got = buf.download(shape, np.float64)
    assert np.isnan(buf.download((guard, 4), np.float64, offset=n_px * 32)).all(), "a store behind the output"
    return got


def _premultiplied(rng, shape):
    img = rng.random(tuple(shape) + (4,))
    img[..., :3] *= img[..., 3:]
    return img


def _window(b_box, s_box):
    """The part of the backdrop's image that the source's box covers: (slice of the backdrop, slice of the source)."""
    r0, c0 = max(b_box[0], s_box[0]), max(b_box[1], s_box[1])
    r1, c1 = min(b_box[0] + b_box[2], s_box[0] + s_box[2]), min(b_box[1] + b_box[3], s_box[1] + s_box[3])
    if r1 <= r0 or c1 <= c0:
        return None
    return ((slice(r0 - b_box[0], r1 - b_box[0]), slice(c0 - b_box[1], c1 - b_box[1])),
            (slice(r0 - s_box[0], r1 - s_box[0]), slice(c0 - s_box[1], c1 - s_box[1])))


@pytest.mark.parametrize("name", MODES)
@pytest.mark.parametrize("s_box", [(30, 290, 20, 40), (-9, -3, 12, 17), (-10, 100, 60, 5)], ids=["below_right", "above_left", "a_column_through"])
def test_mix_blend_in_place_with_a_clipped_window(ctx, name, s_box):
    """The source reaches outside the backdrop: what lies under both is blended, the rest of the backdrop keeps its bytes."""
    import svgrasterize_amd as S

    lib, check, ptr = _lib(ctx)
    rng = _rng("clipped" + name)
    b_img, s_img = _premultiplied(rng, B_BOX[2:]), _premultiplied(rng, s_box[2:])
    acc, src = ctx.from_host(b_img), ctx.from_host(s_img)
    n0 = ctx.launches()
    check(lib.svgr_layer_mix_blend(ctx.handle, acc.handle, _bb(B_BOX), acc.handle, _bb(B_BOX), 4, src.handle, _bb(s_box), 4, S.BLEND_MODES[name]))
    assert ctx.launches() - n0 == 1
    got = acc.download(b_img.shape, np.float64)
    wb, ws = _window(B_BOX, s_box)
    want = b_img.copy()
    want[wb] = R.mix_blend_px(name, b_img[wb], s_img[ws])
    outside = np.ones(B_BOX[2:], dtype=bool)
    outside[wb] = False
    assert 0 < (~outside).sum() < s_box[2] * s_box[3]   # (clipped, and not to nothing)
    assert np.array_equal(got[outside], b_img[outside])
    err = float(np.abs(got - want).max())
    print(f"in place, clipped, {name}: max |err| {err:.3e}, bound 1e-12")
    assert err <= 1e-12   # tests/test_gpu_blend.py: the bound of every mode against this restatement
    assert np.array_equal(src.download(s_img.shape, np.float64), s_img)


@pytest.mark.parametrize("s_box", [(40, 10, 6, 9), (-4, 307, 37, 5), (-30, -30, 26, 36), (0, 20, 0, 7)],
                         ids=["below", "right_touching", "corner_touching", "empty"])
def test_mix_blend_in_place_with_the_source_outside(ctx, s_box):
    """Nothing of the source lies over the backdrop: no launch, and `out` keeps its bytes."""
    import svgrasterize_amd as S

    lib, check, ptr = _lib(ctx)
    rng = _rng("outside")
    b_img, s_img = _premultiplied(rng, B_BOX[2:]), _premultiplied(rng, (max(s_box[2], 1), max(s_box[3], 1)))
    assert _window(B_BOX, s_box) is None
    acc, src = ctx.from_host(b_img), ctx.from_host(s_img)
    n0 = ctx.launches()
    check(lib.svgr_layer_mix_blend(ctx.handle, acc.handle, _bb(B_BOX), acc.handle, _bb(B_BOX), 4, src.handle, _bb(s_box), 4, S.BLEND_MODES["multiply"]))
    assert ctx.launches() == n0
    assert acc.download(b_img.shape, np.float64).tobytes() == b_img.tobytes()


@pytest.mark.parametrize("name", MODES)
@pytest.mark.parametrize("sch", [4, 1])
def test_mix_blend_over_a_one_channel_backdrop(ctx, name, sch):
    """Out of place over the union of the boxes: a 1-channel backdrop is alpha broadcast to all four, like a 1-channel source."""
    import svgrasterize_amd as S

    lib, check, ptr = _lib(ctx)
    rng = _rng(f"b1 {name} {sch}")
    s_box = (20, -30, 30, 280)
    b_img = rng.random(B_BOX[2:] + (1,))
    s_img = _premultiplied(rng, s_box[2:]) if sch == 4 else rng.random(s_box[2:] + (1,))
    want, off = R.mix_blend_layers(name, b_img, B_BOX[:2], s_img, s_box[:2])
    union = off + want.shape[:2]
    back, src = ctx.from_host(b_img), ctx.from_host(s_img)
    guard = union[3] + 1
    out = _poisoned(ctx, union[2] * union[3], guard)
    check(lib.svgr_layer_mix_blend(ctx.handle, out.handle, _bb(union), back.handle, _bb(B_BOX), 1, src.handle, _bb(s_box), sch, S.BLEND_MODES[name]))
    got = _output(out, want.shape, guard)
    err = float(np.abs(got - want).max())
    print(f"1-channel backdrop, {sch}-channel source, {name}: max |err| {err:.3e}, bound 1e-12")
    assert err <= 1e-12   # tests/test_gpu_blend.py
    only_b = (slice(0, 20 - B_BOX[0]), slice(0, B_BOX[3]))   # (rows of the backdrop above the source: alpha in all four channels)
    r0, c0 = B_BOX[0] - off[0], B_BOX[1] - off[1]
    assert np.array_equal(got[r0:r0 + only_b[0].stop, c0:c0 + B_BOX[3]], np.repeat(b_img[only_b], 4, axis=2))
    assert np.array_equal(back.download(b_img.shape, np.float64), b_img) and np.array_equal(src.download(s_img.shape, np.float64), s_img)


REGION = (-4, 7, 20, 300)   # two tile rows (the second of four rows), nineteen tile columns, more than 256 pixels wide
# the source over the region's lower right part, its upper left part, and a band through its middle that starts and ends inside
PARTIAL_SOURCES = {"lower_right": (5, 140, 40, 400), "upper_left": (-30, -50, 36, 200), "band": (2, 100, 9, 177)}


@pytest.mark.parametrize("specular", [False, True])
@pytest.mark.parametrize("which", list(PARTIAL_SOURCES))
def test_lighting_of_a_source_over_part_of_a_wide_region(ctx, which, specular):
    lib, check, ptr = _lib(ctx)
    src_box = PARTIAL_SOURCES[which]
    img = _rng("light " + which).random(src_box[2:] + (4,))
    params = np.array([9.5, 130.25, 21.0, 0.0, 0.0, 0.0, 3.0, 0.55])
    d = np.array([8.0, 150.0, 0.0]) - params[0:3]   # (points into the region)
    params[3:6] = d / np.sqrt((d * d).sum())
    color = np.array([0.95, 0.7, 0.35])
    src = ctx.from_host(img)
    offset, shape = REGION[:2], REGION[2:]
    guard = shape[1] + 1
    out = _poisoned(ctx, shape[0] * shape[1], guard)
    check(lib.svgr_layer_lighting(ctx.handle, out.handle, _bb(REGION), src.handle, _bb(src_box), LR.SPOT, ptr(params), ptr(color), 2.0, 0.9,
                                  17.0 if specular else 1.0, int(specular)))
    got = _output(out, shape + (4,), guard)
    A = LR.region_alpha(img, src_box[:2], offset, shape)
    assert 0.1 < (A != 0).mean() < 0.9   # (part of the region)
    ref = LR.lighting(A, offset, LR.SPOT, params, color, 2.0, 0.9, 17.0 if specular else None)
    err = float(np.abs(got - ref).max())
    print(f"lighting {which} specular {specular}: max |err| {err:.3e}, bound 1e-13")
    assert err <= 1e-13   # tests/test_gpu_filter_paint_seams.py: test_lighting_at_tile_ends
    assert got[..., :3].max() > 0.01
    assert np.array_equal(src.download(img.shape, np.float64), img)


@pytest.mark.parametrize("which", list(PARTIAL_SOURCES))
def test_displacement_map_of_a_source_over_part_of_a_wide_map(ctx, which):
    """A copy of source pixels, transparent where the displaced point leaves the source: bit for bit, at points that keep
    tests/image_cases.py's clearance from every pixel edge."""
    from tests import image_cases as IC

    lib, check, ptr = _lib(ctx)
    src_box = PARTIAL_SOURCES[which]
    rng = _rng("dm " + which)
    src = _premultiplied(rng, src_box[2:])
    disp = rng.random(REGION[2:] + (4,))
    lin, scale = IC.ROT, 6.5
    xc, yc = IC.DM_CHANNELS
    args = (disp, REGION[:2], lin, scale, xc, yc)
    near = F.displacement_clearance(src_box[2:], src_box[:2], *args) < IC.CLEARANCE
    assert not near   # (no displaced point within rounding distance of a pixel edge: the seeded map keeps clear)
    sbuf, dbuf = ctx.from_host(src), ctx.from_host(disp)
    rows, cols = REGION[2:]
    guard = cols + 1
    out = _poisoned(ctx, rows * cols, guard)
    check(lib.svgr_layer_displacement_map(ctx.handle, out.handle, _bb(REGION), dbuf.handle, sbuf.handle, _bb(src_box),
                                          ptr(np.ascontiguousarray(lin, dtype=np.float64).reshape(4)), scale, xc, yc))
    got = _output(out, (rows, cols, 4), guard)
    want = F.displacement_map_wide(src, src_box[:2], *args)
    assert np.array_equal(got, want), np.argwhere((got != want).any(axis=-1))[:3].tolist()
    lit = want.any(axis=-1).mean()
    assert 0.1 < lit < 0.9   # (part of the map reads the source, part falls outside it)
    assert np.array_equal(sbuf.download(src.shape, np.float64), src) and np.array_equal(dbuf.download(disp.shape, np.float64), disp)
