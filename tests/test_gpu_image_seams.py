"""k_image_fill, k_image_prepare and k_image_downsample through the C ABI at their coordinate edges, on the cases of
tests/image_cases.py: boxes that end on, before and behind the 32 x 8 tile, the row-stride loop's second trip, integer and
clamped levels of detail, images one texel wide or tall, boxes far larger than the image, translations of 1e300 and NaN /
infinite maps.  A smooth fill is compared with the long-double sample of the device's own mip chain at
image_ref.fill_tolerance (derived there), nearest sampling and every case with exact coordinates bit for bit; the chain is
checked on its own.  Outputs are poisoned with NaN and end in a guard that must stay NaN.  What the cases rely on -- that no
index leaves a level for any coordinate, clearances, routes -- is shown on the host by tests/test_image_cases_host.py."""
import base64
import ctypes as C

import numpy as np
import pytest

from tests import image_cases as IC
from tests import image_ref as R
from tests.test_gpu_filter_paint_seams import _bb, _output, _poisoned
from tests.util import ulp_f32

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import svgrasterize_amd as S

    return S.Context.get()


def _chain(buf, shape):
    """The device's mip chain of an (h, w) image as a list of float32 (lh, lw, 4) levels."""
    from svgrasterize_amd import _abi

    layout = _abi.image_levels(*shape)
    flat = buf.download((layout[-1][0] + 1, 4), np.float32)
    return [flat[off:off + lh * lw].reshape(lh, lw, 4) for off, lh, lw in layout]


def _fill(ctx, case):
    """svgr_image_fill of a FillCase into a poisoned buffer: (output, the device's chain, the mask)."""
    from svgrasterize_amd import _abi

    px = case.pixels()
    levels = _abi.image_upload(ctx, px, case.linear_rgb)
    im = _abi.ImageArgs()
    im.inv_m6 = (C.c_double * 6)(*case.inv_m[:2].ravel())
    im.height, im.width = case.shape
    im.smooth = int(case.smooth)
    im.lod = case.lam()
    rows, cols = case.bbox[2:]
    mask = case.mask()
    mbuf = ctx.from_host(np.ascontiguousarray(mask))
    guard = cols + 1
    out = _poisoned(ctx, rows * cols, guard)
    _abi._check(ctx.lib.svgr_image_fill(ctx.handle, C.byref(im), levels.handle, mbuf.handle, _bb(case.bbox), out.handle))
    got = _output(out, (rows, cols, 4), guard)
    assert not np.isnan(got).any(), f"pixels never written: {np.argwhere(np.isnan(got).any(axis=-1))[:5].tolist()}"
    assert np.array_equal(mbuf.download(mask.shape, np.float64), mask)
    return got, _chain(levels, case.shape), mask


SMOOTH_WIDE = [c for c in IC.FILL_CASES if c.smooth and c.route not in IC.EXACT_ROUTES]
NEAREST = [c for c in IC.FILL_CASES if not c.smooth and c.route not in IC.EXACT_ROUTES]
EXACT = [c for c in IC.FILL_CASES if c.route in IC.EXACT_ROUTES and c.route != "nonfinite"]


# ====================================================================================== 1. the fill
@pytest.mark.parametrize("case", SMOOTH_WIDE, ids=lambda c: c.name)
def test_smooth_fill_within_the_derived_tolerance(ctx, case):
    got, chain, mask = _fill(ctx, case)
    lam = case.lam()
    want = R.sample_wide(chain, case.inv_m, True, lam, *case.bbox) * mask[..., None].astype(R.LD)
    tol = R.fill_tolerance(case, chain)
    err = float(np.abs(got.astype(R.LD) - want).max())
    print(f"image fill {case.name} (lod {lam:.6g}): max |err| {err:.3e}, bound {tol:.3e}")
    assert err <= tol
    if case.route in ("seam", "stride"):
        assert (got == 0.0).mean() < 0.05


@pytest.mark.parametrize("case", NEAREST, ids=lambda c: c.name)
def test_nearest_fill_bit_for_bit(ctx, case):
    """The texel the long-double coordinates select (every case keeps IC.CLEARANCE from a texel boundary), times the mask."""
    got, chain, mask = _fill(ctx, case)
    texels = R.sample_wide(chain, case.inv_m, False, 0.0, *case.bbox).astype(np.float64)
    want = texels * mask[..., None]
    assert np.array_equal(got, want), np.argwhere((got != want).any(axis=-1))[:3].tolist()
    assert len(np.unique(texels.reshape(-1, 4), axis=0)) > 1 or case.shape == (1, 1)


@pytest.mark.parametrize("case", EXACT, ids=lambda c: c.name)
def test_exact_coordinates_bit_for_bit(ctx, case):
    """Dyadic maps (coordinates on texel boundaries included), translations of 1e300 and a level of detail beyond the chain:
    the coordinates carry no rounding, so the float64 restatement's lerps are the kernel's, operation for operation."""
    got, chain, mask = _fill(ctx, case)
    want = R.sample(chain, case.inv_m, case.smooth, *case.bbox, lam=case.lam()) * mask[..., None]
    assert np.array_equal(got, want), np.argwhere((got != want).any(axis=-1))[:3].tolist()
    if case.route == "lod_top":
        assert np.array_equal(got, chain[-1][0, 0].astype(np.float64) * mask[..., None])


@pytest.mark.parametrize("case", IC.fill_cases("nonfinite"), ids=lambda c: c.name)
def test_non_finite_maps_land_on_the_edge(ctx, case):
    """NaN, + inf, - inf and 1e308 in the map (the C ABI takes them; no loader produces them): the values of image_ref's
    non-finite rule, bit for bit.  tests/test_image_cases_host.py shows on the host build that no index leaves the level."""
    got, chain, mask = _fill(ctx, case)
    want = R.sample(chain, case.inv_m, case.smooth, *case.bbox, lam=case.lam()) * mask[..., None]
    assert np.isfinite(got).all()
    assert np.array_equal(got, want), np.argwhere((got != want).any(axis=-1))[:3].tolist()


# ====================================================================================== 2. the mip chain
@pytest.mark.parametrize("shape", IC.MIP_SHAPES)
def test_mip_chain_srgb_bit_for_bit(ctx, shape):
    from svgrasterize_amd import _abi

    px = R.random_rgba(shape, seed=shape[0] * 7 + shape[1])
    got = _chain(_abi.image_upload(ctx, px, False), shape)
    want = R.mip_chain(px, False)
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(g, w), (k, np.argwhere(g != w)[:3].tolist())


@pytest.mark.parametrize("shape", IC.MIP_SHAPES)
def test_mip_chain_linear_rgb(ctx, shape):
    """Level 0 within one float32 ULP of the long-double formula (a `pow`); every further level bit for bit the downsample of
    the device's own level before it."""
    from svgrasterize_amd import _abi

    px = R.random_rgba(shape, seed=shape[0] * 7 + shape[1])
    got = _chain(_abi.image_upload(ctx, px, True), shape)
    wide = R.prepare_wide(px, True)
    err = np.abs(got[0].astype(R.LD) - wide)
    ulp = ulp_f32(wide.astype(np.float64))
    print(f"image level 0 {shape} linearRGB: max |err| / ULP(f32) {float((err / ulp).max()):.3f}, bound 1")
    assert (err <= ulp).all()
    assert np.array_equal(got[0][..., 3], R.prepare(px, False)[..., 3])   # (alpha has no pow)
    for k in range(1, len(got)):
        want = R.downsample(got[k - 1])
        assert got[k].shape == want.shape and np.array_equal(got[k], want), k


# ====================================================================================== 3. documents
def _uri(px):
    return "data:image/png;base64," + base64.b64encode(R.encode_png(px, 6, 8)).decode()


def _doc(body, w=64, h=48):
    return f'<svg xmlns="http://www.w3.org/2000/svg" width="{w}" height="{h}">{body}</svg>'


def _swap():
    from svgrasterize_amd.geometry import Transform

    return Transform().matrix(0, 1, 0, 1, 0, 0)


def _only_image(scene):
    """(ImagePaint, its FILL path, accumulated transform) of the one image leaf of `scene`."""
    from svgrasterize_amd.geometry import Transform

    kind, args = scene
    tr = Transform()
    while kind != 0:
        if kind == 6:
            tr = tr @ args[1]
        kind, args = args[0]
    return args[1], args[0], tr


def _document(S, ctx, doc, px, linear_rgb=False, w=64, h=48):
    """(rendered canvas, long-double sample x the path's coverage, tolerance, level of detail) of a document with one <image>."""
    from svgrasterize_amd import _abi, paint as P

    scene, _, _ = S.svg_scene_from_str(doc)
    paint, path, tr = _only_image(scene)
    res = scene.render(_swap(), viewport=[0, 0, h, w], linear_rgb=linear_rgb)
    got = np.zeros((h, w, 4)) if res is None else res[0].on_canvas(h, w).image
    full = _swap() @ tr
    mask, _hull = path.mask(full, viewport=[0, 0, h, w])
    m = np.zeros((h, w))
    m[mask.x:mask.x + mask.height, mask.y:mask.y + mask.width] = mask.image[..., 0]
    inv = np.asarray((full @ paint.transform).invert.m, dtype=np.float64)
    chain = _chain(_abi.image_upload(ctx, px, linear_rgb), px.shape[:2])
    lam = P.image_lod(inv, len(chain))
    want = R.sample_wide(chain, inv, True, lam, 0, 0, h, w) * m[..., None].astype(R.LD)
    return got, want, R.fill_tolerance_of(chain, inv, True, lam, 0, 0, h, w), lam, m


def test_document_image_minified_onto_its_top_level(ctx):
    import svgrasterize_amd as S

    px = R.random_rgba((8, 8), seed=21)
    doc = _doc(f'<image href="{_uri(px)}" x="5.25" y="7.25" width="0.5" height="0.5" preserveAspectRatio="none"/>')
    got, want, tol, lam, m = _document(S, ctx, doc, px)
    assert lam == 3.0 and 0.2 < m[7, 5] < 0.3 and np.count_nonzero(m) == 1   # (16 texels a pixel: clamped to the 1 x 1 level)
    err = float(np.abs(got.astype(R.LD) - want).max())
    print(f"document, image on its top level: max |err| {err:.3e}, bound {tol:.3e}")
    assert err <= tol and got[7, 5, 3] > 0


def test_document_one_texel_image_stretched(ctx):
    import svgrasterize_amd as S

    px = np.array([[[200, 90, 17, 153]]], dtype=np.uint8)
    doc = _doc(f'<image href="{_uri(px)}" x="4" y="6" width="40" height="30" preserveAspectRatio="none"/>')
    for linear_rgb in (False, True):
        got, want, tol, lam, m = _document(S, ctx, doc, px, linear_rgb)
        assert lam == 0.0 and set(np.unique(m)) == {0.0, 1.0} and m.sum() == 40 * 30
        err = float(np.abs(got.astype(R.LD) - want).max())
        print(f"document, 1 x 1 image stretched (linearRGB {linear_rgb}): max |err| {err:.3e}, bound {tol:.3e}")
        assert err <= tol and np.array_equal(got[6:36, 4:44], np.broadcast_to(got[6, 4], (30, 40, 4))) and got[6, 4, 3] > 0.5
