"""CPU-side checks of the filter primitives beyond the reference: the feTurbulence arithmetic of csrc/svgr_core.h (host build,
tests/filter_harness.cpp) against the numpy restatement in tests/filter_ref.py, the stitch property, the loader's entries for
the new elements, feDropShadow's expansion and the filter region.  No GPU needed."""
import warnings

import numpy as np
import pytest

from svgrasterize_amd import filters as F
from svgrasterize_amd.geometry import ConvexHull, Transform
from svgrasterize_amd.layer import COMPOSE_IN, Layer, turbulence_seed
from svgrasterize_amd.svg import _filter
from tests import filter_ref as R

import xml.etree.ElementTree as etree


@pytest.fixture(scope="module")
def fh():
    return R.harness()


SEEDS = [0, -1, -7, 3.7, -2.9, 12345, 2 ** 31 - 1, 2 ** 31 + 5, 2 ** 40, -(2 ** 70)]


@pytest.mark.parametrize("seed", SEEDS)
def test_turbulence_lattice_bit_exact(fh, seed):
    sel, grad = R.lattice(seed)
    hsel, hgrad = R.harness_lattice(fh, turbulence_seed(seed))
    assert np.array_equal(sel, hsel)
    assert np.array_equal(grad, hgrad)
    assert sorted(sel[:256]) == list(range(256))


@pytest.mark.parametrize("seed", [0, -5, 2.5, 2 ** 33])
@pytest.mark.parametrize("octaves", [0, 1, 6])
@pytest.mark.parametrize("fractal", [False, True])
@pytest.mark.parametrize("tile", [None, (10.5, -20.0, 37.3, 51.2)])
def test_turbulence_point_bit_exact(fh, seed, octaves, fractal, tile):
    rng = np.random.default_rng(abs(int(seed)) % 1000 + octaves)
    px, py = rng.uniform(-400, 400, 3000), rng.uniform(-400, 400, 3000)
    ref = R.turbulence(seed, (0.043, 0.117), octaves, fractal, tile, px, py)
    got = R.harness_turbulence(fh, turbulence_seed(seed), (0.043, 0.117), octaves, fractal, tile, px, py)
    assert np.array_equal(ref, got)
    if octaves:
        assert ref.std() > 0.01   # (not a constant)


@pytest.mark.parametrize("tile", [(3.25, -7.5, 41.7, 29.3), (0.0, 0.0, 41.7, 29.3), (-10.0, 20.0, 33.1, 47.9)])
@pytest.mark.parametrize("fractal", [False, True])
def test_turbulence_stitch_property(fh, fractal, tile):
    """With stitchTiles a point of the tile and the point one tile width (height) further give the same value -- up to
    rounding: the adjusted frequency times the tile size is an integer only to within an ulp.  The spec wraps a lattice
    coordinate once (bx >= wrap: bx -= width), so the one exception is the tile's last lattice column (row), whose right
    neighbour is the wrap point itself; there the shifted point reads the next tile's cell.  The seam holds everywhere: the
    tile's right edge meets its left edge."""
    rng = np.random.default_rng(3)
    px = rng.uniform(tile[0], tile[0] + tile[2], 2000)
    py = rng.uniform(tile[1], tile[1] + tile[3], 2000)
    freq = (0.07, 0.13)
    fx, fy, _, _, wrap_x, wrap_y = R.turbulence_params(*freq, tile, True)
    inner_x = np.trunc(px * fx + R.PERLIN_N) + 1 < wrap_x
    inner_y = np.trunc(py * fy + R.PERLIN_N) + 1 < wrap_y
    assert inner_x.mean() > 0.25 and inner_y.mean() > 0.25

    def at(x, y, t):
        return R.harness_turbulence(fh, 9, freq, 5, fractal, t, x, y)

    base = at(px, py, tile)
    assert np.abs(at(px + tile[2], py, tile) - base)[inner_x].max() <= 1e-9
    assert np.abs(at(px, py + tile[3], tile) - base)[inner_y].max() <= 1e-9
    both = inner_x & inner_y
    assert np.abs(at(px + tile[2], py + tile[3], tile) - base)[both].max() <= 1e-9
    # the seam: just inside the right (bottom) edge = the left (top) edge
    ys = rng.uniform(tile[1], tile[1] + tile[3], 500)
    assert np.abs(at(np.full(500, tile[0] + tile[2] - 1e-11), ys, tile) - at(np.full(500, tile[0]), ys, tile)).max() <= 1e-9
    # without stitching the shifted points see other lattice cells
    assert np.abs(at(px + tile[2], py, None) - at(px, py, None))[inner_x].max() > 1e-3


def test_turbulence_seed_folding():
    assert turbulence_seed(3.9) == 3 and turbulence_seed(-3.9) == -3
    assert turbulence_seed(2 ** 80) == 2 ** 31 - 2
    assert turbulence_seed(-(2 ** 80)) == -((2 ** 80) % (2 ** 31 - 2))


# -- the loader --------------------------------------------------------------------------------------------------------
def _parse(body, filter_attrs=""):
    el = etree.fromstring(f'<filter xmlns="http://www.w3.org/2000/svg" id="f" {filter_attrs}>{body}</filter>')
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        flt = _filter(el)
    return flt, [str(w.message) for w in caught]


DEFAULT_REGION = (True, None, None, None, None)


def test_loader_flood_defaults_and_style():
    flt, warned = _parse('<feFlood result="a"/><feFlood style="flood-color: #ff0000; flood-opacity: 0.5"/>'
                         '<feFlood flood-color="#0000ff80" flood-opacity="50%"/>')
    assert not warned
    (t0, a0, i0), (t1, a1, _), (t2, a2, _) = flt.filters
    assert t0 == t1 == t2 == F.FE_FLOOD and i0 == []
    assert a0 == ((0.0, 0.0, 0.0, 1.0), DEFAULT_REGION) and flt.names["a"] == 2
    assert a1 == ((1.0, 0.0, 0.0, 0.5), DEFAULT_REGION)
    assert a2[0] == pytest.approx((0.0, 0.0, 1.0, 0.5 * 128 / 255), abs=1e-15)


def test_loader_turbulence():
    flt, warned = _parse('<feTurbulence/><feTurbulence baseFrequency="0.05 0.2" numOctaves="4" seed="-3.7" '
                         'stitchTiles="stitch" type="fractalNoise" result="t"/>')
    assert not warned
    assert flt.filters[0] == (F.FE_TURBULENCE, ((0.0, 0.0), 1, 0.0, False, False, DEFAULT_REGION), [])
    assert flt.filters[1] == (F.FE_TURBULENCE, ((0.05, 0.2), 4, -3.7, True, True, DEFAULT_REGION), [])
    assert flt.names["t"] == 3


def test_loader_component_transfer():
    flt, warned = _parse('<feComponentTransfer in="SourceGraphic" result="c">'
                         '<feFuncR type="table" tableValues="0 0.5 1"/><feFuncG type="discrete" tableValues=""/>'
                         '<feFuncB type="linear" slope="2"/><feFuncA type="gamma" amplitude="0.5" exponent="2" offset="0.1"/>'
                         '</feComponentTransfer><feComponentTransfer/>')
    assert not warned
    (t0, a0, i0), (t1, a1, i1) = flt.filters
    assert t0 == t1 == F.FE_COMPONENT_TRANSFER and i0 == [1] and i1 == [2]
    assert a0 == ((("table", (0.0, 0.5, 1.0)), None, ("linear", 2.0, 0.0), ("gamma", 0.5, 2.0, 0.1)),)
    assert a1 == ((None, None, None, None),)


def test_loader_convolve_matrix():
    flt, warned = _parse('<feConvolveMatrix kernelMatrix="0 -1 0 -1 5 -1 0 -1 0"/>'
                         '<feConvolveMatrix order="3 2" kernelMatrix="1 2 3 4 5 6" divisor="0" bias="0.25" targetX="0" '
                         'targetY="1" edgeMode="wrap" preserveAlpha="true" in="SourceAlpha"/>')
    assert warned == ["convolve matrix divisor 0: the default divisor is used"]
    (t0, a0, i0), (t1, a1, i1) = flt.filters
    assert t0 == t1 == F.FE_CONVOLVE_MATRIX and i0 == [1] and i1 == [0]
    assert np.array_equal(a0[0], [[0, -1, 0], [-1, 5, -1], [0, -1, 0]]) and a0[1:] == (None, 0.0, (1, 1), "duplicate", False)
    assert np.array_equal(a1[0], [[1, 2, 3], [4, 5, 6]]) and a1[1:] == (None, 0.25, (0, 1), "wrap", True)


@pytest.mark.parametrize("body, message", [
    ('<feTurbulence baseFrequency="-0.1"/>', "negative baseFrequency"),
    ('<feConvolveMatrix kernelMatrix="1 2 3"/>', "kernelMatrix needs"),
    ('<feConvolveMatrix order="2" kernelMatrix="1 2 3 4" targetX="2"/>', "target outside the kernel"),
    ('<feConvolveMatrix order="33 1" kernelMatrix="' + " ".join(["1"] * 33) + '"/>', "order above 32"),
    ('<feDisplacementMap in2="x" xChannelSelector="Q"/>', "invalid channel selector"),
])
def test_loader_bad_attributes_skip_the_primitive(body, message):
    flt, warned = _parse('<feOffset dx="1" result="o"/>' + body + '<feGaussianBlur stdDeviation="1"/>')
    assert len(warned) == 1 and message in warned[0], warned
    assert [t for t, _, _ in flt.filters] == [F.FE_OFFSET, F.FE_GAUSSIAN_BLUR]
    assert flt.filters[1][2] == [2]   # (the blur's default input: the offset, the skipped primitive left no result)


def test_loader_displacement_map():
    flt, warned = _parse('<feTurbulence result="t"/><feDisplacementMap in="SourceGraphic" in2="t" scale="12" '
                         'xChannelSelector="R" yChannelSelector="G"/><feDisplacementMap/>')
    assert not warned
    assert flt.filters[1] == (F.FE_DISPLACEMENT_MAP, (12.0, "R", "G"), [1, 2])
    assert flt.filters[2] == (F.FE_DISPLACEMENT_MAP, (0.0, "A", "A"), [3, 3])


def test_drop_shadow_expansion():
    flt, warned = _parse('<feOffset dx="1" result="o"/><feDropShadow in="SourceGraphic" dx="3" dy="-1" stdDeviation="1.5 2" '
                         'flood-color="red" flood-opacity="0.5" result="s"/><feDropShadow/>', 'filterUnits="userSpaceOnUse" x="1"')
    assert not warned
    region = (False, 1.0, None, None, None)
    entries = flt.filters[1:7]
    assert [t for t, _, _ in entries] == [F.FE_COLOR_MATRIX, F.FE_GAUSSIAN_BLUR, F.FE_OFFSET, F.FE_FLOOD, F.FE_COMPOSITE,
                                          F.FE_MERGE]
    assert np.array_equal(entries[0][1][0], F.COLOR_MATRIX_ALPHA) and entries[0][2] == [1]
    assert entries[1][1:] == ((1.5, 2.0), [3])
    assert entries[2][1:] == ((3.0, -1.0), [4])
    assert entries[3][1:] == (((1.0, 0.0, 0.0, 0.5), region), [])
    assert entries[4][1:] == ((COMPOSE_IN,), [6, 5])
    assert entries[5][1:] == ((), [7, 1])
    assert flt.names == {"SourceAlpha": 0, "SourceGraphic": 1, "o": 2, "s": 8}
    # the defaults, input = the previous result (the first shadow's merge)
    second = flt.filters[7:]
    assert second[0][2] == [8] and second[1][1] == (2.0, 2.0) and second[2][1] == (2.0, 2.0)
    assert second[3][1] == ((0.0, 0.0, 0.0, 1.0), region) and second[5][2] == [13, 8]


# -- the filter region -------------------------------------------------------------------------------------------------
def _box(points):
    lo, hi = np.floor(points.min(axis=0)), np.ceil(points.max(axis=0))
    return (int(lo[0]), int(lo[1])), (int(hi[0] - lo[0]), int(hi[1] - lo[1]))


TRANSFORMS = {
    "swap": Transform().matrix(0, 1, 3, 1, 0, -2).scale(2.0),
    "rotated": Transform().matrix(0, 1, 0, 1, 0, 0).translate(40, 30).rotate(0.6).scale(1.5, 0.75),
}


@pytest.mark.parametrize("name", sorted(TRANSFORMS))
def test_filter_region(name):
    tr = TRANSFORMS[name]
    # the node: a user-space rectangle (5, 7) .. (25, 17), hull in device space
    user = np.array([[5.0, 7.0], [25.0, 7.0], [25.0, 17.0], [5.0, 17.0]])
    hull = ConvexHull(tr(user))
    bx, by, bw, bh = hull.bbox(tr)
    layer = Layer(np.zeros((3, 4, 4)), (0, 0), True, True)

    def expect(x, y, w, h):
        return _box(tr(np.array([[x, y], [x + w, y], [x, y + h], [x + w, y + h]])))

    off, shape, rect = F.filter_region(None, tr, layer, hull)
    assert rect == pytest.approx((bx - 0.1 * bw, by - 0.1 * bh, 1.2 * bw, 1.2 * bh))
    assert (off, shape) == expect(*rect)
    assert rect == pytest.approx((3.0, 6.0, 24.0, 12.0))
    off, shape, rect = F.filter_region((True, 0.25, 0.5, 0.5, 0.25), tr, layer, hull)
    assert rect == pytest.approx((10.0, 12.0, 10.0, 2.5)) and (off, shape) == expect(*rect)
    off, shape, rect = F.filter_region((False, -3.0, 2.0, 40.0, 9.5), tr, layer, hull)
    assert rect == (-3.0, 2.0, 40.0, 9.5) and (off, shape) == expect(*rect)
    # no hull: the source layer's extent taken back to user space
    src = Layer(np.zeros((10, 20, 4)), (-4, 6), True, True)
    corners = tr.invert(np.array([[-4, 6], [-4, 26], [6, 6], [6, 26]], dtype=np.float64))
    lo, hi = corners.min(axis=0), corners.max(axis=0)
    off, shape, rect = F.filter_region(None, tr, src)
    size = hi - lo
    assert rect == pytest.approx((lo[0] - 0.1 * size[0], lo[1] - 0.1 * size[1], 1.2 * size[0], 1.2 * size[1]))
    assert (off, shape) == expect(*rect)
