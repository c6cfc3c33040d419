"""The kernels of the filter primitives, the paint servers and <image> through the C ABI at the launch seams their own tests do
not cross, each against the plain reference of its operation: the 8 x 8 tile of k_layer_convolve_matrix and its largest LDS
request, the second trip of the grid-stride loops of k_layer_turbulence, k_layer_component_transfer and k_image_prepare, the
row-stride loop of k_gradient_fill / k_gradient_detneg, the chunk and row-group ends of k_layer_tile, the tile ends of
k_layer_lighting and the index arithmetic of k_pattern_fill.  Outputs are poisoned with NaN before a call and end in a guard
that must stay NaN, inputs are read back after it (tests/test_gpu_layer_kernels.py's discipline).  What the shapes rely on is
shown on the host by tests/test_filter_paint_seams_host.py."""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest

from oracle import oracle as orc
from tests import filter_ref as F
from tests import image_ref as I
from tests import lighting_ref as LR
from tests import paint_ref as P
from tests import subregion_ref as SR

pytestmark = pytest.mark.gpu


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


def _poisoned(ctx, n_px, guard, dtype=np.float64):
    """A device buffer of n_px + guard RGBA pixels of NaN: the output of a call and the guard behind it."""
    return ctx.from_host(np.full((n_px + guard, 4), np.nan, dtype=dtype))


def _output(buf, shape, guard, dtype=np.float64):
    """The output a call left in a `_poisoned` buffer; the guard behind it must be untouched."""
    n_px = int(np.prod(shape[:-1]))
    got = buf.download(shape, dtype)
    behind = buf.download((guard, 4), dtype, offset=n_px * 4 * np.dtype(dtype).itemsize)
    assert np.isnan(behind).all(), "a store behind the output"
    return got


def _premultiplied(rng, shape):
    img = rng.random(shape + (4,))
    img[..., :3] *= img[..., 3:]
    return img


# ====================================================================================== 1. feConvolveMatrix
# (oy, ox): (28, 28) is the last order on 16 x 16 tiles and asks for 65440 bytes of LDS, 96 under the limit; (28, 29) and (29, 28)
# are the first on 8 x 8 tiles, (32, 32) the largest (64 lanes fill a 39 x 39 halo); tests/test_filter_paint_seams_host.py asserts
# the tiles.  Images: 2 x 3 tiles with a remainder of one pixel on both axes for either tile, and two that are smaller than every
# kernel but (1, 1): wrap goes round a 5 x 7 image up to seven times, duplicate clamps from both sides within one halo.
CM_ORDERS = [(28, 28), (28, 29), (29, 28), (32, 32), (1, 1)]
CM_IMAGES = [(17, 33), (9, 17), (5, 7), (1, 1)]
EDGE_MODES = ["duplicate", "wrap", "none"]


@pytest.mark.parametrize("order", CM_ORDERS)
def test_convolve_matrix_on_both_tiles(ctx, order):
    lib, check, ptr = _lib(ctx)
    oy, ox = order
    rng = _rng(f"cm{order}")
    kernel = np.ascontiguousarray(rng.uniform(-1.0, 2.0, (oy, ox)))
    if order == (1, 1):
        kernel[0, 0] = 0.8
    divisor, bias = 0.9 * oy * ox, 0.05   # (the sums stay inside (0, 1): a clamp hides nothing)
    targets = sorted({(0, 0), (ox - 1, oy - 1), (ox // 2, oy // 2)})
    inside = []
    for shape in CM_IMAGES:
        rows, cols = shape
        for preserve in (0, 1):
            img = rng.random(shape + (4,)) if preserve else _premultiplied(rng, shape)
            src = ctx.from_host(img)
            for mode, edge in enumerate(EDGE_MODES):
                for tx, ty in targets:
                    guard = cols + 1
                    out = _poisoned(ctx, rows * cols, guard)
                    k0 = kernel.copy()
                    check(lib.svgr_layer_convolve_matrix(ctx.handle, out.handle, src.handle, rows, cols, ptr(kernel), ox, oy, tx, ty,
                                                         divisor, bias, mode, preserve))
                    got = _output(out, shape + (4,), guard)
                    want = F.convolve_matrix(img, kernel, divisor, bias, (tx, ty), edge, bool(preserve))
                    assert np.array_equal(got, want), (shape, edge, preserve, (tx, ty), float(np.abs(got - want).max()))
                    assert np.array_equal(kernel, k0)
                    inside.append(((want[..., :3] > 0.0) & (want[..., :3] < 1.0)).mean())
            assert np.array_equal(src.download(img.shape, np.float64), img)
    assert np.mean(inside) > 0.7   # (most values are results of the sums, not of the clamps)


# ====================================================================================== 2. feTurbulence
# stride_blocks(n) = min(ceil(n / 256), 1024) workgroups of 256 lanes: the first trip of the grid-stride loop ends at pixel
# 1024 * 256 - 1 = 262143, the second starts at 262144 (lane 0 of workgroup 0).  (513, 512) has 262656 pixels: 262143 is
# [511, 511], 262144 is [512, 0].  (3, 87553) has 262659: both lie in row 2, at columns 87037 and 87038 -- a row and a column that
# come from a division by an odd width.
TURB_SHAPES = [(513, 512), (3, 87553)]
FIRST_SECOND_TRIP = 1024 * 256


def _transforms():
    from svgrasterize_amd.geometry import Transform

    return {
        "swap": Transform().matrix(0, 1, 0, 1, 0, 0).translate(3.5, -2.25).scale(1.5),
        "rotated": Transform().matrix(0, 1, 0, 1, 0, 0).translate(20, 10).rotate(0.7).scale(1.25, 0.8),
    }


@functools.lru_cache(maxsize=None)
def _harness():
    return F.harness()


@pytest.mark.parametrize("name", ["swap", "rotated"])
@pytest.mark.parametrize("stitch", [False, True])
@pytest.mark.parametrize("octaves", [1, 3])
@pytest.mark.parametrize("shape", TURB_SHAPES)
def test_turbulence_beyond_the_first_trip(ctx, shape, octaves, stitch, name):
    from svgrasterize_amd.layer import turbulence_seed

    lib, check, ptr = _lib(ctx)
    rows, cols = shape
    n = rows * cols
    assert n > FIRST_SECOND_TRIP + 256   # (a second trip in more than one workgroup)
    tr = _transforms()[name]
    offset, seed, fractal = (-3, 5), 7 - 24 * octaves, octaves == 3
    tile = (-2.5, 1.75, 230.3, 310.9) if stitch else None
    freq = (0.061, 0.093)
    inv = np.ascontiguousarray(tr.invert.m6(), dtype=np.float64)
    tile4 = np.ascontiguousarray((0, 0, 0, 0) if tile is None else tile, dtype=np.float64)
    guard = cols + 1
    out = _poisoned(ctx, n, guard)
    check(lib.svgr_layer_turbulence(ctx.handle, out.handle, _bb(offset + shape), ptr(inv), freq[0], freq[1], ptr(tile4),
                                    turbulence_seed(seed), octaves, int(fractal), int(stitch)))
    got = _output(out, shape + (4,), guard)
    host = F.harness_turbulence_layer(_harness(), tr, offset, shape, freq, octaves, turbulence_seed(seed), tile, fractal)
    assert np.array_equal(got, host), np.argwhere((got != host).any(axis=-1))[:3].tolist()
    worst = 0.0
    for r in sorted({0, (FIRST_SECOND_TRIP - 1) // cols, FIRST_SECOND_TRIP // cols}):
        ref = F.turbulence_layer(tr, (offset[0] + r, offset[1]), (1, cols), freq, octaves, seed, tile, fractal)
        worst = max(worst, float(np.abs(got[r] - ref[0]).max()))
    print(f"turbulence {shape} octaves {octaves} stitch {stitch} {name}: max |err| {worst:.3e}, bound 1e-15")
    assert worst <= 1e-15
    assert got.reshape(-1, 4)[FIRST_SECOND_TRIP:].std() > 0.01


# ====================================================================================== 3. feComponentTransfer
# The same stride_blocks: 262144 pixels take one trip exactly, 262145 a second trip of one lane, 262144 + 256 + 1 a second trip of
# workgroup 0, all of it, and of one lane of workgroup 1.  The tables fill SVGR_TRANSFER_MAX_VALUES = 4096 (with the 20
# parameters 32928 bytes of dynamic LDS, staged by 256 lanes in 17 rounds).
XFER_N_PX = [FIRST_SECOND_TRIP, FIRST_SECOND_TRIP + 1, FIRST_SECOND_TRIP + 256 + 1]
XFER_SPLITS = {
    "table_4093_1_1_1": [("table", 4093), ("table", 1), ("table", 1), ("table", 1)],
    "discrete_4093_1_1_1": [("discrete", 4093), ("discrete", 1), ("discrete", 1), ("discrete", 1)],
    "table_1024x4": [("table", 1024)] * 4,
    "discrete_1024x4": [("discrete", 1024)] * 4,
    "mixed_with_gamma": [("table", 2048), ("discrete", 2047), ("gamma", 0), ("table", 1)],
}


def _xfer_funcs(split, rng):
    return [("gamma", 0.8, 0.45, 0.1) if kind == "gamma" else (kind, rng.uniform(-0.1, 1.1, n)) for kind, n in XFER_SPLITS[split]]


def _run_transfer(ctx, img, funcs, guard=3):
    from svgrasterize_amd.layer import TRANSFER_TYPES

    lib, check, ptr = _lib(ctx)
    types = np.array([TRANSFER_TYPES[f[0]] for f in funcs], dtype=np.int32)
    params = np.tile(np.array([1.0, 0.0, 1.0, 1.0, 0.0]), (4, 1))
    counts = np.zeros(4, dtype=np.int64)
    tables = [np.zeros(0)]
    for k, f in enumerate(funcs):
        if f[0] == "gamma":
            params[k, 2:5] = f[1:4]
        else:
            counts[k] = len(f[1])
            tables.append(np.asarray(f[1], dtype=np.float64))
    values = np.ascontiguousarray(np.concatenate(tables))
    buf = ctx.from_host(np.concatenate([img, np.full((guard, 4), np.nan)]))
    rc = lib.svgr_layer_component_transfer(ctx.handle, buf.handle, len(img), ptr(types), ptr(params), ptr(counts), ptr(values))
    return rc, buf, int(counts.sum())


@pytest.mark.parametrize("n_px", XFER_N_PX)
@pytest.mark.parametrize("split", list(XFER_SPLITS))
def test_component_transfer_with_full_tables_beyond_the_first_trip(ctx, split, n_px):
    lib, check, ptr = _lib(ctx)
    rng = _rng(split)
    funcs = _xfer_funcs(split, rng)
    img = _rng(f"px{n_px}").uniform(-0.1, 1.1, (n_px, 4))
    img[-1] = (1.0, 0.0, 0.999999, 1.0)   # (the last pixel -- the second trip's, when there is one -- reads the tables' last entries)
    rc, buf, total = _run_transfer(ctx, img, funcs)
    check(rc)
    assert total == 4096
    got = _output(buf, (1, n_px, 4), 3)   # a flat (1, n) layer
    want = F.component_transfer(img.reshape(1, n_px, 4), funcs)
    for k, f in enumerate(funcs):
        if f[0] == "gamma":
            err = float(np.abs(got[..., k] - want[..., k]).max())
            print(f"component transfer {split} n_px {n_px}: gamma max |err| {err:.3e}, bound 1e-14")
            assert err <= 1e-14
        else:
            assert np.array_equal(got[..., k], want[..., k]), (k, np.argwhere(got[..., k] != want[..., k])[:3].tolist())
    assert len(np.unique(got[0, FIRST_SECOND_TRIP - 256:, 0])) > 1


def test_component_transfer_refuses_4097_values(ctx):
    img = _rng("4097").random((300, 4))
    funcs = [("table", np.linspace(0.0, 1.0, 4094)), ("discrete", [0.5]), ("table", [0.25]), ("table", [1.0])]
    rc, buf, total = _run_transfer(ctx, img, funcs)
    assert (total, rc) == (4097, -1) and b"4097 table values" in ctx.lib.svgr_last_error()
    assert np.array_equal(buf.download(img.shape, np.float64), img)   # nothing ran


# ====================================================================================== 4. gradient fill
# The grid is (ceil(cols / 256), min(rows, 32768)) and a lane walks rows blockIdx.y, blockIdx.y + gridDim.y, ...: with 32770 rows
# block rows 0 and 1 take a second trip, to rows 32768 and 32769.  257 columns add a second column block of one lane.  svgr_gradient_fill
# accepts boxes of up to 2^30 - 1 rows, so the loop is reachable through the ABI; it takes a coverage mask always, and the
# oracle's picture is the gradient before the mask: the mask is all ones.
GRAD_TOL = 1e-13   # tests/test_gradient_blur.py: the gradient evaluation against the same oracle


def _gradient_paint(name):
    import svgrasterize_amd as S

    g = P.GRADIENTS[name]
    stops = [(o, np.array(c)) for o, c in g["stops"]]
    if g["kind"] == "linear":
        paint = S.GradLinear(np.array(g["p0"]), np.array(g["p1"]), stops, None, g["spread"], False, True)
    else:
        fc = g.get("fcenter")
        paint = S.GradRadial(np.array(g["center"]), g["radius"], None if fc is None else np.array(fc), g.get("fradius"), stops, None,
                             g["spread"], False, True)
    return paint, S.Transform(np.array(g["user"]))


def _oracle_rows(name, box, lo, hi, off, col):
    g = P.GRADIENTS[name]
    return orc.gradient_image(g["kind"], (box[0] + lo, box[1], hi - lo, box[3]), np.asarray(g["user"]), None, g["spread"], off, col,
                              **P.oracle_kwargs(g))


@pytest.mark.parametrize("cols", [3, 257])
@pytest.mark.parametrize("name", list(P.GRADIENTS))
def test_gradient_fill_beyond_32768_rows(ctx, name, cols):
    """The whole 32770-row box in one call; every pixel must have been written.  3 columns: all of it against the oracle.  257
    columns (8.4 Mpx: the oracle alone would take several seconds): the first 64 rows and the last 66, which hold the last row
    of the first trip (32767) and both rows of the second.  The oracle of a slice masks like the oracle of the box: the slices of
    "focal_detneg" without a negative determinant (the first rows) have no pixel that the flag alone would mask
    (tests/test_filter_paint_seams_host.py), and the last slice holds the negative determinants itself."""
    lib, check, ptr = _lib(ctx)
    box = P.tall_box(cols)
    rows = box[2]
    assert rows > 32768
    paint, user_tr = _gradient_paint(name)
    g, (off, col) = paint.abi(user_tr, True)
    assert g.kind == (1 if name == "linear" else 2 if name == "radial" else 3)
    mask = ctx.from_host(np.ones((rows, cols)))
    guard = cols + 1
    out = _poisoned(ctx, rows * cols, guard)
    check(lib.svgr_gradient_fill(ctx.handle, C.byref(g), mask.handle, _bb(box), out.handle))
    got = _output(out, (rows, cols, 4), guard)
    assert not np.isnan(got).any(), f"rows never written: {np.unique(np.argwhere(np.isnan(got).any(axis=(1, 2))))[:5].tolist()}"
    worst = 0.0
    for lo, hi in [(0, rows)] if cols == 3 else [(0, 64), (rows - 66, rows)]:
        want = _oracle_rows(name, box, lo, hi, off, col)
        worst = max(worst, float(np.abs(got[lo:hi] - want).max()))
    print(f"gradient {name} x {cols} columns: max |err| {worst:.3e}, bound {GRAD_TOL:.0e}")
    assert worst <= GRAD_TOL
    second = got[P.FIRST_SECOND_TRIP_ROW:]
    if name == "focal_detneg":
        assert not second.any() and (got[:P.FIRST_SECOND_TRIP_ROW, :, 3] > 0).all()
    else:
        assert (second[..., 3] > 0).all()
    assert np.array_equal(mask.download((rows, cols), np.float64), np.ones((rows, cols)))


# ====================================================================================== 5. image upload
# k_image_prepare runs min(ceil(n / 256), 2048) workgroups of 256 lanes, each with its own colour table in LDS: the second trip
# starts at texel 2048 * 256 = 524288.  513 x 1025 has 525825 texels: 1537 of them (six workgroups and one lane) are the second
# trip's.  1 x 1 and 1 x 3: the 2 x 2 footprint of a downsampled texel hangs over the bottom (and the right) edge.
@pytest.mark.parametrize("shape", [(513, 1025), (1, 1), (1, 3)])
@pytest.mark.parametrize("linear_rgb", [False, True])
def test_image_upload_mip_chain(ctx, shape, linear_rgb):
    from svgrasterize_amd import _abi

    lib, check, ptr = _lib(ctx)
    h, w = shape
    if h > 1:
        assert h * w > 2048 * 256 + 256
    px = I.random_rgba(shape, seed=h + w)
    px0 = px.copy()
    layout = _abi.image_levels(h, w)
    total = layout[-1][0] + 1
    guard = 5
    buf = _poisoned(ctx, total, guard, np.float32)
    check(lib.svgr_image_upload(ctx.handle, ptr(px), h, w, int(linear_rgb), buf.handle))
    got = _output(buf, (total, 4), guard, np.float32)
    assert not np.isnan(got).any() and np.array_equal(px, px0)
    want = I.mip_chain(px, linear_rgb)
    assert [(lh, lw) for _, lh, lw in layout] == [lv.shape[:2] for lv in want]
    worst = 0.0
    for (off, lh, lw), lv in zip(layout, want):
        worst = max(worst, float(np.abs(got[off:off + lh * lw].reshape(lh, lw, 4).astype(np.float64) - lv).max()))
    print(f"image {shape} linear {linear_rgb}: {len(layout)} levels, max |err| {worst:.3e}, bound 1e-06")
    assert worst <= 1e-6   # tests/test_gpu_image.py: TOL


# ====================================================================================== 6. feTile
# One lane moves one 16-byte half pixel; a workgroup covers a chunk of 256 halves (128 pixels) of 8 rows.  129 columns: the last
# chunk holds two halves; 128: a row ends with its chunk; 257: three chunks, the last of two halves.  9 and 17 rows: a last row
# group of one row; 8: none.
TILE_OUT = [(-3, -5, 9, 129), (0, 0, 8, 128), (2, 1, 17, 257)]


@pytest.mark.parametrize("which", ["above_left", "beyond_source"])
@pytest.mark.parametrize("out_box", TILE_OUT)
def test_tile_at_chunk_and_row_group_ends(ctx, out_box, which):
    lib, check, ptr = _lib(ctx)
    img = _premultiplied(_rng("tile"), (23, 31))
    if which == "above_left":   # a 7 x 5 tile that starts above and left of the output, inside the source
        tile_box = (out_box[0] - 4, out_box[1] - 3, 7, 5)
        off = (tile_box[0] - 1, tile_box[1] - 2)
    else:                       # a tile that reaches beyond the source, below and right of it
        off = (out_box[0] - 9, out_box[1] - 11)
        tile_box = (off[0] + 15, off[1] + 20, 17, 23)
    src = ctx.from_host(img)
    rows, cols = out_box[2:]
    guard = cols + 1
    out = _poisoned(ctx, rows * cols, guard)
    check(lib.svgr_layer_tile(ctx.handle, out.handle, _bb(out_box), src.handle, _bb(off + img.shape[:2]), _bb(tile_box)))
    got = _output(out, (rows, cols, 4), guard)
    want = SR.tile(img, off, out_box, tile_box)
    assert np.array_equal(got, want), np.argwhere((got != want).any(axis=-1))[:3].tolist()
    assert (want != 0).any() and ((want == 0).all(axis=-1).any() == (which == "beyond_source"))
    assert np.array_equal(src.download(img.shape, np.float64), img)


# ====================================================================================== 7. lighting
# 16 x 16 tiles with a one-pixel halo: (16, 16) is one tile exactly (its halo lies outside the region all round), (32, 33) ends one
# column past a tile (the halo's last column of the tiles before is the region's last column), (17, 16) one row past.
LIGHT_REGIONS = [(16, 16), (32, 33), (17, 16)]
LIGHTS = {"distant": (LR.DISTANT, [0.35, -0.52, 0.0, 0, 0, 0, 0, 0]), "spot": (LR.SPOT, [9.5, 30.25, 21.0, 0.0, 0.0, 0.0, 3.0, 0.55])}


@pytest.mark.parametrize("specular", [False, True])
@pytest.mark.parametrize("kind", list(LIGHTS))
def test_lighting_at_tile_ends(ctx, kind, specular):
    lib, check, ptr = _lib(ctx)
    rng = _rng("light")
    code, p = LIGHTS[kind]
    params = np.array(p, dtype=np.float64)
    if code == LR.DISTANT:
        params[2] = np.sqrt(1.0 - params[0] ** 2 - params[1] ** 2)
    else:
        d = np.array([8.0, 20.0, 0.0]) - params[0:3]   # (points into the regions)
        params[3:6] = d / np.sqrt((d * d).sum())
    color = np.array([0.95, 0.7, 0.35])
    se = 17.0 if specular else None
    worst = 0.0
    for shape in LIGHT_REGIONS:
        offset = (-4, 7)
        # the source's last row and column are the region's / stop one short of it / lie beyond it; it starts outside the region
        for over in (0, -1, 2):
            src_off = (offset[0] - 2, offset[1] - 3)
            src_shape = (shape[0] + 2 + over, shape[1] + 3 + over)
            img = rng.random(src_shape + (4,))
            src = ctx.from_host(img)
            guard = shape[1] + 1
            out = _poisoned(ctx, shape[0] * shape[1], guard)
            check(lib.svgr_layer_lighting(ctx.handle, out.handle, _bb(offset + shape), src.handle, _bb(src_off + src_shape), code,
                                          ptr(params), ptr(color), 2.0, 0.9, 17.0 if specular else 1.0, int(specular)))
            got = _output(out, shape + (4,), guard)
            A = LR.region_alpha(img, src_off, offset, shape)
            assert (A[-1, -1] == 0.0) == (over == -1)
            ref = LR.lighting(A, offset, code, params, color, 2.0, 0.9, se)
            err = float(np.abs(got - ref).max())
            worst = max(worst, err)
            assert err <= 1e-13, (shape, over, err)
            assert got[..., :3].max() > 0.01
            assert np.array_equal(src.download(img.shape, np.float64), img)
    print(f"lighting {kind} specular {specular}: max |err| {worst:.3e}, bound 1e-13")


# ====================================================================================== 8. pattern fill
# A 19 x 300 mask: 5700 flat indices, 300 is no multiple of 256, so every workgroup but the first starts inside a row.
PAT_BOX = (-4, 6, 19, 300)


def _rot(angle, sx, sy):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, -s], [s, c]]) @ np.diag([sx, sy])


def _pattern_cases():
    ident = P.pattern_geometry(np.identity(2), (2.0, -3.0, 7.0, 5.0), (1, 1), (5, 4))
    rot = _rot(0.5, 1.7, 1.3)
    return {
        "identity": (ident, (5, 4)),
        "rotated_scaled": (P.pattern_geometry(rot, (1.5, 0.25, 9.0, 6.0), (-3, 2), (11, 9), translate=(3.25, -1.5)), (11, 9)),
        "negative_width": (P.pattern_geometry(_rot(-0.3, 1.2, 0.9), (0.5, 1.0, -8.0, 5.0), (-7, 0), (8, 6)), (8, 6)),
        # the canvas moved by (3, 2): the first offsets are negative and read the canvas's last rows / columns, where the tile is
        "negative_offsets": (dict(ident, min_xy=[3, 2], tile_bbox=[3, 1, 5, 4]), (5, 4)),
        "tile_over_the_edge": (dict(ident, tile_bbox=[-2, 1, 5, 4]), (5, 4)),
        "outside_the_canvas": (dict(ident, pat_shape=[4, 6]), (5, 4)),
    }


def _pattern_args(pat):
    from svgrasterize_amd import _abi

    a = _abi.PatternArgs()
    a.inv_m6, a.fwd_m6, a.cell = (C.c_double * 6)(*pat["inv_m6"]), (C.c_double * 6)(*pat["fwd_m6"]), (C.c_double * 4)(*pat["cell"])
    a.min_xy, a.pat_shape, a.tile_bbox = (C.c_int64 * 2)(*pat["min_xy"]), (C.c_int64 * 2)(*pat["pat_shape"]), (C.c_int64 * 4)(*pat["tile_bbox"])
    return a


@pytest.mark.parametrize("name", list(_pattern_cases()))
def test_pattern_fill_against_the_restatement(ctx, name):
    lib, check, ptr = _lib(ctx)
    pat, tile_shape = _pattern_cases()[name]
    rng = _rng(name)
    tile = rng.uniform(-0.2, 1.2, tile_shape + (4,))
    mask = rng.random(PAT_BOX[2:])
    tbuf, mbuf = ctx.from_host(tile), ctx.from_host(mask)
    n = PAT_BOX[2] * PAT_BOX[3]
    guard = PAT_BOX[3] + 1
    out = _poisoned(ctx, n, guard)
    rc = lib.svgr_pattern_fill(ctx.handle, C.byref(_pattern_args(pat)), tbuf.handle, mbuf.handle, _bb(PAT_BOX), out.handle)
    if name == "outside_the_canvas":
        with pytest.raises(IndexError):
            P.pattern_fill(pat, tile, mask, PAT_BOX)
        assert rc == -1 and b"outside the pattern canvas" in lib.svgr_last_error()
        _output(out, PAT_BOX[2:] + (4,), guard)   # (the guard only)
        return
    check(rc)
    got = _output(out, PAT_BOX[2:] + (4,), guard)
    want = P.pattern_fill(pat, tile, mask, PAT_BOX)
    assert np.array_equal(got, want), np.argwhere((got != want).any(axis=-1))[:3].tolist()
    lit = (want != 0).any(axis=-1)
    assert 0.1 < lit.mean() < 1.0 and want.max() <= 1.0   # (tile and gaps both show; the tile's values above 1 were clipped)
    assert np.array_equal(tbuf.download(tile.shape, np.float64), tile) and np.array_equal(mbuf.download(mask.shape, np.float64), mask)
