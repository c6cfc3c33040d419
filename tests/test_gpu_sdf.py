"""Signed distance fields on the GPU: svgr_batch_distance through the C ABI against the numpy reference (tests/sdf_ref.py, which
has no cull) evaluated on the batch's own flattened edges (``batch.all_edges()``), at the seams of the launch geometry -- B =
svgr_hit_block() points per workgroup, C = svgr_hit_chunk() edges per LDS stage, B paths per round of the path table --; the sign
exactly hit_ref's, the magnitude within the tolerance derived in sdf_ref.py; the cull against the cull-free reference and against
itself under another grouping of the points; the scratch passes; ``Path.sdf`` against ``Path.mask`` as an independent witness that
also pins coordinate order and sign; ``Font.sdf_atlas`` on the committed fonts; and the errors.  tests/test_sdf_host.py checks on
the CPU that the reference and the per-lane header are the same arithmetic."""
import json
import os

import numpy as np
import pytest

from tests import sdf_cases as cases
from tests import sdf_ref as R
from tests.test_gpu_hit import circle_path, make_batch, poly_path, query_points
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import svgrasterize_amd as S

    S.Context.get()
    return S


@pytest.fixture(scope="module")
def seams(S):
    lib = S.load_library()
    return lib.svgr_hit_block(), lib.svgr_hit_chunk()


def record(what, **figures):
    """The differences actually seen, in the test's output (``pytest -s``)."""
    print(json.dumps(dict(what=what, **figures)))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32 if a.dtype == np.float32 else np.uint8)


def check_encoded(got, want_d, tol, spread, out, what):
    """An encoded result against the reference's clamped distances `want_d` with their tolerance: F64 within it; F32 / U8 exact
    except where the reference's value lies within the tolerance of a rounding boundary, there one ulp / one code.  Returns the
    largest absolute difference (F64) or the count of values that differ from the reference's (F32, U8: each by one step at the
    most), and the count of values that have a rounding boundary within the tolerance."""
    if out == "f64":
        assert got.dtype == np.float64 and got.shape == want_d.shape
        both_inf = np.isinf(got) & np.isinf(want_d) & (np.sign(got) == np.sign(want_d))
        diff = np.where(both_inf, 0.0, np.abs(got - np.where(both_inf, 0.0, want_d)))
        assert (diff <= tol).all(), f"{what}: {int((diff > tol).sum())} of {diff.size} beyond the tolerance, worst {diff.max():.3e}"
        return float(diff.max(initial=0.0)), 0
    v = R.unit(want_d, spread)
    vt = R.unit_tolerance(tol, spread)
    want = R.encode(want_d, spread, out)
    assert got.dtype == want.dtype and got.shape == want.shape
    lo, hi = R.f32_bounds(v, vt) if out == "f32" else R.u8_bounds(v, vt)
    near = lo != hi
    assert np.array_equal(got[~near], want[~near]), f"{what}: {int((got[~near] != want[~near]).sum())} values away from every rounding boundary differ"
    assert ((lo <= got) & (got <= hi)).all(), f"{what}: a value next to a rounding boundary is off by more than one step"
    if out == "u8":
        assert (hi.astype(np.int64) - lo.astype(np.int64)).max(initial=0) <= 1
    return float((got != want).sum()), int(near.sum())


def check_against_reference(S, batch, what, pts=None, grid=None, rules=None, spreads=(np.inf, 3.0)):
    """Every form of the query on one batch and one set of points against the reference.  Returns the reference's unclamped signed
    distances."""
    n_paths = batch.n_paths
    rules = np.zeros(n_paths, dtype=np.uint8) if rules is None else np.asarray(rules, dtype=np.uint8)
    edges, edge_path = batch.all_edges()
    if grid is not None:
        rr, cc = np.meshgrid(np.arange(grid[2]), np.arange(grid[3]), indexing="ij")
        points = np.stack([grid[0] + rr.ravel() + 0.5, grid[1] + cc.ravel() + 0.5], axis=1)
    else:
        points = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    inside = R.inside(edges, edge_path, n_paths, points, rules)
    big = R.magnitude(edges, edge_path, n_paths)
    d2 = R.min_d2(edges, edge_path, n_paths, points)          # (once: every form below is this and `inside`)
    raw = R.finish(d2, inside)
    worst = dict(f64=0.0, f32=0.0, u8=0.0)
    near = dict(f32=0, u8=0)
    for spread in spreads:
        for signed in (True, False):
            free = R.finish(d2, inside, np.inf, signed)
            want, tol = R.clamp(free, spread), R.tolerance(free, big[None, :], spread)
            u_free = R.union(free, np.inf)
            u_want, u_tol = R.clamp(u_free, spread), R.tolerance(u_free, big.max(initial=0.0), spread)
            for out in (("f64", "f32", "u8") if spread < np.inf else ("f64",)):
                got = batch.distance(pts, grid, spread=spread, out=out, signed=signed)
                assert got.shape == (len(points), n_paths)
                if out == "f64" and signed:
                    # the sign is hit testing's inside, exactly (signbit: a point ON the outline of a path that holds it is -0.0)
                    assert np.array_equal(np.signbit(got), inside), f"{what}: {int((np.signbit(got) != inside).sum())} signs differ from hit_ref's inside"
                if out == "f64" and not signed:
                    assert not np.signbit(got).any()
                d, k = check_encoded(got, want, tol, spread, out, f"{what} spread {spread} signed {signed} {out}")
                worst[out] = max(worst[out], d)
                got_u = batch.distance(pts, grid, spread=spread, out=out, signed=signed, union=True)
                assert got_u.shape == (len(points),)
                du, ku = check_encoded(got_u, u_want, u_tol, spread, out, f"{what} union spread {spread} signed {signed} {out}")
                worst[out] = max(worst[out], du)
                if out != "f64":
                    near[out] += k + ku
    record(what, points=len(points), paths=n_paths, edges=len(edges), max_abs_diff_f64=worst["f64"], values_off_f32=worst["f32"],
           values_off_u8=worst["u8"], near_boundary_f32=near["f32"], near_boundary_u8=near["u8"])
    return raw


# ---- the launch seams -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["1", "block-1", "block", "block+1", "4*block+1"])
def test_point_counts_at_the_workgroup_seams(S, seams, which):
    block, _chunk = seams
    n = {"1": 1, "block-1": block - 1, "block": block, "block+1": block + 1, "4*block+1": 4 * block + 1}[which]
    paths = [poly_path(S, p) for p in cases.random_polygons(77, 3)]
    raw = check_against_reference(S, make_batch(S, paths), f"points {which}", query_points(n, n))
    assert raw.shape == (n, 3)


@pytest.mark.parametrize("which", ["chunk-1", "chunk", "chunk+1", "2*chunk+1"])
def test_edge_counts_at_the_chunk_seams(S, seams, which):
    block, chunk = seams
    n = {"chunk-1": chunk - 1, "chunk": chunk, "chunk+1": chunk + 1, "2*chunk+1": 2 * chunk + 1}[which]
    batch = make_batch(S, [poly_path(S, cases.regular_polygon(n))])
    rng = np.random.default_rng(n)
    pts = np.concatenate([rng.uniform(5.0, 60.0, size=(block, 2)), cases.regular_polygon(n)[:16]])   # some corners themselves
    raw = check_against_reference(S, batch, f"edges {which}", pts)
    assert len(batch.all_edges()[0]) == n and 0.2 < (raw < 0).mean() < 0.9
    assert (raw[-16:, 0] == 0.0).all()           # on a corner, exactly


@pytest.mark.parametrize("n_paths", [1, 255, 256, 257])
def test_path_counts_at_the_table_seam(S, seams, n_paths):
    block, _chunk = seams
    assert block == 256
    tris = cases.tiny_triangles(n_paths, size=40.0, seed=n_paths)
    rules = (np.arange(n_paths) % 3 == 1).astype(np.uint8)
    batch = make_batch(S, [poly_path(S, t) for t in tris], rules)
    pts = np.concatenate([query_points(n_paths, 90), np.concatenate(tris)[-9:], [t.mean(axis=0) for t in tris[-40:]], [tris[0].mean(axis=0)]])
    raw = check_against_reference(S, batch, f"paths {n_paths}", pts, rules=rules)
    assert (raw[:, -1] < 0).any() and (raw[:, 0] < 0).any()          # the first and the last path hold a point


def test_a_grid_at_a_negative_origin(S, seams):
    paths = [poly_path(S, p - 8.0) for p in cases.random_polygons(11, 5)] + [S.Path([])]
    batch = make_batch(S, paths)
    grid = (-7, -12, 17, 33)           # not a multiple of the tile in either direction, two tiles by three
    raw = check_against_reference(S, batch, "grid 17 x 33", grid=grid)
    assert (raw[:, :5] < 0).any() and np.isinf(raw[:, 5]).all()
    rr, cc = np.meshgrid(np.arange(17), np.arange(33), indexing="ij")
    centres = np.stack([-7 + rr.ravel() + 0.5, -12 + cc.ravel() + 0.5], axis=1)
    for union in (False, True):
        for out, spread in (("f64", np.inf), ("f64", 2.5), ("f32", 2.5), ("u8", 2.5)):
            a, b = batch.distance(grid=grid, spread=spread, out=out, union=union), batch.distance(centres, spread=spread, out=out, union=union)
            assert np.array_equal(bits(a), bits(b))


def test_a_rule_mix_and_a_mirror(S, seams):
    block, _chunk = seams
    mirror = S.Transform().translate(40.0, 3.0).scale(-1.0, 0.75)
    paths = [poly_path(S, p) for p in cases.random_polygons(5, 4)] + [circle_path(S, (20.0, 20.0), 12.0), poly_path(S, cases.pentagram(18.0, (20.0, 20.0))),
                                                                     poly_path(S, cases.pentagram(18.0, (20.0, 20.0)))]
    rules = np.array([0, 1, 0, 1, 0, 0, 1], dtype=np.uint8)
    for name, tr in (("plain", None), ("mirror", mirror)):
        batch = make_batch(S, paths, rules, transform=tr)
        centre = np.array([[20.0, 20.0]]) if tr is None else tr(np.array([[20.0, 20.0]]))
        raw = check_against_reference(S, batch, f"rules {name}", np.concatenate([query_points(9, block + 7), centre]), rules=rules)
        # the middle of the pentagram: inside under nonzero, a hole under even-odd, the same distance; mirrored alike
        assert raw[-1, 5] < 0 and raw[-1, 6] > 0 and raw[-1, 5] == -raw[-1, 6] and raw[-1, 4] < 0
        assert abs(int(batch.winding(centre)[0, 5])) == 2


# ---- the cull ---------------------------------------------------------------------------------------------------------------------
def test_the_cull_cannot_be_seen(S, seams):
    block, _chunk = seams
    n_paths, size, spread = 300, 64, 3.0
    tris = cases.tiny_triangles(n_paths, size=float(size))
    rules = (np.arange(n_paths) % 2).astype(np.uint8)
    batch = make_batch(S, [poly_path(S, t) for t in tris], rules)
    grid = (0, 0, size, size)
    raw = check_against_reference(S, batch, "cull 64 x 64", grid=grid, rules=rules, spreads=(spread,))
    # every tile skips most paths, and different tiles skip different ones
    reach = np.abs(raw) < spread
    tiles = reach.reshape(size // 16, 16, size // 16, 16, n_paths).any(axis=(1, 3)).reshape(-1, n_paths)
    assert (tiles.mean(axis=1) < 0.35).all() and len({t.tobytes() for t in tiles}) == len(tiles) and reach.any(axis=0).all()
    # the same points in another order fall into other workgroups: the results are the same bits
    rr, cc = np.meshgrid(np.arange(size), np.arange(size), indexing="ij")
    centres = np.stack([rr.ravel() + 0.5, cc.ravel() + 0.5], axis=1)
    order = np.random.default_rng(1).permutation(len(centres))
    for union in (False, True):
        for out in ("f64", "f32", "u8"):
            for signed in (True, False):
                tiled = batch.distance(grid=grid, spread=spread, out=out, union=union, signed=signed)
                scattered = batch.distance(centres[order], spread=spread, out=out, union=union, signed=signed)
                assert np.array_equal(bits(tiled[order]), bits(scattered)), (union, out, signed)
    # and with the cull out of play (an infinite spread) the clamped values are the same again
    free = batch.distance(grid=grid)
    assert np.array_equal(bits(R.clamp(free, spread)), bits(batch.distance(grid=grid, spread=spread)))


def test_flattened_outlines_close(S):
    """The cull's one precondition: in what the flatten emits every vertex ends as many edges as it starts, bit for
    bit -- curves under a rotation, a polygon, glyph outlines."""
    with open(os.path.join(GOLDEN, "fonts", "varsynth.ttf"), "rb") as f:
        text, _advance = S.read_ttf(f.read()).str_to_path(48.0, "AVo#")
    paths = [circle_path(S, (20.3, 20.7), 12.0), poly_path(S, cases.pentagram()), circle_path(S, (100.1, 7.7), 300.0), text]
    for tr in (None, S.Transform().translate(40.0, 3.0).scale(-1.0, 0.75).rotate(0.3)):
        edges, edge_path = make_batch(S, paths, transform=tr).all_edges()
        e = edges.reshape(-1, 4)
        assert len(e) > 300
        for p in range(len(paths)):
            own = e[edge_path == p]
            starts, ends = own[:, :2], own[:, 2:]
            assert np.array_equal(starts[np.lexsort(starts.T)], ends[np.lexsort(ends.T)])


def test_scratch_passes(S, seams):
    block, _chunk = seams
    paths = [poly_path(S, p) for p in cases.random_polygons(3, 5)]
    batch = make_batch(S, paths)
    ctx = S.Context.get()
    pts = query_points(4, 1000)
    grid = (-3, 2, 37, 21)
    one = batch.distance(pts)          # (also flattens: not counted below)
    n0 = ctx.launches()
    again = batch.distance(pts)
    n1 = ctx.launches()
    small = batch.distance(pts, scratch_bytes=8 * 5 * block)          # one workgroup's rows
    n2 = ctx.launches()
    assert n1 - n0 == 1 and n2 - n1 == 4, (n0, n1, n2)
    assert np.array_equal(bits(one), bits(again)) and np.array_equal(bits(one), bits(small))
    for union, out, spread in ((False, "f64", np.inf), (True, "u8", 2.0), (False, "f32", 2.0)):
        whole = batch.distance(grid=grid, spread=spread, out=out, union=union)
        n3 = ctx.launches()
        passes = batch.distance(grid=grid, spread=spread, out=out, union=union, scratch_bytes=1)          # a row of tiles at a time
        assert ctx.launches() - n3 == 3 and np.array_equal(bits(whole), bits(passes))


# ---- an independent witness: the renderer -----------------------------------------------------------------------------------------
L_SHAPE = [(6.0, 10.0), (50.0, 10.0), (50.0, 22.0), (20.0, 22.0), (20.0, 58.0), (6.0, 58.0)]   # not symmetric under transposition


@pytest.mark.parametrize("which", ["circle", "L", "pentagram"])
def test_the_field_agrees_with_the_mask(S, which):
    path, rule, (ir, ic) = {"circle": (circle_path(S, (32.3, 31.7), 20.0), None, (32, 32)), "L": (poly_path(S, L_SHAPE), None, (12, 30)),
                            "pentagram": (poly_path(S, cases.pentagram()), "nonzero", (32, 32))}[which]
    size = 64
    layer, _hull = path.mask(S.Transform(), rule, viewport=(0, 0, size, size))
    cov = np.zeros((size, size))
    x, y = layer.offset
    cov[x:x + layer.height, y:y + layer.width] = layer.image[..., 0]
    d = path.sdf(S.Transform(), (0, 0, size, size), 8.0, np.float64, rule)
    assert d.shape == (size, size) and d.dtype == np.float64 and d.min() < -5.0 and d.max() == 8.0
    # a pixel whose centre is farther than half its diagonal from the outline lies wholly on one side of it
    deep, far = d <= -np.sqrt(0.5), d >= np.sqrt(0.5)
    skipped = 1.0 - (deep | far).mean()
    print(f"{which}: {int(deep.sum())} deep, {int(far.sum())} far, skipped share {skipped:.4f}")
    assert (cov[deep] >= 1 - 1e-9).all(), f"{int((cov[deep] < 1 - 1e-9).sum())} pixels deep inside are not fully covered"
    assert (cov[far] <= 1e-9).all(), f"{int((cov[far] > 1e-9).sum())} pixels far outside are covered"
    assert skipped <= 0.12 and deep.sum() > 100
    # the encodings of the same field, and the unsigned distance of the library layer
    f32, u8 = path.sdf(S.Transform(), (0, 0, size, size), 8.0, fill_rule=rule), path.sdf(S.Transform(), (0, 0, size, size), 8.0, np.uint8, rule)
    assert f32.dtype == np.float32 and np.array_equal(f32, R.encode_f32(d, 8.0)) and np.array_equal(u8, R.encode_u8(d, 8.0))
    pts = np.array([(ir + 0.5, ic + 0.5), (0.5, 0.5), (np.nan, 1.0)])
    signed, unsigned = path.distance(pts, fill_rule=rule), path.distance(pts, fill_rule=rule, signed=False)
    assert signed.shape == (3,) and signed[0] < 0 < signed[1] and np.array_equal(unsigned, np.abs(signed)) and signed[2] == np.inf
    assert path.distance(pts, fill_rule=rule, spread=8.0).tolist() == [d[ir, ic], d[0, 0], 8.0]


# ---- glyph atlases ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("face", ["varsynth.ttf", "varsynth.ttf@wght", "cffsynth.otf"])
def test_sdf_atlas_on_the_committed_fonts(S, face):
    name, _, axis = face.partition("@")
    with open(os.path.join(GOLDEN, "fonts", name), "rb") as f:
        font = S.read_font(f.read())
    if axis:
        ax = font.axes[0]
        font = font.instance({ax.tag: (ax.default + ax.maximum) / 2.0 if ax.maximum > ax.default else (ax.default + ax.minimum) / 2.0})
    size, spread, text = 40.0, 3.5, "AVo #D VA"
    atlas = font.sdf_atlas(text, size, spread, max_cols=100)
    placed, _adv = font.str_to_glyphs(text)
    glyphs = {id(g): g for _pen, g in placed}
    assert isinstance(atlas, S.SdfAtlas) and atlas.image.dtype == np.uint8 and len(atlas.cells) == len(glyphs) and atlas.image.shape[1] <= 100
    assert atlas.size == size and atlas.spread == spread
    scale, drawn, taken = size / font.units_per_em, 0, np.zeros(atlas.image.shape, dtype=np.int32)
    from svgrasterize_amd import sdf

    for glyph in glyphs.values():
        cell = atlas.cells[sdf.glyph_key(glyph)]
        assert cell.advance == glyph.advance * scale
        if not glyph.path.subpaths:
            assert (cell.rows, cell.cols) == (0, 0)          # the space
            continue
        drawn += 1
        taken[cell.row0:cell.row0 + cell.rows, cell.col0:cell.col0 + cell.cols] += 1
        got = atlas.image[cell.row0:cell.row0 + cell.rows, cell.col0:cell.col0 + cell.cols]
        assert got.shape == (cell.rows, cell.cols)
        # the cell is the glyph's own field under the cell's transform, exactly: the same edges through the same kernel
        tr = S.Transform().matrix(*sdf.cell_m6(cell, scale))
        alone = glyph.path.sdf(tr, (cell.row0, cell.col0, cell.rows, cell.cols), spread, np.uint8)
        assert np.array_equal(got, alone)
        # the border ring is 0: the glyph is at least the spread inside its cell
        assert not got[0].any() and not got[-1].any() and not got[:, 0].any() and not got[:, -1].any()
        # a point known to be inside the glyph: where the mask of the same outline is fully covered
        home = S.Transform().matrix(0.0, -scale, float(cell.origin_row), scale, 0.0, float(cell.origin_col))          # the cell at the origin
        layer, _hull = glyph.path.mask(home, None, viewport=(0, 0, cell.rows, cell.cols))
        cov = np.zeros((cell.rows, cell.cols))
        r, c = layer.offset
        cov[r:r + layer.height, c:c + layer.width] = layer.image[..., 0]
        full = np.argwhere(cov >= 1 - 1e-9)
        assert len(full) > 10 and (got[full[:, 0], full[:, 1]] > 127).all()
    assert drawn >= 3 and taken.max() == 1
    # the other dtypes are the same field
    f64 = font.sdf_atlas(text, size, spread, np.float64, max_cols=100)
    assert f64.cells == atlas.cells and np.array_equal(R.encode_u8(f64.image, spread), atlas.image)
    assert np.array_equal(font.sdf_atlas(text, size, spread, np.float32, max_cols=100).image, R.encode_f32(f64.image, spread))


# ---- errors and empty queries -----------------------------------------------------------------------------------------------------
def test_errors_and_empty_queries_launch_nothing(S, seams):
    from svgrasterize_amd import _abi

    ctx = S.Context.get()
    lib = S.load_library()
    batch = make_batch(S, [poly_path(S, cases.SQUARE), poly_path(S, cases.TRIANGLE)])
    batch.distance(np.zeros((1, 2)))   # (flattened now: what follows must not launch)
    n0 = ctx.launches()
    pts, out = np.zeros((3, 2)), np.zeros((3, 2))
    grid = _abi._i64x4((0, 0, 1, 3))

    def call(points, grid, n, spread, flags, out=out):
        _abi._check(lib.svgr_batch_distance(batch.handle, _abi.ptr(points) if points is not None else None, grid, n, spread, flags, 0, _abi.ptr(out)))

    for spread in (0.0, -2.0, float("nan"), -np.inf):
        with pytest.raises(ValueError, match="spread"):          # (SVGR_E_INVALID, with a message)
            call(pts, None, 3, spread, _abi.SDF_F64)
    for flags in (_abi.SDF_F32, _abi.SDF_U8, _abi.SDF_U8 | _abi.SDF_UNION):
        with pytest.raises(ValueError, match="finite spread"):
            call(pts, None, 3, np.inf, flags)
    with pytest.raises(ValueError, match="one of them"):
        call(pts, grid, 3, 2.0, _abi.SDF_F64)
    with pytest.raises(ValueError, match="one of them"):
        call(None, None, 3, 2.0, _abi.SDF_F64)
    for flags in (16, 3, 1 << 20, -1):
        with pytest.raises(ValueError, match="unknown"):
            call(pts, None, 3, 2.0, flags)
    with pytest.raises(ValueError, match="rows x cols"):
        call(None, grid, 4, 2.0, _abi.SDF_F64)
    assert ctx.launches() == n0 and not out.any()
    assert batch.distance(np.zeros((0, 2))).shape == (0, 2) and batch.distance(grid=(0, 0, 0, 7), union=True).shape == (0,)
    with pytest.raises(ValueError):
        batch.distance()
    with pytest.raises(ValueError):
        batch.distance(np.zeros((4, 3)))
    # 31 bits, for the per-path form only
    with pytest.raises(_abi.SvgrError, match="status -5"):     # (SVGR_E_OVERFLOW)
        _abi._check(lib.svgr_batch_distance(batch.handle, None, _abi._i64x4((0, 0, 1 << 15, 1 << 15)), 1 << 30, 2.0, _abi.SDF_F64, 0, _abi.ptr(out)))
    assert ctx.launches() == n0
    # (svgr_batch_create refuses a batch without paths; one whose only path has no segments is +inf, or the spread, away)
    hollow = make_batch(S, [S.Path([])])
    assert hollow.distance(np.zeros((5, 2))).tolist() == [[np.inf]] * 5 and hollow.distance(np.zeros((5, 2)), spread=2.0, out="u8", union=True).tolist() == [0] * 5
