"""Multi-channel distance fields on the CPU: the per-lane header (csrc/svgr_msdf.h, through tests/msdf_harness.cpp) against the numpy
reference (tests/msdf_ref.py), exactly; the A channel against tests/sdf_ref.py; mitres worked out by hand on a square and an L; the
sign repair; the colouring of outlines; encodings; and every error of the library layer, all without a device."""
import math
import os
import re

import numpy as np
import pytest

import svgrasterize_amd as S
from svgrasterize_amd import _abi, msdf, sdf
from svgrasterize_amd.geometry import PATH_CLOSED, PATH_CUBIC, PATH_LINE
from tests import msdf_cases as cases
from tests import msdf_ref as M
from tests import sdf_cases
from tests import sdf_ref as R
from tests.test_sdf_host import harness_out_of_reach, host_font
from tests.util import ROOT


def same(a, b):
    """Bit for bit, but for the sign of a zero."""
    return a.shape == b.shape and np.array_equal(a, b)


def both(shape, points, spread):
    want, repairs = M.msdf(shape.edges, shape.edge_path, shape.colour, shape.rules, shape.group_off, shape.orient, points, spread)
    got = cases.harness(shape, points, spread)
    assert same(got, want), f"{int((got != want).sum())} of {got.size} values differ between header and reference"
    return want, repairs


def medians(v):
    return M.median(v[:, 0], v[:, 1], v[:, 2])


# ---- header == reference ----------------------------------------------------------------------------------------------------------
def test_constants_and_exports():
    h = cases.lib()
    assert h.mh_edge_doubles() == 8 and h.mh_sdf_edge_doubles() == 6
    assert "svgr_batch_msdf" in _abi.EXPORTS and callable(_abi.Batch.msdf)
    hdr = open(os.path.join(ROOT, "include", "svgr.h")).read()
    assert re.search(r"\bint svgr_batch_msdf\(svgr_batch\* batch, const double\* points, const int64_t\* grid, int64_t n_points, double spread, int flags,", hdr)
    defines = {k: int(v) for k, v in re.findall(r"#define (SVGR_MSDF_[A-Z0-9_]+) (\d+)", hdr)}
    assert defines == {"SVGR_MSDF_F64": _abi.SDF_F64, "SVGR_MSDF_F32": _abi.SDF_F32, "SVGR_MSDF_U8": _abi.SDF_U8, "SVGR_MSDF_ENCODING_MASK": 3}
    assert _abi.load_library().svgr_abi_version() == 6
    e = np.array([1.0, 2.0, 4.0, 6.0])
    q = np.zeros(8)
    h.mh_prepare(cases.ptr(e), cases.ptr(q))
    assert q.tolist() == [1.0, 2.0, 3.0, 4.0, 1.0 / 25.0, 4.0, 6.0, 1.0 / 5.0] and same(M.prepare(e)[0], q)
    h.mh_prepare(cases.ptr(np.array([3.0, 3.0, 3.0, 3.0])), cases.ptr(q))
    assert q.tolist() == [3.0, 3.0, 0.0, 0.0, 0.0, 3.0, 3.0, 0.0]


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_header_equals_reference_on_random_shapes(seed):
    shape = cases.random_shape(seed)
    pts = cases.random_points(seed, shape)
    assert (np.diff(shape.off) == 0).any() and (np.diff(shape.group_off) == 0).any()            # an empty path, an empty group
    for spread in (np.inf, 3.0, 0.75):
        want, _repairs = both(shape, pts, spread)
        assert same(want[:, 3], M.a_channel(shape.edges, shape.edge_path, shape.rules, shape.group_off, shape.orient, pts, spread))
        assert (want[-4:-1] == spread).all()                                   # NaN and infinite points: +spread in all four
        assert (want[:, 3] < 0).any()
        assert (np.abs(want) <= spread).all()
        if spread < np.inf:
            assert (want[-1] == spread).all()
        # the median's side is A's in every group (the guarantee is a group's: the minimum over groups that overlap or lie within
        # the spread of each other can take its three channels from different groups)
        for g in range(len(shape.orient)):
            one, _repairs = both(shape.only(g), pts, spread)
            assert np.array_equal(medians(one) < 0, one[:, 3] < 0)


def test_no_groups_and_groups_without_edges():
    pts = np.array([(1.0, 2.0), (cases.NAN, 0.0)])
    for shape in (cases.Shape([]), cases.Shape([(1, [])]), cases.Shape([(1, [(7, np.zeros((0, 4)))]), (-1, [])])):
        for spread in (np.inf, 2.0):
            want, repairs = both(shape, pts, spread)
            assert (want == spread).all() and repairs == 0


def test_the_result_does_not_depend_on_the_edges_order():
    """The last tie-break: an edge and its reverse are the same distance away under the same angle; their perp differ in sign."""
    square = cases.hit_cases.polygon_edges(cases.SQUARE)
    doubled = np.concatenate([square, square[:, [2, 3, 0, 1]], square])              # forth, back and forth again: closed, winding 1
    pts = np.concatenate([sdf_cases.integer_points(3, 120, extent=7), cases.square_wedge_points()[0]])
    rng = np.random.default_rng(0)
    first = None
    for _ in range(4):
        order = rng.permutation(len(doubled))
        shape = cases.Shape([(1, [(7, doubled[order])])])
        want, _repairs = both(shape, pts, np.inf)
        first = want if first is None else first
        assert same(want, first)
    # A is the plain square's; outside, the reverse edge wins the tie (the larger perp), its side is the wrong one, and the repair
    # puts A in its place
    plain, _repairs = both(cases.Shape([(1, [(7, square)])]), pts, np.inf)
    assert same(first[:, 3], plain[:, 3]) and np.array_equal(medians(first) < 0, first[:, 3] < 0)
    outside = plain[:, 3] > 0
    assert outside.any() and (first[outside, :3] == first[outside, 3:]).all() and (plain[outside, 0] <= plain[outside, 3]).all()


# ---- exact geometry ---------------------------------------------------------------------------------------------------------------
def test_mitres_of_a_square():
    shape = cases.Shape([cases.one_edge_a_path(cases.SQUARE, cases.SQUARE_COLOURS)])
    pts, legs = cases.square_wedge_points()
    inside = np.array([(9.0, 9.5), (3.0, 2.5), (6.0, 6.0), (2.25, 9.0), (7.5, 3.25), (9.75, 6.0), (4.0, 9.0)])
    for spread in (np.inf, 16.0):
        want, repairs = both(shape, np.concatenate([pts, inside]), spread)
        assert repairs == 0                                    # (a condition: the repair hides no colouring bug below)
        out, ins = want[:len(pts)], want[len(pts):]
        # outside, in a vertex wedge: the median is the mitre, max of the distances to the two adjacent edges' lines; A is Euclidean
        assert medians(out).tolist() == np.maximum(legs[:, 0], legs[:, 1]).tolist()
        assert out[:, 3].tolist() == legs[:, 2].tolist()
        # inside: minus the distance to the nearest side
        sides = np.stack([inside[:, 1] - 2.0, 10.0 - inside[:, 0], 10.0 - inside[:, 1], inside[:, 0] - 2.0], axis=1)
        assert medians(ins).tolist() == (-sides.min(axis=1)).tolist() and ins[:, 3].tolist() == (-sides.min(axis=1)).tolist()
    # the channels themselves at (12.5, 11): red the larger of the two, green edge 2's line, blue edge 1's
    assert cases.harness(shape, [(12.5, 11.0)]).tolist() == [[2.5, 1.0, 2.5, math.hypot(2.5, 1.0)]]


def test_mitres_of_an_l_shape():
    shape = cases.Shape([cases.one_edge_a_path(cases.L_SHAPE, cases.L_COLOURS)])
    legs = np.array(cases.LEGS[:3])
    inside = np.stack([8.0 - legs[:, 0], 8.0 - legs[:, 1]], axis=1)              # inside the L, in the wedge of the reflex corner
    notch = np.stack([8.0 + legs[:, 0], 8.0 + legs[:, 1]], axis=1)               # outside, in the notch
    want, repairs = both(shape, np.concatenate([inside, notch]), np.inf)
    assert repairs == 0
    ins, out = want[:3], want[3:]
    # inside a reflex corner the median is the mitre again (minus the LARGER distance), A minus the distance to the vertex
    assert medians(ins).tolist() == (-np.maximum(legs[:, 0], legs[:, 1])).tolist() and ins[:, 3].tolist() == (-legs[:, 2]).tolist()
    # in the notch both are the distance to the nearer side
    assert medians(out).tolist() == np.minimum(legs[:, 0], legs[:, 1]).tolist() and out[:, 3].tolist() == medians(out).tolist()


# ---- the repair -------------------------------------------------------------------------------------------------------------------
def test_the_repair_puts_the_median_on_as_side():
    hole = [(8.0, 8.0), (24.0, 8.0), (24.0, 24.0), (8.0, 24.0)]                   # counter-clockwise like the outline: wrongly oriented
    outer = [(0.0, 0.0), (32.0, 0.0), (32.0, 32.0), (0.0, 32.0)]
    shape = cases.Shape([(1, [(c, cases.hit_cases.polygon_edges(outer)[k:k + 1]) for k, c in enumerate(cases.SQUARE_COLOURS)] +
                             [(c, cases.hit_cases.polygon_edges(hole)[k:k + 1]) for k, c in enumerate(cases.SQUARE_COLOURS)])], rules=[1])
    rr, cc = np.meshgrid(np.arange(-2, 34), np.arange(-2, 34), indexing="ij")
    pts = np.stack([rr.ravel() + 0.5, cc.ravel() + 0.5], axis=1)
    for spread in (np.inf, 4.0):
        want, repairs = both(shape, pts, spread)
        in_hole = ((pts > 8.0) & (pts < 24.0)).all(axis=1)
        assert repairs > 0 and (want[in_hole, 3] > 0).all()                   # even-odd: the hole is outside
        assert np.array_equal(medians(want) < 0, want[:, 3] < 0)
        near = in_hole & (np.abs(pts - 16.0).max(axis=1) > 5.0)              # near the hole's edges the channels said "inside"
        assert (want[near, :3] == want[near, 3:]).all()


# ---- colour_edges -----------------------------------------------------------------------------------------------------------------
def polygon(pts):
    pts = [tuple(map(float, p)) for p in pts]
    return S.Path([[(PATH_LINE, [list(a), list(b)]) for a, b in zip(pts, pts[1:])] + [(PATH_CLOSED, [list(pts[-1]), list(pts[0])])]])


def circle(r=10.0):
    k = 0.5522847498307936 * r
    quads = [[(r, 0), (r, k), (k, r), (0, r)], [(0, r), (-k, r), (-r, k), (-r, 0)], [(-r, 0), (-r, -k), (-k, -r), (0, -r)], [(0, -r), (k, -r), (r, -k), (r, 0)]]
    return S.Path([[(PATH_CUBIC, [list(map(float, p)) for p in q]) for q in quads]])


def teardrop():
    """Two cubics: a corner at the origin, smooth at (0, 10)."""
    return S.Path([[(PATH_CUBIC, [[0.0, 0.0], [6.0, 4.0], [5.0, 10.0], [0.0, 10.0]]), (PATH_CUBIC, [[0.0, 10.0], [-5.0, 10.0], [-6.0, 4.0], [0.0, 0.0]])]])


def masks_in_order(path, angle=3.0):
    return [msdf.colour_subpath(msdf._pieces(sub), angle)[1] for sub in path.subpaths]


def is_permutation_of_packed(path):
    soups = msdf.colour_edges(path)
    segs, kinds = path.packed()
    got = np.concatenate([np.column_stack([s, k]) for _m, s, k in soups])
    want = np.column_stack([segs, kinds])
    return got.shape == want.shape and sorted(map(tuple, got.tolist())) == sorted(map(tuple, want.tolist()))


def test_colour_edges():
    square = polygon(cases.SQUARE)
    assert masks_in_order(square) == [[6, 5, 3, 5]] and [m for m, _s, _k in msdf.colour_edges(square)] == [6, 5, 3]
    assert is_permutation_of_packed(square)
    assert masks_in_order(circle()) == [[7, 7, 7, 7]] and is_permutation_of_packed(circle())
    # one corner, two segments: cut into six, three colours from the corner on
    drop = teardrop()
    pieces, masks = msdf.colour_subpath(msdf._pieces(drop.subpaths[0]))
    assert masks == [6, 6, 5, 5, 3, 3] and len(pieces) == 6 and all(p.shape == (4, 2) for p in pieces)
    assert all(np.array_equal(a[-1], b[0]) for a, b in zip(pieces, pieces[1:])) and np.array_equal(pieces[0][0], pieces[-1][-1])
    assert np.allclose(pieces[0][-1], S.Path([[drop.subpaths[0][0]]]).packed()[0].reshape(4, 2)[0] * (8 / 27) + np.array([6.0, 4.0]) * (12 / 27) +
                       np.array([5.0, 10.0]) * (6 / 27) + np.array([0.0, 10.0]) * (1 / 27))         # the cubic at t = 1/3
    assert sum(len(s) for _m, s, _k in msdf.colour_edges(drop)) == 6
    # seven corners: the last span is magenta, so that it differs from the first (cyan) and from the one before (yellow)
    hepta = polygon(cases.hit_cases.regular_polygon(7))
    assert masks_in_order(hepta) == [[6, 5, 3, 6, 5, 3, 5]] and is_permutation_of_packed(hepta)
    # adjacent spans never share all their channels, across the wrap as well
    for n in range(2, 14):
        masks = masks_in_order(polygon(cases.hit_cases.regular_polygon(n)) if n > 2 else S.Path([[(PATH_LINE, [[0.0, 0.0], [4.0, 0.0]]), (PATH_CLOSED, [[4.0, 0.0], [0.0, 0.0]])]]))[0]
        assert len(masks) == n and all(a != b and a in (6, 5, 3) for a, b in zip(masks, masks[1:] + masks[:1]))
    # a smooth joint inside a span: the rounded square keeps four corners' worth of spans only where it turns sharply
    blunt = polygon([(0, 0), (10, 0), (20, 0.5), (20, 10), (0, 10)])              # (10, 0) turns by under 3 degrees: no corner
    assert masks_in_order(blunt) == [[6, 6, 5, 3, 5]] and masks_in_order(blunt, angle=math.pi) == [[6, 5, 3, 6, 5]]
    # two subpaths are coloured each on its own; a segment that is a point is white
    two = S.Path(polygon(cases.SQUARE).subpaths + circle().subpaths)
    assert masks_in_order(two) == [[6, 5, 3, 5], [7, 7, 7, 7]] and [m for m, _s, _k in msdf.colour_edges(two)] == [7, 6, 5, 3]
    dot = S.Path([[(PATH_LINE, [[0.0, 0.0], [4.0, 0.0]]), (PATH_LINE, [[4.0, 0.0], [4.0, 0.0]]), (PATH_LINE, [[4.0, 0.0], [4.0, 4.0]]), (PATH_CLOSED, [[4.0, 4.0], [0.0, 0.0]])]])
    assert masks_in_order(dot) == [[6, 7, 5, 3]]
    assert msdf.colour_edges(S.Path([])) == []


def test_orientation_flips_with_a_mirror():
    square = polygon(cases.SQUARE)
    backwards = polygon(cases.SQUARE[::-1])
    mirror = S.Transform().scale(-1.0, 1.0)
    assert msdf.orientation(square) == 1 and msdf.orientation(backwards) == -1
    assert msdf.orientation(square, mirror.m6()) == -1 and msdf.orientation(backwards, mirror.m6()) == 1
    assert msdf.orientation(square, S.Transform().rotate(2.0).m6()) == 1
    assert msdf.orientation(S.Path([])) == 1 and msdf.orientation(square, np.zeros(6)) == 1
    # the convention of svgr_batch_msdf: sigma * ((a1 - a0) * (pb - b0) - (pa - a0) * (b1 - b0)) > 0 inside
    (a0, b0), (a1, b1) = cases.SQUARE[0], cases.SQUARE[1]
    assert msdf.orientation(square) * ((a1 - a0) * (6.0 - b0) - (6.0 - a0) * (b1 - b0)) > 0


# ---- the kernel's cull ------------------------------------------------------------------------------------------------------------
def test_a_group_out_of_reach_is_exactly_the_spread_away_in_every_channel():
    """The claim k_msdf_distance's cull rests on: where sdf_out_of_reach holds for the union of the extents of a
    group's paths, the group's R, G, B and A are +spread at every point of the box."""
    rng = np.random.default_rng(7)
    for i in range(12):
        poly, spread, pts = sdf_cases.reach_case(rng, i % sdf_cases.REACH_SIDES, ("above", "far")[i // 4 % 2])
        edges = sdf_cases.polygon_edges(poly)
        k = 2 + i % 3                                                      # the polygon's edges dealt out to 2 .. 4 paths
        paths = [(int(rng.integers(1, 8)), edges[j::k]) for j in range(k)]
        shape = cases.Shape([(int(rng.choice([-1, 1])), paths)], [i & 1])
        extents = np.array([sdf_cases.extent_of(e.reshape(-1, 2)) for _, e in paths if len(e)])
        union = np.concatenate([extents[:, :2].min(axis=0), extents[:, 2:].max(axis=0)])
        assert harness_out_of_reach(union, sdf_cases.box_of(pts), spread).all(), f"group {i} is no case: it is within reach"
        got = cases.harness(shape, pts, spread)
        assert (got == spread).all(), f"group {i}, out of reach at spread {spread!r}: {got.tolist()}"


# ---- encodings and errors ---------------------------------------------------------------------------------------------------------
def test_encodings_per_channel():
    shape = cases.Shape([cases.one_edge_a_path(cases.SQUARE, cases.SQUARE_COLOURS)])
    spread = 4.0
    d = sdf_cases.u8_tie_distances(spread)
    pts = np.stack([10.0 + d, 10.0 + d / 2.0], axis=1)          # around the vertex (10, 10): the channels differ
    want, _repairs = both(shape, pts, spread)
    assert (want[:, 0] != want[:, 1]).any() and (want[:, 3] != want[:, 0]).any()
    f32, u8 = cases.harness_encode(want, spread)
    assert f32.shape == want.shape and np.array_equal(f32, R.encode_f32(want, spread)) and np.array_equal(u8, R.encode_u8(want, spread))
    assert np.array_equal(u8, _abi.sdf_encode(want, spread, "u8")) and np.array_equal(f32, _abi.sdf_encode(want, spread, "f32"))
    # the ties themselves: k + 1/2 goes to the even code in whatever channel it turns up
    flat = np.repeat(d[:, None], 4, axis=1)
    f32, u8 = cases.harness_encode(flat, spread)
    assert np.array_equal(u8, R.encode_u8(flat, spread)) and (u8 == u8[:, :1]).all()
    exact = R.unit(d, spread) * 255.0
    ties = exact - np.floor(exact) == 0.5
    assert ties.sum() >= 1 and (u8[ties, 0] % 2 == 0).all()
    # sdf.median is the shader's median, on any dtype
    assert np.array_equal(sdf.median(u8), np.sort(u8[:, :3], axis=1)[:, 1]) and sdf.median(u8).dtype == np.uint8
    assert np.array_equal(sdf.median(want), np.sort(want[:, :3], axis=1)[:, 1]) and sdf.median(want[None]).shape == (1, len(want))
    h = cases.lib()
    assert [h.mh_median(*p) for p in ((1.0, 2.0, 3.0), (3.0, 1.0, 2.0), (2.0, 3.0, 1.0), (2.0, 2.0, 5.0), (-1.0, -1.0, -1.0))] == [2.0, 2.0, 2.0, 2.0, -1.0]


def test_errors_before_any_device_work():
    path, font = polygon(cases.SQUARE), host_font()
    if _abi.load_library().svgr_device_count() == 0:
        with pytest.raises(_abi.SvgrError):
            path.msdf(None, (0, 0, 4, 4))                    # (a good call does reach for the device, and there is none)
    for spread in (0.0, -1.0, float("nan"), -np.inf, "wide"):
        with pytest.raises(ValueError, match="spread"):
            path.msdf(None, (0, 0, 8, 8), spread)
        with pytest.raises(ValueError, match="spread"):
            font.msdf_atlas("A", 48.0, spread)
    for dtype in (np.int32, np.float16, "bool", object):
        with pytest.raises(TypeError):
            path.msdf(None, (0, 0, 8, 8), 4.0, dtype=dtype)
        with pytest.raises(TypeError):
            font.msdf_atlas("A", 48.0, 4.0, dtype=dtype)
    for dtype in (np.float32, np.uint8):
        with pytest.raises(ValueError, match="finite spread"):
            path.msdf(None, (0, 0, 8, 8), np.inf, dtype=dtype)
    with pytest.raises(ValueError, match="finite spread"):
        font.msdf_atlas("A", 48.0, np.inf, dtype=np.float64)
    with pytest.raises(ValueError, match="fill rule"):
        path.msdf(None, (0, 0, 8, 8), 4.0, fill_rule="odd")
    with pytest.raises(ValueError, match="viewport"):
        path.msdf(None, (0, 0, -1, 8), 4.0)
    for angle in (-0.1, 4.0, float("nan"), "sharp"):
        with pytest.raises(ValueError, match="angle"):
            path.msdf(None, (0, 0, 8, 8), 4.0, angle=angle)
        with pytest.raises(ValueError, match="angle"):
            font.msdf_atlas("A", 48.0, 4.0, angle=angle)
    for size in (0.0, -3.0, np.inf):
        with pytest.raises(ValueError, match="size"):
            font.msdf_atlas("A", size, 4.0)
    with pytest.raises(ValueError, match="max_cols"):
        font.msdf_atlas("A", 48.0, 4.0, max_cols=0)
    # an empty path, an empty viewport, a space and an empty string touch no device
    empty = S.Path([])
    assert np.array_equal(empty.msdf(None, (0, 0, 2, 3), 4.0, np.float64), np.full((2, 3, 4), 4.0))
    assert np.array_equal(empty.msdf(None, (0, 0, 2, 3)), np.zeros((2, 3, 4), dtype=np.float32)) and empty.msdf(None, (0, 0, 2, 3), 4.0, np.uint8).dtype == np.uint8
    assert path.msdf(None, (0, 0, 0, 5), 4.0).shape == (0, 5, 4)
    for string, keys in (("", []), ("  ", [" "])):
        for dtype in (np.uint8, np.float32, np.float64):
            atlas = font.msdf_atlas(string, 48.0, 4.0, dtype=dtype)
            assert isinstance(atlas, S.SdfAtlas) and atlas.image.shape == (0, 0, 4) and atlas.image.dtype == dtype and list(atlas.cells) == keys
    assert font.msdf_atlas(" ", 48.0, 4.0).cells == font.sdf_atlas(" ", 48.0, 4.0).cells
    # Batch.msdf's own argument checks sit in front of the C call
    for call in (lambda: _abi.Batch.msdf(None, [7], [0, 1], [1], np.zeros((1, 2)), out="f16"), lambda: _abi.Batch.msdf(None, [7], [0, 1], [1], np.zeros((1, 2)), spread=0.0),
                 lambda: _abi.Batch.msdf(None, [7], [0, 1], [1], np.zeros((1, 2)), spread=np.inf, out="u8")):
        with pytest.raises(ValueError):
            call()
