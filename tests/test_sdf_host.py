"""Signed distance fields on the CPU: the per-lane header (csrc/svgr_sdf.h, through tests/sdf_harness.cpp) against the numpy
reference (tests/sdf_ref.py), exactly; both against exact rational arithmetic, 3-4-5 configurations and the closed-form distance
to a box; the sign under both fill rules; clamp, encodings and uint8 ties; the union's documented value; the atlas packer; and every
error of the library layer, all without a device."""
import ctypes
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import svgrasterize_amd as S
from svgrasterize_amd import _abi, sdf
from svgrasterize_amd.fonts import Font, Glyph
from svgrasterize_amd.geometry import PATH_CLOSED, PATH_LINE
from tests import hit_ref
from tests import sdf_cases as cases
from tests import sdf_ref as R
from tests.util import ROOT, host_build

P = ctypes.c_void_p


def lib():
    h = host_build("sdf_harness")
    h.sh_clamp.restype = ctypes.c_double
    h.sh_clamp.argtypes = [ctypes.c_double, ctypes.c_double]
    h.sh_terms.argtypes = [P, ctypes.c_double, ctypes.c_double, P]
    return h


def ptr(a):
    return a.ctypes.data_as(P)


def harness_distance(edges, off, points, rules=None, spread=np.inf, signed=True):
    edges = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1, 4)
    off = np.ascontiguousarray(off, dtype=np.int32)
    pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2)
    n_paths = len(off) - 1
    rules = np.zeros(n_paths, dtype=np.uint8) if rules is None else np.ascontiguousarray(rules, dtype=np.uint8)
    out = np.full((len(pts), n_paths), 99.0)
    lib().sh_distance(ptr(edges), ptr(off), ptr(rules), ctypes.c_longlong(n_paths), ptr(pts), ctypes.c_longlong(len(pts)), ctypes.c_double(spread),
                      int(signed), ptr(out))
    return out


def harness_union(d, spread):
    d = np.ascontiguousarray(d, dtype=np.float64)
    out = np.full(len(d), 99.0)
    lib().sh_union(ptr(d), ctypes.c_longlong(d.shape[0]), ctypes.c_longlong(d.shape[1]), ctypes.c_double(spread), ptr(out))
    return out


def harness_encode(d, spread):
    d = np.ascontiguousarray(d, dtype=np.float64).reshape(-1)
    f32, u8 = np.zeros(len(d), dtype=np.float32), np.zeros(len(d), dtype=np.uint8)
    lib().sh_encode(ptr(d), ctypes.c_longlong(len(d)), ctypes.c_double(spread), ptr(f32), ptr(u8))
    return f32, u8


def same(a, b):
    """Bit for bit, but for the sign of a zero."""
    return a.shape == b.shape and np.array_equal(a, b)


def both(edges, ep, off, points, rules=None, spread=np.inf, signed=True):
    """The reference's and the harness' distances, asserted identical."""
    n_paths = len(off) - 1
    want = R.distance(edges, ep, n_paths, points, rules, spread, signed)
    got = harness_distance(edges, off, points, rules, spread, signed)
    assert same(got, want), f"{int((got != want).sum())} of {got.size} distances differ between header and reference"
    return want


# ---- header == reference ----------------------------------------------------------------------------------------------------------
def test_constants_and_exports():
    h = lib()
    assert h.sh_edge_doubles() == 6 and [h.sh_elem_bytes(k) for k in range(3)] == [8, 4, 1]
    assert "svgr_batch_distance" in _abi.EXPORTS and all(name in S.__all__ for name in ("SdfAtlas", "SdfCell"))
    hdr = open(os.path.join(ROOT, "include", "svgr.h")).read()
    defines = {k: int(v) for k, v in re.findall(r"#define (SVGR_SDF_[A-Z0-9_]+) (\d+)", hdr)}
    assert defines == {"SVGR_SDF_F64": _abi.SDF_F64, "SVGR_SDF_F32": _abi.SDF_F32, "SVGR_SDF_U8": _abi.SDF_U8, "SVGR_SDF_ENCODING_MASK": 3,
                       "SVGR_SDF_UNION": _abi.SDF_UNION, "SVGR_SDF_UNSIGNED": _abi.SDF_UNSIGNED}


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_header_equals_reference_on_random_polygons(seed):
    polys = cases.random_polygons(seed, 6)
    polys.insert(2, np.zeros((0, 2)))   # an empty path between others
    edges, ep, off = cases.edge_table(polys)
    rng = np.random.default_rng(seed)
    corners = np.concatenate([p for p in polys if len(p)])
    mids = (edges[:, :2] + edges[:, 2:]) / 2.0                  # on the edges (exactly representable: integer corners)
    pts = np.concatenate([rng.uniform(-5.0, 45.0, size=(300, 2)), cases.integer_points(seed, 100), corners, mids,
                          [(cases.NAN, 5.0), (5.0, cases.INF), (-cases.INF, cases.NAN), (1e9, -1e9)]])
    rules = (np.arange(len(polys)) % 2).astype(np.uint8)
    for spread, signed in ((np.inf, True), (3.0, True), (0.75, False), (np.inf, False)):
        want = both(edges, ep, off, pts, rules, spread, signed)
        cap = spread
        assert (want[:, 2] == cap).all()                       # the empty path: +inf, or the spread
        assert (want[-4:-1] == cap).all()                      # NaN and infinite points: +inf away from everything, outside
        assert np.isfinite(want[-1, [0, 1, 3]]).all() or spread < np.inf
        if signed:
            ins = R.inside(edges, ep, len(polys), pts, rules)
            assert np.array_equal(want < 0, ins & (want != 0)) and (want < 0).any()
        else:
            assert (want >= 0).all()
    # on a corner the distance is exactly 0 (t is 0 on the edge that starts there)
    d = both(edges, ep, off, corners, rules)
    own = np.concatenate([np.full(len(p), k) for k, p in enumerate(polys) if len(p)])
    assert (d[np.arange(len(corners)), own] == 0.0).all()
    # on an edge it is 0 up to the rounding of the projection: far below the tolerance's floor for d = 0
    d = both(edges, ep, off, mids, rules)
    assert (np.abs(d[np.arange(len(mids)), ep]) <= R.tolerance(np.zeros(len(mids)), 40.0)).all()


def test_the_shared_winding_term_is_hit_testings():
    rng = np.random.default_rng(9)
    h = lib()
    n = 0
    for scale in (1.0, 1e-3, 7.3e5):
        e = rng.uniform(-10.0, 10.0, size=(200, 4)) * scale
        e[::7, 3] = e[::7, 1]      # edges along a
        e[::11, 2:] = e[::11, :2]  # edges of length zero
        pts = rng.uniform(-10.0, 10.0, size=(200, 2)) * scale
        pts[::5, 1] = e[::5, 1]    # level with an end
        for k in range(len(e)):
            term = ctypes.c_int(99)
            row = np.ascontiguousarray(e[k])
            got = h.sh_terms(ptr(row), pts[k, 0], pts[k, 1], ctypes.byref(term))
            assert got == term.value
            n += got != 0
    assert n > 50


def test_degenerate_edges():
    sq = cases.polygon_edges(cases.SQUARE)
    edges = np.concatenate([sq[:2], [[20.0, 20.0, 20.0, 20.0]], sq[2:], sq])     # a zero-length edge far off; the outline twice
    off = np.array([0, len(edges)], dtype=np.int32)
    ep = np.zeros(len(edges), dtype=np.int32)
    pts = np.array([(23.0, 24.0), (20.0, 20.0), (6.0, 5.0), (17.0, 16.0)])
    want = both(edges, ep, off, pts, signed=False)
    assert want[:, 0].tolist() == [5.0, 0.0, 3.0, 5.0]       # the distance to a zero-length edge is the distance to its point
    only = np.array([[20.0, 20.0, 20.0, 20.0]])
    assert both(only, np.zeros(1, dtype=np.int32), np.array([0, 1], dtype=np.int32), pts)[:, 0].tolist() == [5.0, 0.0, math.hypot(14.0, 15.0), 5.0]
    q = np.zeros(6)
    lib().sh_prepare(ptr(np.array([20.0, 20.0, 20.0, 20.0])), ptr(q))
    assert q.tolist() == [20.0, 20.0, 0.0, 0.0, 0.0, 20.0]   # inv = 0, not inf


# ---- exact witnesses --------------------------------------------------------------------------------------------------------------
def exact_cases(poly, pts):
    """Of `pts`, those whose distance to the integer polygon `poly` the float arithmetic must get exactly, with the exact d2: the
    nearest feature is a vertex (the projection clamps, with room) or an axis-aligned edge the point is not on (the error of the
    projection's foot is along the edge, and its square drowns in d2), and so for every edge that is as near."""
    edges = cases.polygon_edges(poly)
    out = []
    for pa, pb in pts.tolist():
        pa, pb = Fraction(pa), Fraction(pb)
        per_edge = []
        for a0, b0, a1, b1 in edges.tolist():
            a0, b0, a1, b1 = Fraction(a0), Fraction(b0), Fraction(a1), Fraction(b1)
            x, y = a1 - a0, b1 - b0
            len2 = x * x + y * y
            if not len2:
                per_edge.append(((pa - a0) ** 2 + (pb - b0) ** 2, True))
                continue
            t = ((pa - a0) * x + (pb - b0) * y) / len2
            tc = min(max(t, Fraction(0)), Fraction(1))
            d2 = (pa - a0 - tc * x) ** 2 + (pb - b0 - tc * y) ** 2
            clamps = t <= 0 or t >= Fraction(1001, 1000)
            along_axis = (x == 0 or y == 0) and 0 < t < 1 and d2 >= Fraction(1, 4)
            per_edge.append((d2, clamps or along_axis))
        best = min(d for d, _ok in per_edge)
        if all(ok for d, ok in per_edge if d <= best * Fraction(1001, 1000) + Fraction(1, 1000)):
            out.append(((float(pa), float(pb)), best))
    return out


@pytest.mark.parametrize("seed", [4, 5])
def test_exact_rational_witnesses(seed):
    polys = cases.random_polygons(seed, 3) + [np.array(cases.SQUARE), np.array([(0.0, 0.0), (8.0, 0.0), (8.0, 16.0), (4.0, 16.0), (4.0, 4.0), (0.0, 4.0)])]
    pts = cases.integer_points(seed, 160)
    n = 0
    for poly in polys:
        edges, ep, off = cases.edge_table([poly])
        sel = exact_cases(poly, pts)
        n += len(sel)
        points = np.array([p for p, _d in sel])
        d2 = R.min_d2(edges, ep, 1, points)[:, 0]
        want = np.array([float(d) for _p, d in sel])
        assert all(Fraction(w) == d for w, (_p, d) in zip(want.tolist(), sel))      # quarter-integers: representable
        assert np.array_equal(d2, want)
        assert np.array_equal(R.d2_exact(edges, points[0]), sel[0][1])
        dist = both(edges, ep, off, points, signed=False)[:, 0]
        assert np.array_equal(dist, np.sqrt(want))
    assert n > 300


def test_three_four_five():
    edges, ep, off = cases.edge_table([np.array(cases.SQUARE)])
    pts = np.array([p for p, _d in cases.PYTHAGOREAN])
    want = both(edges, ep, off, pts)
    assert want[:, 0].tolist() == [d for _p, d in cases.PYTHAGOREAN]
    assert both(edges, ep, off, pts, signed=False)[:, 0].tolist() == [abs(d) for _p, d in cases.PYTHAGOREAN]


def test_rectangle_against_the_closed_form():
    edges, ep, off = cases.edge_table([np.array(cases.SQUARE)])
    rng = np.random.default_rng(8)
    pts = np.concatenate([rng.uniform(-8.0, 20.0, size=(2000, 2)), cases.integer_points(8, 400, extent=10)])
    got = both(edges, ep, off, pts)[:, 0]
    want = cases.rect_distance(cases.RECT, pts)
    # the closed form's own error: a handful of roundings at coordinates below 32, each 2^-53 * 32 at the most
    assert np.abs(got - want).max() <= 8 * 2.0 ** -53 * 32.0
    clear = np.abs(want) > 1e-9
    assert np.array_equal(got[clear] < 0, want[clear] < 0) and (want < 0).sum() > 100


def test_the_sign_follows_the_fill_rule():
    star = cases.pentagram()
    centre = np.array([(32.0, 32.0), (32.0, 8.0), (2.0, 2.0)])      # the pentagon in the middle, a tip, outside
    edges, ep, off = cases.edge_table([star, star])
    d = both(edges, ep, off, centre, rules=np.array([0, 1], dtype=np.uint8))
    assert abs(int(hit_ref.winding(edges, ep, 2, centre)[0, 0])) == 2
    assert d[0, 0] < 0 < d[0, 1] and d[0, 0] == -d[0, 1]      # nonzero: inside; even-odd: a hole -- the same outline, the same distance
    assert d[1, 0] < 0 and d[1, 1] < 0 and d[2, 0] > 0 and d[2, 1] > 0
    # mirrored (a -> 64 - a) the outline winds the other way round and the field is the mirror image
    flipped = star * np.array([-1.0, 1.0]) + np.array([64.0, 0.0])
    e2, ep2, off2 = cases.edge_table([flipped, flipped])
    d2 = both(e2, ep2, off2, centre * np.array([-1.0, 1.0]) + np.array([64.0, 0.0]), rules=np.array([0, 1], dtype=np.uint8))
    assert hit_ref.winding(e2, ep2, 2, [(32.0, 32.0)])[0, 0] == -hit_ref.winding(edges, ep, 2, [(32.0, 32.0)])[0, 0]
    assert np.array_equal(np.sign(d2), np.sign(d)) and np.abs(np.abs(d2) - np.abs(d)).max() <= R.tolerance(d, 64.0).max()


# ---- clamp, encodings, union ------------------------------------------------------------------------------------------------------
def test_clamp_and_encodings_at_the_spread():
    spread = 1.5
    edges, ep, off = cases.edge_table([np.array(cases.SQUARE)])
    #                 0            +spread     +2 spread    -spread     -2 spread (the rectangle's deepest)
    pts = np.array([(2.0, 2.0), (6.0, 0.5), (6.0, -1.0), (6.0, 3.5), (6.0, 5.0)])
    raw = both(edges, ep, off, pts)[:, 0]
    assert raw.tolist() == [0.0, 1.5, 3.0, -1.5, -3.0]
    d = both(edges, ep, off, pts, spread=spread)[:, 0]
    assert d.tolist() == [0.0, 1.5, 1.5, -1.5, -1.5]
    assert both(edges, ep, off, pts, spread=spread, signed=False)[:, 0].tolist() == [0.0, 1.5, 1.5, 1.5, 1.5]
    f32, u8 = harness_encode(d, spread)
    assert f32.tolist() == [0.5, 0.0, 0.0, 1.0, 1.0] and u8.tolist() == [128, 0, 0, 255, 255]       # 127.5 goes to the even code
    assert np.array_equal(R.encode_f32(d, spread), f32) and np.array_equal(R.encode_u8(d, spread), u8)
    h = lib()
    assert h.sh_clamp(7.0, np.inf) == 7.0 and h.sh_clamp(-7.0, np.inf) == -7.0 and h.sh_clamp(np.inf, 2.0) == 2.0


def test_uint8_ties_and_boundaries():
    n_ties = 0
    for spread in (4.0, 1.0, 3.0, 255.0):
        d = cases.u8_tie_distances(spread)
        f32, u8 = harness_encode(d, spread)
        assert np.array_equal(u8, R.encode_u8(d, spread)) and np.array_equal(f32, R.encode_f32(d, spread))
        for dk, code in zip(d.tolist(), u8.tolist()):
            s = (0.5 - dk / (2.0 * spread)) * 255.0            # (Python floats: the same IEEE operations)
            assert code == min(max(round(s), 0), 255)          # round(): ties to even
            n_ties += Fraction(s) % 1 == Fraction(1, 2)
        assert u8.min() == 0 and u8.max() == 254 and len(set(u8.tolist())) > 128
    assert n_ties >= 8


def test_the_union_is_the_minimum_over_the_paths():
    squares = cases.overlapping_squares()
    edges, ep, off = cases.edge_table(squares)
    rng = np.random.default_rng(2)
    pts = np.concatenate([rng.uniform(-6.0, 22.0, size=(600, 2)), [(8.0, 5.0), (7.0, 5.0), (3.0, 5.0)]])
    for spread in (np.inf, 2.5):
        d = both(edges, ep, off, pts, spread=spread)
        u = R.union(d, spread)
        assert np.array_equal(harness_union(d, spread), u) and np.array_equal(u, d.min(axis=1))
        whole = R.clamp(cases.rect_distance((0.0, 0.0, 16.0, 10.0), pts), spread)      # the true field of the union
        outside = (d > 0).all(axis=1)
        assert outside.sum() > 100 and np.abs(u[outside] - whole[outside]).max() <= 8 * 2.0 ** -53 * 32.0      # exact outside
        assert np.array_equal(u < 0, whole < 0)                                                            # and on the sign
    d = both(edges, ep, off, pts)
    u = R.union(d, np.inf)
    # inside both squares: the depth in the deepest single path, not the depth in the union (5 at all three points)
    assert u[-3:].tolist() == [-2.0, -3.0, -3.0] and cases.rect_distance((0.0, 0.0, 16.0, 10.0), pts[-3:]).tolist() == [-5.0, -5.0, -3.0]
    assert np.array_equal(R.union(np.zeros((4, 0)), 2.0), np.full(4, 2.0)) and np.array_equal(harness_union(np.zeros((4, 0)), 2.0), np.full(4, 2.0))


# ---- the kernels' cull ------------------------------------------------------------------------------------------------------------
def harness_out_of_reach(ext, box, spread):
    ext, box = np.ascontiguousarray(ext, dtype=np.float64).reshape(-1, 4), np.ascontiguousarray(box, dtype=np.float64).reshape(-1, 5)
    spread = np.ascontiguousarray(np.broadcast_to(np.asarray(spread, dtype=np.float64), (len(ext),)))
    out = np.full(len(ext), 9, dtype=np.uint8)
    lib().sh_out_of_reach(ptr(ext), ptr(box), ptr(spread), ctypes.c_longlong(len(ext)), ptr(out))
    assert set(out.tolist()) <= {0, 1}
    return out.astype(bool)


def reach_tables(n=360, seed=11):
    """The cases of cases.reach_cases as arrays: (cases, extents (n, 4), boxes (n, 5), spreads (n,))."""
    cs = cases.reach_cases(seed, n)
    return (cs, np.array([cases.extent_of(poly) for _, _, poly, _, _ in cs]), np.array([cases.box_of(pts) for *_, pts in cs]),
            np.array([spread for _, _, _, spread, _ in cs]))


def test_out_of_reach_equals_its_reference_case_for_case():
    cs, ext, box, spread = reach_tables()
    clauses = R.out_of_reach_clauses(ext, box, spread)
    want = clauses.any(axis=0)
    assert np.array_equal(harness_out_of_reach(ext, box, spread), want)
    assert not harness_out_of_reach(ext, box, np.inf).any() and not R.out_of_reach(ext, box, np.inf).any()     # no cull without a spread
    # what the cases are: each clause decides some case alone, on both sides of its threshold within 2^-30 of it
    side = np.array([c[0] for c in cs])
    mode = np.array([c[1] for c in cs])
    thr = np.array([cases.reach_threshold(e, s) for e, s in zip(ext, spread)])
    gap = np.choose(side, [ext[:, 1] - box[:, 3], box[:, 2] - ext[:, 3], box[:, 0] - ext[:, 2], ext[:, 0] - box[:, 1]])
    alone = clauses.sum(axis=0) == 1
    for k in range(4):
        assert (alone & clauses[k]).any(), f"clause {k} decides no case alone"
        below, above = (side == k) & (mode == "below"), (side == k) & (mode == "above")
        assert below.sum() >= 5 and above.sum() >= 5
        assert (gap[below] < thr[below]).all() and (gap[below] >= thr[below] * (1.0 - 2.0 ** -29)).all() and not clauses[k][below].any()
        assert (gap[above] > thr[above]).all() and (gap[above] <= thr[above] * (1.0 + 2.0 ** -29)).all() and clauses[k][above].all()
    # the side the rays run through: suppressed where a point has |pb| < 2^-400, and only there
    tiny = box[:, 4] < 2.0 ** -400
    suppressed = tiny & (side == 3) & (gap > thr)
    assert suppressed.sum() >= 5 and not clauses[3][suppressed].any() and (suppressed & ~want).any()
    assert (tiny & (side == 2) & clauses[2]).any() and clauses[3][~tiny & (side == 3) & (gap > thr)].all()
    assert spread.min() == 2.0 ** -100 and spread.max() == 2.0 ** 40 and np.abs(ext).max() > 2.0 ** 48 and np.abs(ext).max() <= 2.0 ** 50
    assert want.mean() >= 0.25 and (~want).mean() >= 0.25


@pytest.mark.parametrize("signed", [True, False])
def test_a_path_out_of_reach_is_exactly_the_spread_away(signed):
    """The claim the cull rests on: where the predicate holds for a path's true extent, the walk gives every point
    of the box +spread -- at its corners and at its points nearest the extent, under both rules.  Every culled case is checked."""
    cs, ext, box, spread = reach_tables()
    want = R.out_of_reach(ext, box, spread)
    n_checked = 0
    for (_, _, poly, s, pts), culled in zip(cs, want):
        if not culled:
            continue
        edges, _, off = cases.edge_table([poly, poly])
        d = harness_distance(edges, off, pts, rules=[0, 1], spread=s, signed=signed)
        assert (d == s).all(), f"a path out of reach at spread {s!r}: {d.tolist()}"
        n_checked += 1
    assert n_checked == want.sum() >= len(cs) // 4


# ---- the atlas packer -------------------------------------------------------------------------------------------------------------
def check_layout(cells, rows, cols, boxes, scale, spread, max_cols):
    pad = math.ceil(spread)
    taken = np.zeros((rows, cols), dtype=np.int32)
    for (key, cell), box in zip(cells.items(), boxes):
        if box is None:
            assert (cell.rows, cell.cols) == (0, 0)
            continue
        assert cell.row0 >= 0 and cell.col0 >= 0 and cell.row0 + cell.rows <= rows and cell.col0 + cell.cols <= cols      # inside the image
        taken[cell.row0:cell.row0 + cell.rows, cell.col0:cell.col0 + cell.cols] += 1
        # the glyph's box in the cell, at least ceil(spread) from every border
        x0, y0, x1, y1 = box
        top, bottom = cell.origin_row - y1 * scale, cell.origin_row - y0 * scale
        left, right = cell.origin_col + x0 * scale, cell.origin_col + x1 * scale
        assert top >= pad and left >= pad and cell.rows - bottom >= pad and cell.cols - right >= pad
        assert top < pad + 1 and left < pad + 1 and cell.rows - bottom < pad + 1 and cell.cols - right < pad + 1          # and no more than needed
    assert taken.max(initial=0) <= 1          # disjoint
    assert cols <= max_cols


def test_atlas_layout():
    rng = np.random.default_rng(3)
    boxes = []
    for _ in range(60):
        x0, y0 = rng.uniform(-200.0, 100.0, size=2)
        boxes.append((x0, y0, x0 + rng.uniform(50.0, 900.0), y0 + rng.uniform(50.0, 1100.0)))
    boxes[7] = boxes[31] = None
    keys = [chr(48 + k) for k in range(len(boxes))]
    advances = rng.uniform(200.0, 900.0, size=len(boxes)).tolist()
    for size, spread, max_cols in ((48.0, 4.0, 256), (20.0, 2.5, 64), (64.0, 8.0, 1024), (31.0, 0.5, 40)):
        cells, rows, cols = sdf.atlas_layout(keys, boxes, advances, size, 1000.0, spread, max_cols)
        assert list(cells) == keys and rows > 0
        check_layout(cells, rows, cols, boxes, size / 1000.0, spread, max_cols)
        assert cells["7"].advance == advances[7] * (size / 1000.0)
        if max_cols < 1024:
            assert rows > max(c.rows for c in cells.values())          # more than one shelf
    with pytest.raises(ValueError, match="max_cols"):
        sdf.atlas_layout(keys, boxes, advances, 48.0, 1000.0, 4.0, 16)
    assert sdf.pack_cells([], 10) == ([], 0, 0)
    assert sdf.pack_cells([(0, 0), (3, 4), (0, 0)], 10) == ([(0, 0), (0, 0), (0, 0)], 3, 4)
    assert sdf.pack_cells([(3, 4), (5, 4), (2, 4)], 8) == ([(0, 4), (0, 0), (5, 0)], 7, 8)


def host_font():
    glyphs = {" ": Glyph(" ", 300.0, ""), "f": Glyph("f", 300.0, "M0 0L200 0L200 700L0 700Z"), "A": Glyph("A", 600.0, "M0 0L500 0L250 700Z"), "fi": Glyph("fi", 700.0, "M0 -100L600 -100L600 600L0 600Z")}
    return Font("host", 400, "normal", 800, -200, 1000, glyphs=glyphs, missing_glyph=Glyph(None, 500.0, "M50 0L450 0L450 500L50 500Z", name="notdef"))


def test_a_space_and_an_empty_string_need_no_device():
    font = host_font()
    for string, keys in (("", []), ("  ", [" "])):
        for dtype in (np.uint8, np.float32, np.float64):
            atlas = font.sdf_atlas(string, 48.0, 4.0, dtype=dtype)
            assert isinstance(atlas, S.SdfAtlas) and atlas.image.shape == (0, 0) and atlas.image.dtype == dtype
            assert list(atlas.cells) == keys and atlas.size == 48.0 and atlas.spread == 4.0
    cell = font.sdf_atlas(" ", 48.0, 4.0).cells[" "]
    assert isinstance(cell, S.SdfCell) and cell == (0, 0, 0, 0, 0, 0, 300.0 * 48.0 / 1000.0) and cell.advance == 14.4
    # the glyphs of a string as the atlas keys them: a ligature once, the missing glyph under its name
    placed, _adv = font.str_to_glyphs("AfiA?")
    assert [sdf.glyph_key(g) for _pen, g in placed] == ["A", "fi", "A", "notdef"]
    geo = sdf.cell_geometry(font.glyphs["fi"].path.user_box(), 0.048, 4)
    assert geo == (34 + 8, 29 + 8, 4 + 29, 4)      # rows: floor(-28.8) .. ceil(4.8); cols: 0 .. ceil(28.8); the origin 29 rows down


# ---- errors, with no device -------------------------------------------------------------------------------------------------------
def square_path():
    pts = [tuple(map(float, p)) for p in cases.SQUARE]
    return S.Path([[(PATH_LINE, [list(a), list(b)]) for a, b in zip(pts, pts[1:])] + [(PATH_CLOSED, [list(pts[-1]), list(pts[0])])]])


def test_errors_before_any_device_work():
    if _abi.load_library().svgr_device_count() == 0:
        with pytest.raises(_abi.SvgrError):
            square_path().distance([(1.0, 2.0)])          # (a good call does reach for the device, and there is none)
    path = square_path()
    for bad in (np.zeros((4, 3)), [1.0, 2.0, 3.0], np.zeros((2, 2, 2))):
        with pytest.raises(ValueError):
            path.distance(bad)
    with pytest.raises(ValueError, match="fill rule"):
        path.distance([(1.0, 2.0)], fill_rule="odd")
    for spread in (0.0, -1.0, float("nan"), -np.inf, "wide"):
        with pytest.raises(ValueError, match="spread"):
            path.distance([(1.0, 2.0)], spread=spread)
        with pytest.raises(ValueError, match="spread"):
            path.sdf(None, (0, 0, 8, 8), spread)
        with pytest.raises(ValueError, match="spread"):
            host_font().sdf_atlas("A", 48.0, spread)
    for dtype in (np.int32, np.float16, "bool", object):
        with pytest.raises(TypeError):
            path.sdf(None, (0, 0, 8, 8), 4.0, dtype=dtype)
        with pytest.raises(TypeError):
            host_font().sdf_atlas("A", 48.0, 4.0, dtype=dtype)
    for dtype in (np.float32, np.uint8):
        with pytest.raises(ValueError, match="finite spread"):
            path.sdf(None, (0, 0, 8, 8), np.inf, dtype=dtype)
    with pytest.raises(ValueError, match="finite spread"):
        host_font().sdf_atlas("A", 48.0, np.inf, dtype=np.float64)
    with pytest.raises(ValueError, match="fill rule"):
        path.sdf(None, (0, 0, 8, 8), 4.0, fill_rule="odd")
    with pytest.raises(ValueError, match="viewport"):
        path.sdf(None, (0, 0, -1, 8), 4.0)
    for size in (0.0, -3.0, np.inf):
        with pytest.raises(ValueError, match="size"):
            host_font().sdf_atlas("A", size, 4.0)
    with pytest.raises(ValueError, match="max_cols"):
        host_font().sdf_atlas("A", 48.0, 4.0, max_cols=0)
    # an empty path and no points touch no device either
    assert S.Path([]).distance([(1.0, 2.0), (3.0, 4.0)]).tolist() == [np.inf, np.inf] and S.Path([]).distance([(1.0, 2.0)], spread=3.0).tolist() == [3.0]
    assert path.distance(np.zeros((0, 2))).shape == (0,)
    empty = S.Path([])
    assert np.array_equal(empty.sdf(None, (0, 0, 2, 3), 4.0, np.float64), np.full((2, 3), 4.0))
    assert np.array_equal(empty.sdf(None, (0, 0, 2, 3), 4.0), np.zeros((2, 3), dtype=np.float32)) and empty.sdf(None, (0, 0, 2, 3), 4.0, np.uint8).dtype == np.uint8
    assert path.sdf(None, (0, 0, 0, 5), 4.0).shape == (0, 5)
    # Batch.distance's own argument checks sit in front of the C call
    for call in (lambda: _abi.Batch.distance(None, np.zeros((1, 2)), out="f16"), lambda: _abi.Batch.distance(None, np.zeros((1, 2)), spread=0.0),
                 lambda: _abi.Batch.distance(None, np.zeros((1, 2)), spread=np.inf, out="u8")):
        with pytest.raises(ValueError):
            call()
