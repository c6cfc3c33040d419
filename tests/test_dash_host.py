"""Dashed strokes on the CPU: the host reference (tests/dash_ref.py) pinned on cases whose answers are known, the dasher's
per-lane header (csrc/svgr_dash.h, compiled for the host by tests/dash_harness.cpp) against that reference, the conditions
the shared test inputs must meet, and the SVG loader's dash attributes.  No GPU needed."""
import ctypes as C
import math
import os
import warnings

import numpy as np
import pytest

from tests import dash_cases as cases
from tests import dash_ref as R
from tests.util import ROOT, host_build

RECT = R.polyline([(0, 0), (100, 0), (100, 50), (0, 50)], closed=True)


def subpaths(types, params, sizes):
    out, k = [], 0
    for n in sizes:
        out.append([(int(types[i]), params[i]) for i in range(k, k + int(n))])
        k += int(n)
    return out


# ---- the reference, pinned ------------------------------------------------------------------------------------------------
def test_rectangle_10_10_boundaries_on_the_corners():
    t, p, s = R.dash(*RECT, [10, 10])
    assert list(s) == [2] * 15
    # dash d covers [20 d, 20 d + 10) of the perimeter 0..300: exact end points
    def at(u):
        if u <= 100: return (u, 0.0)
        if u <= 150: return (100.0, u - 100)
        if u <= 250: return (250.0 - u, 50.0)
        return (0.0, 300.0 - u)
    for d, sub in enumerate(subpaths(t, p, s)):
        (t0, q0), (t1, q1) = sub
        assert (t0, t1) == (R.LINE, R.UNCLOSED)
        assert tuple(q0[:4]) == (*at(20 * d), *at(20 * d + 10))
        assert tuple(q1[:4]) == (*at(20 * d + 10), *at(20 * d)) and not q0[4:].any() and not q1[4:].any()


def test_rectangle_25_10_dashes_turn_corners_and_the_wrap_around_merges():
    t, p, s = R.dash(*RECT, [25, 10])
    subs = subpaths(t, p, s)
    assert list(s) == [2, 2, 2, 3, 2, 2, 3, 3]
    # [35, 60) .. ; the dash [105, 130) turns the corner at 150?  no: [140, 165) does -- the fourth output subpath
    corner = subs[3]
    assert tuple(corner[0][1][:4]) == (100.0, 40.0, 100.0, 50.0) and tuple(corner[1][1][:4]) == (100.0, 50.0, 85.0, 50.0)
    # the last subpath: the trailing dash [280, 300) first, then the leading dash [0, 25): a join at the start point, no caps
    last = subs[-1]
    assert tuple(last[0][1][:4]) == (0.0, 20.0, 0.0, 0.0) and tuple(last[1][1][:4]) == (0.0, 0.0, 25.0, 0.0)
    assert last[2][0] == R.UNCLOSED and tuple(last[2][1][:4]) == (25.0, 0.0, 0.0, 20.0)
    # and the first output subpath is the SECOND dash of the pattern
    assert tuple(subs[0][0][1][:4]) == (35.0, 0.0, 60.0, 0.0)


def test_a_dash_longer_than_a_closed_subpath_keeps_it_closed():
    for offset in (0, 50, 410 * 3 + 20, -400):
        t, p, s = R.dash(*RECT, [400, 10], offset)
        assert list(s) == [4] and list(t) == [R.LINE, R.LINE, R.LINE, R.CLOSED]
        assert np.array_equal(p, np.array(RECT[1], dtype=np.float64))
    open_rect = R.polyline([(0, 0), (100, 0), (100, 50), (0, 50)])
    t, p, s = R.dash(*open_rect, [400, 10])
    assert list(s) == [4] and list(t) == [R.LINE, R.LINE, R.LINE, R.UNCLOSED]


def test_circle_dashes_have_their_nominal_length():
    k = 4 * (math.sqrt(2) - 1) / 3 * 50
    arcs = [(R.CUBIC, [50, 0, 50, k, k, 50, 0, 50]), (R.CUBIC, [0, 50, -k, 50, -50, k, -50, 0]),
            (R.CUBIC, [-50, 0, -50, -k, -k, -50, 0, -50]), (R.CUBIC, [0, -50, k, -50, 50, -k, 50, 0])]
    path = R.from_segments(arcs, closed=True)
    t, p, s = R.dash(*path, [23.0, 11.0], 0.0)
    full = 0
    for sub in subpaths(t, p, s)[:-1]:   # (the last one is the merged wrap-around or a partial dash)
        length = sum(R.true_length(ty, q) for ty, q in sub[:-1])
        assert abs(length - 23.0) <= R.METRIC_ACCURACY * 23.0, length
        full += 1
    assert full >= 8


def test_odd_counts_offsets_and_path_length():
    line = R.polyline([(0, 0), (60, 0)])
    starts = lambda res: [float(q[0]) for ty, q in zip(res[0], res[1]) if ty == R.LINE]  # noqa: E731
    assert starts(R.dash(*line, [5])) == starts(R.dash(*line, [5, 5])) == [0, 10, 20, 30, 40, 50]
    assert starts(R.dash(*line, [5, 3, 2])) == starts(R.dash(*line, [5, 3, 2, 5, 3, 2])) == [0, 8, 15, 20, 28, 35, 40, 48, 55]
    # a positive offset moves the pattern towards the start; negative and beyond-the-period offsets wrap
    assert starts(R.dash(*line, [5, 5], 2)) == [0, 8, 18, 28, 38, 48, 58]
    assert starts(R.dash(*line, [5, 5], -2)) == starts(R.dash(*line, [5, 5], 8)) == starts(R.dash(*line, [5, 5], 10 ** 9 * 10 + 8))
    assert starts(R.dash(*line, [5, 5], -2)) == [2, 12, 22, 32, 42, 52]
    # pathLength 30 on a path 60 long: everything doubles
    assert starts(R.dash(*line, [2.5, 2.5], 1, 30)) == starts(R.dash(*line, [5, 5], 2))
    # solid: the input comes back
    for solid in ([], None, [-1, 2], [0, 0], [float("nan"), 1], [5, 0]):
        t, p, s = R.dash(*line, solid)
        assert list(t) == line[0] and list(s) == line[2]
    # every subpath restarts the pattern
    two = R.concat(R.polyline([(0, 0), (7, 0)]), R.polyline([(0, 5), (7, 5)]))
    assert starts(R.dash(*two, [2, 3], 0)) == [0, 5, 0, 5]


def test_zero_length_segments_and_zero_length_dashes():
    path = R.polyline([(0, 0), (0, 0), (10, 0), (10, 0), (10, 10), (10, 10)])
    t, p, s = R.dash(*path, [3, 2])
    assert list(s) == [2, 2, 2, 2]   # [0, 3) [5, 8) [10, 13) [15, 18): the third begins exactly at the corner, on the second line
    path2 = R.polyline([(0, 0), (10, 0)])
    t, p, s = R.dash(*path2, [0, 3, 2, 1])   # the dots of "0 3" are dropped; [3, 5) stays
    assert list(s) == [2, 2] and [float(q[0]) for ty, q in zip(t, p) if ty == R.LINE] == [3, 9]
    t, p, s = R.dash(*path2, [0, 5])
    assert len(t) == 0 and len(s) == 0


# ---- the conditions on the shared inputs ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def inputs():
    return cases.fixed_cases(), cases.fuzz_cases()


def test_inputs_keep_boundaries_away_from_joints(inputs):
    fixed, fuzz = inputs
    for name, path, dashes, offset, plen, exact in fixed:
        detail = {"exact": exact}
        R.dash(*path, dashes, offset, plen, detail=detail)
        assert detail.get("clearance", math.inf) >= 1e-6, (name, detail.get("clearance"))   # the fixed cases leave out none
    dropped = 0
    for name, path, dashes, offset, plen, exact in fuzz:
        detail = {}
        R.dash(*path, dashes, offset, plen, detail=detail)
        dropped += detail["clearance"] < 1e-6
    assert len(fuzz) == 200 and max(len(p[0]) for _n, p, *_r in fuzz) <= 42   # (<= 40 segments + their terminators)
    assert dropped <= len(fuzz) * 0.05, dropped


def test_newton_spread_is_what_the_docstring_says(inputs):
    """Long double against float64, sequential against pairwise sums: the largest distance between their outputs over every
    fixed case that is not exact and the whole fuzz set (less the paths the clearance condition drops), which the tolerance
    takes 4 times."""
    fixed, fuzz = inputs
    worst = 0.0
    for name, path, dashes, offset, plen, exact in [c for c in fixed if not c[5]] + fuzz:
        detail = {}
        R.dash(*path, dashes, offset, plen, detail=detail)
        if detail["clearance"] < 1e-6:
            continue
        spread = R.spread(*path, dashes, offset, plen)
        assert spread is not None, name
        worst = max(worst, spread)
    print(f"newton spread: {worst:.3e} (recorded: {R.NEWTON_SPREAD:.3e})")
    assert worst <= R.NEWTON_SPREAD


def test_cubic_outline_distance_is_as_recorded():
    """The end-to-end document's cubic: dash_ref in float64 against long double, the distance the GPU test allows 4 times."""
    path = R.from_segments([(R.CUBIC, [4, 40, 20, 20, 40, 60, 60, 40])])
    a = R.dash(*path, [5, 3])
    b = R.dash(*path, [5, 3], long_double=True)
    assert list(a[0]) == list(b[0]) and float(np.abs(a[1] - b[1]).max()) <= cases.CUBIC_DISTANCE


# ---- the per-lane header against the reference ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dh():
    L = host_build("dash_harness")
    f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
    i64p = np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")
    L.dh_sub_lengths.argtypes = [f64p, f64p]
    L.dh_invert.argtypes = [f64p, C.c_double]
    L.dh_invert.restype = C.c_double
    L.dh_split.argtypes = [f64p, C.c_double, C.c_double, f64p]
    L.dh_count.argtypes = [f64p, C.c_int, C.c_double, C.c_double, C.c_int, C.c_double, C.c_double, C.c_int, i64p]
    L.dh_mode.argtypes = [f64p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int]
    L.dh_piece.argtypes = [f64p, C.c_int, C.c_double, C.c_int, f64p, C.c_longlong, f64p]
    return L


CUBICS = [[0, 0, 60, 90, 30, -70, 100, 10], [0, 0, 120, 80, -20, 80, 100, 0], [0, 0, 100, 60.5, 0, 60, 100, 0],
          [10, 20, 30, 25, 50, 22, 70, 20], [0, 0, 0, 0, 50, 50, 50, 50]]
LD = R._Num(True)


def test_header_sub_interval_lengths(dh):
    for c in CUBICS:
        c = np.array(c, dtype=np.float64)
        got = np.empty(32)
        dh.dh_sub_lengths(c, got)
        want = [float(v) for v in R.sub_lengths(LD, [np.longdouble(v) for v in c])]
        # 4 speeds of ~20 roundings each on values <= 6 M, summed and scaled: (roundings + 1) u x magnitude
        tol = 25 * R.U * 6 * np.abs(c).max() / 32 * 4
        assert np.abs(got - want).max() <= tol


def test_header_inversion_and_split(dh):
    for c in CUBICS:
        c = np.array(c, dtype=np.float64)
        wide = [np.longdouble(v) for v in c]
        tab = R.cubic_table(LD, wide)
        M = np.abs(c).max()
        for frac in (0.013, 0.25, 0.5, 0.77, 0.999):
            s = float(tab[-1]) * frac
            t_got = dh.dh_invert(c, s)
            t_want = float(R.invert(LD, wide, tab, np.longdouble(s)))
            # the point on the curve, not the parameter, is what the tolerance speaks of (a near-cusp has dt/ds unbounded)
            pt = lambda t: np.array(R.split(R._Num(False), list(map(float, c)), 0.0, t)[6:8]) if t < 1 else c[6:8]  # noqa: E731
            assert np.abs(pt(t_got) - pt(t_want)).max() <= 4 * R.NEWTON_SPREAD * M + 50 * R.U * M, (c, frac)
        got = np.empty(8)
        dh.dh_split(c, 0.3, 0.85, got)
        want = np.array([float(v) for v in R.split(LD, wide, np.longdouble(0.3), np.longdouble(0.85))])
        assert np.abs(got - want).max() <= 19 * R.U * 2 * M
        dh.dh_split(c, 0.0, 1.0, got)
        assert np.array_equal(got, c)


def test_header_counts_pieces_like_the_reference(dh):
    rng = np.random.default_rng(7)
    num = R._Num(False)
    out = np.empty(2, dtype=np.int64)
    for _ in range(300):
        m = int(rng.integers(1, 7))
        dashes = [float(v) for v in rng.integers(0, 5, m)]
        if R.is_solid(dashes):
            continue
        offset = float(rng.integers(-20, 40))
        s0 = float(rng.integers(0, 30))
        s1 = s0 + float(rng.integers(1, 60))
        pat = R.Pattern(num, dashes, offset, 1.0)
        ka, ja, ra = pat.idx_ge(s0 + pat.phase)
        want = pat.count_between((ka, ja), pat.idx_lt(s1 + pat.phase))
        cont = want > 0 and ja in pat.on and s0 != 0 and ra > pat.pre[ja]
        dh.dh_count(np.array(dashes), m, offset, 1.0, R.LINE, s0, s1, 0, out)
        assert (int(out[0]), int(out[1])) == (want, want - int(cont)), (dashes, offset, s0, s1)
    # a subpath that stays whole: every segment is one piece, only the first starts the dash, and the closing line -- which comes
    # back as the terminator -- counts nothing
    for type_, s0, want in ((R.LINE, 0.0, (1, 1)), (R.CUBIC, 5.0, (1, 0)), (R.CLOSED, 5.0, (0, 0)), (R.CLOSED, 0.0, (0, 0))):
        dh.dh_count(np.array([400.0, 10.0]), 2, 0.0, 1.0, type_, s0, s0 + 7.0, 2, out)
        assert (int(out[0]), int(out[1])) == want
    # the modes of a closed subpath
    d = np.array([25.0, 10.0])
    assert dh.dh_mode(d, 2, 0.0, 1.0, 300.0, 1) == 1 and dh.dh_mode(d, 2, 0.0, 1.0, 300.0, 0) == 0
    assert dh.dh_mode(np.array([400.0, 10.0]), 2, 50.0, 1.0, 300.0, 1) == 2 and dh.dh_mode(np.array([10.0, 10.0]), 2, 0.0, 1.0, 300.0, 1) == 0


def test_header_pieces_of_a_lone_segment(dh):
    for c, dashes, offset in [(CUBICS[0], [9.3, 4.1], 1.7), (CUBICS[1], [11.7, 3.9], 0.9), (CUBICS[2], [8.9, 5.3], 2.1)]:
        path = R.from_segments([(R.CUBIC, c)])
        detail = {}
        t, p, s = R.dash(*path, dashes, offset, long_double=True, detail=detail)
        pieces = [q for ty, q in zip(t, p) if ty == R.CUBIC]
        tol = R.tolerance(np.array(c), 1, detail["length"], detail["period"])
        got = np.empty(8)
        for q, want in enumerate(pieces):
            assert dh.dh_piece(np.array(dashes), len(dashes), offset, R.CUBIC, np.array(c, dtype=np.float64), q, got) == R.CUBIC
            assert np.abs(got - want).max() <= tol, (c, q)
        assert dh.dh_piece(np.array(dashes), len(dashes), offset, R.CUBIC, np.array(c, dtype=np.float64), len(pieces), got) == -1


# ---- Path.dash and the loader ---------------------------------------------------------------------------------------------
def test_path_dash_solid_patterns_need_no_device():
    import svgrasterize_amd as S

    path = S.Path.from_svg("M0,0 L10,0 Q15,5 10,10 z")
    for solid in ([], [0, 0], [5, 0], [-1, 2]):
        out = path.dash(solid)
        assert isinstance(out, S.Path) and len(out.subpaths) == 1 and len(out.subpaths[0]) == 3
        assert out.subpaths[0][1][0] == S.PATH_CUBIC   # (converted as Path.stroke converts)


SVG = """<svg xmlns="http://www.w3.org/2000/svg" width="64" height="64">
  <rect id="a" x="8" y="8" width="40" height="20" fill="none" stroke="#000" stroke-dasharray="6, 2 1" stroke-dashoffset="3" pathLength="60"/>
  <g stroke-dasharray="4 2" stroke-dashoffset="-1" stroke="#00f" fill="none">
    <path d="M4,40 C20,20 40,60 60,40"/>
    <line x1="0" y1="60" x2="64" y2="60" style="stroke-dasharray: none"/>
    <circle cx="32" cy="32" r="5" stroke-dasharray="1mm"/>
  </g>
  <path d="M0,0 L5,5" stroke="#000" stroke-dasharray="10% 5"/>
  <path d="M0,0 L5,5" stroke="#000" stroke-dasharray="3 -1"/>
  <path d="M0,0 L5,5" stroke="#000" stroke-dasharray="0 4"/>
  <path d="M0,0 L5,6" stroke="#000" stroke-dasharray="0 5"/>
</svg>"""


def _strokes(scene, out):
    import svgrasterize_amd as S

    kind, args = scene
    if kind == S.RENDER_STROKE:
        out.append(args)
    elif kind == S.RENDER_GROUP:
        for child in args:
            _strokes(child, out)
    elif kind in (S.RENDER_TRANSFORM, S.RENDER_OPACITY, S.RENDER_FILTER, S.RENDER_BLEND):
        _strokes(args[0], out)
    return out


def test_loader_reads_the_dash_attributes_without_a_device():
    import svgrasterize_amd as S
    from svgrasterize_amd.geometry import DashedPath

    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        scene, _ids, _size = S.svg_scene_from_str(SVG)
    strokes = _strokes(scene, [])
    assert len(strokes) == 8 and all(len(a) == 5 for a in strokes)   # the node stays the five-field tuple
    rect, curve, line, circle, pct, neg, dots, dots2 = [a[0] for a in strokes]
    assert isinstance(rect, DashedPath) and rect.dasharray == (6.0, 2.0, 1.0) and rect.dashoffset == 3.0 and rect.path_length == 60.0
    assert isinstance(curve, DashedPath) and curve.dasharray == (4.0, 2.0) and curve.dashoffset == -1.0 and curve.path_length is None
    assert type(line) is S.Path                                  # none: solid
    assert isinstance(circle, DashedPath) and abs(circle.dasharray[0] - 96 / 25.4) < 1e-12 and circle.dashoffset == -1.0
    assert type(pct) is S.Path and type(neg) is S.Path
    assert isinstance(dots, DashedPath) and isinstance(dots2, DashedPath)
    texts = [str(w.message) for w in caught]
    assert sum("needs the viewport" in t for t in texts) == 1 and sum("negative stroke-dasharray" in t for t in texts) == 1
    assert sum("length 0 are not drawn" in t for t in texts) == 1   # once per document
    text = repr(scene)
    assert "DASH 6 2 1 offset:3 pathLength:60\n" in text and "DASH 4 2 offset:-1\n" in text and text.count("DASH ") == 5
    # Scene.stroke builds the same thing; a solid list leaves the plain path
    node = S.Scene.stroke(S.Path.from_svg("M0,0 L9,0"), np.ones(4), 2.0, dasharray=[3, 1], dashoffset=1.0)
    assert isinstance(node[1][0], DashedPath) and len(node[1]) == 5
    assert type(S.Scene.stroke(S.Path.from_svg("M0,0 L9,0"), np.ones(4), 2.0, dasharray=[3, 0])[1][0]) is S.Path


def test_documents_without_dashes_dump_as_before():
    """The document above without its dash attributes, against what the commit in front of the dasher made of it
    (tests/golden/dash_plain_scene.*: the scene's repr, and scenedump's tree and arrays)."""
    import json

    import svgrasterize_amd as S
    from svgrasterize_amd import scenedump

    plain = SVG.replace("stroke-dasharray", "data-x").replace("stroke-dashoffset", "data-y").replace("pathLength", "data-z")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        scene, _ids, _size = S.svg_scene_from_str(plain)
    assert all(type(a[0]) is S.Path for a in _strokes(scene, []))
    golden = os.path.join(ROOT, "tests", "golden", "dash_plain_scene")
    with open(golden + ".txt") as f:
        assert repr(scene) == f.read()
    tree, arrays = scenedump.dump_scene(scene)   # (strokes through the host stroker alone: no device)
    with open(golden + ".json") as f:
        assert json.loads(json.dumps(tree)) == json.load(f)
    with np.load(golden + ".npz") as before:
        assert sorted(before.files) == sorted(arrays)
        for key in before.files:
            assert arrays[key].dtype == before[key].dtype and np.array_equal(arrays[key], before[key]), key
