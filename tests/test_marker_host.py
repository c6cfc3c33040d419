"""Markers on the CPU: the reference (tests/marker_ref.py) against hand-computed vertices, the marker pass's per-lane header
(csrc/svgr_marker.h, through tests/marker_harness.cpp) against the reference on the shapes the GPU test runs, the fuzz set's
clearance, and the library layer without a device: the loader, the lazy MARKERS node and every walker, with the reference
standing in for ``Path.vertices``."""
import ctypes
import math
import warnings

import numpy as np
import pytest

from tests import marker_cases as cases
from tests import marker_ref as R
from tests.util import host_build

P = ctypes.c_void_p
H = math.sqrt(0.5)


def harness(path, flags=None):
    """The header's three lane functions over a whole path, as (xy, direction, kind)."""
    lib = host_build("marker_harness")
    lib.mh_path.restype = ctypes.c_longlong
    types = np.ascontiguousarray(path[0], dtype=np.int32)
    params = np.ascontiguousarray(path[1], dtype=np.float64).reshape(-1, 8)
    sizes = [int(s) for s in path[2] if s]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    fl = None if flags is None else np.ascontiguousarray(flags, dtype=np.int32)
    cap = len(types) + len(sizes)
    xyuv, kind = np.zeros((cap, 4)), np.zeros(cap, dtype=np.int32)
    n = lib.mh_path(types.ctypes.data_as(P), params.ctypes.data_as(P), None if fl is None else fl.ctypes.data_as(P),
                    off.ctypes.data_as(P), len(sizes), ctypes.c_longlong(cap), xyuv.ctypes.data_as(P), kind.ctypes.data_as(P))
    assert n >= 0
    return xyuv[:n, :2].copy(), xyuv[:n, 2:].copy(), kind[:n].copy()


def both(path, flags=None):
    """The reference's vertices, checked against the header's: (xy, directions as float64, kinds)."""
    want = R.vertices(*path, flags)
    R.check(harness(path, flags), want)
    return want[0], want[1].astype(np.float64), list(want[2])


def close(got, want):
    return np.allclose(np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), rtol=0, atol=1e-15)


# ---- hand-computed cases ------------------------------------------------------------------------------------------------------
def test_l_shaped_polyline():
    xy, u, kind = both(R.polyline([(0, 0), (10, 0), (10, 10)]))
    assert xy.tolist() == [[0, 0], [10, 0], [10, 10]] and kind == [0, 1, 2]
    assert close(u, [(1, 0), (H, H), (0, 1)])


def test_closed_triangle_shares_one_bisector_at_its_ends():
    xy, u, kind = both(R.polyline([(0, 0), (10, 0), (0, 10)], closed=True))
    assert xy.tolist() == [[0, 0], [10, 0], [0, 10], [0, 0]] and kind == [0, 1, 1, 2]
    # in: the closing line (0, -1); out: the first line (1, 0)
    assert close(u[0], (H, -H)) and close(u[3], (H, -H))
    a = np.array([1.0, 0.0]) + np.array([-H, H])
    assert close(u[1], a / np.hypot(*a))


def test_cubics_with_coincident_control_points():
    _xy, u, _k = both(R.from_segments([(R.CUBIC, [0, 0, 0, 0, 5, 5, 10, 0])]))
    assert close(u, [(H, H), (H, -H)])           # start: P2 - P0; end: P3 - P2
    _xy, u, _k = both(R.from_segments([(R.CUBIC, [0, 0, 0, 0, 0, 0, 3, 4])]))
    assert close(u, [(0.6, 0.8), (0.6, 0.8)])    # P3 - P0 at both ends
    _xy, u, _k = both(R.from_segments([(R.CUBIC, [0, 0, 3, 4, 6, 8, 6, 8])]))
    assert close(u, [(0.6, 0.8), (0.6, 0.8)])    # end: P3 - P2 is (0, 0), P3 - P1 is not


def test_zero_length_segments_borrow_a_direction():
    _xy, u, _k = both(R.polyline([(0, 0), (10, 0), (10, 0), (10, 10)]))
    assert close(u, [(1, 0), (1, 0), (H, H), (0, 1)])     # between two lines: the earlier line's direction
    _xy, u, _k = both(R.polyline([(5, 5), (5, 5), (5, 15)]))
    assert close(u, [(0, 1), (0, 1), (0, 1)])             # at the start: the later line's
    xy, u, _k = both(R.polyline([(5, 5), (5, 5), (5, 5)]))
    assert len(xy) == 3 and close(u, [(1, 0)] * 3)        # nothing to borrow from


def test_no_wrap_around_on_a_closed_subpath():
    # the first segment is degenerate: it looks forwards, not back across the closing line
    _xy, u, _k = both(R.polyline([(0, 0), (0, 0), (10, 0), (10, 10)], closed=True))
    b = np.array([-H, -H]) + np.array([1.0, 0.0])          # in: closing line; out: the first segment's borrowed (1, 0)
    assert close(u[0], b / np.hypot(*b)) and close(u[1], (1, 0))


def test_move_and_close_has_two_coincident_vertices():
    from svgrasterize_amd import Path

    types, params, sizes, flags = Path.from_svg("M3,4z")._flagged_segment_arrays()
    xy, u, kind = both((types, params, sizes), flags)
    assert xy.tolist() == [[3, 4], [3, 4]] and kind == [0, 2] and close(u, [(1, 0), (1, 0)])
    assert Path.from_svg("M3,4")._flagged_segment_arrays()[0] == []   # a lone move is dropped by the path reader


def test_kinds_over_two_subpaths():
    path = R.concat(R.polyline([(0, 0), (10, 0), (10, 10)]), R.polyline([(20, 0), (30, 0), (30, 10)], closed=True))
    xy, u, kind = both(path)
    assert kind == [0, 1, 1, 1, 1, 1, 2] and len(xy) == 7
    assert close(u[2], (0, 1)) and close(u[3], u[6])       # an inner open end keeps its own direction; the closed ends share one


def test_exact_reversal_turns_left():
    _xy, u, _k = both(R.polyline([(0, 0), (10, 0), (0, 0)]))
    assert close(u, [(1, 0), (0, 1), (-1, 0)])


def test_an_arc_is_one_segment():
    from svgrasterize_amd import Path

    types, params, sizes, flags = Path.from_svg("M0,0 A10,10 0 0 1 20,0")._flagged_segment_arrays()
    assert len(types) > 2 and sum(flags[:-1]) == 1          # several cubics, one vertex among them
    xy, u, kind = both((types, params, sizes), flags)
    assert len(xy) == 2 and kind == [0, 2]
    assert np.allclose(xy, [(0, 0), (20, 0)], atol=1e-14) and np.allclose(u, [(0, -1), (0, 1)], atol=1e-14)
    # existing callers of _segment_arrays see three lists, as before
    three = Path.from_svg("M0,0 L5,0 A10,10 0 0 1 20,0")._segment_arrays()
    assert len(three) == 3 and len(three[0]) == len(three[1]) == sum(three[2])


# ---- the header on the GPU test's shapes ----------------------------------------------------------------------------------------
FIXED = cases.fixed_cases()


@pytest.mark.parametrize("case", FIXED, ids=[c[0] for c in FIXED])
def test_header_agrees_with_the_reference(case):
    name, path, flags = case
    detail = {}
    want = R.vertices(*path, flags, detail=detail)
    assert detail["clearance"] > 1e-3, name   # (a fixed case is nowhere near a reversal, or is one exactly)
    R.check(harness(path, flags), want, name)


def test_degenerate_subpath_on_a_seam_borrows_from_neither_neighbour():
    for name, path, flags in FIXED:
        if not name.startswith("degenerate_subpath_on_"):
            continue
        xy, u, _kind, _tol = R.vertices(*path, flags)
        dot = np.nonzero((xy == (50, 60)).all(axis=1))[0]
        assert len(dot) == 7 and (u[dot].astype(np.float64) == (1.0, 0.0)).all(), name


def test_fixed_cases_sit_on_the_seams():
    count = {name: len(path[0]) for name, path, _f in FIXED}
    for n in (1, 2, cases.B - 1, cases.B, cases.B + 1, cases.S - 1, cases.S, cases.S + 1, 2 * cases.S + 1):
        assert count[f"stairs{n}"] == count[f"cubics{n}"] == count[f"mix{n}"] == n
    for seam, tag in ((cases.B, "B"), (cases.S, "S")):
        t, _p, sizes = next(path for name, path, _f in FIXED if name == f"boundary_on_{tag}")
        assert sizes[0] == seam and t[seam - 1] == R.CLOSED
        t, _p, sizes = next(path for name, path, _f in FIXED if name == f"closed_across_{tag}")
        assert sizes[0] == 3 and sum(sizes) - 1 > seam and t[-1] == R.CLOSED


def test_fuzz_set_clearance_and_agreement():
    fuzz = cases.fuzz_cases()
    assert len(fuzz) == 200
    low = 0
    for name, path, flags in fuzz:
        detail = {}
        want = R.vertices(*path, flags, detail=detail)
        if detail["clearance"] < 1e-6:
            low += 1
            continue
        R.check(harness(path, flags), want, name)
    assert low <= 10, low   # at most 5 % of the set may be that close to a reversal


def test_tolerance_is_the_derived_one():
    _xy, _u, _kind, tol = R.vertices(*R.polyline([(0, 0), (10, 0), (10, 10)]))
    assert tol[0] == tol[2] == 12 * 2.0 ** -53
    assert tol[1] == pytest.approx(12 * 2.0 ** -53 + math.sqrt(2) * 25 * 2.0 ** -53 / math.sqrt(2), rel=1e-12)


# ---- the library layer, without a device ----------------------------------------------------------------------------------------
DOC = """<svg xmlns="http://www.w3.org/2000/svg" width="64" height="64">
<defs>
<marker id="a" markerWidth="4" markerHeight="6" refX="1" refY="2" viewBox="0 0 8 4" preserveAspectRatio="xMinYMax slice"
        orient="auto-start-reverse" markerUnits="userSpaceOnUse" style="overflow:visible"><path d="M0,0 L4,2 L0,4z" fill="red"/></marker>
<marker id="b" orient="30deg"><circle cx="1" cy="1" r="1"/></marker>
<marker id="c" orient="auto" overflow="auto" refX="left"><rect width="2" height="2"/></marker>
<linearGradient id="g"><stop offset="0" stop-color="red"/><stop offset="1" stop-color="blue"/></linearGradient>
</defs>
<g marker-end="url(#a)" stroke-width="3">
  <path id="p" d="M4,4 L20,4 A10,10 0 0 1 40,24" fill="none" stroke="black" marker-start="url(#b)"/>
  <rect id="r" width="5" height="5"/><circle id="o" cx="9" cy="9" r="2"/>
  <line id="l" x1="1" y1="2" x2="30" y2="40" stroke="none" fill="none"/>
</g>
<polyline id="s" points="1,1 5,5 9,1" style="marker:url(#b);marker-mid:url(#c)"/>
<polygon id="n" points="1,1 5,5 9,1" marker="url(#b)" marker-mid="none" marker-end="url(#g)"/>
</svg>"""


def load(text):
    import svgrasterize_amd as S

    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        scene, ids, _size = S.svg_scene_from_str(text)
    return scene, ids, [str(w.message) for w in caught]


def nodes(scene, kind):
    out = []

    def walk(s):
        if s[0] == kind:
            out.append(s)
        if s[0] == 2:
            for c in s[1]:
                walk(c)
        elif s[0] in (3, 4, 5, 6, 7, 8):
            walk(s[1][0])
    walk(scene)
    return out


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to reach a device fails the test."""
    from svgrasterize_amd import _abi

    def refuse(*_a, **_k):
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(_abi.Context, "get", classmethod(refuse))
    monkeypatch.setattr(_abi, "path_markers", refuse)


def test_loader_reads_markers_without_a_device(no_device):
    from svgrasterize_amd import scene as SC

    scene, ids, warned = load(DOC)
    marked = nodes(scene, SC.RENDER_MARKERS)
    assert len(marked) == 4 and SC.RENDER_MARKERS == 9
    a, b, c = ids["a"], ids["b"], ids["c"]
    assert (a.ref, a.size, a.viewbox, a.preserve_aspect_ratio) == ((1.0, 2.0), (4.0, 6.0), (0.0, 0.0, 8.0, 4.0), "xMinYMax slice")
    assert (a.units_stroke_width, a.orient, a.clip) == (False, "auto-start-reverse", False)
    assert (b.ref, b.size, b.viewbox, b.units_stroke_width, b.orient, b.clip) == ((0.0, 0.0), (3.0, 3.0), None, True, 30.0, True)
    assert (c.orient, c.clip, c.ref) == ("auto", False, (0.0, 0.0)) and any("refX" in w for w in warned)
    p, line, s, n = (m[1] for m in marked)
    # the path: marker-start its own attribute, marker-end from the <g>, the stroke width from the <g>; behind fill and stroke
    assert (p.start, p.mid, p.end, p.stroke_width) == (b, None, a, 3.0)
    assert ids["p"][0] == SC.RENDER_GROUP and [c[0] for c in ids["p"][1]] == [SC.RENDER_STROKE, SC.RENDER_MARKERS]
    # neither fill nor stroke: the markers alone
    assert ids["l"][0] == SC.RENDER_MARKERS and (line.start, line.end, line.stroke_width) == (None, a, 3.0)
    # the shorthand in style, a longhand of the same element over it
    assert (s.start, s.mid, s.end, s.stroke_width) == (b, c, b, 1.0)
    # the shorthand as an attribute, "none", and a reference that is no marker
    assert (n.start, n.mid, n.end) == (b, None, None) and any("marker-end" in w and "not a marker" in w for w in warned)
    # rect, circle: none, although the <g> hands marker-end down
    assert ids["r"][0] == SC.RENDER_FILL and ids["o"][0] == SC.RENDER_FILL
    text = repr(scene)
    assert text.count("MARKERS stroke_width:") == 4 and "MARKER_START" in text and "orient:auto-start-reverse" in text
    assert all(m[1].scene is None and not m[1]._expanded for m in marked)   # printing expanded nothing


def test_text_gets_no_markers(no_device):
    from svgrasterize_amd import scene as SC

    font = ('<font id="f" horiz-adv-x="10"><font-face font-family="T" units-per-em="10"/>'
            '<glyph unicode="a" d="M0,0 L5,0 L5,5z"/></font>')
    doc = (f'<svg xmlns="http://www.w3.org/2000/svg" width="64" height="64"><defs>{font}<marker id="m"><rect width="1" height="1"/>'
           f'</marker></defs><g marker-start="url(#m)"><text font-family="T" x="5" y="20">aa</text></g></svg>')
    scene, _ids, _w = load(doc)
    assert scene is not None and not nodes(scene, SC.RENDER_MARKERS) and nodes(scene, SC.RENDER_FILL)


def test_unused_marker_changes_nothing():
    """A document without marker properties builds the tree it always has: with an unused <marker> in <defs> it dumps exactly
    like the copy without one."""
    from svgrasterize_amd import scenedump

    body = ('<g stroke="#00f" fill="none" stroke-width="2"><path d="M4,40 C20,20 40,60 60,40"/><polyline points="1,1 9,9 20,3"/></g>'
            '<rect x="8" y="8" width="30" height="12" rx="3" fill="#c00" opacity="0.5"/><line x1="1" y1="2" x2="30" y2="40" stroke="black"/>'
            '<polygon points="40,40 60,40 50,60"/>')
    head = '<svg xmlns="http://www.w3.org/2000/svg" width="64" height="64">'
    marker = '<defs><marker id="m" markerWidth="4" markerHeight="4" orient="auto"><path d="M0,0 L4,2 L0,4z"/></marker></defs>'
    plain, _i, w0 = load(head + body + "</svg>")
    extra, ids, w1 = load(head + marker + body + "</svg>")
    assert repr(plain) == repr(extra) and w0 == w1 == [] and "m" in ids
    (ta, aa), (tb, ab) = scenedump.dump_scene(plain), scenedump.dump_scene(extra)
    assert ta == tb and sorted(aa) == sorted(ab) and all(np.array_equal(aa[k], ab[k]) for k in aa)


class HostVertices:
    """Stands in for Path.vertices: the reference on the host; counts its calls."""

    def __init__(self):
        self.calls = 0

    def __call__(self, path):
        self.calls += 1
        types, params, sizes, flags = path._flagged_segment_arrays()
        xy, u, kind, _tol = R.vertices(types, np.array(params).reshape(-1, 8), sizes, flags)
        return xy, u.astype(np.float64), kind


@pytest.fixture
def host_vertices(monkeypatch, no_device):
    from svgrasterize_amd import geometry

    host = HostVertices()
    monkeypatch.setattr(geometry.Path, "vertices", lambda self: host(self))
    return host


def matrix(node):
    from svgrasterize_amd import scene as SC

    assert node[0] == SC.RENDER_TRANSFORM
    return np.asarray(node[1][1].m, dtype=np.float64)[:2]


def test_instances_are_separate_nodes_in_vertex_order(host_vertices):
    import svgrasterize_amd as S
    from svgrasterize_amd import scene as SC

    tip = S.Scene.fill(S.Path.from_svg("M0,0 L4,2 L0,4z"), np.array([1.0, 0, 0, 1]))
    dot = S.Scene.fill(S.Path.from_svg("M0,0 L1,0 L1,1z"), np.array([0, 0, 1.0, 1]))
    start = S.Marker(tip, ref=(1.0, 2.0), size=(4.0, 4.0), orient="auto-start-reverse")
    mid = S.Marker(dot, ref=(0.5, 0.25), size=(2.0, 2.0), viewbox=(0.0, 0.0, 4.0, 2.0), preserve_aspect_ratio="xMaxYMin slice",
                   units_stroke_width=False, orient=90.0)
    end = S.Marker(tip, ref=(1.0, 2.0), size=(4.0, 4.0), orient="auto", clip=False)
    node = S.Scene.markers(S.Path.from_svg("M10,10 L30,10 L30,40"), start, mid, end, stroke_width=2.0)
    assert node[0] == SC.RENDER_MARKERS and host_vertices.calls == 0 and "MARKERS" in repr(node) and host_vertices.calls == 0
    group = SC._expanded(node)
    assert SC._expanded(node) is group and host_vertices.calls == 1     # one expansion per node
    assert group[0] == SC.RENDER_GROUP and len(group[1]) == 3
    first, middle, last = group[1]
    # start, reversed: translate(10, 10) rotate(180) scale(2) translate(-1, -2)
    assert np.allclose(matrix(first), [[-2, 0, 12], [0, -2, 14]], atol=1e-15)
    # mid: viewBox 4 x 2 sliced into 2 x 2 -> scale 1, no stroke-width scaling; rotate(90) about the vertex, (0.5, 0.25) on it
    assert np.allclose(matrix(middle), [[0, -1, 30.25], [1, 0, 9.5]], atol=1e-15)
    # end: direction (0, 1), scale 2
    assert np.allclose(matrix(last), [[0, -2, 34], [2, 0, 38]], atol=1e-15)
    # the clipped ones are CLIP nodes under their transform: the viewport in content coordinates
    assert first[1][0][0] == SC.RENDER_CLIP and middle[1][0][0] == SC.RENDER_CLIP and last[1][0] is tip
    assert first[1][0][1][1][1][0].user_box() == (0.0, 0.0, 4.0, 4.0)
    assert middle[1][0][1][1][1][0].user_box() == (2.0, 0.0, 4.0, 2.0)   # xMax: the right half of the viewBox is visible


def test_markers_that_draw_nothing(host_vertices):
    import svgrasterize_amd as S
    from svgrasterize_amd import scene as SC

    tip = S.Scene.fill(S.Path.from_svg("M0,0 L4,2 L0,4z"), np.array([1.0, 0, 0, 1]))
    path = S.Path.from_svg("M10,10 L30,10 L30,40")
    for marker in (S.Marker(tip, size=(0.0, 4.0)), S.Marker(tip, size=(4.0, 0.0)), S.Marker(None), S.Marker(tip, viewbox=(0.0, 0.0, 0.0, 4.0))):
        node = S.Scene.markers(path, marker, marker, marker)
        assert SC._expanded(node) is None
        assert SC._batchable_leaves(node, S.Transform(), False) == []
        assert repr(S.Scene.group([S.Scene.fill(path, np.ones(4)), node]).to_path(S.Transform())) == repr(path)
    assert host_vertices.calls == 0   # nothing to place: the vertices were never asked for
    # only mid vertices, a path with none
    node = S.Scene.markers(S.Path.from_svg("M1,1 L9,9"), None, S.Marker(tip), None)
    assert SC._expanded(node) is None and host_vertices.calls == 1


def test_walkers_go_on_with_the_expanded_group(host_vertices):
    import svgrasterize_amd as S
    from svgrasterize_amd import displaylist, scenedump
    from svgrasterize_amd import scene as SC

    scene, _ids, _w = load(DOC)
    marked = nodes(scene, SC.RENDER_MARKERS)
    tr = S.Transform()
    # to_path: every instance's outline, transformed
    line = marked[1]
    outline = line.to_path(tr)
    want = SC._expanded(line).to_path(tr)
    assert len(outline.subpaths) == len(want.subpaths) == 1 and repr(outline) == repr(want)
    # the leaf analysis (the walk's and the display list's) sees the instances' leaves
    leaves = SC._batchable_leaves(line, tr, False)
    again = SC._batchable_leaves(SC._expanded(line), tr, False)
    assert leaves is not None and len(leaves) == len(again) == 1 and leaves[0][0] is again[0][0] and np.array_equal(leaves[0][1], again[0][1])
    sym = SC._batchable_leaves_(S.Scene.group([S.Scene.fill(S.Path.from_svg("M0,0 L9,0 L9,9z"), np.ones(4)), line]), (), False, None,
                                displaylist._Symbolic)
    assert sym is not None and len(sym) == 2
    # the dump holds the expanded group in the node's place
    tree, _arrays = scenedump.dump_scene(line)
    assert tree == scenedump.dump_scene(SC._expanded(line))[0] and tree["t"] == "transform"
    # the pre-pass routes like the walk
    jobs, runs, fills = [], [], []
    SC._collect_mask_jobs(S.Scene.group([line, line]), tr, False, False, jobs, runs, fills)
    assert len(runs) == 1 and len(runs[0]) == 2
    assert host_vertices.calls == 1
