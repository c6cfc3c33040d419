"""Text on a path on the CPU: the per-lane header (csrc/svgr_textpath.h, through tests/textpath_harness.cpp) against the
reference (tests/textpath_ref.py) on the shapes the GPU test runs, the conditions those shapes must keep -- by the reference
alone, so that the GPU test cannot hide a failure behind skips --, closed-form placements, and the library layer without a
device: the loader and the lazy node, with the harness standing in for the two device calls."""
import ctypes
import math
import os
import warnings

import numpy as np
import pytest

from tests import textpath_cases as cases
from tests import textpath_ref as R
from tests.util import ROOT, host_build

P = ctypes.c_void_p


def _lib():
    lib = host_build("textpath_harness")
    lib.th_sample.restype = ctypes.c_double
    return lib


def _p(a):
    return a.ctypes.data_as(P)


def harness_sample(types, params, sizes, s):
    """svgr_path_sample by the header: (xy, direction, inside, L)."""
    types = np.ascontiguousarray(types, dtype=np.int32)
    params = np.ascontiguousarray(params, dtype=np.float64).reshape(-1, 8)
    s = np.ascontiguousarray(s, dtype=np.float64).reshape(-1)
    xyuv, inside = np.zeros((len(s), 4)), np.zeros(len(s), dtype=np.int32)
    if not len(types):
        return xyuv[:, :2].copy(), xyuv[:, 2:].copy(), inside != 0, 0.0
    L = _lib().th_sample(_p(types), _p(params), len(types), _p(s), len(s), _p(xyuv), _p(inside))
    return xyuv[:, :2].copy(), xyuv[:, 2:].copy(), inside != 0, L


def harness_place(types, params, sizes, a_types, a_params, a_off, glyph, s_mid, half, dy):
    """svgr_path_place_glyphs by the header: (params (n_out, 8), visible, L)."""
    types = np.ascontiguousarray(types, dtype=np.int32)
    params = np.ascontiguousarray(params, dtype=np.float64).reshape(-1, 8)
    a_types = np.ascontiguousarray(a_types, dtype=np.int32)
    a_params = np.ascontiguousarray(a_params, dtype=np.float64).reshape(-1, 8)
    a_off = np.ascontiguousarray(a_off, dtype=np.int32)
    glyph = np.ascontiguousarray(glyph, dtype=np.int32)
    s_mid, half, dy = (np.ascontiguousarray(a, dtype=np.float64) for a in (s_mid, half, dy))
    off = np.concatenate([[0], np.cumsum(np.diff(a_off)[glyph])]).astype(np.int32)
    out, visible = np.zeros((int(off[-1]), 8)), np.zeros(len(glyph), dtype=np.int32)
    if not len(types):
        return out, visible != 0, 0.0
    rc = _lib().th_place_glyphs(_p(types), _p(params), len(types), _p(a_types), _p(a_params), len(a_types), _p(a_off), _p(glyph), _p(off),
                                _p(s_mid), _p(half), _p(dy), len(glyph), _p(out), _p(visible))
    assert rc == 0
    return out, visible != 0, harness_sample(types, params, sizes, [])[3]


def run_case(atlas, case, sample, place):
    """One case through `sample` / `place` (the harness here, the C ABI in the GPU test) against the reference; returns the
    largest share of the tolerance."""
    worst = 0.0
    if case["s"] is not None:
        d = {}
        want = R.sample(*case["path"], case["s"], case["exact"], d)
        got = sample(*case["path"], case["s"])
        worst = max(worst, R.check_sample(got[:3], want, d["fragile"], case["exact"], case["name"]))
        assert abs(got[3] - float(want[5])) <= d["d_point"], (case["name"], got[3], float(want[5]))
    if case["inst"] is not None:
        d = {}
        want = R.place(*case["path"], *atlas, *case["inst"], case["exact"], d)
        got = place(*case["path"], *atlas, *case["inst"])
        worst = max(worst, R.check_place(got[:2], want, d["fragile"], case["exact"], case["name"]))
        assert abs(got[2] - float(want[4])) <= d["d_point"], (case["name"], got[2], float(want[4]))
    return worst


FIXED_ATLAS, FIXED = cases.fixed_cases()


# ---- the conditions of the inputs, by the reference alone ---------------------------------------------------------------------
def test_fixed_cases_keep_their_clearance():
    for case in FIXED:
        assert cases.clearance(FIXED_ATLAS, case) > cases.CLEARANCE, case["name"]


def test_fuzz_set_stays_within_its_cap():
    low = [case["name"] for atlas, case in cases.fuzz_cases() if cases.clearance(atlas, case) < cases.FUZZ_CLEARANCE]
    assert len(low) <= cases.FUZZ_MAY_SKIP * 200, low


def test_reference_on_hand_computed_frames():
    path = R.polyline([(0, 0), (3, 0), (3, 4), (0, 0)])      # the 3-4-5 triangle, drawn open: 12 long
    xy, uv, inside, _txy, _tdir, L = R.sample(*path, [0, 3, 5, 7, 9.5, 12, 12.5, -1], exact=True)
    assert float(L) == 12.0
    assert np.allclose(xy.astype(float), [(0, 0), (3, 0), (3, 2), (3, 4), (1.5, 2), (0, 0), (0, 0), (0, 0)], atol=1e-15)
    assert np.allclose(uv.astype(float), [(1, 0), (0, 1), (0, 1), (-0.6, -0.8), (-0.6, -0.8), (-0.6, -0.8), (-0.6, -0.8), (1, 0)], atol=1e-15)
    assert inside.tolist() == [True] * 6 + [False, False]


# ---- the header against the reference -------------------------------------------------------------------------------------------
def test_searches():
    lib = _lib()
    a = np.array([1.0, 1.0, 2.0, 4.0, 4.0, 7.0])
    for n in range(0, 7):
        for s in (0.0, 1.0, 1.5, 2.0, 4.0, 6.9, 7.0, 8.0):
            assert lib.th_count(_p(a), n, ctypes.c_double(s), 0) == int((a[:n] <= s).sum())
            assert lib.th_count(_p(a), n, ctypes.c_double(s), 1) == int((a[:n] < s).sum())
    off = np.array([0, 0, 3, 3, 3, 8, 9], dtype=np.int32)   # 6 ranges, three of them empty
    for j in range(9):
        k = lib.th_owner(_p(off), 6, j)
        assert off[k] <= j < off[k + 1]


@pytest.mark.parametrize("case", FIXED + cases.joint_cases(), ids=lambda c: c["name"])
def test_header_matches_reference(case):
    run_case(FIXED_ATLAS, case, harness_sample, harness_place)


def test_header_matches_reference_on_the_fuzz_set():
    ran = 0
    for atlas, case in cases.fuzz_cases():
        if cases.clearance(atlas, case) < cases.FUZZ_CLEARANCE:
            continue
        run_case(atlas, case, harness_sample, harness_place)
        ran += 1
    assert ran >= 190


def test_place_is_the_definition():
    """Two fused multiply-adds per coordinate: two roundings of values below 120, against the long double form."""
    rng = np.random.default_rng(3)
    lib = _lib()
    for _ in range(200):
        f = rng.uniform(-50, 50, 4)
        f[2:] /= np.hypot(*f[2:])
        h, dy, x, y = rng.uniform(-9, 9, 4)
        out = np.zeros(2)
        lib.th_place(_p(f), ctypes.c_double(h), ctypes.c_double(dy), ctypes.c_double(x), ctypes.c_double(y), _p(out))
        a, b = x - h, y + dy
        want = (R.LD(f[0]) + R.LD(f[2]) * R.LD(a) - R.LD(f[3]) * R.LD(b), R.LD(f[1]) + R.LD(f[3]) * R.LD(a) + R.LD(f[2]) * R.LD(b))
        assert abs(float(out[0] - want[0])) <= 2 * R.U * 120 and abs(float(out[1] - want[1])) <= 2 * R.U * 120


# ---- the library layer, the harness standing in for the device ---------------------------------------------------------------------
@pytest.fixture()
def on_host(monkeypatch):
    """The two device calls answered by the header's host build; any other way to a device fails the test."""
    from svgrasterize_amd import _abi

    def sample(types, params, sizes, s=(), ctx=None):
        return harness_sample(types, params, sizes, s)

    def place(types, params, sizes, a_types, a_params, a_off, glyph, s_mid, half, dy, ctx=None):
        return harness_place(types, params, sizes, a_types, a_params, a_off, glyph, s_mid, half, dy)

    def no_device(*_a, **_k):
        raise AssertionError("a device was asked for")

    monkeypatch.setattr(_abi, "path_sample", sample)
    monkeypatch.setattr(_abi, "path_place_glyphs", place)
    monkeypatch.setattr(_abi.Context, "get", classmethod(no_device))
    return _abi


def _font():
    import svgrasterize_amd as S

    fonts = S.FontsDB()
    S.svg_scene_from_str(cases.document(""), fonts=fonts)
    return fonts.resolve("TP")


def _arrays(path):
    types, params, sizes = path._segment_arrays()
    return np.array(types), np.array(params).reshape(-1, 8), list(sizes)


def test_triangle_length_is_twelve(on_host):
    import svgrasterize_amd as S

    assert S.Path.from_svg("M0,0 L3,0 L3,4 Z").length() == 12.0
    assert S.Path([]).length() == 0.0
    xy, direction, inside = S.Path.from_svg("M0,0 L3,0 L3,4 Z").point_at([5.0, 13.0])
    assert xy.tolist() == [[3.0, 2.0], [0.0, 0.0]] and direction[0].tolist() == [0.0, 1.0] and inside.tolist() == [True, False]
    assert S.Path.from_svg("M0,0 L3,0").point_at(1.5)[0].tolist() == [[1.5, 0.0]]


def test_straight_path_is_str_to_path_translated(on_host):
    import svgrasterize_amd as S

    font = _font()
    line = S.Path.from_svg("M0,0 H1000")
    for offset in (0.0, 37.25, 411.0):
        on, advance = font.str_on_path(line, 48.0, "AOI A", offset)
        straight, advance2 = font.str_to_path(48.0, "AOI A")
        assert advance == advance2
        t1, p1, s1 = _arrays(on)
        t2, p2, s2 = _arrays(straight)
        assert t1.tolist() == t2.tolist() and s1 == s2
        moved = p2.copy()
        moved[:, 0::2] += offset
        moved[(t2 != 2)[:, None] & (np.arange(8) >= 4)[None, :]] = 0.0
        # a few ulp of the coordinates (< 1000): the two sides scale and add in different orders
        assert np.abs(p1 - moved).max() <= 8 * 2.0 ** -52 * 1000


def test_circle_spaces_glyphs_by_equal_angles(on_host):
    import svgrasterize_amd as S
    from svgrasterize_amd.svg import ellipse_path_data

    font = _font()
    r, size = 100.0, 20.0
    circle = S.Path.from_svg(ellipse_path_data(0.0, 0.0, r, r))
    L = circle.length()
    assert abs(L - 2 * math.pi * r) < 1e-3 * r           # (the circle is four arcs turned into cubics: not a circle exactly)
    on, _advance = font.str_on_path(circle, size, "IIIIII", 10.0)
    t, p, sizes = _arrays(on)
    assert sizes == [4] * 6
    # the glyph "I" is the box (100, 0)-(200, 700) of a 300 advance: its first segment is its baseline, from x = 100 to 200
    base = p[0::4]
    mid = (base[:, 0:2] + base[:, 2:4]) / 2                # the middle of each baseline: the anchor itself
    angle = np.unwrap(np.arctan2(mid[:, 1], mid[:, 0]))
    step = np.diff(angle)
    assert np.abs(step - step[0]).max() < 1e-3 and abs(step[0] - 300 * size / 1000 / r) < 1e-3   # equal advances, equal angles
    assert np.abs(np.hypot(mid[:, 0], mid[:, 1]) - r).max() < 1e-3 * r
    d = base[:, 2:4] - base[:, 0:2]
    assert np.abs((d * mid).sum(axis=1)).max() < 1e-3 * r * np.hypot(d[:, 0], d[:, 1]).max()     # tangent: across the radius


def test_glyph_arrays_are_converted_once():
    font = _font()
    glyph = font.glyphs["O"]
    assert glyph.arrays is glyph.arrays and glyph.arrays[0].tolist().count(2) == 8 and glyph.arrays[2].tolist() == [5, 5]


DOC = cases.document("""
<path id="wave" d="M20,120 C80,20 160,220 236,110" fill="none" stroke="none" pathLength="200"/>
<rect id="box" x="10" y="10" width="40" height="30" fill="none" transform="translate(100,100)"/>
<g id="group"><path d="M0,0 H9"/></g>
<text font-family="TP" font-size="24" x="7" y="9">lead
  <textPath href="#wave" startOffset="25%" text-anchor="middle" fill="#ff0000">A<tspan dx="3" dy="-2" fill="#0000ff" stroke="#000" stroke-dasharray="2 1">O  I</tspan> A</textPath>
  <textPath xlink:href="#box" startOffset="30" method="stretch" side="right" x="5" y="6">IO</textPath>
  <textPath href="#nowhere">A</textPath>
  <textPath href="#group">A</textPath>
tail</text>""")


def _find(scene, kind, out):
    import svgrasterize_amd as S

    if scene[0] == kind:
        out.append(scene)
    elif scene[0] == S.RENDER_GROUP:
        for child in scene[1]:
            _find(child, kind, out)
    elif scene[0] in (S.RENDER_OPACITY, S.RENDER_CLIP, S.RENDER_MASK, S.RENDER_TRANSFORM, S.RENDER_FILTER, S.RENDER_BLEND):
        _find(scene[1][0], kind, out)
    return out


def test_loader_builds_the_lazy_node_without_a_device(on_host):
    import svgrasterize_amd as S

    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        scene, _ids, _size = S.svg_scene_from_str(DOC)
    nodes = _find(scene, S.RENDER_MARKERS, [])
    assert len(nodes) == 2 and all(isinstance(n[1], S.TextOnPath) and n[1].scene is None for n in nodes)
    wave, box = (n[1] for n in nodes)
    assert (wave.start_offset, wave.percent, wave.anchor, wave.path_length) == (25.0, True, "middle", 200.0)
    assert [(r.text, r.size, r.dx, r.dy) for r in wave.runs] == [("A", 24.0, 0.0, 0.0), ("O I", 24.0, 3.0, -2.0), (" A", 24.0, 0.0, 0.0)]
    assert wave.runs[0].attrs["fill"] == "#ff0000" and wave.runs[1].attrs["fill"] == "#0000ff" and wave.runs[2].attrs["fill"] == "#ff0000"
    assert wave.runs[1].attrs["stroke-dasharray"] == "2 1" and "stroke-dasharray" not in wave.runs[2].attrs
    assert (box.start_offset, box.percent, box.anchor, box.path_length) == (30.0, False, None, None)
    assert [(r.text, r.dx, r.dy) for r in box.runs] == [("IO", 0.0, 0.0)]      # x / y inside a textPath are ignored
    assert np.allclose(np.array(box.path.subpaths[0][0][1], dtype=float), [[110, 110], [150, 110]])   # the rect's own transform
    texts = [str(w.message) for w in caught]
    assert sum('method="stretch"' in t for t in texts) == 1 and sum('side="right"' in t for t in texts) == 1
    assert sum("not a shape referenced" in t for t in texts) == 2
    text = repr(scene)          # (printing does not expand either)
    assert text.count("TEXT_ON_PATH") == 2 and "start_offset:25% anchor:middle pathLength:200" in text and "RUN 'O I'" in text
    assert wave.scene is None and box.scene is None
    # the straight runs around them stay where they were: "lead " at the pen, "tail" after it, nothing moved by the textPaths
    assert text.count("TRANSFORM") == 3       # the document's viewBox and the two straight runs
    # -- expansion, the harness standing in for the device: one FILL per run, the second run also a dashed STROKE
    group = wave.expand()
    assert group[0] == S.RENDER_GROUP and [n[0] for n in group[1]] == [S.RENDER_FILL, S.RENDER_FILL, S.RENDER_STROKE, S.RENDER_FILL]
    from svgrasterize_amd.geometry import DashedPath

    assert isinstance(group[1][2][1][0], DashedPath) and wave.expand() is group
    # startOffset 25 % of the length, middle anchor: the chunk is centred there
    L = wave.path.length()
    centre = L * 0.25
    first = _arrays(group[1][0][1][0])[1]
    xy, _u, _in = wave.path.point_at(centre - wave.advance() / 2 + 0.35 * 24)   # the anchor of the first "A" (advance 700)
    assert np.abs(first[:, :4].reshape(-1, 2) - xy[0]).max() < 24.0


def test_scene_text_on_path_without_a_loader(on_host):
    import svgrasterize_amd as S

    font = _font()
    node = S.Scene.text_on_path(S.Path.from_svg("M0,50 H200"), [("AI", font, 20.0, {}, 0.0, 0.0)], start_offset=100.0, anchor="end")
    assert node[0] == S.RENDER_MARKERS and node[1].scene is None
    fill = node[1].expand()
    assert fill[0] == S.RENDER_FILL
    params = _arrays(fill[1][0])[1]
    xs = params[:, 0:4:2]
    assert xs.max() <= 100.0 + 1e-9 and xs.min() >= 100.0 - 20.0 + 1e-9 - 1e-9        # (700 + 300) / 1000 * 20 = 20 wide, ending at 100
    with pytest.raises(ValueError):
        S.Scene.text_on_path(S.Path([]), [], anchor="centre")


def test_documents_without_textpath_build_as_before():
    """A document of straight text with nested tspans against what the commit in front of this feature made of it
    (tests/golden/textpath_plain_scene.txt: the scene's repr)."""
    import svgrasterize_amd as S

    plain = DOC.replace("textPath", "tspan")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        scene, _ids, _size = S.svg_scene_from_str(plain)
    assert not _find(scene, S.RENDER_MARKERS, [])
    with open(os.path.join(ROOT, "tests", "golden", "textpath_plain_scene.txt")) as f:
        assert repr(scene) == f.read()
