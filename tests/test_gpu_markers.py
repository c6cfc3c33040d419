"""Markers on the GPU: svgr_path_markers through the C ABI against the host reference (tests/marker_ref.py) on shapes at the
seams of its launch geometry -- B = svgr_marker_block_segments() segments per workgroup of its own kernels, S =
svgr_dash_scan_segments() per workgroup of the scans -- and marker documents end to end against the same documents with every
marker instance written out by hand.  Positions and kinds are compared exactly, directions within the reference's derived
tolerance; tests/test_marker_host.py checks on the CPU that the inputs are what they are meant to be."""
import math
import warnings

import numpy as np
import pytest

from tests import marker_cases as cases
from tests import marker_ref as R
from tests.util import assert_close64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def abi():
    from svgrasterize_amd import _abi

    _abi.Context.get()
    return _abi


FIXED = cases.fixed_cases()


def run(abi, path, flags):
    return abi.path_markers(path[0], np.array(path[1], dtype=np.float64), path[2], flags)


def test_seams_are_what_the_cases_assume(abi):
    assert abi.marker_block_segments() == cases.B and abi.dash_scan_segments() == cases.S


@pytest.mark.parametrize("case", FIXED, ids=[c[0] for c in FIXED])
def test_fixed_case(abi, case):
    name, path, flags = case
    worst = R.check(run(abi, path, flags), R.vertices(*path, flags), name)
    print(f"{name}: largest error / tolerance {worst:.3f}")


def test_fuzz_set(abi):
    ran = 0
    for name, path, flags in cases.fuzz_cases():
        detail = {}
        want = R.vertices(*path, flags, detail=detail)
        if detail["clearance"] < 1e-6:
            continue
        R.check(run(abi, path, flags), want, name)
        ran += 1
    assert ran >= 190


def test_two_runs_are_byte_identical(abi):
    for wanted in (f"mix{2 * cases.S + 1}", "degenerate_run_forward_S", "vertex_flags_across_S"):
        _name, path, flags = next(c for c in FIXED if c[0] == wanted)
        a, b = run(abi, path, flags), run(abi, path, flags)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), wanted


def test_bad_and_empty_input(abi):
    xy, u, kind = abi.path_markers([], np.zeros((0, 8)), [])
    assert xy.shape == (0, 2) and u.shape == (0, 2) and len(kind) == 0
    before = abi.Context.get().launches()
    xy, _u, _kind = abi.path_markers([R.UNCLOSED], np.zeros((1, 8)), [1])   # a subpath without an outline: no vertex, no launch
    assert len(xy) == 0 and abi.Context.get().launches() == before
    line = R.polyline([(0, 0), (10, 0), (10, 10)])
    for bad in (float("nan"), float("inf"), -float("inf"), 1e155):
        params = np.array(line[1], dtype=np.float64)
        params[1, 2] = bad
        with pytest.raises(ValueError):
            abi.path_markers(line[0], params, line[2])
        assert abi.Context.get().launches() == before   # nothing was launched
    with pytest.raises(ValueError):
        abi.path_markers([R.LINE, R.QUAD, R.UNCLOSED], np.array(line[1], dtype=np.float64), line[2])
    with pytest.raises(ValueError):
        abi.path_markers(line[0], np.array(line[1], dtype=np.float64), line[2], [1, 1])   # flags that do not match
    assert abi.Context.get().launches() == before


def test_path_vertices(abi):
    from svgrasterize_amd import Path

    xy, u, kind = Path.from_svg("M0,0 A10,10 0 0 1 20,0").vertices()
    assert len(xy) == 2 and list(kind) == [0, 2] and np.allclose(u, [(0, -1), (0, 1)], atol=1e-14)
    xy, u, kind = Path.from_svg("M0,0 L10,0 L0,0").vertices()
    assert xy.tolist() == [[0, 0], [10, 0], [0, 0]] and u.tolist() == [[1, 0], [0, 1], [-1, 0]] and list(kind) == [0, 1, 2]
    xy, u, kind = Path([]).vertices()
    assert xy.shape == u.shape == (0, 2) and kind.shape == (0,)


# ---- end to end ---------------------------------------------------------------------------------------------------------------
SIZE = 128
HEAD = f'<svg xmlns="http://www.w3.org/2000/svg" width="{SIZE}" height="{SIZE}">'
# name -> what the <marker> says and, worked out by hand, what it comes to: the scale of its viewBox mapping and its viewport in
# content coordinates.
#   arrow: viewBox 8 x 4 sliced into 6 x 6: scale max(6 / 8, 6 / 4) = 1.5, xMax: shifted by 6 - 12 = -6, YMid: by (6 - 6) / 2 = 0;
#          the viewport is x in [6 / 1.5, 12 / 1.5] = [4, 8], y in [0, 4] of the content: the arrow's left half hangs out of it
#   dot:   no viewBox: scale 1, the viewport is [0, 4] x [0, 4]
#   tail:  viewBox 6 x 3 into 3 x 3 with "none": scale (0.5, 1), the viewport is the viewBox
MARKERS = {
    "arrow": dict(attrs='viewBox="0 0 8 4" markerWidth="6" markerHeight="6" preserveAspectRatio="xMaxYMid slice" refX="6" refY="2" orient="auto"',
                  content='<path d="M0,0 L8,2 L0,4z" fill="#c00"/>', ref=(6, 2), scale=(1.5, 1.5), clip=(4, 0, 8, 4), orient="auto",
                  stroke_units=True),
    "dot": dict(attrs='markerWidth="4" markerHeight="4" refX="2" refY="2" markerUnits="userSpaceOnUse" orient="30"',
                content='<circle cx="2" cy="2" r="2" fill="#00c"/><rect x="1.5" y="-1" width="1" height="6" fill="#0c0"/>', ref=(2, 2),
                scale=(1, 1), clip=(0, 0, 4, 4), orient=30.0, stroke_units=False),
    "tail": dict(attrs='viewBox="0 0 6 3" markerWidth="3" markerHeight="3" preserveAspectRatio="none" refX="0.5" refY="1.5" '
                       'orient="auto-start-reverse"',
                 content='<path d="M0,0 L6,1.5 L0,3z" fill="#080"/>', ref=(0.5, 1.5), scale=(0.5, 1), clip=(0, 0, 6, 3),
                 orient="auto-start-reverse", stroke_units=True),
}
# (shape, its stroke width, its marker-start / -mid / -end)
SHAPES = [
    ('<polyline points="20,20 60,20 60,50 100,50" fill="none" stroke="#000" stroke-width="2" {m}/>', "M20,20 60,20 60,50 100,50", 2.0,
     ("tail", "dot", "arrow")),
    ('<polygon points="20,70 50,70 35,100" fill="#ddd" stroke-width="1.5" {m}/>', "M20,70 50,70 35,100z", 1.5, ("dot", "dot", "dot")),
    ('<path d="M70,80 L90,80 A15,15 0 0 1 110,110" fill="none" stroke="#333" {m}/>', "M70,80 L90,80 A15,15 0 0 1 110,110", 1.0,
     ("tail", "arrow", "arrow")),
]


def defs(visible=()):
    out = []
    for name, m in MARKERS.items():
        extra = ' overflow="visible"' if name in visible else ""
        out.append(f'<marker id="{name}" {m["attrs"]}{extra}>{m["content"]}</marker>')
    return "<defs>" + "".join(out) + "</defs>"


def marker_document(visible=()):
    body = []
    for k, (shape, _d, _sw, (s, m, e)) in enumerate(SHAPES):
        props = f'marker-start="url(#{s})" marker-mid="url(#{m})" marker-end="url(#{e})"'
        if k == 1:
            props = f'style="marker:url(#{s})"'   # the shorthand, in style
        body.append(shape.format(m=props))
    return HEAD + defs(visible) + "".join(body) + "</svg>"


def instance_matrix(m, x, y, ux, uy, stroke_width, at_start):
    """translate(x, y) rotate scale translate(-ref), as 3 x 3 products."""
    if m["orient"] == "auto":
        c, s = ux, uy
    elif m["orient"] == "auto-start-reverse":
        c, s = (-ux, -uy) if at_start else (ux, uy)
    else:
        c, s = math.cos(math.radians(m["orient"])), math.sin(math.radians(m["orient"]))
    k = stroke_width if m["stroke_units"] else 1.0
    T = np.array([[1, 0, x], [0, 1, y], [0, 0, 1.0]])
    Rm = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
    Sm = np.diag([k * m["scale"][0], k * m["scale"][1], 1.0])
    T2 = np.array([[1, 0, -m["ref"][0]], [0, 1, -m["ref"][1]], [0, 0, 1.0]])
    return T @ Rm @ Sm @ T2


def expanded_document(visible=()):
    """The marker document with every instance written out: <g transform="matrix(...)"> around the marker's content, clipped by
    an explicit clipPath; the vertices are the reference's."""
    from svgrasterize_amd import Path

    clips = []
    for name, m in MARKERS.items():
        x0, y0, x1, y1 = m["clip"]
        clips.append(f'<clipPath id="clip_{name}"><path d="M{x0!r},{y0!r} L{x1!r},{y0!r} L{x1!r},{y1!r} L{x0!r},{y1!r}z"/></clipPath>')
    body = []
    for shape, d, sw, names in SHAPES:
        body.append(shape.format(m=""))
        types, params, sizes, flags = Path.from_svg(d)._flagged_segment_arrays()
        xy, u, kind, _tol = R.vertices(types, np.array(params).reshape(-1, 8), sizes, flags)
        for (x, y), (ux, uy), k in zip(xy.tolist(), u.astype(np.float64).tolist(), kind.tolist()):
            name = names[k]
            M = instance_matrix(MARKERS[name], x, y, ux, uy, sw, k == 0)
            matrix = " ".join(repr(float(v)) for v in (M[0, 0], M[1, 0], M[0, 1], M[1, 1], M[0, 2], M[1, 2]))
            clip = "" if name in visible else f' clip-path="url(#clip_{name})"'
            body.append(f'<g transform="matrix({matrix})"{clip}>{MARKERS[name]["content"]}</g>')
    return HEAD + "<defs>" + "".join(clips) + "</defs>" + "".join(body) + "</svg>"


def load(text):
    import svgrasterize_amd as S

    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        scene, _ids, _size = S.svg_scene_from_str(text)
    assert not caught, [str(w.message) for w in caught]
    return scene


def find(scene, kind):
    """The nodes of one kind under GROUP and TRANSFORM nodes."""
    if scene[0] == kind:
        return [scene]
    if scene[0] == 2:
        return [n for c in scene[1] for n in find(c, kind)]
    return find(scene[1][0], kind) if scene[0] == 6 else []


def canvas(scene):
    import svgrasterize_amd as S

    view = S.Transform().matrix(0, 1, 0, 1, 0, 0)   # (render_svg's: x along the columns)
    out = scene.render(view, viewport=[0, 0, SIZE, SIZE], linear_rgb=True)
    assert out is not None
    layer = out[0]
    full = np.zeros((SIZE, SIZE, 4))
    img = np.asarray(layer.image, dtype=np.float64)
    y, x = layer.offset
    full[y:y + img.shape[0], x:x + img.shape[1]] = img
    return full


@pytest.fixture(scope="module")
def renders(abi):
    """The marker document and its hand-expanded twin, clipped and with the arrow's overflow visible: rendered once."""
    import svgrasterize_amd as S

    S.clear_render_cache()
    return {key: (canvas(load(marker_document(vis))), canvas(load(expanded_document(vis)))) for key, vis in (("clipped", ()), ("visible", ("arrow",)))}


@pytest.mark.parametrize("key", ["clipped", "visible"])
def test_document_renders_like_its_hand_expanded_twin(renders, key):
    got, want = renders[key]
    assert got[..., 3].max() > 0.99
    err = np.abs(got - want)
    print(f"{key}: max |delta| {err.max():.3e} over {int((err > 0).sum())} differing values")
    assert_close64(got, want, what=key)


def test_overflow_shows_where_the_marker_overhangs(renders):
    clipped, visible = renders["clipped"][0], renders["visible"][0]
    # the polyline's last vertex (100, 50), direction (1, 0), stroke width 2: the arrow is drawn at scale 1.5 x 2 = 3 with refX 6 on
    # the vertex, so the visible right half of its content (x in [4, 8]) covers x in [94, 106] and the clipped left half x in
    # [82, 94]; y in [44, 56]
    differ = np.abs(clipped - visible).max(axis=2) > 1e-6
    assert differ[48:53, 84:93].all()                                                    # the overhang
    assert np.abs(clipped[44:57, 95:107] - visible[44:57, 95:107]).max() <= 1e-12        # inside the viewport both draw the same
    assert clipped[49:51, 96:100, 3].min() > 0.99   # (at x = 100 the arrow reaches y = 50 +- 1.5)
    assert not differ[:40].any() and not differ[60:, :60].any()   # the tails and dots of the first two shapes are as they were


def test_markers_are_drawn_without_fill_or_stroke(abi):
    doc = (HEAD + defs() + '<line x1="20" y1="20" x2="100" y2="20" stroke="none" fill="none" stroke-width="2" marker-end="url(#arrow)"/></svg>')
    full = canvas(load(doc))
    # the arrow at (100, 20), clipped to its right half: x in [94, 106]; nothing else is drawn
    assert full[18:23, 95:105, 3].max() > 0.99 and full[:, :93, 3].max() == 0.0
    # stroke-width scales it although nothing is stroked: at x = 95.5 the arrow reaches y = 20 +- 2.6 (+- 1.3 at scale 1.5)
    assert full[18, 95, 3] > 0.99 and full[12, 95, 3] == 0.0


def test_every_render_route_draws_the_same(abi, monkeypatch, renders):
    import svgrasterize_amd as S
    from svgrasterize_amd import displaylist

    want = renders["clipped"][0]
    text = marker_document()
    monkeypatch.setattr(displaylist, "ENABLED", False)    # the scene walk
    walk = canvas(load(text))
    assert_close64(walk, want, what="scene walk")
    monkeypatch.setattr(displaylist, "ENABLED", True)
    scene = load(text)
    assert displaylist.get(scene, True) is not None       # the display list holds the instances' leaves
    assert_close64(canvas(scene), want, what="display list")
    S.set_render_cache(2)
    try:
        scene = load(text)
        cold, warm = canvas(scene), canvas(scene)
    finally:
        S.set_render_cache(0)
    assert_close64(cold, want, what="render cache, first render")
    assert_close64(warm, want, what="render cache, second render")
    # one expansion per node, whichever routes drew it
    from svgrasterize_amd import scene as SC
    marked = find(scene, SC.RENDER_MARKERS)
    assert len(marked) == 3 and all(m[1]._expanded and m[1].scene is not None for m in marked)
