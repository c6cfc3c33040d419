"""Stylesheets, display / visibility, <symbol>, <switch> and <a> in the loader (svgrasterize.py_amd/svg.py): every styled document
of tests/css_cases.py loads to exactly the scene of its plain twin, and documents that use none of it load to exactly the scene
they loaded to before the loader knew stylesheets (tests/golden/loader_dumps_before_css.npz: the scene dumps of the demo
documents and of tests/svg_cases.py, recorded on the commit before)."""
import hashlib
import json
import os
import warnings

import numpy as np
import pytest

from tests import css_cases, svg_cases

GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEMO = os.path.join(GOLD, "demo")


def load(name, text, styled):
    import svgrasterize_amd as S

    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        scene, ids, size = S.svg_scene_from_str(text, **(css_cases.OPTIONS.get(name, {}) if styled else {}))
    return scene, ids, size, [str(w.message) for w in caught]


def lazy_view(value):
    """A scene as nested lists without asking the device for anything: a MARKERS node stays its path, markers and stroke width, a
    dashed stroke its path and pattern.  For the pairs whose dump needs marker vertices or dashes from the device."""
    from svgrasterize_amd import Marker, Path, Scene, Transform
    from svgrasterize_amd.geometry import DashedPath
    from svgrasterize_amd.markers import MarkerInstances

    if isinstance(value, Scene):
        return [value[0], lazy_view(value[1])]
    if isinstance(value, MarkerInstances):
        return ["markers", lazy_view(value.path), [lazy_view(m) for m in (value.start, value.mid, value.end)], value.stroke_width]
    if isinstance(value, Marker):
        return ["marker", lazy_view(value.scene), value.ref, value.size, value.viewbox, value.preserve_aspect_ratio, value.units_stroke_width,
                value.orient, value.clip]
    if isinstance(value, DashedPath):
        return ["dashed", list(value.dasharray), value.dashoffset, value.path_length, lazy_view(Path(value.subpaths))]
    if isinstance(value, Path):
        segs, kinds = value.packed()
        return [segs.tolist(), kinds.tolist()]
    if isinstance(value, np.ndarray):
        return value.tolist()
    if isinstance(value, Transform):
        return value.m.tolist()
    if isinstance(value, (tuple, list)):
        return [lazy_view(v) for v in value]
    return value


@pytest.mark.parametrize("name,styled,plain", css_cases.CASES, ids=[c[0] for c in css_cases.CASES])
def test_styled_document_loads_like_its_plain_twin(name, styled, plain):
    from svgrasterize_amd import scenedump

    got, _ids, got_size, warned = load(name, styled, True)
    want, _ids, want_size, _warned = load(name, plain, False)
    assert not [w for w in warned if "unsupported element type" in w]
    assert got is not None and want is not None and got_size == want_size == (64.0, 64.0)
    if name in css_cases.NEEDS_DEVICE:   # (the same pairs are dumped and compared in tests/test_gpu_css_documents.py)
        assert lazy_view(got) == lazy_view(want)
        return
    diffs = scenedump.compare_dumps(*scenedump.dump_scene(got), *scenedump.dump_scene(want), tol=0.0)
    assert diffs == []


def test_warnings_of_the_styled_documents():
    """What the cases are meant to warn about, and nothing else."""
    expected = {
        "media_screen_and_print": ["@media"],
        "two_style_elements": ["style of type 'text/x-scss' is not read"],
        "selector_list_with_an_invalid_selector": ["rule dropped, invalid selector '.t, rect:frobnicate'"],
    }
    for name, styled, _plain in css_cases.CASES:
        warned = load(name, styled, True)[3]
        want = expected.get(name, [])
        assert len(warned) == len(want) and all(w in got for w, got in zip(want, warned)), (name, warned)


def test_css_wide_keywords_warn_once_and_drop_the_declaration():
    doc = ('<svg xmlns="http://www.w3.org/2000/svg" width="64" height="64"><style>:root { --brand: #c00 } .a { fill: var(--brand); stroke: initial }'
           ' .b { fill: unset }</style><rect id="a" class="a" fill="#0a0" stroke="#222" width="8" height="8"/>'
           '<rect id="b" class="b" fill="#00c" style="stroke: UNSET" width="8" height="8"/></svg>')
    _scene, ids, _size, warned = load("css_wide", doc, False)
    assert warned == ["initial, unset and custom properties (var()) are not supported: the declaration is dropped"]
    assert ids["a"][1][0][1][1].tolist() == pytest.approx([0.0, 0.4019777798321958, 0.0, 1.0])   # (#0a0, linear: the attribute stands)
    assert len(ids["a"][1]) == 2 and ids["b"][0] == 0   # a keeps its stroke (GROUP of fill and stroke); b has none (one FILL)


def test_symbol_record_and_instance():
    import svgrasterize_amd as S

    doc = ('<svg xmlns="http://www.w3.org/2000/svg" width="64" height="64"><symbol id="sym" viewBox="0 0 8 16" x="1" y="2" width="4" height="8"'
           ' preserveAspectRatio="xMaxYMid meet" overflow="auto"><rect width="8" height="16"/></symbol>'
           '<symbol id="bare"><rect width="8" height="16"/></symbol><symbol id="empty" viewBox="0 0 4 4"/><use href="#nowhere"/></svg>')
    scene, ids, _size, warned = load("symbol", doc, False)
    assert scene is None and warned == []   # (a symbol is never drawn where it stands)
    sym = ids["sym"]
    assert isinstance(sym, S.Symbol) and sym.viewbox == (0.0, 0.0, 8.0, 16.0) and (sym.x, sym.y, sym.width, sym.height) == (1.0, 2.0, 4.0, 8.0)
    assert sym.preserve_aspect_ratio == "xMaxYMid meet" and sym.clip is False
    assert sym.viewport() == (4.0, 8.0) and sym.viewport(20, None) == (20.0, 8.0)
    assert ids["bare"].viewport() == (None, None) and ids["empty"].instance() is None and sym.instance(0, 0, 0, 5) is None
    # viewBox 8 x 16 into 20 x 8 with xMaxYMid meet: scale min(20 / 8, 8 / 16) = 0.5, xMax: shifted by 20 - 4 = 16; with the
    # instance's (10, 20) and the symbol's own (1, 2): translate(27, 22) scale(0.5)
    kind, (content, transform) = sym.instance(10, 20, 20, None)
    assert kind == S.RENDER_TRANSFORM and content[0] == S.RENDER_FILL
    assert transform.m[:2].tolist() == [[0.5, 0.0, 27.0], [0.0, 0.5, 22.0]]
    bare = ids["bare"].instance(3, 4)   # no viewBox and no size: neither scaled nor clipped
    assert bare[0] == S.RENDER_TRANSFORM and bare[1][0][0] == S.RENDER_FILL and bare[1][1].m[:2].tolist() == [[1.0, 0.0, 3.0], [0.0, 1.0, 4.0]]
    clipped = ids["bare"].instance(0, 0, 4, 4)
    assert clipped[1][0][0] == S.RENDER_CLIP


def test_switch_conditions():
    import svgrasterize_amd as S

    def first(body, **options):
        doc = f'<svg xmlns="http://www.w3.org/2000/svg" width="64" height="64"><switch>{body}</switch></svg>'
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            scene, _ids, _size = S.svg_scene_from_str(doc, **options)
        return None if scene is None else round(float(scene[1][0][1][0].subpaths[0][1][1][1][0]))   # the rect's width

    rects = '<rect systemLanguage="fr" width="1" height="1"/><rect systemLanguage="en-GB" width="2" height="1"/><rect systemLanguage="EN" width="3" height="1"/>'
    assert first(rects) == 3                                      # "en": en-GB is no prefix of it, EN is it
    assert first(rects, languages=("en-gb",)) == 2
    assert first(rects, languages=("de", "fr-CA")) == 1
    assert first(rects, languages=()) is None
    assert first('<rect requiredExtensions="" width="1" height="1"/><rect requiredFeatures="http://www.w3.org/TR/SVG11/feature#Shape" width="2" height="1"/>') == 2
    assert first('<foreignObject width="1" height="1"/><rect width="2" height="1"/>') is None   # (it passes, and draws nothing)


def _digest(arrays):
    h = hashlib.sha256()
    for k in sorted(arrays):
        a = np.ascontiguousarray(arrays[k])
        h.update(k.encode())
        h.update(str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def _documents():
    out = [("demo_" + name, os.path.join(DEMO, f + "z"), width) for name, f, width in
           (("tiger", "icons/tiger.svg", 2048), ("material", "material-design.svg", 4096), ("icons", "icons.svg", None), ("prompt", "prompt.svg", 256))]
    return out + [("case_" + name, text, width) for name, text, width in svg_cases.CASES]


@pytest.fixture(scope="module")
def before():
    z = np.load(os.path.join(GOLD, "loader_dumps_before_css.npz"), allow_pickle=False)
    return json.loads(str(z["docs"]))


@pytest.mark.parametrize("name,source,width", _documents(), ids=[d[0] for d in _documents()])
def test_documents_without_the_new_constructs_load_as_before(before, name, source, width):
    """``css=None``, no <style>: the tree, every paint and transform in it and every outline, bit for bit what the loader built
    before (the trees are compared as data, the outlines by their digest)."""
    import svgrasterize_amd as S
    from svgrasterize_amd import scenedump

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if name.startswith("demo_"):
            fonts = S.FontsDB()
            fonts.register_file(os.path.join(DEMO, "fonts.svgz"))
            scene, _ids, size = S.svg_scene_from_filepath(source, width=width, fonts=fonts, css=None)
        else:
            scene, _ids, size = S.svg_scene_from_str(source, width=width, css=None)
    want = before[name]
    assert (scene is None) == want["none"]
    if scene is None:
        return
    tree, arrays = scenedump.dump_scene(scene)
    assert (None if size is None else [float(v) for v in size]) == want["size"]
    assert json.loads(json.dumps(tree)) == want["tree"]
    assert (len(arrays["lines"]), len(arrays["cubics"])) == (want["lines"], want["cubics"])
    assert _digest(arrays) == want["arrays"]


def test_the_old_path_builds_no_maps(monkeypatch):
    """Without a rule the loader maps no parents and resolves properties with ``_expand_style`` alone."""
    from svgrasterize_amd import svg

    seen = []
    real = svg._Loader.stylesheets

    def spy(self, root, css=None):
        real(self, root, css)
        seen.append(self.matcher)

    monkeypatch.setattr(svg._Loader, "stylesheets", spy)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        svg.svg_scene_from_str(svg_cases.CASES[0][1])
        svg.svg_scene_from_str(svg_cases.CASES[0][1], css="/* nothing */ @media print { a { fill: red } }")
        svg.svg_scene_from_str(svg_cases.CASES[0][1], css="rect { fill: red }")
    assert seen[0] is None and seen[1] is None and seen[2] is not None
