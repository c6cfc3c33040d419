"""TrueType fonts on the CPU: the parser (truetype.read_ttf) against the points handed to the font builder of
tests/ttf_cases.py, the flattening of composite glyphs, the per-lane header csrc/svgr_glyf.h -- compiled for the host,
tests/glyf_harness.cpp -- bit for bit against tests/ttf_ref.py, the loader (which needs no device), the refusals and malformed
input.  Nothing here touches a GPU."""
import ctypes as C
import glob
import os
import struct
import warnings

import numpy as np
import pytest

import svgrasterize_amd as S
from svgrasterize_amd import _abi, svg, truetype

from tests import ttf_cases as K
from tests import ttf_ref as R
from tests.util import host_build

_P = C.c_void_p
E_INVALID, E_OVERFLOW = -1, -5


@pytest.fixture(scope="module")
def gh():
    lib = host_build("glyf_harness")
    lib.gh_validate.restype = lib.gh_outline.restype = C.c_int
    return lib


def _args(a):
    p = lambda x: x.ctypes.data_as(_P)   # noqa: E731
    return [p(a["pt_on"]), C.c_int64(len(a["pt_on"])), p(a["contour_off"]), C.c_int64(len(a["contour_off"]) - 1), p(a["glyph_contour_off"]),
            C.c_int64(len(a["glyph_contour_off"]) - 1), p(a["part_glyph"]), p(a["part_m"]), p(a["part_pen"]), p(a["part_sx"]), p(a["part_sy"]),
            C.c_int64(len(a["part_glyph"]))]


def harness_validate(gh, a):
    counts = np.zeros(3, dtype=np.int64)
    return gh.gh_validate(*_args(a), counts.ctypes.data_as(_P)), counts


def harness_outline(gh, a):
    rc, counts = harness_validate(gh, a)
    assert rc == 0, rc
    types = np.zeros(counts[1], dtype=np.int32)
    params = np.full((counts[1], 8), np.nan)
    sizes = np.zeros(counts[2], dtype=np.int32)
    rc = gh.gh_outline(a["pt_xy"].ctypes.data_as(_P), *_args(a), types.ctypes.data_as(_P), params.ctypes.data_as(_P), sizes.ctypes.data_as(_P))
    assert rc == 0, rc
    return types, params, sizes


def _same(got, want, what):
    for g, w, name in zip(got, want, ("types", "params", "sizes")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, name)


# ---- the parser -------------------------------------------------------------------------------------------------------
VARIANTS = {
    "default": {},
    "loca_long": dict(loca_long=True),
    "cmap12": dict(cmap_format=12, cmap_platform=(3, 10)),
    "cmap4_glyph_array": dict(cmap_by_array=True),
    "cmap_platform0": dict(cmap_platform=(0, 3)),
    "no_flag_repeat": dict(flag_repeat=False),
    "long_vectors": dict(short_vectors=False),
    "no_same_as_previous": dict(same_as_previous=False),
    "plain": dict(flag_repeat=False, short_vectors=False, same_as_previous=False, loca_long=True),
    "name_mac": dict(name_platform=1, family="Synth\xe9tique"),
    "no_os2_bold_italic": dict(with_os2=False, mac_style=3),
    "no_os2_regular": dict(with_os2=False),
    "os2_light_italic": dict(weight=300, italic=True),
    "mac_style_italic": dict(mac_style=2),
    "short_hmtx": dict(n_hmetrics=11),
    "true_tag": dict(sfnt=b"true"),
}


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_parser_gives_back_what_the_builder_was_given(name):
    opts = VARIANTS[name]
    font = S.read_ttf(K.synthetic_ttf(**opts))
    assert isinstance(font, S.TrueTypeFont) and isinstance(font, S.Font)
    for gid, glyph in enumerate(K.GLYPHS):
        got = font.simple_glyph(gid)
        pts = [p for c in glyph for p in c] if not isinstance(glyph, dict) else []
        assert got.xy.dtype == np.int16 and got.on.dtype == np.uint8
        assert got.xy.tolist() == [[p[0], p[1]] for p in pts], gid
        assert got.on.tolist() == [int(p[2]) for p in pts], gid
        assert got.ends.tolist() == (np.cumsum([len(c) for c in glyph]) - 1).tolist() if pts else len(got.ends) == 0, gid
        assert font.advance(gid) == K.ADVANCES[gid]
    assert font.cmap() == K.CMAP
    assert all(font.glyph_id(code) == gid for code, gid in K.CMAP.items())
    assert font.glyph_id(ord("#")) == 0 and font.glyph_id(0x1F600) == 0 and font.glyph_id(-1) == 0
    assert font.hkern == {pair: -float(v) for pair, v in K.KERN.items()}
    assert (font.units_per_em, font.ascent, font.descent) == (1000.0, 800.0, -200.0)
    assert font.family == opts.get("family", "Synthetic")
    if opts.get("with_os2", True):
        want = (opts.get("weight", 400), "italic" if opts.get("italic") or opts.get("mac_style", 0) & 2 else "normal")
    else:
        want = (700 if opts.get("mac_style", 0) & 1 else 400, "italic" if opts.get("mac_style", 0) & 2 else "normal")
    assert (font.weight, font.style) == want


def test_the_builder_variants_do_differ():
    """Each encoding the decoder has to handle is in the default font's bytes: leaving one out makes the glyf table longer;
    and the points have short x and y vectors of both signs."""
    def glyf_bytes(repeat=True, short=True, same=True):   # (before the records are padded)
        return sum(len(K._simple_glyph(g, repeat, short, same)) for g in K.GLYPHS if not isinstance(g, dict))

    base = glyf_bytes()
    assert glyf_bytes(repeat=False) > base and glyf_bytes(short=False) > base and glyf_bytes(same=False) > base
    for axis in (0, 1):
        deltas = [b[axis] - a[axis] for g in K.GLYPHS if not isinstance(g, dict) for c in g for a, b in zip(c, c[1:])]
        assert any(-256 < d < 0 for d in deltas) and any(0 < d < 256 for d in deltas) and any(d == 0 for d in deltas) and any(abs(d) > 255 for d in deltas)


def test_cmap_preference_and_supplementary_plane():
    other = {ord("A"): 4}
    # platform 0 first in the file, then 3 / 1, then 3 / 10: the last one wins, whatever the order
    data = K.build_ttf(K.GLYPHS, {**K.CMAP, 0x1F600: 3}, K.ADVANCES, cmap_format=12, cmap_platform=(3, 10),
                       extra_cmap=[(0, 3, 4, other), (3, 1, 4, other)])
    font = S.read_ttf(data)
    assert font.glyph_id(ord("A")) == 2 and font.glyph_id(0x1F600) == 3 and font.cmap()[0x1F600] == 3
    # 3 / 1 before platform 0; a subtable of another format (here: 3 / 10 in a format the parser is not offered) is passed over
    font = S.read_ttf(K.build_ttf(K.GLYPHS, K.CMAP, K.ADVANCES, cmap_platform=(3, 1), extra_cmap=[(0, 3, 4, other)]))
    assert font.glyph_id(ord("A")) == 2
    font = S.read_ttf(K.build_ttf(K.GLYPHS, other, K.ADVANCES, cmap_platform=(0, 4), cmap_format=12, extra_cmap=[(1, 0, 4, K.CMAP)]))
    assert font.glyph_id(ord("A")) == 4 and font.glyph_id(ord("o")) == 0
    # a glyph id beyond the font's glyphs is .notdef
    font = S.read_ttf(K.build_ttf(K.GLYPHS, {ord("A"): 99}, K.ADVANCES))
    assert font.glyph_id(ord("A")) == 0 and font.cmap() == {}


def test_kern_subtables_that_are_not_read():
    for coverage in (0x0000, 0x0005, 0x0201):   # vertical, cross-stream, format 2
        assert S.read_ttf(K.synthetic_ttf(kern_coverage=coverage)).hkern == {}
    assert S.read_ttf(K.build_ttf(K.GLYPHS, K.CMAP, K.ADVANCES)).hkern == {}


def test_str_to_glyphs_is_host_arithmetic():
    font = S.read_ttf(K.synthetic_ttf())
    placed, advance = font.str_to_glyphs("AVA o#\xf3")
    assert [g.gid for _pen, g in placed] == [2, 4, 2, 1, 3, 0, 6]
    assert [pen for pen, _g in placed] == [0.0, 620.0, 1150.0, 1850.0, 2150.0, 2750.0, 3250.0] and advance == 3850.0
    assert placed[0][1] is placed[2][1] and placed[5][1] is font.missing_glyph
    _atlas, _parts, total = R.string_parts(K.GLYPHS, K.CMAP, K.ADVANCES, K.KERN, "AVA o#\xf3")
    assert total == advance
    assert font.str_to_glyphs("") == ([], 0.0)


# ---- composite glyphs ------------------------------------------------------------------------------------------------
def test_composites_flatten_to_the_reference_matrices():
    font = S.read_ttf(K.synthetic_ttf())
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for gid in range(len(K.GLYPHS)):
            got, want = font.glyph_parts(gid), R.flatten(K.GLYPHS, gid)
            assert [p[0] for p in got] == [p[0] for p in want], gid
            assert np.array([p[1:] for p in got], dtype=np.float64).tobytes() == np.array([p[1:] for p in want], dtype=np.float64).tobytes(), gid
        font.glyph_parts(9)
    assert len(caught) == 1 and "point matching" in str(caught[0].message)   # (once per font)
    assert [p[0] for p in font.glyph_parts(7)] == [3, 5, 2] and font.glyph_parts(1) == [] and len(font.glyph_parts(2)) == 1
    nested = font.glyph_parts(7)
    assert nested[0][1:] == (0.5, 0.0, 0.0, 0.5, 100.0, -20.0)
    assert nested[1][1:] == (0.5, 0.0, 0.0, 0.5, 220 * 0.5 + 100, 560 * 0.5 - 20)        # the accent: offset scaled by the outer component
    assert nested[2][1:] == (K.COS, K.SIN, -K.SIN, K.COS, -300.0, 40.0)
    assert font.glyph_parts(8) == [(4, 0.75, 0.0, 0.0, -0.5, 10.0, -100.0)]
    assert font.glyph_parts(9)[1] == (5, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0)


def test_cycles_and_deep_nesting_leave_the_glyph_empty():
    square = [[(0, 0, True), (10, 0, True), (10, 10, True)]]
    cyclic = [square, dict(components=[dict(glyph=2)]), dict(components=[dict(glyph=0), dict(glyph=1)])]
    font = S.read_ttf(K.build_ttf(cyclic, {65: 1}, [10, 10, 10]))
    with pytest.warns(UserWarning, match="contains itself"):
        assert font.glyph_parts(1) == []
    deep = [square] + [dict(components=[dict(glyph=k)]) for k in range(12)]
    font = S.read_ttf(K.build_ttf(deep, {65: 1}, [10] * 13))
    assert font.glyph_parts(8) == [(0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0)]    # nesting of 8
    with pytest.warns(UserWarning, match="nested deeper"):
        assert font.glyph_parts(12) == []
    wide = [square, dict(components=[dict(glyph=0)] * 70), dict(components=[dict(glyph=1)] * 70)]
    font = S.read_ttf(K.build_ttf(wide, {65: 1}, [10] * 3))
    assert len(font.glyph_parts(1)) == 70
    with pytest.warns(UserWarning, match="parts"):
        assert font.glyph_parts(2) == []
    # a hostile nest -- 300 components per composite, eight deep -- ends at the bound, each record parsed once
    nest = [square] + [dict(components=[dict(glyph=k)] * 300) for k in range(8)]
    font = S.read_ttf(K.build_ttf(nest, {65: 8}, [10] * 9, loca_long=True))
    with pytest.warns(UserWarning, match="parts"):
        assert font.glyph_parts(8) == []
    assert sorted(font._composite) == list(range(9)) and font._composite[0] is None and len(font._composite[8]) == 300


# ---- the per-lane header -----------------------------------------------------------------------------------------------
CASES = K.outline_cases()


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_harness_equals_reference_bit_for_bit(gh, name):
    _name, atlas, parts = next(c for c in CASES if c[0] == name)
    _same(harness_outline(gh, K.pack(atlas, parts)), R.outline(atlas, parts), name)


def test_harness_fuzz_equals_reference_bit_for_bit(gh):
    for seed in range(200):
        atlas, parts = K.fuzz_case(seed)
        _same(harness_outline(gh, K.pack(atlas, parts)), R.outline(atlas, parts), seed)


def test_outline_rule_by_hand():
    """The reference itself, on a contour small enough to work out on paper: on, off, off, on."""
    types, params = R.contour([(0, 0, True), (10, 0, False), (10, 10, False), (0, 10, True)])
    assert types.tolist() == [R.PATH_CUBIC, R.PATH_CUBIC, R.PATH_LINE, R.PATH_CLOSED]
    assert params[0, [0, 1, 6, 7]].tolist() == [0, 0, 10, 5] and params[1, [0, 1, 6, 7]].tolist() == [10, 5, 0, 10]
    assert params[0, 2:6].tolist() == [(1 / 3) * 0 + (2 / 3) * 10, 0.0, (2 / 3) * 10 + (1 / 3) * 10, (2 / 3) * 0 + (1 / 3) * 5]
    assert params[2].tolist() == [0, 10, 0, 0, 0, 0, 0, 0] and params[3].tolist() == [0, 0, 0, 0, 0, 0, 0, 0]
    # the chain is closed: every segment begins where the one before it ended
    for seed in range(20):
        atlas, parts = K.fuzz_case(seed)
        for g, m, pen, sx, sy in parts:
            for points in atlas[g]:
                got = R.contour(points, m, pen, sx, sy)
                if got is None:
                    assert len(points) < 2
                    continue
                t, p = got
                end = np.where((t == R.PATH_CUBIC)[:, None], p[:, 6:8], p[:, 2:4])
                assert np.array_equal(p[1:, 0:2], end[:-1]) and np.array_equal(end[-1], p[0, 0:2]) and t[-1] == R.PATH_CLOSED


def test_harness_validation(gh):
    atlas, parts = CASES[0][1], CASES[0][2]
    good = K.pack(atlas, parts)
    assert harness_validate(gh, good)[0] == 0

    def changed(key, index, value):
        a = {k: v.copy() for k, v in good.items()}
        a[key].reshape(-1)[index] = value
        return a

    assert harness_validate(gh, changed("contour_off", 1, 9999))[0] == E_INVALID        # decreases afterwards
    assert harness_validate(gh, changed("contour_off", -1, int(good["contour_off"][-1]) + 1))[0] == E_INVALID   # ends beyond the points
    assert harness_validate(gh, changed("contour_off", 0, 1))[0] == E_INVALID
    assert harness_validate(gh, changed("glyph_contour_off", -1, 1))[0] == E_INVALID
    assert harness_validate(gh, changed("glyph_contour_off", 1, 99))[0] == E_INVALID
    assert harness_validate(gh, changed("part_glyph", 1, 2))[0] == E_INVALID
    assert harness_validate(gh, changed("part_glyph", 0, -1))[0] == E_INVALID
    for key in ("part_pen", "part_sx", "part_sy", "part_m"):
        for value in (np.nan, np.inf, -np.inf, 2e150):
            assert harness_validate(gh, changed(key, -1, value))[0] == E_INVALID, (key, value)
        assert harness_validate(gh, changed(key, -1, -1e150))[0] == 0
    # no parts, and parts of empty glyphs only: valid, and nothing to do
    rc, counts = harness_validate(gh, K.pack(atlas, []))
    assert rc == 0 and counts.tolist() == [0, 0, 0]
    rc, counts = harness_validate(gh, K.pack([[], [[(1, 1, True)]]], [(0, K.IDENTITY, 0.0, 1.0, 1.0)] * 3))
    assert rc == 0 and counts.tolist() == [0, 0, 0]
    rc, counts = harness_validate(gh, K.pack([[], [[(1, 1, True)]]], [(1, K.IDENTITY, 0.0, 1.0, 1.0)] * 3))
    assert rc == 0 and counts.tolist() == [3, 0, 0]


# ---- the loader --------------------------------------------------------------------------------------------------------
def _find(scene, kind, out):
    if scene[0] == kind:
        out.append(scene)
    if scene[0] == S.RENDER_GROUP:
        for child in scene[1]:
            _find(child, kind, out)
    elif scene[0] in (S.RENDER_TRANSFORM, S.RENDER_OPACITY, S.RENDER_CLIP, S.RENDER_MASK, S.RENDER_FILTER, S.RENDER_BLEND):
        _find(scene[1][0], kind, out)
    return out


def _document(family, defs=""):
    return (f'<svg xmlns="http://www.w3.org/2000/svg" width="128" height="128" viewBox="0 0 128 128"><defs>{defs}</defs>'
            f'<text x="6" y="40" font-family="{family}" font-size="20" fill="#204080">AV<tspan dy="30" fill="#c02000">o A</tspan>V</text></svg>')


@pytest.fixture()
def no_device(monkeypatch):
    def refuse(*_a, **_k):
        raise AssertionError("a device context was asked for")

    monkeypatch.setattr(_abi.Context, "get", classmethod(refuse))
    monkeypatch.setattr(_abi.Context, "__init__", refuse)


def test_loader_needs_no_device(no_device):
    db = S.FontsDB()
    font = db.register_ttf(K.synthetic_ttf())
    assert db.resolve("Synthetic") is font and db.resolve("synthetic", 700) is font
    scene, _ids, _size = S.svg_scene_from_str(_document("Synthetic"), fonts=db)
    moved = [n for n in _find(scene, S.RENDER_TRANSFORM, []) if n[1][0][0] == S.RENDER_MARKERS]
    assert len(moved) == 3 and not _find(scene, S.RENDER_FILL, [])
    payloads = [n[1][0][1] for n in moved]
    assert all(isinstance(p, S.TextOutline) and p.font is font and p.size == 20.0 for p in payloads)
    assert [p.text for p in payloads] == ["AV", "o A", "V"]
    text = repr(scene)
    assert "TEXT 'AV' font:Synthetic size:20" in text and "TEXT 'o A' font:Synthetic size:20" in text
    assert all(p.scene is None and not p._expanded for p in payloads)     # printing did not expand them
    # the pen of every run: where the run before it ended, by the host's advances (AV kerns by -80, the V after A by -80 again)
    scale = 20.0 / 1000.0
    pens = [(float(n[1][1].m[0, 2]), float(n[1][1].m[1, 2])) for n in moved]
    first = font.str_to_glyphs("AV")[1] * scale
    second = font.str_to_glyphs("o A")[1] * scale
    assert first == (700 - 80 + 600) * scale and second == (600 + 300 + 700) * scale
    assert pens == [(6.0, 40.0), (6.0 + first, 70.0), (6.0 + first + second, 70.0)]
    assert payloads[1].attrs["fill"] == "#c02000" and payloads[0].attrs["fill"] == "#204080"


SVG_FONT = """<font id="f" horiz-adv-x="600"><font-face font-family="Plain" units-per-em="1000" ascent="800" descent="-200"/>
<missing-glyph horiz-adv-x="500" d="M50,0 H450 V700 H50 Z"/>
<glyph unicode="A" horiz-adv-x="700" d="M50,0 L350,700 L650,0 Z"/>
<glyph unicode="V" horiz-adv-x="600" d="M0,700 L600,700 L300,0 Z"/>
<glyph unicode="o" horiz-adv-x="600" d="M50,250 Q50,500 300,500 Q550,500 550,250 Q550,0 300,0 Q50,0 50,250 Z"/>
<glyph unicode=" " horiz-adv-x="300" d=""/>
<hkern u1="A" u2="V" k="80"/>
</font>"""


def test_svg_font_runs_take_the_unchanged_path(no_device):
    """The same document set in an SVG font: exactly the nodes the lines of before make -- `Font.str_to_path` at load time,
    one FILL per run under the pen's translation -- and no lazy node."""
    db = S.FontsDB()
    db.register_ttf(K.synthetic_ttf())    # (registered, and not asked for)
    scene, _ids, _size = S.svg_scene_from_str(_document("Plain", SVG_FONT), fonts=db)
    font = db.resolve("Plain")
    assert type(font) is S.Font and not _find(scene, S.RENDER_MARKERS, [])
    got = [n for n in _find(scene, S.RENDER_TRANSFORM, []) if n[1][0][0] == S.RENDER_FILL]
    want, pen = [], (6.0, 40.0)
    for words, colour, dy in (("AV", "#204080", 0.0), ("o A", "#c02000", 30.0), ("V", "#204080", 0.0)):
        path, advance = S.Font.str_to_path(font, 20.0, words)
        pen = (pen[0], pen[1] + dy)
        paint = svg.parse_paint(colour, {})
        want.append(S.Scene.fill(path, paint, S.PATH_FILL_NONZERO).transform(S.Transform().translate(*pen)))
        pen = (pen[0] + advance, pen[1])
    assert [repr(n) for n in got] == [repr(n) for n in want]
    for g, w in zip(got, want):
        assert np.array_equal(g[1][1].m, w[1][1].m) and np.array_equal(g[1][0][1][1], w[1][0][1][1])
        assert g[1][0][1][0].subpaths.__len__() == w[1][0][1][0].subpaths.__len__()


def test_scene_text_is_lazy_and_prints_as_built(no_device):
    font = S.read_ttf(K.synthetic_ttf())
    node = S.Scene.text(font, 12, "Ao", {"fill": np.array([1.0, 0.0, 0.0, 1.0])})
    assert node[0] == S.RENDER_MARKERS and isinstance(node[1], S.TextOutline)
    assert repr(node) == "TEXT 'Ao' font:Synthetic size:12" and node[1].scene is None
    assert repr(S.Scene.group([node, node.transform(S.Transform().translate(1, 2))])).count("TEXT 'Ao'") == 2


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_name_the_cause(tmp_path):
    good = K.synthetic_ttf()
    for tag, word in ((b"OTTO", "CFF"), (b"ttcf", "collection"), (b"wOFF", "WOFF"), (b"wOF2", "WOFF2")):
        with pytest.raises(ValueError, match=word):
            S.read_ttf(tag + good[4:])
    with pytest.raises(ValueError, match="glyf"):
        S.read_ttf(K.synthetic_ttf(drop=("glyf",)))
    with pytest.raises(ValueError, match="hmtx / loca"):
        S.read_ttf(K.synthetic_ttf(drop=("loca", "hmtx")))
    with pytest.raises(ValueError, match="not a TrueType font"):
        S.read_ttf(b"<svg xmlns='http://www.w3.org/2000/svg'/>")
    with pytest.raises(ValueError, match="family"):
        S.read_ttf(K.synthetic_ttf(name_platform=None))
    assert S.read_ttf(K.synthetic_ttf(name_platform=None), family="Given").family == "Given"
    assert S.read_ttf(good, family="Alias").family == "Alias"
    db = S.FontsDB()
    for tag in (b"OTTO", b"ttcf", b"wOFF", b"wOF2"):
        path = tmp_path / f"{tag.decode()}.font"
        path.write_bytes(tag + good[4:])
        with pytest.warns(UserWarning, match=tag.decode()):
            db.register_file(str(path))
    for name, data in (("cut.ttf", good[:len(good) // 2]), ("noglyf.ttf", K.synthetic_ttf(drop=("glyf",)))):
        (tmp_path / name).write_bytes(data)
        with pytest.warns(UserWarning, match="font file skipped"):    # a malformed TrueType file: skipped too, nothing raised
            db.register_file(str(tmp_path / name))
    assert not db.fonts and not db.fonts_files
    # a TrueType file is read at once and registered under its family -- or, without one, under its file's name; anything
    # else waits as an SVG document, as before
    (tmp_path / "a.ttf").write_bytes(good)
    (tmp_path / "Nameless.ttf").write_bytes(K.synthetic_ttf(name_platform=None))
    (tmp_path / "fonts.svg").write_text(f'<svg xmlns="http://www.w3.org/2000/svg"><defs>{SVG_FONT}</defs></svg>')
    for name in ("a.ttf", "Nameless.ttf", "fonts.svg"):
        db.register_file(str(tmp_path / name))
    assert sorted(db.fonts) == ["nameless", "synthetic"] and db.fonts_files == [str(tmp_path / "fonts.svg")]
    assert type(db.resolve("Plain")) is S.Font and isinstance(db.resolve("Nameless"), S.TrueTypeFont)
    alias = db.register_ttf(str(tmp_path / "a.ttf"), family="Label Sans")
    assert db.resolve("label sans") is alias and alias.family == "Synthetic"
    with pytest.raises(ValueError, match="family"):
        db.register_ttf(K.synthetic_ttf(name_platform=None))
    assert db.register_ttf(K.synthetic_ttf(name_platform=None), family="Mine").family == "Mine"


# ---- malformed input -----------------------------------------------------------------------------------------------------
def _exercise(data, gh):
    """Parse, use every glyph and every table, and hand what parsed to the harness's validation; ValueError is the only way out."""
    try:
        font = truetype.read_ttf(data, family="F")
        font.cmap()
        font.str_to_glyphs("AVo \xf3QxPIJK#")
        parts = []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for gid in range(font.n_glyphs):
                parts.extend((part, 0.0) for part in font.glyph_parts(gid))
        index, atlas = {}, []
        for part, _pen in parts:
            if part[0] not in index:
                index[part[0]] = len(atlas)
                atlas.append(font.simple_glyph(part[0]))
    except ValueError:
        return "refused"
    contour_off, glyph_contour_off, n = [0], [0], 0
    for g in atlas:
        contour_off.extend((g.ends.astype(np.int64) + 1 + n).tolist())
        n += len(g.on)
        glyph_contour_off.append(len(contour_off) - 1)
    a = dict(pt_xy=np.concatenate([g.xy for g in atlas] + [np.zeros((0, 2), np.int16)]), pt_on=np.concatenate([g.on for g in atlas] + [np.zeros(0, np.uint8)]),
             contour_off=np.array(contour_off, dtype=np.int32), glyph_contour_off=np.array(glyph_contour_off, dtype=np.int32),
             part_glyph=np.array([index[p[0]] for p, _pen in parts], dtype=np.int32),
             part_m=np.array([p[1:] for p, _pen in parts], dtype=np.float64).reshape(-1, 6), part_pen=np.zeros(len(parts)),
             part_sx=np.ones(len(parts)), part_sy=np.ones(len(parts)))
    rc, counts = harness_validate(gh, a)
    assert rc in (0, E_INVALID), rc
    if rc == 0:    # (in range by the harness's own checks: running the lanes reads nothing out of range)
        types, _params, sizes = harness_outline(gh, a)
        assert len(types) == counts[1] == sizes.sum()
    return "parsed"


def test_malformed_fonts_raise_value_error_only(gh):
    good = K.synthetic_ttf()
    assert _exercise(good, gh) == "parsed"
    rng = np.random.default_rng(950)
    cuts = sorted(set(K.table_bounds(good)) | {int(v) for v in rng.integers(0, len(good), 64)} | {0, 3, 4, 11, 12})
    outcomes = {"parsed": 0, "refused": 0}
    for cut in cuts:
        outcomes[_exercise(good[:cut], gh)] += 1
    assert outcomes["refused"] >= len(K.table_bounds(good)) - 1
    for at, value in zip(rng.integers(0, len(good), 256).tolist(), rng.integers(0, 256, 256).tolist()):
        bad = bytearray(good)
        bad[at] = value if value != good[at] else value ^ 0xFF
        outcomes[_exercise(bytes(bad), gh)] += 1
    assert outcomes["parsed"] > 0 and outcomes["refused"] > 0, outcomes


def test_fields_that_claim_more_than_the_file_holds():
    good = bytearray(K.synthetic_ttf(cmap_format=12, cmap_platform=(3, 10)))
    tables = S.read_ttf(bytes(good)).tables

    def poke(tag, off, fmt, value):
        bad = bytearray(good)
        struct.pack_into(fmt, bad, tables[tag][0] + off, value)
        return bytes(bad)

    for data in (poke("maxp", 4, ">H", 0xFFFF), poke("hhea", 34, ">H", 0xFFFF), poke("cmap", 2, ">H", 0xFFFF), poke("head", 50, ">h", 7),
                 poke("head", 18, ">H", 0), poke("kern", 10, ">H", 0xFFFF), poke("name", 2, ">H", 0xFFFF), poke("loca", 2, ">H", 0xFFFF),
                 bytes(good[:4]) + struct.pack(">H", 0xFFFF) + bytes(good[6:])):
        with pytest.raises(ValueError):
            font = S.read_ttf(data)
            for gid in range(font.n_glyphs):
                font.glyph_parts(gid)
    sub = tables["cmap"][0] + struct.unpack_from(">I", good, tables["cmap"][0] + 8)[0]
    bad = bytearray(good)
    struct.pack_into(">I", bad, sub + 12, 0x0FFFFFFF)   # nGroups
    with pytest.raises(ValueError):
        S.read_ttf(bytes(bad))
    bad = bytearray(good)
    struct.pack_into(">II", bad, sub + 16, 0, 0xFFFFFFFF)   # one group that claims every code there is, and more
    with pytest.raises(ValueError):
        S.read_ttf(bytes(bad))


# ---- a real font, where the machine has one -----------------------------------------------------------------------------
def _dejavu():
    found = glob.glob("/usr/share/fonts/**/DejaVuSans.ttf", recursive=True)
    try:
        import matplotlib

        found += glob.glob(os.path.join(matplotlib.get_data_path(), "fonts", "ttf", "DejaVuSans.ttf"))
    except ImportError:
        pass
    return found[0] if found else None


def test_real_font_equals_fonttools():
    ttlib = pytest.importorskip("fontTools.ttLib")
    path = _dejavu()
    if path is None:
        pytest.skip("no DejaVuSans.ttf on this machine")
    with open(path, "rb") as f:
        font = S.read_ttf(f.read())
    ref = ttlib.TTFont(path)
    glyf, order, hmtx = ref["glyf"], ref.getGlyphOrder(), ref["hmtx"]
    assert font.n_glyphs == len(order) and font.family == "DejaVu Sans" and font.units_per_em == ref["head"].unitsPerEm
    for gid, name in enumerate(order):
        g = glyf[name]
        assert font.advance(gid) == hmtx[name][0], name
        got = font.simple_glyph(gid)
        if g.numberOfContours > 0:
            assert got.xy.tolist() == [list(p) for p in g.coordinates], name
            assert got.on.tolist() == [f & 1 for f in g.flags], name
            assert got.ends.tolist() == list(g.endPtsOfContours), name
        else:
            assert len(got.on) == 0, name
    want = {code: ref.getGlyphID(name) for code, name in ref.getBestCmap().items()}
    assert font.cmap() == {code: gid for code, gid in want.items() if gid}
