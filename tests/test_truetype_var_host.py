"""Variable fonts on the CPU (no device is touched): the parser of ``fvar`` / ``avar`` / ``gvar`` against what the writers of
tests/gvar_cases.py were handed, malformed input, the per-lane header csrc/svgr_gvar.h compiled for the host
(tests/gvar_harness.cpp) against the reference tests/gvar_ref.py bit for bit, the reference and the parser against a record
made with fontTools (tests/tools/gen_gvar_golden.py), the host arithmetic of an instance (advances, composite offsets), the
loader and `FontsDB.resolve`.  tests/test_gpu_truetype_var.py checks the same delta cases on the GPU."""
import ctypes as C
import json
import os
import struct
import warnings

import numpy as np
import pytest

import svgrasterize_amd as S
from svgrasterize_amd import truetype_var as TV
from tests import gvar_cases as G
from tests import gvar_ref as V
from tests import ttf_cases as K
from tests import ttf_ref as R
from tests.util import GOLDEN, host_build

_P = C.c_void_p
E_INVALID, E_OVERFLOW = -1, -5
VAR = G.variations()
ENCODINGS = {
    "default": {},
    "long_offsets": dict(long_offsets=True),
    "embedded_peaks": dict(shared_peaks=False),
    "private_points": dict(shared_points=False),
    "point_words": dict(point_words=True),
    "delta_words": dict(delta_mode="words"),
    "delta_bytes_no_zero_runs": dict(delta_mode="no_zero"),
    "everything_else": dict(long_offsets=True, shared_peaks=False, shared_points=False, point_words=True, delta_mode="words"),
}
LOCATIONS = [{"wght": 650, "wdth": 80}, {"wght": 900}, {"wght": 100, "wdth": 125}, {"wght": 2000, "wdth": 0}, {"wght": 525}, {"wdth": 111}]


def quiet(call, *args, **kwargs):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # (glyph 9 of the synthetic font is placed by point matching)
        return call(*args, **kwargs)


@pytest.fixture(scope="module")
def font():
    return S.read_ttf(G.synthetic_var_ttf())


# ---- the parser ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ENCODINGS))
def test_every_encoding_round_trips(name):
    font = S.read_ttf(G.synthetic_var_ttf(gvar_options=ENCODINGS[name]))
    assert font.is_variable and font.axes == tuple(S.Axis(*a) for a in G.AXES)
    for gid, (glyph, tuples) in enumerate(zip(K.GLYPHS, VAR)):
        got = quiet(TV.glyph_tuples, font, gid)
        assert len(got) == len(tuples), gid
        n = G.point_count(glyph)
        for g, t in zip(got, tuples):
            assert g.peak == tuple(V.f2dot14(v) for v in t["peak"])
            if t.get("start") is None:
                assert g.start is None and g.end is None
            else:
                assert g.start == tuple(V.f2dot14(v) for v in t["start"]) and g.end == tuple(V.f2dot14(v) for v in t["end"])
            points = list(range(n + 4)) if t.get("points") is None else t["points"]
            assert g.index.tolist() == points and g.index.dtype == np.int32
            assert g.dxy.tolist() == [list(d) for d in t["deltas"]] and g.dxy.dtype == np.int16


def test_points_beyond_the_glyph_are_dropped_and_a_repeat_keeps_the_later_delta():
    var = [[] for _ in K.GLYPHS]
    var[5] = [dict(peak=(1.0, 0.0), points=[2, 2, 9, 10, 11], deltas=[(1, 1), (7, -7), (3, 0), (4, 4), (5, 5)])]   # 6 points: 10 and 11 are none
    font = S.read_ttf(G.synthetic_var_ttf(var))
    t, = TV.glyph_tuples(font, 5)
    assert t.index.tolist() == [2, 9] and t.dxy.tolist() == [[7, -7], [3, 0]]


def test_a_static_font_has_no_axes_and_is_its_own_instance():
    static = S.read_ttf(K.synthetic_ttf())
    assert static.axes == () and not static.is_variable
    assert static.instance() is static and static.instance({}) is static
    with pytest.raises(ValueError, match="truetype: "):
        static.instance(wght=700)


def test_fvar_without_gvar_has_axes_and_default_outlines(font):
    bare = S.read_ttf(G.synthetic_var_ttf(with_gvar=False))
    assert bare.axes == font.axes
    bold = bare.instance(wght=700)
    assert bold is not bare and bold.weight == 700 and bold.advance(2) == 700.0
    assert quiet(bold.glyph_parts, 7) == quiet(bare.glyph_parts, 7)
    assert TV.tuple_arrays(bare, [2, 3], bold.normalised)["tuple_scalar"].shape == (0,)


def test_avar_version_2_warns_once_and_is_not_applied():
    with pytest.warns(UserWarning, match="avar version 2") as caught:
        font = S.read_ttf(G.synthetic_var_ttf(avar_version=2))
    assert len(caught) == 1
    assert font.instance(wght=650).normalised == (0.5, 0.0)          # (the map would make it 0.25)
    assert S.read_ttf(G.synthetic_var_ttf()).instance(wght=650).normalised == (0.25, 0.0)
    assert S.read_ttf(G.synthetic_var_ttf(with_avar=False)).instance(wght=650).normalised == (0.5, 0.0)


def _exercise(data):
    """Read `data` and use every glyph at two locations: "parsed", or "refused" (a ValueError that says truetype)."""
    try:
        font = S.read_ttf(data, family="X")
        for user in ({"wght": 900, "wdth": 75}, {"wght": 250}) if font.is_variable else ():
            inst = font.instance({tag: v for tag, v in user.items() if tag in [a.tag for a in font.axes]})
            for gid in range(font.n_glyphs):
                inst.advance(gid)
                inst.glyph_parts(gid)
                if inst is not font:
                    TV.tuple_arrays(font, [gid], inst.normalised)
    except ValueError as why:
        assert "truetype" in str(why) or "cmap" in str(why), why
        return "refused"
    return "parsed"


def test_truncated_and_damaged_files_raise_value_error():
    good = G.synthetic_var_ttf()
    rng = np.random.default_rng(7)
    outcomes = {"parsed": 0, "refused": 0}
    tables = S.read_ttf(good).tables
    cuts = set(K.table_bounds(good))
    for tag in ("fvar", "avar", "gvar"):   # inside the three tables too, every fourth byte
        cuts.update(range(tables[tag][0], tables[tag][0] + tables[tag][1], 4))
    for cut in sorted(cuts):
        outcomes[quiet(_exercise, good[:cut])] += 1
    assert outcomes["refused"] >= len(K.table_bounds(good)) - 1
    for tag in ("fvar", "avar", "gvar"):   # and single bytes changed inside them
        off, length = tables[tag]
        for at, value in zip(rng.integers(off, off + length, 200).tolist(), rng.integers(0, 256, 200).tolist()):
            bad = bytearray(good)
            bad[at] = value if value != good[at] else value ^ 0xFF
            outcomes[quiet(_exercise, bytes(bad))] += 1
    assert outcomes["parsed"] > 0 and outcomes["refused"] > 0, outcomes


def test_hand_made_defects():
    def with_gvar(**options):
        return G.add_tables(K.synthetic_ttf(), {"fvar": G.fvar_table(G.AXES), "gvar": G.gvar_table(2, VAR, **options)})

    with pytest.raises(ValueError, match="truetype: gvar: axisCount"):
        S.read_ttf(with_gvar(axis_count=3))
    with pytest.raises(ValueError, match="truetype: gvar: glyphCount"):
        S.read_ttf(with_gvar(glyph_count=len(K.GLYPHS) + 1))
    with pytest.raises(ValueError, match="truetype: gvar: version"):
        S.read_ttf(with_gvar(version=2))
    good = with_gvar(long_offsets=True, shared_points=False)
    font = S.read_ttf(good)
    off = font.tables["gvar"][0]
    data_at = struct.unpack_from(">I", good, off + 16)[0]
    offsets = struct.unpack_from(f">{len(K.GLYPHS) + 1}I", good, off + 20)
    record = off + data_at + offsets[2]   # glyph 2's variation data: five tuples

    def poke(at, fmt, value):
        bad = bytearray(good)
        struct.pack_into(fmt, bad, at, value)
        return S.read_ttf(bytes(bad))

    with pytest.raises(ValueError, match="truetype: gvar"):   # a tuple count whose headers run past the glyph's data
        TV.glyph_tuples(poke(record, ">H", 0x0FFF), 2)
    with pytest.raises(ValueError, match="truetype: gvar"):   # a shared tuple index out of range
        TV.glyph_tuples(poke(record + 6, ">H", 0x2000 | 0x0FFF), 2)
    with pytest.raises(ValueError, match="truetype: gvar"):   # the first tuple's data size beyond the record
        TV.glyph_tuples(poke(record + 4, ">H", 0xFFFF), 2)
    # a delta run past its end: the last tuple's data cut short by two bytes (its size says so)
    size_at = record + 4 + 4 * 4   # the header of the fifth tuple, behind the count, the data offset and four headers of 4 bytes
    size, = struct.unpack_from(">H", good, size_at)
    with pytest.raises(ValueError, match="truetype: gvar"):
        TV.glyph_tuples(poke(size_at, ">H", size - 2), 2)
    assert len(TV.glyph_tuples(font, 2)) == 5


# ---- the per-lane header on the host against the reference -----------------------------------------------------------------
@pytest.fixture(scope="module")
def gv():
    lib = host_build("gvar_harness")
    lib.gv_deltas.restype = lib.gv_outline_var.restype = C.c_int
    return lib


@pytest.fixture(scope="module")
def gh():
    lib = host_build("glyf_harness")
    lib.gh_validate.restype = lib.gh_outline.restype = C.c_int
    return lib


def _p(x):
    return x.ctypes.data_as(_P)


def _tuple_args(a):
    return [_p(a["glyph_tuple_off"]), _p(a["tuple_scalar"]), C.c_int64(len(a["tuple_scalar"])), _p(a["tuple_pt_off"]), _p(a["tp_index"]),
            _p(a["tp_dxy"]), C.c_int64(len(a["tp_index"]))]


def harness_deltas(gv, a, fill=np.nan):
    out = np.full((len(a["pt_xy"]), 2), fill)
    rc = gv.gv_deltas(_p(a["pt_xy"]), C.c_int64(len(a["pt_xy"])), _p(a["contour_off"]), C.c_int64(len(a["contour_off"]) - 1),
                      _p(a["glyph_contour_off"]), C.c_int64(len(a["glyph_contour_off"]) - 1), *_tuple_args(a), _p(out))
    return rc, out


def harness_outline_var(gv, gh, atlas, tuples, parts):
    a = {**K.pack(atlas, parts), **G.pack(atlas, tuples)}
    glyf = [_p(a["pt_on"]), C.c_int64(len(a["pt_on"])), _p(a["contour_off"]), C.c_int64(len(a["contour_off"]) - 1), _p(a["glyph_contour_off"]),
            C.c_int64(len(a["glyph_contour_off"]) - 1), _p(a["part_glyph"]), _p(a["part_m"]), _p(a["part_pen"]), _p(a["part_sx"]), _p(a["part_sy"]),
            C.c_int64(len(a["part_glyph"]))]
    counts = np.zeros(3, dtype=np.int64)
    assert gh.gh_validate(*glyf, _p(counts)) == 0
    types, params, sizes = np.zeros(counts[1], dtype=np.int32), np.full((counts[1], 8), np.nan), np.zeros(counts[2], dtype=np.int32)
    rc = gv.gv_outline_var(_p(a["pt_xy"]), *glyf, *_tuple_args(a), _p(types), _p(params), _p(sizes))
    assert rc == 0, rc
    return types, params, sizes


def _same(got, want, what):
    for g, w, name in zip(got, want, ("types", "params", "sizes")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, name)


CASES = G.delta_cases()


def test_the_case_list_has_the_totals_it_claims():
    totals = {name: G.points_of(atlas) for name, atlas, _t in CASES}
    assert [totals[f"points_{n}"] for n in ("B-1", "B", "B+1", "2B+1")] == [G.B - 1, G.B, G.B + 1, 2 * G.B + 1]
    assert max(len(c) for c in next(c for c in CASES if c[0] == "glyph_larger_than_block")[1][0]) > G.B
    for name in ("straddle_touched_behind", "straddle_touched_in_front"):
        _n, atlas, tuples = next(c for c in CASES if c[0] == name)
        first, second = (len(c) for c in atlas[0])
        assert first < G.B < first + second
        touched = [e[0] for e in tuples[0][0][1]]
        assert all(first <= i for i in touched) and (all(i >= G.B for i in touched) or all(i < G.B for i in touched))


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_harness_equals_reference(gv, gh, name):
    _name, atlas, tuples = next(c for c in CASES if c[0] == name)
    rc, got = harness_deltas(gv, G.pack(atlas, tuples))
    want = V.flat(V.deltas(atlas, tuples))
    assert rc == 0 and got.shape == want.shape and got.tobytes() == want.tobytes()
    parts = G.rotated_parts(atlas)
    _same(harness_outline_var(gv, gh, atlas, tuples, parts), V.outline_var(atlas, tuples, parts), name)


def test_harness_equals_reference_on_the_fuzz_set(gv, gh):
    for seed in range(200):
        atlas, tuples = G.fuzz_case(seed)
        rc, got = harness_deltas(gv, G.pack(atlas, tuples))
        assert rc == 0 and got.tobytes() == V.flat(V.deltas(atlas, tuples)).tobytes(), seed
        if seed % 8 == 0:
            parts = G.rotated_parts(atlas)
            _same(harness_outline_var(gv, gh, atlas, tuples, parts), V.outline_var(atlas, tuples, parts), seed)


def test_without_tuples_the_outline_is_the_static_one(gv, gh):
    _name, atlas, _tuples = CASES[0]
    parts = G.rotated_parts(atlas)
    _same(harness_outline_var(gv, gh, atlas, [[] for _ in atlas], parts), R.outline(atlas, parts), "no tuples")


def test_refusals_leave_the_output_untouched(gv):
    _name, atlas, tuples = CASES[0]    # (glyph 0 has 100 points, 9 and 30 touched by its two tuples)
    good = G.pack(atlas, tuples)
    rc, out = harness_deltas(gv, good, fill=7.0)
    assert rc == 0 and not (out == 7.0).all()
    for what, a, status in G.refusals(good):
        rc, out = harness_deltas(gv, a, fill=7.0)
        assert rc == status and (out == 7.0).all(), what
    # counts beyond INT32_MAX / 2 are an overflow (nothing is read: the walk refuses first)
    n = C.c_int64(2 ** 30)
    rc = gv.gv_deltas(_p(good["pt_xy"]), n, _p(good["contour_off"]), C.c_int64(1), _p(good["glyph_contour_off"]), C.c_int64(1),
                      *_tuple_args(good), None)
    assert rc == E_OVERFLOW


# ---- the fontTools record ----------------------------------------------------------------------------------------------------
GOLDEN_FONT = os.path.join(GOLDEN, "fonts", "varsynth.ttf")


def _check_record(rec, data):
    """`rec` (gen_gvar_golden.record) against the parser, the host arithmetic, the harness-free reference: every value equal
    as a number (+0 and -0 alike), at every location."""
    from tests.tools import gen_gvar_golden as T

    font = S.read_ttf(data)
    tags = [a.tag for a in font.axes]
    assert tags == [a[0] for a in T.AXES]
    glyphs = [dict(components=[dict(glyph=T.ORDER.index(b), dx=dx, dy=dy) for b, dx, dy in T.COMPONENTS[name]]) if name in T.COMPONENTS
              else T.OUTLINES[name] for name in T.ORDER]
    assert len(rec["locations"]) == len(T.LOCATIONS) >= 12
    for i, user in enumerate(rec["locations"]):
        user = dict(zip(tags, user.tolist()))
        inst = font.instance(user)
        normal = TV.coordinates(font, user)[1]
        assert normal == tuple(rec["normalised"][i].tolist()), (user, normal)
        for gid, glyph in enumerate(glyphs):
            assert inst.advance(gid) == rec["advances"][i][gid], (user, gid)
            want = rec[f"points_{gid}"][i]
            if isinstance(glyph, dict):
                got = np.array([m[4:6] for _child, m in inst._placed_components(gid)], dtype=np.float64).reshape(-1, 2)
            else:
                # the parser's tuples through the reference's arithmetic: the device's arithmetic is held against the same
                # reference bit for bit elsewhere
                a = TV.tuple_arrays(font, [gid], normal)
                tuples = [(float(a["tuple_scalar"][t]), [(int(a["tp_index"][k]), int(a["tp_dxy"][k, 0]), int(a["tp_dxy"][k, 1]))
                                                       for k in range(a["tuple_pt_off"][t], a["tuple_pt_off"][t + 1])])
                          for t in range(len(a["tuple_scalar"]))]
                got = np.array([(x, y) for c in V.varied([glyph], [tuples])[0] for x, y, _on in c], dtype=np.float64).reshape(-1, 2)
            assert got.shape == want.shape and (got == want).all(), (user, gid, got, want)


def test_reference_and_parser_equal_the_fonttools_record():
    with open(GOLDEN_FONT, "rb") as f:
        data = f.read()
    with np.load(os.path.join(GOLDEN, "gvar_kat.npz"), allow_pickle=False) as npz:
        rec = {k: npz[k] for k in npz.files}
    assert json.loads(str(rec["meta"]))["axes"] == ["wght", "wdth"]
    _check_record(rec, data)


def test_the_record_recomputed_live_with_fonttools(tmp_path):
    pytest.importorskip("fontTools")
    from fontTools.ttLib import TTFont

    from tests.tools import gen_gvar_golden as T

    path = tmp_path / "live.ttf"
    T.build().save(str(path))
    live = T.record(TTFont(str(path)))
    with np.load(os.path.join(GOLDEN, "gvar_kat.npz"), allow_pickle=False) as npz:
        for key, value in live.items():
            assert (np.asarray(value) == npz[key]).all(), key
    _check_record(live, path.read_bytes())


# ---- an instance's host arithmetic, the loader, resolve ------------------------------------------------------------------------
@pytest.mark.parametrize("user", LOCATIONS, ids=[",".join(f"{k}={v}" for k, v in u.items()) for u in LOCATIONS])
def test_instance_host_arithmetic_equals_reference(font, user):
    inst = font.instance(user)
    coords = V.location(G.AXES, G.AVAR, user)
    assert inst.normalised == coords and inst.parent is font
    for gid, glyph in enumerate(K.GLYPHS):
        assert quiet(inst.advance, gid) == V.advance(K.GLYPHS, K.ADVANCES, VAR, coords, gid)
        assert quiet(inst.glyph_parts, gid) == V.flatten(K.GLYPHS, VAR, coords, gid), gid
    text = "AVo #\xf3Q V"
    placed, total = inst.str_to_glyphs(text)
    _atlas, parts, want_total = V.string_parts(K.GLYPHS, K.CMAP, K.ADVANCES, K.KERN, VAR, coords, text)
    assert total == want_total
    assert [(part, pen) for pen, glyph in placed for part in glyph.parts] == [((g, *m), pen) for g, m, pen in parts]
    # what goes to the device is what the reference would hand it
    want = V.device_tuples(K.GLYPHS, VAR, coords)
    simple = [gid for gid, g in enumerate(K.GLYPHS) if not isinstance(g, dict)]
    got = TV.tuple_arrays(font, simple, coords)
    packed = G.pack([K.GLYPHS[g] for g in simple], [[t for t in want[g] if t[1]] for g in simple])
    for key in ("glyph_tuple_off", "tuple_scalar", "tuple_pt_off", "tp_index", "tp_dxy"):
        assert got[key].dtype == packed[key].dtype and got[key].tobytes() == packed[key].tobytes(), key


def test_instance_interface(font):
    assert font.instance() is font and font.instance(wght=400, wdth=100) is font and font.instance({"wght": 400}) is font
    bold = font.instance(wght=700)
    assert isinstance(bold, S.TrueTypeFont) and bold is font.instance({"wght": 700.0}) and bold.instance(wght=400) is font
    assert bold.weight == 700 and font.weight == 400 and bold.family == font.family and bold.axes == font.axes
    assert font.instance(wght=5000) is font.instance(wght=900) and font.instance(wght=5000).coords == {"wght": 900.0, "wdth": 100.0}
    assert font.instance(wdth=80).weight == 400
    with pytest.raises(ValueError, match="truetype: .*slnt"):
        font.instance(slnt=-8)
    assert bold.glyph(2) is not font.glyph(2) and bold.glyph(2).advance != font.glyph(2).advance
    assert bold._simple is font._simple   # (the decoded glyphs are shared)


def test_composite_offsets_vary(font):
    wide = font.instance(wdth=125)
    default, varied = font.glyph_parts(6), wide.glyph_parts(6)
    assert default[0] == varied[0] and default[1][:5] == varied[1][:5]
    assert varied[1][5:] == (220.0 + 70.0, 560.0 + 5.0) and wide.advance(6) == 600.0 + 150.0


def doc(attributes):
    return (f'<svg xmlns="http://www.w3.org/2000/svg" width="96" height="32" viewBox="0 0 96 32"><text x="2" y="24" font-family="VarSynth" '
            f'font-size="24" {attributes}>AV\xf3#</text></svg>')


def runs_of(scene, out):
    kind, args = scene
    if kind == S.RENDER_MARKERS:
        out.append(args)
    elif kind == S.RENDER_GROUP:
        for child in args:
            runs_of(child, out)
    elif kind == S.RENDER_TRANSFORM:
        runs_of(args[0], out)
    return out


def test_loader_builds_instances_without_a_device(font):
    db = S.FontsDB()
    db.register(font)

    def face(attributes):
        scene, _ids, _size = S.svg_scene_from_str(doc(attributes), fonts=db)
        run, = runs_of(scene, [])
        return run.font

    assert face("") is font and face('font-weight="400"') is font and face('font-variation-settings="normal"') is font
    assert face('font-weight="700"') is font.instance(wght=700) and face('font-weight="bold"') is font.instance(wght=700)
    assert face('''font-variation-settings="'wght' 650, 'wdth' 80"''') is font.instance(wght=650, wdth=80)
    assert face('''style="font-variation-settings: &quot;wdth&quot; 80.5"''') is font.instance(wdth=80.5)
    assert face('''font-weight="700" font-variation-settings="'wght' 650"''') is font.instance(wght=650)      # the setting wins
    assert face('''font-variation-settings="'opsz' 14, 'wght' 650"''') is font.instance(wght=650)            # an axis the face lacks
    assert face('font-stretch="condensed"') is font.instance(wdth=75) and face('font-stretch="semi-expanded"') is font.instance(wdth=112.5)
    assert face('font-stretch="90%"') is font.instance(wdth=90)
    assert face('''font-stretch="expanded" font-variation-settings="'wdth' 80"''') is font.instance(wdth=80)
    for bad in ('wght 650', "'wght'", "'wgh' 650", "'wght' 650 'wdth' 80", "'wght' heavy"):
        with pytest.warns(UserWarning, match="font-variation-settings"):
            assert face(f'font-variation-settings="{bad}"') is font
    with pytest.warns(UserWarning, match="font-stretch"):
        assert face('font-stretch="squeezed"') is font
    # inherited by a tspan, and the pen advances by the instance's advances
    scene, _ids, _size = S.svg_scene_from_str(
        '<svg xmlns="http://www.w3.org/2000/svg" width="96" height="32"><text y="24" font-family="VarSynth" font-size="1000" '
        '''font-variation-settings="'wdth' 125">A<tspan>A</tspan></text></svg>''', fonts=db)
    first, second = runs_of(scene, [])
    assert first.font is second.font is font.instance(wdth=125)
    assert font.instance(wdth=125).advance(2) == 850.0 and "850" in repr(scene)
    # and along a path
    scene, _ids, _size = S.svg_scene_from_str(
        '<svg xmlns="http://www.w3.org/2000/svg" width="96" height="32"><path id="p" d="M0,20 L90,20"/><text font-family="VarSynth" '
        'font-weight="700"><textPath href="#p">AV</textPath></text></svg>', fonts=db)
    on_path, = [args for args in _payloads(scene) if hasattr(args, "runs")]
    assert on_path.runs[0].font is font.instance(wght=700)


def _payloads(scene):
    kind, args = scene
    if kind == S.RENDER_GROUP:
        for child in args:
            yield from _payloads(child)
    elif kind == S.RENDER_TRANSFORM:
        yield from _payloads(args[0])
    else:
        yield args


def test_resolve(font):
    db = S.FontsDB()
    db.register(font)
    got = [db.resolve("VarSynth", weight, None, None) for weight in (100, 400, 650, 1000)]
    assert got[1] is font and [g.coords["wght"] for g in (got[0], got[2], got[3])] == [100.0, 650.0, 900.0]
    assert got[0] is font.instance(wght=100) and got[2].weight == 650 and got[3] is font.instance(wght=900)
    assert db.resolve("VarSynth", 650, None, {"wdth": 80, "opsz": 14, "XXXX": 1}) is font.instance(wght=650, wdth=80)
    assert db.resolve("VarSynth", 400, None, {"wght": 300}) is font.instance(wght=300)
    assert db.resolve("VarSynth") is font
    # a static Bold beside a variable face whose range ends at 500: weight 700 is nearer the static one
    narrow = S.read_ttf(G.add_tables(K.synthetic_ttf(family="Pair"), {"fvar": G.fvar_table([("wght", 100.0, 400.0, 500.0)])}))
    bold = S.read_ttf(K.synthetic_ttf(family="Pair", weight=700))
    db.register(narrow)
    db.register(bold)
    assert db.resolve("Pair", 700, None, None) is bold and db.resolve("Pair", 700, None, {"wght": 450}) is bold
    assert db.resolve("Pair", 450, None, None) is narrow.instance(wght=450) and db.resolve("Pair", 580, None, None) is narrow.instance(wght=500)
    assert db.resolve("Pair", 620, None, None) is bold
