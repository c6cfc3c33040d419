"""Variable fonts on the GPU: svgr_gvar_deltas and svgr_glyf_outline_var through the C ABI against the elementwise reference
(tests/gvar_ref.py) on shapes at the seams of the launch -- B = svgr_gvar_block() points per workgroup of k_gvar_delta -- and
on every branch of the delta rule, the public API of an instance, the record made with fontTools, and documents end to end
against their twins built from the reference's paths.  Everything is compared bit for bit: the arithmetic is fixed to the
operation and nothing here is discontinuous.  tests/test_truetype_var_host.py checks the same cases on the CPU."""
import os

import numpy as np
import pytest

from tests import gvar_cases as G
from tests import gvar_ref as V
from tests import ttf_cases as K
from tests import ttf_ref as R
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu

CASES = G.delta_cases()
VAR = G.variations()


@pytest.fixture(scope="module")
def abi():
    from svgrasterize_amd import _abi

    _abi.Context.get()
    return _abi


@pytest.fixture(scope="module")
def wanted():
    """The reference's deltas of every fixed case, computed once."""
    return {name: V.flat(V.deltas(atlas, tuples)) for name, atlas, tuples in CASES}


def same(got, want, what):
    for g, w, name in zip(got, want, ("types", "params", "sizes")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, name)


def outline_var(abi, atlas, tuples, parts):
    return abi.glyf_outline_var(**K.pack(atlas, parts), **{k: v for k, v in G.pack(atlas, tuples).items() if k.startswith(("glyph_tuple", "tuple_", "tp_"))})


def test_block_is_what_the_cases_assume(abi):
    assert abi.gvar_block() == G.B == 256
    totals = {name: G.points_of(atlas) for name, atlas, _t in CASES}
    assert [totals[f"points_{n}"] for n in ("B-1", "B", "B+1", "2B+1")] == [G.B - 1, G.B, G.B + 1, 2 * G.B + 1]
    assert max(len(c) for c in next(c for c in CASES if c[0] == "glyph_larger_than_block")[1][0]) > G.B
    for name in ("straddle_touched_behind", "straddle_touched_in_front"):
        _n, atlas, _tuples = next(c for c in CASES if c[0] == name)
        assert len(atlas[0][0]) < G.B < len(atlas[0][0]) + len(atlas[0][1])


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_fixed_case(abi, wanted, name):
    _name, atlas, tuples = next(c for c in CASES if c[0] == name)
    got = abi.gvar_deltas(**G.pack(atlas, tuples))
    assert got.dtype == np.float64 and got.shape == wanted[name].shape and got.tobytes() == wanted[name].tobytes()
    parts = G.rotated_parts(atlas)
    same(outline_var(abi, atlas, tuples, parts), V.outline_var(atlas, tuples, parts), name)


def test_fuzz_set(abi):
    for seed in range(200):
        atlas, tuples = G.fuzz_case(seed)
        got = abi.gvar_deltas(**G.pack(atlas, tuples))
        assert got.tobytes() == V.flat(V.deltas(atlas, tuples)).tobytes(), seed
        if seed % 4 == 0:
            parts = G.rotated_parts(atlas)
            same(outline_var(abi, atlas, tuples, parts), V.outline_var(atlas, tuples, parts), seed)


def test_without_tuples_the_outline_is_svgr_glyf_outline(abi):
    for name in ("points_2B+1", "glyph_base"):
        _name, atlas, _tuples = next(c for c in CASES if c[0] == name)
        parts = G.rotated_parts(atlas)
        same(outline_var(abi, atlas, [[] for _ in atlas], parts), abi.glyf_outline(**K.pack(atlas, parts)), name)
        assert not abi.gvar_deltas(**G.pack(atlas, [[] for _ in atlas])).any()


def test_two_runs_are_byte_identical(abi):
    for name in ("points_2B+1", "glyph_larger_than_block", "no_tuple_next_to_five"):
        _name, atlas, tuples = next(c for c in CASES if c[0] == name)
        parts = G.rotated_parts(atlas)
        same(outline_var(abi, atlas, tuples, parts), outline_var(abi, atlas, tuples, parts), name)
        assert abi.gvar_deltas(**G.pack(atlas, tuples)).tobytes() == abi.gvar_deltas(**G.pack(atlas, tuples)).tobytes()


def test_refusals_launch_nothing_and_good_calls_launch_what_they_say(abi, wanted):
    ctx = abi.Context.get()
    name, atlas, tuples = CASES[0]
    good = G.pack(atlas, tuples)
    parts = G.rotated_parts(atlas)
    glyf = K.pack(atlas, parts)
    before = ctx.launches()
    for _what, a, _status in G.refusals(good):
        with pytest.raises(ValueError):
            abi.gvar_deltas(**a)
        with pytest.raises(ValueError):
            abi.glyf_outline_var(**{**glyf, **{k: v for k, v in a.items() if k != "pt_xy"}})
    assert not abi.gvar_deltas(**G.pack([], [])).size and not abi.gvar_deltas(**G.pack(atlas, [[] for _ in atlas])).any()   # nothing to do
    assert ctx.launches() == before   # nothing was launched by any of these
    assert abi.gvar_deltas(**good).tobytes() == wanted[name].tobytes()
    assert ctx.launches() == before + 1
    same(outline_var(abi, atlas, tuples, parts), V.outline_var(atlas, tuples, parts), name)
    assert ctx.launches() == before + 3


# ---- the public API ----------------------------------------------------------------------------------------------------
USER = {"wght": 650, "wdth": 80}
TEXT = "AVo #\xf3Q V"   # kerning (AV), an unmapped character, varied composites (one of them nested), the space


@pytest.fixture(scope="module")
def font(abi):
    import svgrasterize_amd as S

    return S.read_ttf(G.synthetic_var_ttf())


def reference_path(text, size, user):
    """The reference's outline of `text` in the synthetic variable font at `size` and the location `user`, and the advance."""
    scale = size / 1000.0
    coords = V.location(G.AXES, G.AVAR, user)
    atlas, parts, advance = V.string_parts(K.GLYPHS, K.CMAP, K.ADVANCES, K.KERN, VAR, coords, text)
    return R.outline(atlas, [(g, m, pen, scale, -scale) for g, m, pen in parts]), advance * scale


def arrays_of(path):
    types, params, sizes = path._segment_arrays()
    return np.array(types, dtype=np.int32), np.array(params, dtype=np.float64).reshape(-1, 8), np.array(sizes, dtype=np.int32)


def test_instance_str_to_path_equals_reference(font):
    inst = font.instance(wght=650, wdth=80)
    path, advance = inst.str_to_path(24.0, TEXT)
    want, want_advance = reference_path(TEXT, 24.0, USER)
    same(arrays_of(path), want, TEXT)
    assert advance == want_advance
    static, static_advance = font.str_to_path(24.0, TEXT)
    assert advance != static_advance and arrays_of(static)[1].tobytes() != want[1].tobytes()
    # a glyph on its own: glyph units, y up; a composite through its varied offsets
    coords = V.location(G.AXES, G.AVAR, USER)
    varied = V.varied([[] if isinstance(g, dict) else g for g in K.GLYPHS], V.device_tuples(K.GLYPHS, VAR, coords))
    glyph = inst.str_to_glyphs("o")[0][0][1]
    same(glyph.arrays, R.outline(varied, [(3, K.IDENTITY, 0.0, 1.0, 1.0)]), "o")
    composite = inst.str_to_glyphs("\xf3")[0][0][1]
    parts = [(g, tuple(m), 0.0, 1.0, 1.0) for g, *m in V.flatten(K.GLYPHS, VAR, coords, 6)]
    same(composite.arrays, R.outline(varied, parts), "oacute")
    assert len(composite.path.subpaths) == 3
    # along a path: the contours of the visible glyphs
    import svgrasterize_amd as S

    on_path, along = inst.str_on_path(S.Path.from_svg("M0,50 L400,50"), 20.0, "Ao A")
    assert len(on_path.subpaths) == 2 + 2 + 0 + 2 and along == sum(inst.advance(g) for g in (2, 3, 1, 2)) * 0.02


def test_glyph_deltas_equal_the_fonttools_record(abi):
    import svgrasterize_amd as S

    with open(os.path.join(GOLDEN, "fonts", "varsynth.ttf"), "rb") as f:
        golden = S.read_ttf(f.read())
    tags = [a.tag for a in golden.axes]
    with np.load(os.path.join(GOLDEN, "gvar_kat.npz"), allow_pickle=False) as rec:
        for i, user in enumerate(rec["locations"]):
            for gid in range(golden.n_glyphs):
                base = golden.simple_glyph(gid).xy.astype(np.float64)
                if not len(base):
                    assert golden.glyph_deltas(gid, dict(zip(tags, user.tolist()))).shape == (0, 2)
                    continue
                got = base + golden.glyph_deltas(gid, dict(zip(tags, user.tolist())))
                assert got.shape == rec[f"points_{gid}"][i].shape and (got == rec[f"points_{gid}"][i]).all(), (user, gid)


# ---- end to end ----------------------------------------------------------------------------------------------------------
ROWS, COLS = 32, 96


def doc(attributes):
    return (f'<svg xmlns="http://www.w3.org/2000/svg" width="{COLS}" height="{ROWS}" viewBox="0 0 {COLS} {ROWS}">'
            f'<text x="2" y="24" font-family="VarSynth" font-size="24" fill="#204080" {attributes}>AV\xf3#</text></svg>')


def canvas_in_list_order(scene):
    """The scene as one batch on a canvas of doubles through `render_canvas(deterministic=True)`: the bits of the picture are a
    function of the geometry alone (tests/test_gpu_truetype.py says why equal bytes need that)."""
    import svgrasterize_amd as S

    view = S.Transform().matrix(0, 1, 0, 1, 0, 0)
    img, _stats = S.render_canvas(scene, view, [0, 0, ROWS, COLS], linear_rgb=True, out_f64=True, deterministic=True)
    return img


def twin_of(scene, user, made):
    """`scene` with every text node replaced by the FILL of the reference's path of its run at the location `user`."""
    import svgrasterize_amd as S
    from svgrasterize_amd import svg

    kind, args = scene
    if kind == S.RENDER_MARKERS:
        run = args
        (types, params, sizes), _advance = reference_path(run.text, run.size, user)
        made.append(run.text)
        return S.Scene.fill(S.Path.from_segments(types, params, sizes), svg.parse_paint(run.attrs["fill"], {}), S.PATH_FILL_NONZERO)
    if kind == S.RENDER_GROUP:
        return S.Scene(kind, tuple(twin_of(child, user, made) for child in args))
    if kind == S.RENDER_TRANSFORM:
        return S.Scene(kind, (twin_of(args[0], user, made), args[1]))
    raise AssertionError(f"the document has a node of kind {kind}")


@pytest.mark.parametrize("attributes, user", [('font-weight="700"', {"wght": 700}),
                                              ('''font-variation-settings="'wght' 650, 'wdth' 80"''', USER)], ids=["bold", "settings"])
def test_document_renders_like_its_twin(font, attributes, user):
    import svgrasterize_amd as S

    db = S.FontsDB()
    db.register(font)
    scene, _ids, _size = S.svg_scene_from_str(doc(attributes), fonts=db)
    made = []
    twin = twin_of(scene, user, made)
    assert made == ["AV\xf3#"] and "TEXT" not in repr(twin)
    got, want = canvas_in_list_order(scene), canvas_in_list_order(twin)
    assert got[..., 3].max() > 0.9 and (got[..., 3] > 0).sum() > 300
    assert got.tobytes() == want.tobytes()
    regular, _ids, _size = S.svg_scene_from_str(doc('font-weight="400"'), fonts=db)
    plain = canvas_in_list_order(regular)
    assert plain.tobytes() != got.tobytes() and (plain[..., 3] > 0).sum() > 300
