"""OpenType / CFF outlines on the GPU: svgr_cff_outline through the C ABI against the elementwise reference (tests/cff_ref.py)
on shapes at the seams of the launch -- B = svgr_cff_block() output segments per workgroup of k_cff_emit -- and on every branch
of the outline rule, the public API on the committed font (tests/golden/fonts/cffsynth.otf) against the contours fontTools
recorded for it (tests/golden/cff_kat.npz), and a document end to end against its twin built from the reference's paths.  Types
and sizes are compared exactly, coordinates bit for bit: the arithmetic is fixed to the operation and nothing here is
discontinuous.  tests/test_cff_host.py checks the same cases on the CPU."""
import os

import numpy as np
import pytest

from tests import cff_cases as K
from tests import cff_ref as R
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu

CASES = K.outline_cases()


@pytest.fixture(scope="module")
def abi():
    from svgrasterize_amd import _abi

    _abi.Context.get()
    return _abi


def run(abi, atlas, parts):
    return abi.cff_outline(**K.pack(atlas, parts))


def same(got, want, what):
    for g, w, name in zip(got, want, ("types", "params", "sizes")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, name)


def test_block_is_what_the_cases_assume(abi):
    assert abi.cff_block() == K.B
    totals = {name: K.segments(atlas, parts) for name, atlas, parts in CASES}
    assert [totals[f"segments_{n}"] for n in ("B-1", "B", "B+1", "2B+1")] == [K.B - 1, K.B, K.B + 1, 2 * K.B + 1]
    assert totals["glyph_larger_than_block"] > K.B and totals["same_glyph_B+1_parts"] == 5 * (K.B + 1)
    _name, atlas, parts = next(c for c in CASES if c[0] == "closing_line_first_lane_of_block")
    types, _params, sizes = R.outline(atlas, parts)
    assert types[K.B] == R.PATH_CLOSED and types[K.B - 1] != R.PATH_CLOSED and sizes[0] < K.B < sizes[0] + sizes[1]


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_fixed_case(abi, name):
    _name, atlas, parts = next(c for c in CASES if c[0] == name)
    same(run(abi, atlas, parts), R.outline(atlas, parts), name)


def test_fuzz_set(abi):
    for seed in range(200):
        atlas, parts = K.fuzz_case(seed)
        same(run(abi, atlas, parts), R.outline(atlas, parts), seed)


def test_two_runs_are_byte_identical(abi):
    for name in ("segments_2B+1", "same_glyph_B+1_parts", "rotated_part"):
        _name, atlas, parts = next(c for c in CASES if c[0] == name)
        same(run(abi, atlas, parts), run(abi, atlas, parts), name)


def test_bad_and_empty_input(abi):
    from tests.test_cff_host import refusals

    ctx = abi.Context.get()
    good, bad = refusals()
    before = ctx.launches()
    one = (0, K.IDENTITY, 0.0, 1.0, 1.0)
    for a in (K.pack(CASES[0][1], []), K.pack([[], [K.ring(np.random.default_rng(3), 4)]], [one] * 3), K.pack([[[(1.0, 2.0, K.MOVE)]]], [one])):
        types, params, sizes = abi.cff_outline(**a)    # no part; parts of an empty glyph; a lone MOVE: nothing to launch
        assert types.shape == (0,) and params.shape == (0, 8) and sizes.shape == (0,)
    for what, a, _status in bad:
        with pytest.raises(ValueError):
            abi.cff_outline(**a)
        assert ctx.launches() == before, what   # nothing was launched by any of these
    _name, atlas, parts = CASES[0]
    same(abi.cff_outline(**good), R.outline(atlas, parts), "good")
    assert ctx.launches() == before + 1


# ---- the public API on the committed font --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def font(abi):
    import svgrasterize_amd as S

    with open(os.path.join(GOLDEN, "fonts", "cffsynth.otf"), "rb") as f:
        return S.read_otf(f.read())


@pytest.fixture(scope="module")
def record():
    """What fontTools recorded for the committed font: (glyphs as lists of contours, cmap, advances, kern)."""
    npz = np.load(os.path.join(GOLDEN, "cff_kat.npz"), allow_pickle=False)
    glyphs = []
    for gid in range(int(npz["n_glyphs"])):
        xy, kind, first, contours = npz[f"xy_{gid}"], npz[f"kind_{gid}"], 0, []
        for end in npz[f"ends_{gid}"].tolist():
            contours.append([(float(x), float(y), int(k)) for (x, y), k in zip(xy[first:end + 1].tolist(), kind[first:end + 1].tolist())])
            first = end + 1
        glyphs.append(contours)
    return (glyphs, {int(c): int(g) for c, g in npz["cmap"]}, npz["advances"].tolist(), {(int(a), int(b)): int(v) for a, b, v in npz["kern"]})


def reference_path(record, text, size):
    """The reference's outline of `text` in the committed font at `size`: (types, params, sizes), and the advance."""
    scale = size / 1000.0
    atlas, parts, advance = R.string_parts(*record, text)
    return R.outline(atlas, [(g, m, pen, scale, -scale) for g, m, pen in parts]), advance * scale


def arrays_of(path):
    types, params, sizes = path._segment_arrays()
    return np.array(types, dtype=np.int32), np.array(params, dtype=np.float64).reshape(-1, 8), np.array(sizes, dtype=np.int32)


def test_str_to_path_equals_reference(font, record):
    text = "AVo #D V"    # kerning (AV), an unmapped character, the space, subroutines, a flex with a fractional operand
    path, advance = font.str_to_path(24.0, text)
    want, want_advance = reference_path(record, text, 24.0)
    same(arrays_of(path), want, text)
    assert advance == want_advance and len(want[2]) == 2 + 1 + 2 + 2 + 1 + 1
    assert R.PATH_CUBIC in want[0] and R.PATH_LINE in want[0]
    empty, advance = font.str_to_path(24.0, "  ")
    assert empty.subpaths == [] and advance == 2 * 300 * 24.0 / 1000.0
    # a glyph on its own: glyph units, y up
    glyph = font.str_to_glyphs("o")[0][0][1]
    same(glyph.arrays, R.outline([record[0][3]], [(0, K.IDENTITY, 0.0, 1.0, 1.0)]), "o")
    assert len(glyph.path.subpaths) == 2


def test_str_on_path_places_the_visible_glyphs_contours(font, record):
    import svgrasterize_amd as S

    line = S.Path.from_svg("M0,50 L400,50")
    on_path, advance = font.str_on_path(line, 20.0, "Ao AD")
    assert len(on_path.subpaths) == 2 + 2 + 0 + 2 + 1 and advance == (700 + 600 + 300 + 700 + 650) * 0.02
    short = S.Path.from_svg("M0,50 L20,50")    # room for the A and the o's middle only
    on_path, _advance = font.str_on_path(short, 20.0, "Ao AD")
    assert len(on_path.subpaths) == 2 + 2
    # on a straight horizontal path a glyph keeps its shape: the A of the string against the reference's A, moved
    a_only, _advance = font.str_on_path(line, 20.0, "A")
    (types, params, sizes), _ = reference_path(record, "A", 20.0)
    got = arrays_of(a_only)
    assert got[0].tolist() == types.tolist() and got[2].tolist() == sizes.tolist()
    moved = params.copy()
    moved[:, 1::2] += 50.0
    used = np.repeat((types == R.PATH_CUBIC)[:, None], 8, axis=1) | (np.arange(8) < 4)[None, :]
    assert np.abs(got[1] - moved)[used].max() <= 1e-9


# ---- end to end ----------------------------------------------------------------------------------------------------------
SIZE = 128
DOC = (f'<svg xmlns="http://www.w3.org/2000/svg" width="{SIZE}" height="{SIZE}" viewBox="0 0 {SIZE} {SIZE}">'
       '<text x="5" y="52" font-family="CFF Synth" font-size="40" fill="#204080" stroke="#c02000" stroke-width="1.5" stroke-dasharray="4 2.5">'
       '<tspan>AV</tspan><tspan x="8" dy="50" font-size="34">oD #</tspan></text></svg>')


def canvas(scene):
    """The scene through `Scene.render`, the caller's route, on a SIZE x SIZE canvas of doubles."""
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


def canvas_in_list_order(scene):
    """The scene as one batch on a canvas of doubles through `render_canvas(deterministic=True)`: one wave does every
    accumulation in list order, so the bits of the picture are a function of the geometry alone ("Render window")."""
    import svgrasterize_amd as S

    view = S.Transform().matrix(0, 1, 0, 1, 0, 0)
    img, _stats = S.render_canvas(scene, view, [0, 0, SIZE, SIZE], linear_rgb=True, out_f64=True, deterministic=True)
    return img


def twin_of(scene, record, made):
    """`scene` with every text node replaced by the FILL and STROKE of the reference's path of its run."""
    import svgrasterize_amd as S
    from svgrasterize_amd import svg

    kind, args = scene
    if kind == S.RENDER_MARKERS:
        run = args
        (types, params, sizes), _advance = reference_path(record, run.text, run.size)
        path = S.Path.from_segments(types, params, sizes)
        made.append(run.text)
        return S.Scene.group([
            S.Scene.fill(path, svg.parse_paint(run.attrs["fill"], {}), S.PATH_FILL_NONZERO),
            S.Scene.stroke(path, svg.parse_paint(run.attrs["stroke"], {}), 1.5, None, None, dasharray=[4.0, 2.5], dashoffset=0.0)])
    if kind == S.RENDER_GROUP:
        return S.Scene(kind, tuple(twin_of(child, record, made) for child in args))
    if kind == S.RENDER_TRANSFORM:
        return S.Scene(kind, (twin_of(args[0], record, made), args[1]))
    raise AssertionError(f"the document has a node of kind {kind}")


def test_document_renders_like_its_twin(font, record):
    """tests/test_gpu_truetype.py's document test for the CFF font: the document and its twin -- every run a `Scene.fill` /
    `Scene.stroke` of the reference's path, built from arrays -- give byte-identical canvases in list order
    (`render_canvas(deterministic=True)`), and through `Scene.render`, whose accumulation order is free, agree within the bound
    that test derives: a pixel's value is a sum of at most 64 edge terms of magnitude at most 1 per path, over 4 paths, and
    reordering a sum of n terms moves it by at most (n - 1) u times the sum of their magnitudes: 256 * 256 * 2^-53 = 7.3e-12."""
    import io

    import svgrasterize_amd as S

    db = S.FontsDB()
    db.register(font)
    scene, _ids, _size = S.svg_scene_from_str(DOC, fonts=db)
    made = []
    twin = twin_of(scene, record, made)
    assert made == ["AV", "oD #"] and "TEXT" not in repr(twin) and repr(scene).count("TEXT") == 2
    got, want = canvas_in_list_order(scene), canvas_in_list_order(twin)
    assert got[..., 3].max() > 0.99 and (got[..., 3] > 0).sum() > 500
    differ = int((got != want).sum())
    print(f"list order: {differ} of {got.size} values differ, by at most {np.abs(got - want).max():.3e}")
    assert got.tobytes() == want.tobytes()
    again = canvas_in_list_order(scene)
    assert got.tobytes() == again.tobytes()
    loose, loose_twin = canvas(scene), canvas(twin)
    print(f"Scene.render: {int((loose != loose_twin).sum())} of {loose.size} values differ, by at most {np.abs(loose - loose_twin).max():.3e}")
    assert loose[..., 3].max() > 0.99 and np.abs(loose - loose_twin).max() <= 256 * 256 * 2.0 ** -53
    # and through the front door: the labels are in the PNG
    png = S.render_svg(io.StringIO(DOC), fonts=db, linear_rgb=True)
    pixels = S.read_png(png)
    assert pixels.shape[:2] == (SIZE, SIZE) and (np.asarray(pixels)[..., 3] > 0).sum() > 500
