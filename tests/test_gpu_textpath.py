"""Text on a path on the GPU: svgr_path_sample and svgr_path_place_glyphs through the C ABI against the host reference
(tests/textpath_ref.py) on shapes at the seams of the launch geometry -- B = svgr_textpath_block() queries / output segments
per workgroup of the pass's own kernels, S = svgr_dash_scan_segments() per workgroup of the scan --, the public API, and a
document end to end against its twin with every visible glyph written out by hand.  Structure and flags are compared exactly,
coordinates within the reference's derived tolerance; tests/test_textpath_host.py checks on the CPU that the inputs are what
they are meant to be."""
import ctypes
import warnings

import numpy as np
import pytest

from tests import textpath_cases as cases
from tests import textpath_ref as R
from tests.test_textpath_host import run_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def abi():
    from svgrasterize_amd import _abi

    _abi.Context.get()
    return _abi


FIXED_ATLAS, FIXED = cases.fixed_cases()


def sample(abi):
    return lambda types, params, sizes, s: abi.path_sample(types, np.array(params, dtype=np.float64), sizes, s)


def place(abi):
    return lambda types, params, sizes, *rest: abi.path_place_glyphs(types, np.array(params, dtype=np.float64), sizes, *rest)


def test_seams_are_what_the_cases_assume(abi):
    assert abi.textpath_block() == cases.B and abi.dash_scan_segments() == cases.S


@pytest.mark.parametrize("case", FIXED + cases.joint_cases(), ids=lambda c: c["name"])
def test_fixed_case(abi, case):
    worst = run_case(FIXED_ATLAS, case, sample(abi), place(abi))
    print(f"{case['name']}: largest error / tolerance {worst:.3f}")


def test_fuzz_set(abi):
    ran, worst = 0, 0.0
    for atlas, case in cases.fuzz_cases():
        if cases.clearance(atlas, case) < cases.FUZZ_CLEARANCE:
            continue
        worst = max(worst, run_case(atlas, case, sample(abi), place(abi)))
        ran += 1
    print(f"fuzz: {ran} ran, largest error / tolerance {worst:.3f}")
    assert ran >= 190


def test_two_runs_are_byte_identical(abi):
    for wanted in (f"mixed{2 * cases.S + 1}", f"instances{cases.B + 1}", "glyph_over_a_block"):
        case = next(c for c in FIXED if c["name"] == wanted)
        for _ in range(2):
            if case["s"] is not None:
                a, b = (sample(abi)(*case["path"], case["s"]) for _ in range(2))
                assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b)), wanted
            a, b = (place(abi)(*case["path"], *FIXED_ATLAS, *case["inst"]) for _ in range(2))
            assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b)), wanted


def test_bad_and_empty_input(abi):
    a_types, a_params, a_off = FIXED_ATLAS
    inst = (np.array([0, 1], dtype=np.int32), np.array([1.0, 5.0]), np.array([3.0, 5.0]), np.zeros(2))
    ctx = abi.Context.get()
    before = ctx.launches()
    # no segments: nothing is launched, nothing is inside, the length is 0
    xy, u, inside, L = abi.path_sample([], np.zeros((0, 8)), [], [0.0, 1.0])
    assert xy.shape == u.shape == (2, 2) and not inside.any() and L == 0.0
    out, visible, L = abi.path_place_glyphs([], np.zeros((0, 8)), [], a_types, a_params, a_off, *inst)
    assert out.shape == (1 + 10, 8) and not out.any() and not visible.any() and L == 0.0
    assert ctx.launches() == before
    line = R.polyline([(0, 0), (10, 0), (10, 10)])
    good = np.array(line[1], dtype=np.float64)
    for bad in (float("nan"), float("inf"), -float("inf"), 1e155):
        params = good.copy()
        params[1, 2] = bad
        with pytest.raises(ValueError):
            abi.path_sample(line[0], params, line[2], [1.0])
        with pytest.raises(ValueError):
            abi.path_place_glyphs(line[0], params, line[2], a_types, a_params, a_off, *inst)
        broken = a_params.copy()
        broken[0, 1] = bad
        with pytest.raises(ValueError):
            abi.path_place_glyphs(line[0], good, line[2], a_types, broken, a_off, *inst)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            abi.path_sample(line[0], good, line[2], [1.0, bad])
        for k in (1, 2, 3):
            hurt = [a.copy() for a in inst]
            hurt[k][1] = bad
            with pytest.raises(ValueError):
                abi.path_place_glyphs(line[0], good, line[2], a_types, a_params, a_off, *hurt)
    with pytest.raises(ValueError):
        abi.path_sample([R.LINE, R.QUAD, R.UNCLOSED], good, line[2], [1.0])
    for glyph in (-1, 4):
        with pytest.raises(ValueError):
            abi.path_place_glyphs(line[0], good, line[2], a_types, a_params, a_off, np.array([0, glyph], dtype=np.int32), *inst[1:])
    # counts that leave 32 bits: 2^15 instances of a glyph of 2^16 segments (the result is never allocated: the call is refused)
    lib, P = abi.load_library(), ctypes.c_void_p
    big_types, big_params = np.zeros(1 << 16, dtype=np.int32), np.zeros((1 << 16, 8))
    big_off, n_inst = np.array([0, 1 << 16], dtype=np.int32), 1 << 15
    glyph, zeros = np.zeros(n_inst, dtype=np.int32), np.zeros(n_inst)
    types, sizes = np.array(line[0], dtype=np.int32), np.array(line[2], dtype=np.int32)
    rc = lib.svgr_path_place_glyphs(ctx.handle, types.ctypes.data_as(P), good.ctypes.data_as(P), sizes.ctypes.data_as(P), 1,
                                    big_types.ctypes.data_as(P), big_params.ctypes.data_as(P), big_off.ctypes.data_as(P), 1,
                                    glyph.ctypes.data_as(P), zeros.ctypes.data_as(P), zeros.ctypes.data_as(P), zeros.ctypes.data_as(P), n_inst,
                                    None, glyph.ctypes.data_as(P), None)
    assert rc == -5
    assert ctx.launches() == before   # nothing was launched by any of these
    # only the length: n = 0
    assert abi.path_sample(line[0], good, line[2])[3] == 20.0 and ctx.launches() > before


def test_public_api(abi):
    from svgrasterize_amd import Path

    assert Path.from_svg("M0,0 L3,0 L3,4 Z").length() == 12.0
    assert Path([]).length() == 0.0
    xy, u, inside = Path.from_svg("M0,0 L3,0 L3,4 Z").point_at([5.0, 13.0, 0.0])
    assert xy.tolist() == [[3, 2], [0, 0], [0, 0]] and u.tolist() == [[0, 1], [-0.6, -0.8], [1, 0]] and inside.tolist() == [True, False, True]
    xy, u, inside = Path.from_svg("M10,0 A10,10 0 0 1 -10,0").point_at(Path.from_svg("M10,0 A10,10 0 0 1 -10,0").length() / 2)
    assert np.allclose(xy, [[0, 10]], atol=1e-4) and np.allclose(u, [[-1, 0]], atol=1e-4) and inside.all()


# ---- end to end ---------------------------------------------------------------------------------------------------------------
SIZE = 256
HEAD = (f'<svg xmlns="http://www.w3.org/2000/svg" xmlns:xlink="http://www.w3.org/1999/xlink" width="{SIZE}" height="{SIZE}">'
        f"<defs>{cases.FONT32}</defs>")
# (the referenced path: its data, its own transform; the textPath's attributes; the run's paint; the text.  The dash lengths keep
#  every dash boundary off the glyphs' corners -- "A" and "I" have sides of 4 and 6 --, the condition of the dasher's own tests: on a
#  corner, rounding decides whether a dash gets a join there, and the two documents measure the sides in different frames)
RUNS = [
    ("wave", "M20,80 C90,40 170,120 236,70", None, 'startOffset="25%" text-anchor="middle"', 'fill="#a00000"', "AOI"),
    ("two", "M16,150 H120 M136,170 L240,140", None, 'startOffset="8"', 'fill="none" stroke="#0000a0" stroke-width="1.5" stroke-dasharray="3.7 2.1"',
     "OIAOI AOI"),
    ("moved", "M0,0 C30,-12 60,12 100,0", "translate(120,232) rotate(-8)", "", 'fill="#007000"', "IOA"),
]
FONT_SIZE = 32.0


def shapes():
    return "".join(f'<path id="{name}" d="{d}" fill="none"{"" if tr is None else f" transform=" + chr(34) + tr + chr(34)}/>'
                   for name, d, tr, _a, _p, _t in RUNS)


def document(tag="textPath"):
    body = "".join(f'<{tag} xlink:href="#{name}" {a} {paint}>{text}</{tag}>' for name, _d, _tr, a, paint, text in RUNS)
    return HEAD + shapes() + f'<text font-family="TQ" font-size="{FONT_SIZE:g}" x="10" y="40">{body}</text></svg>'


def glyph_data(glyph, scale):
    """The glyph's outline as path data in scaled, y-down units relative to its origin -- what the atlas holds.  (Not the font's
    y-up data under a reflecting matrix: the stroker decides between a miter and a bevel by the lengths of the two legs in the
    order it walks them, as the reference does, so the outline of a dash that turns a corner is not the mirror image of its mirror
    image's outline.)"""
    types, params, sizes = glyph.arrays
    words, k = [], 0
    for size in sizes:
        for j in range(int(size)):
            t, q = int(types[k]), [repr(float(v)) for v in params[k] * np.array([scale, -scale] * 4)]
            if j == 0:
                words.append(f"M{q[0]},{q[1]}")
            if t == R.CUBIC:
                words.append(f"C{q[2]},{q[3]} {q[4]},{q[5]} {q[6]},{q[7]}")
            elif t == R.LINE:
                words.append(f"L{q[2]},{q[3]}")
            elif t == R.CLOSED:
                words.append("Z")
            k += 1
    return " ".join(words)


def twin_document():
    """Every visible glyph as its own <path d="outline" transform="matrix(...)">, a rotation and a translation from the
    reference's frame; returns the document and the largest placement tolerance of its glyphs."""
    import svgrasterize_amd as S
    from svgrasterize_amd.svg import parse_transform

    fonts = S.FontsDB()
    S.svg_scene_from_str(HEAD + "</svg>", fonts=fonts)
    font = fonts.resolve("TQ")
    scale = FONT_SIZE / font.units_per_em
    assert scale == 1.0
    body, delta = [], 0.0
    for _name, d, tr, attrs, paint, text in RUNS:
        path = S.Path.from_svg(d)
        if tr is not None:
            path = path.transform(parse_transform(tr))
        types, params, sizes = path._segment_arrays()
        placed, advance = font.str_to_glyphs(text)
        m = R.Measured(types, np.array(params), sizes)
        start = float(m.L) * 0.25 - 0.5 * advance * scale if "25%" in attrs else (8.0 if "8" in attrs else 0.0)
        s_mid = [start + (pen + g.advance / 2) * scale for pen, g in placed]
        detail = {}
        xy, uv, inside, _txy, tol_dir, _L = R.sample(types, np.array(params), sizes, s_mid, detail=detail, measured=m)
        assert detail["clearance"] > cases.CLEARANCE     # which glyphs show is not a matter of rounding
        for (pen, glyph), (px, py), (ux, uy), ins, td in zip(placed, xy, uv, inside, tol_dir):
            if not ins or not glyph.path_source:
                continue
            h = R.LD(glyph.advance) * scale / 2
            # (x, y) of the scaled, y-down outline -> P + u (x - h) + n y, n = (-uy, ux)
            matrix = [ux, uy, -uy, ux, px - ux * h, py - uy * h]
            body.append(f'<path d="{glyph_data(glyph, scale)}" transform="matrix({" ".join(repr(float(v)) for v in matrix)})" {paint}/>')
            delta = max(delta, detail["d_point"] + 40.0 * td + 10 * R.U * SIZE)    # (a lever arm of at most hypot(24, 26) < 40)
    return HEAD + "".join(body) + "</svg>", delta


def load(text):
    import svgrasterize_amd as S

    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        scene, _ids, _size = S.svg_scene_from_str(text)
    assert not caught, [str(w.message) for w in caught]
    return scene


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
    import svgrasterize_amd as S

    S.clear_render_cache()
    twin, delta = twin_document()
    return canvas(load(document())), canvas(load(twin)), canvas(load(document("tspan"))), delta


def test_document_renders_like_its_hand_placed_twin(renders):
    """The tolerance is the placement tolerance carried to coverage.  Both documents place the same outlines, ours by
    svgr_path_place_glyphs, the twin's by a matrix made from the reference's frame, so a control point differs by at most delta =
    d_point + rho d_dir + 10 U Mx (textpath_ref; rho < 40, Mx = 256) plus the twin's own rounding -- six matrix entries rounded to
    doubles and applied in doubles, two products and two sums per coordinate: 8 roundings of values below 2 x 256, 9 U 512.  Points
    of a flattened curve and the corners of a stroke's outline are convex combinations and offsets of control points and move by as
    much (the stroker's and the dasher's own roundings are of the order of U x 256 as well and ride in the factor below).  A pixel's
    coverage is a sum of the signed areas its edges cut off; an edge whose ends move by e changes its term by at most 2 e (a
    pixel is 1 wide and 1 high), and at most 32 edges of these outlines meet one pixel: 64 e.  The paint multiplies by at most 1.
    tol = 64 (delta + 9 U 512)."""
    got, want, _straight, delta = renders
    assert got[..., 3].max() > 0.99
    tol = 64 * (delta + 9 * R.U * 512)
    err = np.abs(got - want)
    print(f"textpath document: max |delta| {err.max():.3e} over {int((err > 0).sum())} differing values; tolerance {tol:.3e}")
    assert err.max() <= tol


def test_text_on_a_path_is_not_straight_text(renders):
    got, _want, straight, _delta = renders
    assert np.abs(got - straight).max() > 0.5
    assert straight[150:, :, 3].max() == 0.0 and got[150:, :, 3].max() > 0.99    # straight text stays on its line at y = 40
