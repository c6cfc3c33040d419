"""The path-pass entries' argument checks on the CPU: svgr_path_dash, svgr_path_markers, svgr_path_sample, svgr_path_place_glyphs,
svgr_glyf_outline(_var), svgr_gvar_deltas and svgr_cff_outline, called raw with ctx = NULL.  Every refusal pinned here happens
before the entry asks for its context, so no device is needed: a valid non-empty input ends in "no context", which proves that
validation passed and nothing else ran.  Statuses and messages are each entry's own (the entry's name in front)."""
import ctypes as C

import numpy as np
import pytest

from svgrasterize_amd import _abi

LINE, QUAD, CUBIC, CLOSED, UNCLOSED = 0, 1, 2, 4, 5
E_INVALID, E_OVERFLOW = -1, -5
PATH_ENTRIES = ["svgr_path_dash", "svgr_path_markers", "svgr_path_sample", "svgr_path_place_glyphs"]


@pytest.fixture(scope="module")
def abi():
    return _abi.load_library()


def _err(abi):
    return abi.svgr_last_error().decode()


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _i32(*v):
    return np.array(v, dtype=np.int32)


def _f64(*v):
    return np.array(v, dtype=np.float64)


def _path():
    """Two subpaths: line, cubic, closing line; line, UNCLOSED."""
    types = _i32(LINE, CUBIC, CLOSED, LINE, UNCLOSED)
    params = np.zeros((5, 8))
    params[0, :4] = [0, 0, 10, 0]
    params[1] = [10, 0, 12, 3, 12, 7, 10, 10]
    params[2, :4] = [10, 10, 0, 0]
    params[3, :4] = [20, 0, 30, 5]
    params[4, :4] = [30, 5, 20, 0]
    return types, params, _i32(3, 2)


def _stroke_out(abi, out):
    n, ns = C.c_int64(), C.c_int64()
    assert abi.svgr_stroke_out_counts(out, C.byref(n), C.byref(ns)) == 0
    types, params, sizes = np.empty(n.value, np.int32), np.empty((n.value, 8)), np.empty(ns.value, np.int32)
    abi.svgr_stroke_out_copy(out, _p(types), _p(params), _p(sizes))
    abi.svgr_stroke_out_free(out)
    return types, params, sizes


class Glyphs:
    """The glyph side of svgr_path_place_glyphs: an atlas of two glyphs (a line and its close; one cubic), two instances."""

    def __init__(self):
        self.atypes = _i32(LINE, CLOSED, CUBIC)
        self.aparams = np.zeros((3, 8))
        self.aparams[0, :4] = [0, 0, 1, 1]
        self.aparams[1, :4] = [1, 1, 0, 0]
        self.aparams[2] = [0, 0, 1, 2, 2, 2, 3, 0]
        self.goff = _i32(0, 2, 3)
        self.n_glyphs = 2
        self.iglyph = _i32(0, 1)
        self.s = _f64(1.0, 4.0)
        self.half = _f64(0.5, 0.5)
        self.dy = _f64(0.0, 1.0)
        self.n_inst = 2
        self.params_out = np.full((3, 8), 7.0)
        self.visible = _i32(9, 9)
        self.total = C.c_double(-1.0)


def _call(abi, entry, types, params, sizes, n_sub=None, out=None, **kw):
    """One of the four path entries on the path (types, params, sizes) with otherwise valid arguments."""
    n_sub = len(sizes) if n_sub is None and sizes is not None else n_sub
    if entry == "svgr_path_dash":
        dashes = kw.get("dashes", _f64(3.0, 2.0))
        res = out if out is not None else C.c_void_p()
        return abi.svgr_path_dash(None, _p(types), _p(params), _p(sizes), n_sub, _p(dashes), 0 if dashes is None else len(dashes),
                                  kw.get("offset", 0.0), 0.0, C.byref(res))
    if entry == "svgr_path_markers":
        res = out if out is not None else C.c_void_p()
        return abi.svgr_path_markers(None, _p(types), _p(params), _p(kw.get("seg_vertex")), _p(sizes), n_sub, C.byref(res))
    if entry == "svgr_path_sample":
        s = kw.get("s", _f64(1.0, 4.0))
        xyuv, inside, total = kw.get("xyuv", np.full((len(s), 4), 7.0)), kw.get("inside", np.full(len(s), 9, np.int32)), kw.get("total", C.c_double(-1))
        return abi.svgr_path_sample(None, _p(types), _p(params), _p(sizes), n_sub, _p(s), len(s), _p(xyuv), _p(inside), C.byref(total))
    g = kw.get("glyphs") or Glyphs()
    return abi.svgr_path_place_glyphs(None, _p(types), _p(params), _p(sizes), n_sub, _p(g.atypes), _p(g.aparams), _p(g.goff), g.n_glyphs,
                                      _p(g.iglyph), _p(g.s), _p(g.half), _p(g.dy), g.n_inst, _p(g.params_out), _p(g.visible),
                                      C.byref(g.total))


# ------------------------------------------------------------------------------------------------------------------------------
# the four entries that take a path
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", PATH_ENTRIES)
def test_path_valid_input_reaches_no_context(abi, entry):
    assert _call(abi, entry, *_path()) == E_INVALID and _err(abi) == f"{entry}: no context"


@pytest.mark.parametrize("entry", PATH_ENTRIES)
def test_path_null_arguments(abi, entry):
    types, params, sizes = _path()
    bad = f"{entry}: bad arguments"
    assert _call(abi, entry, types, params, None, n_sub=2) == E_INVALID and _err(abi) == bad
    assert _call(abi, entry, None, params, sizes) == E_INVALID and _err(abi) == bad
    assert _call(abi, entry, types, None, sizes) == E_INVALID and _err(abi) == bad
    assert _call(abi, entry, types, params, sizes, n_sub=-1) == E_INVALID and _err(abi) == bad
    if entry == "svgr_path_dash":
        assert abi.svgr_path_dash(None, _p(types), _p(params), _p(sizes), 2, None, 0, 0.0, 0.0, None) == E_INVALID and _err(abi) == bad
        assert abi.svgr_path_dash(None, _p(types), _p(params), _p(sizes), 2, None, 2, 0.0, 0.0, C.byref(C.c_void_p())) == E_INVALID
        assert _err(abi) == bad
    elif entry == "svgr_path_markers":
        assert abi.svgr_path_markers(None, _p(types), _p(params), None, _p(sizes), 2, None) == E_INVALID and _err(abi) == bad
    elif entry == "svgr_path_sample":
        s, xyuv, inside = _f64(1.0), np.zeros(4), _i32(0)
        for a in [(None, xyuv, inside), (s, None, inside), (s, xyuv, None)]:
            assert abi.svgr_path_sample(None, _p(types), _p(params), _p(sizes), 2, _p(a[0]), 1, _p(a[1]), _p(a[2]), None) == E_INVALID
            assert _err(abi) == bad
    else:
        for field in ["goff", "iglyph", "s", "half", "dy", "visible", "atypes", "aparams", "params_out"]:
            g = Glyphs()
            setattr(g, field, None)
            assert _call(abi, entry, types, params, sizes, glyphs=g) == E_INVALID and _err(abi) == bad, field


@pytest.mark.parametrize("entry", PATH_ENTRIES)
def test_path_subpath_sizes(abi, entry):
    types, params, _ = _path()
    assert _call(abi, entry, types, params, _i32(3, -1)) == E_INVALID and _err(abi) == f"{entry}: negative subpath size"
    # the sizes alone decide: the segment arrays are one dummy element
    one_t, one_p = _i32(LINE), np.zeros((1, 8))
    assert _call(abi, entry, one_t, one_p, _i32(1 << 29, 1 << 29, 1)) == E_OVERFLOW and _err(abi) == f"{entry}: more than 2^30 segments"


@pytest.mark.parametrize("entry", PATH_ENTRIES)
def test_path_segment_types_and_coordinates(abi, entry):
    types, params, sizes = _path()
    for t in (QUAD, 3, 6, -1):
        bad_t = types.copy()
        bad_t[2] = t
        assert _call(abi, entry, bad_t, params, sizes) == E_INVALID
        assert _err(abi) == f"{entry}: segment 2 has type {t} (quadratics and arcs are converted by the caller)"
    msg = "{}: segment {} has a coordinate that is not finite or beyond 1e150"
    for v in (np.nan, np.inf, 1e155, -np.inf):
        for seg, slot in [(0, 2), (3, 0), (1, 5), (1, 7)]:   # a used slot of a line and of a cubic
            bad_p = params.copy()
            bad_p[seg, slot] = v
            assert _call(abi, entry, types, bad_p, sizes) == E_INVALID and _err(abi) == msg.format(entry, seg), (v, seg, slot)
    ok_p = params.copy()
    ok_p[0, 4:] = np.nan   # slots 4-7 of a line are nobody's
    ok_p[3, 4:] = np.inf
    assert _call(abi, entry, types, ok_p, sizes) == E_INVALID and _err(abi) == f"{entry}: no context"
    edge = params.copy()
    edge[0, 2] = 1e150
    assert _call(abi, entry, types, edge, sizes) == E_INVALID and _err(abi) == f"{entry}: no context"


def test_path_one_empty_subpath_and_null_segments(abi):
    """n_subpaths = 1, size 0, null segment arrays: svgr_path_dash refuses, the other three see an empty path."""
    sizes = _i32(0)
    assert _call(abi, "svgr_path_dash", None, None, sizes) == E_INVALID and _err(abi) == "svgr_path_dash: bad arguments"
    out = C.c_void_p()
    assert _call(abi, "svgr_path_markers", None, None, sizes, out=out) == 0 and out.value
    n = C.c_int64(-1)
    assert abi.svgr_marker_out_counts(out, C.byref(n)) == 0 and n.value == 0
    abi.svgr_marker_out_free(out)
    assert _call(abi, "svgr_path_sample", None, None, sizes) == 0
    assert _call(abi, "svgr_path_place_glyphs", None, None, sizes) == 0


# ------------------------------------------------------------------------------------------------------------------------------
# svgr_path_dash
# ------------------------------------------------------------------------------------------------------------------------------
def test_dash_empty_input(abi):
    out = C.c_void_p()
    assert abi.svgr_path_dash(None, None, None, None, 0, _p(_f64(3.0, 2.0)), 2, 0.0, 0.0, C.byref(out)) == 0 and out.value
    types, params, sizes = _stroke_out(abi, out)
    assert len(types) == 0 and len(params) == 0 and len(sizes) == 0


def test_dash_offset_and_entry_count(abi):
    path = _path()
    for off in (np.nan, np.inf, -np.inf):
        assert _call(abi, "svgr_path_dash", *path, offset=off) == E_INVALID and _err(abi) == "svgr_path_dash: the offset is not finite"
    assert _call(abi, "svgr_path_dash", *path, dashes=np.ones(65)) == E_INVALID
    assert _err(abi) == "svgr_path_dash: 130 dash entries (at most 64, counting an odd list twice)"
    assert _call(abi, "svgr_path_dash", *path, dashes=np.ones(33)) == E_INVALID
    assert _err(abi) == "svgr_path_dash: 66 dash entries (at most 64, counting an odd list twice)"
    assert _call(abi, "svgr_path_dash", *path, dashes=np.ones(66)) == E_INVALID
    assert _err(abi) == "svgr_path_dash: 66 dash entries (at most 64, counting an odd list twice)"
    for n in (32, 64, 31):
        assert _call(abi, "svgr_path_dash", *path, dashes=np.ones(n)) == E_INVALID and _err(abi) == "svgr_path_dash: no context", n


@pytest.mark.parametrize("dashes", [None, [5.0, 0.0], [0.0, 0.0], [3.0, np.nan], [3.0, -1.0], [np.inf, 2.0]],
                         ids=["none", "no-gap", "zeros", "nan", "negative", "inf"])
def test_dash_solid_patterns_return_the_input(abi, dashes):
    types, params, _ = _path()
    sizes = _i32(3, 0, 2)   # (an empty subpath comes back too)
    out = C.c_void_p()
    d = None if dashes is None else np.array(dashes)
    assert _call(abi, "svgr_path_dash", types, params, sizes, dashes=d, out=out) == 0 and out.value
    got = _stroke_out(abi, out)
    assert np.array_equal(got[0], types) and np.array_equal(got[1], params) and np.array_equal(got[2], sizes)
    # a solid pattern is still checked
    assert _call(abi, "svgr_path_dash", types, params, _i32(3, -2), dashes=d) == E_INVALID and "negative subpath size" in _err(abi)


# ------------------------------------------------------------------------------------------------------------------------------
# svgr_path_markers
# ------------------------------------------------------------------------------------------------------------------------------
def test_markers_empty_input(abi):
    out = C.c_void_p()
    assert abi.svgr_path_markers(None, None, None, None, None, 0, C.byref(out)) == 0 and out.value
    n = C.c_int64(-1)
    assert abi.svgr_marker_out_counts(out, C.byref(n)) == 0 and n.value == 0
    abi.svgr_marker_out_free(out)


@pytest.mark.parametrize("with_vertex", [False, True])
def test_markers_no_device_when_no_subpath_has_a_vertex(abi, with_vertex):
    """Every subpath a lone UNCLOSED: the vertex count, made on the host, is 0 and nothing needs a device."""
    types, params, sizes = _i32(UNCLOSED, UNCLOSED), np.zeros((2, 8)), _i32(1, 1)
    out = C.c_void_p()
    sv = _i32(1, 1) if with_vertex else None
    assert _call(abi, "svgr_path_markers", types, params, sizes, seg_vertex=sv, out=out) == 0 and out.value
    n = C.c_int64(-1)
    assert abi.svgr_marker_out_counts(out, C.byref(n)) == 0 and n.value == 0
    abi.svgr_marker_out_free(out)
    # one real segment and a device is asked for -- unless seg_vertex says that no segment ends in a vertex
    types = _i32(LINE, UNCLOSED, UNCLOSED)
    params = np.zeros((3, 8))
    params[0, :4] = [0, 0, 1, 0]
    assert _call(abi, "svgr_path_markers", types, params, _i32(2, 1), seg_vertex=_i32(1, 1, 1) if with_vertex else None) == E_INVALID
    assert _err(abi) == "svgr_path_markers: no context"
    assert _call(abi, "svgr_path_markers", *_path(), seg_vertex=_i32(0, 1, 0, 0, 0) if with_vertex else None) == E_INVALID
    assert _err(abi) == "svgr_path_markers: no context"


# ------------------------------------------------------------------------------------------------------------------------------
# svgr_path_sample / svgr_path_place_glyphs
# ------------------------------------------------------------------------------------------------------------------------------
def test_sample_and_place_arc_lengths(abi):
    path = _path()
    for v in (np.nan, np.inf):
        assert _call(abi, "svgr_path_sample", *path, s=_f64(1.0, v)) == E_INVALID
        assert _err(abi) == "svgr_path_sample: arc length 1 is not finite"
        g = Glyphs()
        g.s[0] = v
        assert _call(abi, "svgr_path_place_glyphs", *path, glyphs=g) == E_INVALID
        assert _err(abi) == "svgr_path_place_glyphs: arc length 0 is not finite"


def test_place_glyph_tables(abi):
    path, entry = _path(), "svgr_path_place_glyphs"
    g = Glyphs()
    g.goff = _i32(1, 2, 3)
    assert _call(abi, entry, *path, glyphs=g) == E_INVALID and _err(abi) == f"{entry}: the glyph offsets do not begin at 0"
    g = Glyphs()
    g.goff = _i32(0, 3, 2)
    assert _call(abi, entry, *path, glyphs=g) == E_INVALID and _err(abi) == f"{entry}: the glyph offsets decrease at glyph 1"
    for bad in (2, -1):
        g = Glyphs()
        g.iglyph = _i32(0, bad)
        assert _call(abi, entry, *path, glyphs=g) == E_INVALID and _err(abi) == f"{entry}: instance 1 names glyph {bad} of 2"
    for field in ("half", "dy"):
        for v in (np.nan, -np.inf):
            g = Glyphs()
            getattr(g, field)[1] = v
            assert _call(abi, entry, *path, glyphs=g) == E_INVALID
            assert _err(abi) == f"{entry}: instance 1 has an advance or a shift that is not finite"
    g = Glyphs()   # the atlas is checked like the path
    g.atypes[2] = QUAD
    assert _call(abi, entry, *path, glyphs=g) == E_INVALID
    assert _err(abi) == f"{entry}: segment 2 has type 1 (quadratics and arcs are converted by the caller)"
    g = Glyphs()
    g.aparams[0, 3] = np.nan
    assert _call(abi, entry, *path, glyphs=g) == E_INVALID and _err(abi) == f"{entry}: segment 0 has a coordinate that is not finite or beyond 1e150"


@pytest.mark.parametrize("n_sub", [0, 2])
def test_sample_and_place_without_segments(abi, n_sub):
    """A path of no segments: the outputs are zeroed, total_length is 0, no context is asked for."""
    sizes = _i32(0, 0) if n_sub else None
    xyuv, inside, total = np.full((2, 4), 7.0), _i32(9, 9), C.c_double(-1.0)
    assert _call(abi, "svgr_path_sample", None, None, sizes, n_sub=n_sub, xyuv=xyuv, inside=inside, total=total) == 0
    assert not xyuv.any() and not inside.any() and total.value == 0.0
    g = Glyphs()
    assert _call(abi, "svgr_path_place_glyphs", None, None, sizes, n_sub=n_sub, glyphs=g) == 0
    assert not g.params_out.any() and not g.visible.any() and g.total.value == 0.0
    # no queries at all: nothing to write, still status 0
    assert abi.svgr_path_sample(None, None, None, None, 0, None, 0, None, None, None) == 0


# ------------------------------------------------------------------------------------------------------------------------------
# svgr_glyf_outline(_var), svgr_gvar_deltas, svgr_cff_outline
# ------------------------------------------------------------------------------------------------------------------------------
class Font:
    """An atlas of one glyph with one contour of three points, placed once."""

    def __init__(self):
        self.xy16 = np.array([[0, 0], [100, 0], [50, 80]], dtype=np.int16)
        self.on = np.array([1, 1, 1], dtype=np.uint8)
        self.xy = self.xy16.astype(np.float64)
        self.kind = np.array([0, 1, 1], dtype=np.uint8)   # MOVE, LINE, LINE
        self.coff, self.goff = _i32(0, 3), _i32(0, 1)
        self.pglyph, self.m = _i32(0), _f64(1, 0, 0, 1, 0, 0)
        self.pen, self.sx, self.sy = _f64(0.0), _f64(1.0), _f64(1.0)
        self.n_parts = 1
        # one tuple that moves point 1
        self.toff, self.scalar, self.poff, self.index = _i32(0, 1), _f64(0.5), _i32(0, 1), _i32(1)
        self.dxy = np.array([[10, -4]], dtype=np.int16)

    def atlas(self, pts, flags):
        return [_p(pts), _p(flags), 3, _p(self.coff), 1, _p(self.goff), 1, _p(self.pglyph), _p(self.m), _p(self.pen), _p(self.sx),
                _p(self.sy), self.n_parts]

    def tuples(self):
        return [_p(self.toff), _p(self.scalar), len(self.scalar), _p(self.poff), _p(self.index), _p(self.dxy), len(self.index)]

    def call(self, abi, entry, out=None):
        res = C.byref(out if out is not None else C.c_void_p())
        if entry == "svgr_glyf_outline":
            return abi.svgr_glyf_outline(None, *self.atlas(self.xy16, self.on), res)
        if entry == "svgr_glyf_outline_var":
            return abi.svgr_glyf_outline_var(None, *self.atlas(self.xy16, self.on), *self.tuples(), res)
        if entry == "svgr_cff_outline":
            return abi.svgr_cff_outline(None, *self.atlas(self.xy, self.kind), res)
        self.deltas = np.full((3, 2), 7.0)
        return abi.svgr_gvar_deltas(None, _p(self.xy16), 3, _p(self.coff), 1, _p(self.goff), 1, *self.tuples(), _p(self.deltas))


FONT_ENTRIES = ["svgr_glyf_outline", "svgr_glyf_outline_var", "svgr_gvar_deltas", "svgr_cff_outline"]


@pytest.mark.parametrize("entry", FONT_ENTRIES)
def test_font_valid_input_reaches_no_context(abi, entry):
    assert Font().call(abi, entry) == E_INVALID and _err(abi) == f"{entry}: no context"


@pytest.mark.parametrize("entry", FONT_ENTRIES)
def test_font_null_arguments(abi, entry):
    bad = f"{entry}: bad arguments"
    if entry != "svgr_gvar_deltas":
        f = Font()
        args = f.atlas(f.xy, f.kind) if entry == "svgr_cff_outline" else f.atlas(f.xy16, f.on)
        fn = getattr(abi, entry)
        tail = f.tuples() if entry == "svgr_glyf_outline_var" else []
        assert fn(None, *args, *tail, None) == E_INVALID and _err(abi) == bad
        for k in (0, 1, 3, 5, 7, 8, 9, 10, 11):   # every array of the atlas and the parts
            a = list(args)
            a[k] = None
            assert fn(None, *a, *tail, C.byref(C.c_void_p())) == E_INVALID and _err(abi) == bad, k
    if entry in ("svgr_gvar_deltas", "svgr_glyf_outline_var"):
        for field in ("toff", "scalar", "poff", "index", "dxy"):
            f = Font()
            setattr(f, field, None)
            f.tuples = lambda f=f: [_p(f.toff), _p(f.scalar), 1, _p(f.poff), _p(f.index), _p(f.dxy), 1]
            assert f.call(abi, entry) == E_INVALID and _err(abi) == bad, field
    if entry == "svgr_gvar_deltas":
        f = Font()
        assert abi.svgr_gvar_deltas(None, None, 3, _p(f.coff), 1, _p(f.goff), 1, *f.tuples(), _p(np.zeros(6))) == E_INVALID and _err(abi) == bad
        assert abi.svgr_gvar_deltas(None, _p(f.xy16), 3, _p(f.coff), 1, _p(f.goff), 1, *f.tuples(), None) == E_INVALID and _err(abi) == bad


@pytest.mark.parametrize("entry", FONT_ENTRIES)
def test_font_empty_input(abi, entry):
    f = Font()
    f.coff, f.goff, f.n_parts = _i32(0), _i32(0), 0
    f.toff, f.scalar, f.poff, f.index, f.dxy = _i32(0), _f64(), _i32(0), _i32(), np.zeros((0, 2), np.int16)
    if entry == "svgr_gvar_deltas":
        assert abi.svgr_gvar_deltas(None, None, 0, _p(f.coff), 0, _p(f.goff), 0, *f.tuples(), None) == 0
        return
    fn, out = getattr(abi, entry), C.c_void_p()
    args = [None, None, 0, _p(f.coff), 0, _p(f.goff), 0, None, None, None, None, None, 0]
    assert fn(None, *args, *(f.tuples() if entry == "svgr_glyf_outline_var" else []), C.byref(out)) == 0 and out.value
    types, params, sizes = _stroke_out(abi, out)
    assert len(types) == 0 and len(params) == 0 and len(sizes) == 0
    # parts of an empty glyph: an atlas with points, nothing to emit, no context
    f, out = Font(), C.c_void_p()
    f.goff, f.pglyph = _i32(0, 0, 1), _i32(0)
    args = f.atlas(f.xy, f.kind) if entry == "svgr_cff_outline" else f.atlas(f.xy16, f.on)
    args[6] = 2
    f.toff = _i32(0, 0, 1)
    assert fn(None, *args, *(f.tuples() if entry == "svgr_glyf_outline_var" else []), C.byref(out)) == 0 and out.value
    assert all(len(a) == 0 for a in _stroke_out(abi, out))


@pytest.mark.parametrize("entry", FONT_ENTRIES)
def test_font_table_errors_carry_the_entry_name(abi, entry):
    f = Font()
    f.coff = _i32(0, 2)
    assert f.call(abi, entry) == E_INVALID and _err(abi) == f"{entry}: contour offsets that do not end at the point count"
    if entry != "svgr_gvar_deltas":
        f = Font()
        f.pglyph = _i32(1)
        assert f.call(abi, entry) == E_INVALID and _err(abi) == f"{entry}: a part's glyph id out of range"
    if entry in ("svgr_gvar_deltas", "svgr_glyf_outline_var"):
        f = Font()
        f.index = _i32(3)
        assert f.call(abi, entry) == E_INVALID and _err(abi) == f"{entry}: a tuple's point index outside its glyph"
        f = Font()
        f.scalar = _f64(1.5)
        assert f.call(abi, entry) == E_INVALID and _err(abi) == f"{entry}: a tuple scalar that is not finite or lies outside [-1, 1]"
    if entry == "svgr_cff_outline":
        f = Font()
        f.kind = np.array([0, 1, 4], dtype=np.uint8)
        assert f.call(abi, entry) == E_INVALID and _err(abi) == f"{entry}: a CURVE without its C1 and C2"
        f = Font()
        f.xy[1, 1] = np.nan
        assert f.call(abi, entry) == E_INVALID and _err(abi) == f"{entry}: a coordinate that is not finite or beyond 1e150"


def test_gvar_zero_tuples_write_zeros_without_a_context(abi):
    f = Font()
    f.toff, f.scalar, f.poff, f.index, f.dxy = _i32(0, 0), _f64(), _i32(0), _i32(), np.zeros((0, 2), np.int16)
    assert f.call(abi, "svgr_gvar_deltas") == 0 and not f.deltas.any()
    # svgr_glyf_outline_var without tuples is svgr_glyf_outline: it needs its device
    assert f.call(abi, "svgr_glyf_outline_var") == E_INVALID and _err(abi) == "svgr_glyf_outline_var: no context"
