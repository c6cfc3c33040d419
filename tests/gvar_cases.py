"""Test-side pieces of the variable-font tests: `add_tables`, which puts further tables into a font made by
`ttf_cases.build_ttf`; writers of ``fvar`` / ``avar`` / ``gvar`` that can be told which encodings to use, so that every path of the
decoder is met; the synthetic variable font; and the arrays of the C ABI (`pack`) with the case list of the delta pass
(`delta_cases`, `fuzz_case`), shared by the host harness test and the GPU test.

A tuple of a glyph is ``dict(peak=(per axis), start=None, end=None, points=None, deltas=[(dx, dy), ...])``: `points` None means
"all points" -- the glyph's points and its four phantom points, so `deltas` has n + 4 entries --, else the increasing point
numbers the deltas belong to.  For the delta pass, a tuple is ``(scalar, [(glyph-local point index, dx, dy), ...])``."""
import struct

import numpy as np

from tests import ttf_cases as T

B = 256   # lanes per workgroup of k_gvar_delta (svgr_gvar_block; the first GPU test asserts it)
E_INVALID, E_OVERFLOW = -1, -5   # SVGR_E_INVALID, SVGR_E_OVERFLOW


def add_tables(ttf: bytes, more: dict) -> bytes:
    """`ttf` with the tables `more`, ``{tag: bytes}``, added (or replaced): the directory is written again."""
    n, = struct.unpack_from(">H", ttf, 4)
    tables = {}
    for i in range(n):
        tag, _sum, off, length = struct.unpack_from(">4sIII", ttf, 12 + 16 * i)
        tables[tag.decode("latin-1")] = ttf[off:off + length]
    tables.update(more)
    tags = sorted(tables)
    out, at = ttf[:4] + struct.pack(">HHHH", len(tags), 0, 0, 0), 12 + 16 * len(tags)
    for tag in tags:
        out += struct.pack(">4sIII", tag.encode("latin-1"), 0, at, len(tables[tag]))
        at += len(T._pad4(tables[tag]))
    return out + b"".join(T._pad4(tables[tag]) for tag in tags)


def _fixed(v: float) -> int:
    return int(round(v * 65536))


def _f2dot14(v: float) -> int:
    return int(round(v * 16384))


def fvar_table(axes, n_instances=1) -> bytes:
    """`axes`: ``[(tag, minimum, default, maximum)]``; `n_instances` named instances (at the defaults) for the reader to skip."""
    out = struct.pack(">HHHHHHHH", 1, 0, 16, 2, len(axes), 20, n_instances, 4 + 4 * len(axes))
    for k, (tag, lo, default, hi) in enumerate(axes):
        out += struct.pack(">4siiiHH", tag.encode("latin-1"), _fixed(lo), _fixed(default), _fixed(hi), 0, 256 + k)
    for k in range(n_instances):
        out += struct.pack(">HH", 300 + k, 0) + b"".join(struct.pack(">i", _fixed(a[2])) for a in axes)
    return out


def avar_table(maps, version=1) -> bytes:
    """`maps`: per axis ``[(from, to)]`` or None (the identity map of three entries)."""
    out = struct.pack(">HHHH", version, 0, 0, len(maps))
    for pairs in maps:
        pairs = pairs or [(-1.0, -1.0), (0.0, 0.0), (1.0, 1.0)]
        out += struct.pack(">H", len(pairs)) + b"".join(struct.pack(">hh", _f2dot14(k), _f2dot14(v)) for k, v in pairs)
    return out


def packed_points(points, words=False) -> bytes:
    """Packed point numbers; `points` None: the single 0 of "all points".  `words` forces 16-bit runs."""
    if points is None:
        return b"\0"
    n = len(points)
    assert 0 < n < 0x8000
    out = bytes([n]) if n < 0x80 else struct.pack(">H", n | 0x8000)
    diffs = [p - q for p, q in zip(points, [0, *points[:-1]])]
    assert all(d >= 0 for d in diffs)
    i = 0
    while i < n:
        wide = words or diffs[i] > 255
        j = i
        while j < n and j - i < 128 and (words or (diffs[j] > 255) == wide):
            j += 1
        run = diffs[i:j]
        out += bytes([(0x80 if wide else 0) | (len(run) - 1)]) + struct.pack(f">{len(run)}{'H' if wide else 'B'}", *run)
        i = j
    return out


def packed_deltas(values, mode="auto") -> bytes:
    """Packed deltas.  `mode`: ``auto`` (zero runs, bytes where they fit, else words), ``no_zero`` (zeros as bytes), ``words``."""
    out, i, n = b"", 0, len(values)

    def kind(v):
        if mode == "words":
            return "w"
        if v == 0 and mode == "auto":
            return "z"
        return "b" if -128 <= v <= 127 else "w"

    while i < n:
        k, j = kind(values[i]), i
        while j < n and j - i < 64 and kind(values[j]) == k:
            j += 1
        run = values[i:j]
        if k == "z":
            out += bytes([0x80 | (len(run) - 1)])
        elif k == "w":
            out += bytes([0x40 | (len(run) - 1)]) + struct.pack(f">{len(run)}h", *run)
        else:
            out += bytes([len(run) - 1]) + struct.pack(f">{len(run)}b", *run)
        i = j
    return out


def gvar_table(n_axes, glyph_tuples, *, long_offsets=False, shared_peaks=True, shared_points=True, point_words=False, delta_mode="auto",
               version=1, axis_count=None, glyph_count=None) -> bytes:
    """The ``gvar`` table of `glyph_tuples`, one list of tuples per glyph.  `shared_peaks`: peaks go to the shared tuples (else
    they are embedded); `shared_points`: a glyph whose tuples all name the same points writes them once.  `axis_count` /
    `glyph_count` write another count into the header than is true."""
    shared = []
    if shared_peaks:
        for tuples in glyph_tuples:
            for t in tuples:
                if tuple(t["peak"]) not in shared:
                    shared.append(tuple(t["peak"]))
    records = []
    for tuples in glyph_tuples:
        if not tuples:
            records.append(b"")
            continue
        same = shared_points and len(tuples) > 1 and all(t.get("points") == tuples[0].get("points") for t in tuples)
        headers, bodies = b"", packed_points(tuples[0].get("points"), point_words) if same else b""
        for t in tuples:
            body = b"" if same else packed_points(t.get("points"), point_words)
            body += packed_deltas([d[0] for d in t["deltas"]], delta_mode) + packed_deltas([d[1] for d in t["deltas"]], delta_mode)
            index = 0 if same else 0x2000
            coords = b""
            if shared_peaks:
                index |= shared.index(tuple(t["peak"]))
            else:
                index |= 0x8000
                coords += struct.pack(f">{n_axes}h", *[_f2dot14(v) for v in t["peak"]])
            if t.get("start") is not None:
                index |= 0x4000
                coords += struct.pack(f">{2 * n_axes}h", *[_f2dot14(v) for v in (*t["start"], *t["end"])])
            headers += struct.pack(">HH", len(body), index) + coords
            bodies += body
        record = struct.pack(">HH", len(tuples) | (0x8000 if same else 0), 4 + len(headers)) + headers + bodies
        records.append(record + b"\0" * (len(record) % 2))
    offsets, at = [0], 0
    for r in records:
        at += len(r)
        offsets.append(at)
    n = len(glyph_tuples)
    offs = struct.pack(f">{n + 1}I", *offsets) if long_offsets else struct.pack(f">{n + 1}H", *[o // 2 for o in offsets])
    shared_at = 20 + len(offs)
    shared_bytes = b"".join(struct.pack(f">{n_axes}h", *[_f2dot14(v) for v in peak]) for peak in shared)
    head = struct.pack(">HHHHIHHI", version, 0, n_axes if axis_count is None else axis_count, len(shared), shared_at,
                       n if glyph_count is None else glyph_count, 1 if long_offsets else 0, shared_at + len(shared_bytes))
    return head + offs + shared_bytes + b"".join(records)


# ----------------------------------------------------------------------------------------------------------------------
# the synthetic variable font of the tests: the glyphs of ttf_cases.GLYPHS on two axes
# ----------------------------------------------------------------------------------------------------------------------
AXES = [("wght", 100.0, 400.0, 900.0), ("wdth", 75.0, 100.0, 125.0)]
AVAR = [[(-1.0, -1.0), (0.0, 0.0), (0.5, 0.25), (1.0, 1.0)], None]


def point_count(glyph) -> int:
    return len(glyph["components"]) if isinstance(glyph, dict) else sum(len(c) for c in glyph)


def _all(glyph, fx, fy, phantom):
    """An "all points" delta list: (fx(x, y), fy(x, y)) per point, then the four phantom deltas."""
    pts = [p for c in glyph for p in c]
    return [(int(fx(x, y)), int(fy(x, y))) for x, y, _on in pts] + list(phantom)


def variations(glyphs=T.GLYPHS) -> list:
    """Per glyph of the synthetic font its tuples.  Bold (wght peak 1) widens, Light (peak -1) thins, wdth scales x; a corner
    tuple (1, 1), an intermediate one on wght, private point subsets that leave most points to interpolation, a varied
    composite, and phantom deltas that move the advance."""
    g = glyphs
    out = [[] for _ in g]
    out[0] = [dict(peak=(1.0, 0.0), points=[0, 2, 5, 8, 9], deltas=[(-20, 0), (25, 10), (15, -8), (0, 0), (40, 0)])]   # 8, 9: phantoms
    out[1] = [dict(peak=(0.0, 1.0), points=[1], deltas=[(60, 0)]), dict(peak=(0.0, -1.0), points=[0, 1], deltas=[(5, 0), (-40, 0)])]
    out[2] = [
        dict(peak=(1.0, 0.0), points=None, deltas=_all(g[2], lambda x, y: (x - 350) // 10, lambda x, y: y // 70, [(0, 0), (55, 0), (0, 0), (0, 0)])),
        dict(peak=(-1.0, 0.0), points=[0, 2, 4, 5, 7, 9, 11], deltas=[(12, 0), (-12, 0), (-9, 14), (9, 14), (6, -5), (0, 3), (-30, 0)]),
        dict(peak=(0.0, 1.0), points=[1, 3, 6, 11], deltas=[(0, 0), (130, 0), (-10, 0), (150, 0)]),
        dict(peak=(1.0, 1.0), points=[1, 8], deltas=[(7, -3), (-300, 200)]),
        dict(peak=(0.5, 0.0), start=(0.25, 0.0), end=(0.75, 0.0), points=[1, 9], deltas=[(0, 33), (4, -17)]),
    ]
    out[3] = [
        dict(peak=(1.0, 0.0), points=[1, 5, 8, 10, 13], deltas=[(-30, 0), (30, 0), (40, 35), (-40, -35), (44, 0)]),
        dict(peak=(0.0, 1.0), points=[1, 5, 8, 10, 13], deltas=[(0, 0), (140, 0), (20, 0), (110, 0), (150, 0)]),
        dict(peak=(0.0, -1.0), points=[1, 5, 8, 10, 13], deltas=[(0, 0), (-130, 0), (-20, 0), (-100, 0), (-140, 0)]),
    ]
    out[4] = [dict(peak=(1.0, 0.0), points=[5], deltas=[(0, -60)]),
              dict(peak=(0.3, 0.0), start=(0.0, 0.0), end=(1.0, 0.0), points=[0, 4, 8, 12], deltas=[(-300, 0), (260, 1), (300, 0), (33, 0)])]
    out[5] = [dict(peak=(1.0, -1.0), points=[3], deltas=[(11, 13)])]
    out[6] = [dict(peak=(1.0, 0.0), points=[1, 3], deltas=[(35, 42), (44, 0)]),
              dict(peak=(0.0, 1.0), points=None, deltas=[(0, 0), (70, 5), (0, 0), (150, 0), (0, 0), (0, 0)])]
    out[7] = [dict(peak=(0.0, 1.0), points=[0, 1], deltas=[(-25, 10), (60, -12)])]
    out[10] = [dict(peak=(1.0, 0.0), points=[0, 1, 2, 3, 4], deltas=[(-35, 0), (35, 0), (35, 0), (-35, 0), (9, 9)])]
    return out


def synthetic_var_ttf(var=None, *, with_avar=True, avar_version=1, with_gvar=True, gvar_options=None, **options) -> bytes:
    """`ttf_cases.synthetic_ttf` with ``fvar``, ``avar`` and ``gvar``; `gvar_options` are `gvar_table`'s."""
    more = {"fvar": fvar_table(AXES)}
    if with_avar:
        more["avar"] = avar_table(AVAR, avar_version)
    if with_gvar:
        more["gvar"] = gvar_table(len(AXES), variations() if var is None else var, **(gvar_options or {}))
    options.setdefault("family", "VarSynth")
    return add_tables(T.synthetic_ttf(**options), more)


# ----------------------------------------------------------------------------------------------------------------------
# the delta pass: the arrays of the C ABI, and the cases
# ----------------------------------------------------------------------------------------------------------------------
def pack(atlas, tuples):
    """The arrays of svgr_gvar_deltas.  `atlas`: glyphs as lists of contours of ``(x, y, on)``; `tuples`: per glyph
    ``[(scalar, [(local index, dx, dy)])]``."""
    contour_off, glyph_contour_off = [0], [0]
    for g in atlas:
        for c in g:
            contour_off.append(contour_off[-1] + len(c))
        glyph_contour_off.append(len(contour_off) - 1)
    pts = [p for g in atlas for c in g for p in c]
    glyph_tuple_off, scalars, tuple_pt_off, index, dxy = [0], [], [0], [], []
    for g in tuples:
        for s, entries in g:
            scalars.append(s)
            index.extend(e[0] for e in entries)
            dxy.extend((e[1], e[2]) for e in entries)
            tuple_pt_off.append(len(index))
        glyph_tuple_off.append(len(scalars))
    return dict(
        pt_xy=np.array([[p[0], p[1]] for p in pts], dtype=np.int16).reshape(-1, 2),
        contour_off=np.array(contour_off, dtype=np.int32), glyph_contour_off=np.array(glyph_contour_off, dtype=np.int32),
        glyph_tuple_off=np.array(glyph_tuple_off, dtype=np.int32), tuple_scalar=np.array(scalars, dtype=np.float64),
        tuple_pt_off=np.array(tuple_pt_off, dtype=np.int32), tp_index=np.array(index, dtype=np.int32),
        tp_dxy=np.array(dxy, dtype=np.int16).reshape(-1, 2))


def points_of(atlas) -> int:
    return sum(len(c) for g in atlas for c in g)


def touch(rng, glyph, k=None, lo=-300, hi=300):
    """A tuple's entries on `glyph`: `k` random points (None: a random number of them, at least one when there is a point)."""
    n = sum(len(c) for c in glyph)
    if n == 0:
        return []
    k = int(rng.integers(1, n + 1)) if k is None else min(k, n)
    chosen = sorted(rng.choice(n, size=k, replace=False).tolist())
    return [(int(i), int(rng.integers(lo, hi + 1)), int(rng.integers(lo, hi + 1))) for i in chosen]


def _scalar(rng) -> float:
    return float(rng.choice([1.0, -1.0, 0.5, 0.3, 1.0 / 3, -0.7, float(rng.uniform(-1, 1))]))


def _total(rng, total):
    """An atlas of `total` points -- a glyph of two contours, an empty glyph, a glyph for the rest -- with tuples on both."""
    a = [T.ring(rng, 37), T.ring(rng, 63)]
    rest = total - 100
    b = [T.ring(rng, rest - rest // 2), T.ring(rng, rest // 2)]
    atlas = [a, [], b]
    tuples = [[(_scalar(rng), touch(rng, a, 9)), (_scalar(rng), touch(rng, a, 30))], [], [(_scalar(rng), touch(rng, b, 11)), (_scalar(rng), touch(rng, b))]]
    assert points_of(atlas) == total
    return atlas, tuples


def _axis_glyph():
    """One contour for the branches of the interpolation rule, both axes at once (x and y take different branches)."""
    #        0 touched      1 below/above      2 between        3 on a reference   4 touched (descending pair with 0)   5 beyond
    return [[(100, -50, True), (40, 700, False), (250, 10, True), (100, 300, True), (300, 300, False), (999, -400, True)]]


def delta_cases(b=B):
    """[(name, atlas, tuples)]: the seams of the launch, and every branch of the delta rule."""
    rng = np.random.default_rng(20261020)
    cases = [(f"points_{name}", *_total(rng, total)) for name, total in (("B-1", b - 1), ("B", b), ("B+1", b + 1), ("2B+1", 2 * b + 1))]
    big = [T.ring(rng, b + 44), T.ring(rng, 7)]
    cases.append(("glyph_larger_than_block", [big], [[(0.75, touch(rng, big, 17)), (-0.5, touch(rng, big, 3))]]))
    # a contour over the workgroup boundary whose only touched points lie behind it (the lanes in front wrap backwards) ...
    first, second = T.ring(rng, b - 10), T.ring(rng, 40)
    cases.append(("straddle_touched_behind", [[first, second]], [[(1.0, [(b + 3, 40, -30), (b + 9, -25, 60)])]]))
    # ... and in front of it (the lanes behind wrap forwards)
    cases.append(("straddle_touched_in_front", [[first, second]], [[(1.0, [(b - 9, 40, -30), (b - 4, -25, 60)])]]))
    ring6 = T.ring(rng, 6)
    for k in (0, 1, 2, 6):
        cases.append((f"contour_touched_{k}", [[T.ring(rng, 5), ring6]], [[(0.6, [(0, 3, 4)] + [(5 + i, 10 * i - 7, 5 - 9 * i) for i in range(k)])]]))
    cases.append(("single_point_contours", [[[(5, 5, True)], [(9, 9, False)], T.ring(rng, 4)]], [[(1.0, [(0, 8, -8), (3, 1, 2)]), (0.5, [(1, -6, 6)])]]))
    g3 = T.ring(rng, 5)
    cases.append(("empty_glyph_between", [[T.ring(rng, 5)], [], [g3]], [[(1.0, [(1, 5, 5)])], [], [(1.0, [(2, -9, 9)])]]))
    # the second glyph's local indices are the first glyph's atlas indices: a forgotten base reads the wrong points
    ga, gb = [T.ring(rng, 7)], [T.ring(rng, 4), T.ring(rng, 6)]
    cases.append(("glyph_base", [ga, gb], [[(1.0, [(1, 10, 20), (5, -30, 40)])], [(0.5, [(1, 11, 21), (5, -31, 41), (8, 7, 7)])]]))
    g5 = [T.ring(rng, 9), T.ring(rng, 5)]
    cases.append(("no_tuple_next_to_five", [[T.ring(rng, 8)], g5], [[], [(_scalar(rng), touch(rng, g5)) for _ in range(5)]]))
    cases.append(("disjoint_tuples", [[T.ring(rng, 10)]], [[(1.0, [(0, 5, 6), (3, -7, 8)]), (-0.25, [(5, 9, -10), (8, 11, 12)])]]))
    axis = _axis_glyph()
    cases.append(("axis_branches", [axis], [[(1.0, [(0, 10, -20), (4, -30, 40)]), (0.5, [(0, -30, 40), (4, 10, -20)])]]))
    # equal reference coordinates: x of 0 and 3 are equal (100), with equal and with different deltas
    # and y of 3 and 4 (300)
    cases.append(("equal_references", [axis], [[(1.0, [(0, 12, 5), (3, 12, 9)]), (1.0, [(0, 12, 5), (3, -4, 5)]), (0.5, [(3, 1, 9), (4, 2, 9)]),
                                                (-1.0, [(3, 1, 9), (4, 2, -3)])]]))
    extreme = [[(-32767, 32767, True), (0, 1, False), (32767, -32767, True), (32766, -32766, False), (-1, -2, True)]]
    cases.append(("extremes", [extreme], [[(1.0, [(0, 32767, -32767), (2, -32767, 32767)]), (-1.0, [(0, -32767, -32767), (2, 32767, 32767)])]]))
    return cases


def rotated_parts(atlas):
    """Parts over `atlas` for the outline comparison: every non-empty glyph plain, mirrored and turned."""
    cos, sin = T.f2dot14(np.cos(0.5)), T.f2dot14(np.sin(0.5))
    parts = []
    for g, glyph in enumerate(atlas):
        parts.append((g, T.IDENTITY, 10.0 * g, 0.0234375, -0.0234375))
        parts.append((g, (cos, sin, -sin, cos, 120.0, -35.0), 300.0, 0.0234375, 0.0234375))
    return parts


def fuzz_case(seed: int):
    """A random atlas (1-6 glyphs, 0-5 contours of 1-40 points, coordinates over a small range so that equal coordinates are
    common) with 0-5 tuples per glyph."""
    rng = np.random.default_rng(seed)
    span = int(rng.choice([3, 50, 2000]))

    def contour(n):
        return [(int(x), int(y), bool(f)) for x, y, f in zip(rng.integers(-span, span + 1, n), rng.integers(-span, span + 1, n), rng.integers(0, 2, n))]

    atlas = [[contour(int(rng.integers(1, 41))) for _ in range(int(rng.integers(0, 6)))] for _ in range(int(rng.integers(1, 7)))]
    tuples = [[(_scalar(rng), touch(rng, g, lo=-span, hi=span)) for _ in range(int(rng.integers(0, 6)))] if points_of([g]) else [] for g in atlas]
    return atlas, tuples


def refusals(good):
    """[(what, arrays, status)]: every refusal of gvar_tables, made from the good arrays of a case."""
    def changed(key, index, value):
        a = {k: v.copy() for k, v in good.items()}
        a[key].reshape(-1)[index] = value
        return a

    last_t, last_p = int(good["glyph_tuple_off"][-1]), int(good["tuple_pt_off"][-1])
    swapped = {k: v.copy() for k, v in good.items()}
    swapped["tp_index"][[0, 1]] = swapped["tp_index"][[1, 0]]
    return [
        ("glyph_tuple_off decreases", changed("glyph_tuple_off", 1, 99), E_INVALID),
        ("glyph_tuple_off does not begin at 0", changed("glyph_tuple_off", 0, 1), E_INVALID),
        ("glyph_tuple_off does not end at the count", changed("glyph_tuple_off", -1, last_t - 1), E_INVALID),
        ("tuple_pt_off decreases", changed("tuple_pt_off", 1, 9999), E_INVALID),
        ("tuple_pt_off does not begin at 0", changed("tuple_pt_off", 0, 1), E_INVALID),
        ("tuple_pt_off does not end at the count", changed("tuple_pt_off", -1, last_p - 1), E_INVALID),
        ("contour_off does not end at the count", changed("contour_off", -1, int(good["contour_off"][-1]) + 1), E_INVALID),
        ("glyph_contour_off decreases", changed("glyph_contour_off", 1, 99), E_INVALID),
        ("tp_index repeats", changed("tp_index", 1, int(good["tp_index"][0])), E_INVALID),
        ("tp_index decreases", swapped, E_INVALID),
        ("tp_index negative", changed("tp_index", 0, -1), E_INVALID),
        ("tp_index beyond its glyph", changed("tp_index", int(good["tuple_pt_off"][1]) - 1, 100), E_INVALID),
        ("scalar nan", changed("tuple_scalar", 0, np.nan), E_INVALID),
        ("scalar inf", changed("tuple_scalar", 1, -np.inf), E_INVALID),
        ("scalar beyond 1", changed("tuple_scalar", 0, 1.0000001), E_INVALID),
    ]
