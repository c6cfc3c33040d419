"""Test-side pieces of the TrueType tests: `build_ttf`, a small sfnt writer that can be told which encodings to use so that
every path of the decoder is met, the arrays of the C ABI (`pack`) and the case list of the outline pass (`outline_cases`,
`fuzz_case`), shared by the host harness test and the GPU test.

A glyph is a list of contours, a contour a list of ``(x, y, on)``; a composite glyph is a ``dict(components=[...])`` whose
components are ``dict(glyph=, dx=0, dy=0, scale=None, words=None, match=None)``: `scale` None, a number, ``(sx, sy)`` or
``(xscale, scale01, scale10, yscale)`` -- numbers are written as F2Dot14, give values that are k / 16384 --, `words` forces 16-bit
arguments (None: when they are needed), `match` = ``(parent point, child point)`` places by point matching instead of an offset."""
import struct

import numpy as np

B = 256   # lanes per workgroup of k_glyf_emit (svgr_glyf_block; the first GPU test asserts it)

ON, X_SHORT, Y_SHORT, REPEAT, X_SAME, Y_SAME = 1, 2, 4, 8, 16, 32
WORDS, XY, SCALE, MORE, XY_SCALE, TWO_BY_TWO = 0x1, 0x2, 0x8, 0x20, 0x40, 0x80


def f2dot14(v: float) -> float:
    """`v` rounded to what an F2Dot14 holds."""
    return round(v * 16384) / 16384.0


def _pad4(b: bytes) -> bytes:
    return b + b"\0" * (-len(b) % 4)


def _simple_glyph(contours, repeat, short, same) -> bytes:
    pts = [p for c in contours for p in c]
    if not pts:
        return b""
    ends, n = [], 0
    for c in contours:
        assert len(c) >= 1
        n += len(c)
        ends.append(n - 1)
    xs, ys = [p[0] for p in pts], [p[1] for p in pts]
    flags, xb, yb = [], b"", b""
    px = py = 0
    for x, y, on in pts:
        f = ON if on else 0
        dx, dy = x - px, y - py
        px, py = x, y
        if dx == 0 and same:
            f |= X_SAME
        elif short and -256 < dx < 256:
            f |= X_SHORT | (X_SAME if dx >= 0 else 0)
            xb += bytes([abs(dx)])
        else:
            xb += struct.pack(">h", dx)
        if dy == 0 and same:
            f |= Y_SAME
        elif short and -256 < dy < 256:
            f |= Y_SHORT | (Y_SAME if dy >= 0 else 0)
            yb += bytes([abs(dy)])
        else:
            yb += struct.pack(">h", dy)
        flags.append(f)
    fb, i = b"", 0
    while i < len(flags):
        j = i
        while repeat and j + 1 < len(flags) and flags[j + 1] == flags[i] and j - i < 255:
            j += 1
        if j > i:
            fb += bytes([flags[i] | REPEAT, j - i])
        else:
            fb += bytes([flags[i]])
        i = j + 1
    instructions = b"\xb0\x00"   # (two bytes the decoder has to step over)
    head = struct.pack(">hhhhh", len(contours), min(xs), min(ys), max(xs), max(ys))
    return head + struct.pack(f">{len(ends)}H", *ends) + struct.pack(">H", len(instructions)) + instructions + fb + xb + yb


def _composite_glyph(components) -> bytes:
    out = struct.pack(">hhhhh", -1, 0, 0, 0, 0)
    for k, comp in enumerate(components):
        flags = MORE if k + 1 < len(components) else 0
        match = comp.get("match")
        a1, a2 = match if match is not None else (comp.get("dx", 0), comp.get("dy", 0))
        if match is None:
            flags |= XY
        words = comp.get("words")
        fits = (0 <= a1 < 256 and 0 <= a2 < 256) if match is not None else (-128 <= a1 < 128 and -128 <= a2 < 128)
        if words is None:
            words = not fits
        assert words or fits
        if words:
            flags |= WORDS
        scale = comp.get("scale")
        if scale is not None:
            scale = (scale,) if isinstance(scale, (int, float)) else tuple(scale)
            flags |= {1: SCALE, 2: XY_SCALE, 4: TWO_BY_TWO}[len(scale)]
        out += struct.pack(">HH", flags, comp["glyph"])
        if words:
            out += struct.pack(">hh" if match is None else ">HH", a1, a2)
        else:
            out += struct.pack(">bb" if match is None else ">BB", a1, a2)
        if scale is not None:
            out += struct.pack(f">{len(scale)}h", *[round(v * 16384) for v in scale])
    return out


def _runs(cmap):
    """[(first code, last code, first glyph)] of runs of consecutive codes with consecutive glyph ids."""
    runs = []
    for code in sorted(cmap):
        gid = cmap[code]
        if runs and runs[-1][1] + 1 == code and runs[-1][2] + (code - runs[-1][0]) == gid:
            runs[-1][1] = code
        else:
            runs.append([code, code, gid])
    return runs


def _cmap4(cmap, by_array) -> bytes:
    runs = [r for r in _runs(cmap) if r[0] < 0xFFFF]
    if by_array:   # one segment per run of consecutive codes, every glyph id through glyphIdArray
        merged = []
        for first, last, _g in runs:
            if merged and merged[-1][1] + 1 == first:
                merged[-1][1] = last
            else:
                merged.append([first, last])
        segs = [(first, last, 0, None) for first, last in merged]
    else:
        segs = [(first, last, (gid - first) & 0xFFFF, 0) for first, last, gid in runs]
    segs.append((0xFFFF, 0xFFFF, 1, 0))
    n = len(segs)
    array, offsets = [], []
    for i, (first, last, _delta, off) in enumerate(segs):
        if off is None:
            offsets.append(2 * (n - i) + 2 * len(array))
            array.extend(cmap[c] for c in range(first, last + 1))
        else:
            offsets.append(0)
    search = 2 * (1 << (n.bit_length() - 1))
    body = struct.pack(">HHHH", 2 * n, search, n.bit_length() - 1, 2 * n - search)
    body += struct.pack(f">{n}H", *[s[1] for s in segs]) + b"\0\0" + struct.pack(f">{n}H", *[s[0] for s in segs])
    body += struct.pack(f">{n}H", *[s[2] for s in segs]) + struct.pack(f">{n}H", *offsets) + struct.pack(f">{len(array)}H", *array)
    return struct.pack(">HHH", 4, 6 + len(body), 0) + body


def _cmap12(cmap) -> bytes:
    runs = _runs(cmap)
    body = b"".join(struct.pack(">III", first, last, gid) for first, last, gid in runs)
    return struct.pack(">HHIII", 12, 0, 16 + len(body), 0, len(runs)) + body


def build_ttf(glyphs, cmap, advances, kern=None, *, family="Synthetic", units_per_em=1000, ascent=800, descent=-200, weight=400,
              italic=False, mac_style=0, loca_long=False, cmap_format=4, cmap_by_array=False, cmap_platform=(3, 1), extra_cmap=(),
              name_platform=3, with_os2=True, n_hmetrics=None, flag_repeat=True, short_vectors=True, same_as_previous=True,
              kern_coverage=0x0001, sfnt=b"\x00\x01\x00\x00", drop=()) -> bytes:
    """The bytes of a TrueType font: `glyphs` (above), `cmap` ``{code: glyph id}``, `advances` per glyph, `kern`
    ``{(left, right): value}``.  `extra_cmap`: further ``(platform, encoding, format, {code: glyph})`` subtables, written in front of
    the main one.  `name_platform` 3, 1 or None (no name table); `n_hmetrics` below the glyph count needs equal advances behind
    it; `drop`: tables to leave out."""
    n = len(glyphs)
    assert len(advances) == n
    records = [_pad4(_composite_glyph(g["components"]) if isinstance(g, dict) else _simple_glyph(g, flag_repeat, short_vectors, same_as_previous))
               for g in glyphs]
    loca, at = [0], 0
    for r in records:
        at += len(r)
        loca.append(at)
    tables = {"glyf": b"".join(records)}
    tables["loca"] = struct.pack(f">{n + 1}I", *loca) if loca_long else struct.pack(f">{n + 1}H", *[v // 2 for v in loca])
    head = bytearray(54)
    struct.pack_into(">IIII", head, 0, 0x00010000, 0x00010000, 0, 0x5F0F3CF5)
    struct.pack_into(">H", head, 18, units_per_em)
    struct.pack_into(">H", head, 44, mac_style)
    struct.pack_into(">h", head, 50, 1 if loca_long else 0)
    tables["head"] = bytes(head)
    maxp = bytearray(32)
    struct.pack_into(">IH", maxp, 0, 0x00010000, n)
    tables["maxp"] = bytes(maxp)
    nh = n if n_hmetrics is None else n_hmetrics
    assert 1 <= nh <= n and all(a == advances[nh - 1] for a in advances[nh:])
    hhea = bytearray(36)
    struct.pack_into(">Ihh", hhea, 0, 0x00010000, ascent, descent)
    struct.pack_into(">H", hhea, 34, nh)
    tables["hhea"] = bytes(hhea)
    tables["hmtx"] = b"".join(struct.pack(">Hh", a, 0) for a in advances[:nh]) + struct.pack(f">{n - nh}h", *([0] * (n - nh)))
    subtables = [(p, e, _cmap4(c, False) if f == 4 else _cmap12(c)) for p, e, f, c in extra_cmap]
    subtables.append((*cmap_platform, _cmap4(cmap, cmap_by_array) if cmap_format == 4 else _cmap12(cmap)))
    cm, at = struct.pack(">HH", 0, len(subtables)), 4 + 8 * len(subtables)
    for p, e, body in subtables:
        cm += struct.pack(">HHI", p, e, at)
        at += len(body)
    tables["cmap"] = cm + b"".join(body for _p, _e, body in subtables)
    if name_platform is not None:
        text = family.encode("utf-16-be") if name_platform == 3 else family.encode("latin-1")
        rec = (3, 1, 0x409) if name_platform == 3 else (1, 0, 0)
        tables["name"] = struct.pack(">HHH", 0, 1, 18) + struct.pack(">HHHHHH", *rec, 1, len(text), 0) + text
    if with_os2:
        os2 = bytearray(96)
        struct.pack_into(">H", os2, 4, weight)
        struct.pack_into(">H", os2, 62, 1 if italic else 0)
        tables["OS/2"] = bytes(os2)
    if kern:
        pairs = sorted(kern.items())
        body = struct.pack(">HHHH", len(pairs), 0, 0, 0) + b"".join(struct.pack(">HHh", left, right, v) for (left, right), v in pairs)
        tables["kern"] = struct.pack(">HH", 0, 1) + struct.pack(">HHH", 0, 6 + len(body), kern_coverage) + body
    for tag in drop:
        tables.pop(tag, None)
    tags = sorted(tables)
    out, at = sfnt + struct.pack(">HHHH", len(tags), 0, 0, 0), 12 + 16 * len(tags)
    for tag in tags:
        out += struct.pack(">4sIII", tag.encode("latin-1"), 0, at, len(tables[tag]))
        at += len(_pad4(tables[tag]))
    return out + b"".join(_pad4(tables[tag]) for tag in tags)


def table_bounds(data: bytes) -> list:
    """Every table's begin and end in the file, sorted."""
    n, = struct.unpack_from(">H", data, 4)
    out = set()
    for i in range(n):
        _tag, _sum, off, length = struct.unpack_from(">4sIII", data, 12 + 16 * i)
        out.update((off, off + length))
    return sorted(out)


# ----------------------------------------------------------------------------------------------------------------------
# the outline pass: the arrays of the C ABI, and the cases
# ----------------------------------------------------------------------------------------------------------------------
IDENTITY = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)


def pack(atlas, parts):
    """The arrays of svgr_glyf_outline.  `atlas`: glyphs as lists of contours; `parts`: ``[(glyph index, (m00, m01, m10, m11,
    dx, dy), pen, sx, sy)]``."""
    pts = [p for g in atlas for c in g for p in c]
    contour_off, glyph_contour_off = [0], [0]
    for g in atlas:
        for c in g:
            contour_off.append(contour_off[-1] + len(c))
        glyph_contour_off.append(len(contour_off) - 1)
    return dict(
        pt_xy=np.array([[p[0], p[1]] for p in pts], dtype=np.int16).reshape(-1, 2),
        pt_on=np.array([1 if p[2] else 0 for p in pts], dtype=np.uint8),
        contour_off=np.array(contour_off, dtype=np.int32),
        glyph_contour_off=np.array(glyph_contour_off, dtype=np.int32),
        part_glyph=np.array([p[0] for p in parts], dtype=np.int32),
        part_m=np.array([p[1] for p in parts], dtype=np.float64).reshape(-1, 6),
        part_pen=np.array([p[2] for p in parts], dtype=np.float64),
        part_sx=np.array([p[3] for p in parts], dtype=np.float64),
        part_sy=np.array([p[4] for p in parts], dtype=np.float64),
    )


def lanes(atlas, parts) -> int:
    return sum(sum(len(c) for c in atlas[p[0]]) for p in parts)


def ring(rng, n, on=None):
    """A contour of n random points; `on`: the flags (None: random)."""
    flags = rng.integers(0, 2, n).tolist() if on is None else list(on)
    return [(int(x), int(y), bool(f)) for x, y, f in zip(rng.integers(-2000, 2000, n), rng.integers(-2000, 2000, n), flags)]


def _part(rng, g, m=IDENTITY, mirror=True):
    return (g, m, float(rng.integers(0, 5000)), 0.0234375, -0.0234375 if mirror else 0.0234375)


def _total(rng, total):
    """An atlas and parts with `total` lanes: one glyph of two contours twice, one glyph for the rest."""
    a = [ring(rng, 37), ring(rng, 63)]
    rest = total - 200
    b = [ring(rng, rest - rest // 2), ring(rng, rest // 2)] if rest >= 2 else [ring(rng, rest)]
    atlas, parts = [a, b], [_part(rng, 0), _part(rng, 1), _part(rng, 0)]
    assert lanes(atlas, parts) == total
    return atlas, parts


def outline_cases(b=B):
    """[(name, atlas, parts)]: the seams of the launch, and every branch of the outline rule."""
    rng = np.random.default_rng(20261019)
    cos, sin = f2dot14(np.cos(0.5)), f2dot14(np.sin(0.5))
    rotated = (cos, sin, -sin, cos, 120.0, -35.0)
    cases = [(f"lanes_{name}", *_total(rng, total)) for name, total in (("B-1", b - 1), ("B", b), ("B+1", b + 1), ("2B+1", 2 * b + 1))]
    cases.append(("contour_straddles_block", [[ring(rng, b - 6)], [ring(rng, 20)]], [_part(rng, 0), _part(rng, 1)]))
    cases.append(("glyph_larger_than_block", [[ring(rng, b + 44), ring(rng, 7)]], [_part(rng, 0)]))
    tiny = [[(5, 5, True)], [(0, 0, True), (10, 20, True)], [(0, 0, True), (10, 20, False)], [(3, 4, False), (10, 20, True)],
            [(3, 4, False), (11, 21, False)], [(7, 7, False)]]
    cases.append(("one_and_two_points", [tiny], [_part(rng, 0)]))
    cases.append(("only_single_points", [[[(5, 5, True)], [(6, 6, False)]], [ring(rng, 5)]], [_part(rng, 0), _part(rng, 1), _part(rng, 0)]))
    cases.append(("all_off_4", [[ring(rng, 4, [0, 0, 0, 0])]], [_part(rng, 0)]))
    cases.append(("first_off_last_on", [[ring(rng, 5, [0, 1, 1, 0, 1])]], [_part(rng, 0)]))
    cases.append(("first_off_last_off", [[ring(rng, 5, [0, 1, 1, 0, 0])]], [_part(rng, 0)]))
    cases.append(("first_on_last_off", [[ring(rng, 5, [1, 1, 0, 1, 0])]], [_part(rng, 0)]))
    cases.append(("three_off_in_a_row", [[ring(rng, 7, [1, 0, 0, 0, 1, 1, 0])]], [_part(rng, 0)]))
    glyph, space = [ring(rng, 9), ring(rng, 4)], []
    cases.append(("space_first", [space, glyph], [_part(rng, 0), _part(rng, 1), _part(rng, 1)]))
    cases.append(("space_middle", [glyph, space], [_part(rng, 0), _part(rng, 1), _part(rng, 1), _part(rng, 0)]))
    cases.append(("space_last", [glyph, space], [_part(rng, 0), _part(rng, 0), _part(rng, 1)]))
    cases.append(("same_glyph_B+1_parts", [[ring(rng, 3), ring(rng, 2)]], [_part(rng, 0) for _ in range(b + 1)]))
    cases.append(("mirrored_and_not", [glyph], [_part(rng, 0, mirror=True), _part(rng, 0, mirror=False)]))
    cases.append(("rotated_part", [glyph, [ring(rng, 6)]], [_part(rng, 0, rotated), _part(rng, 1), _part(rng, 1, (0.5, 0.0, 0.0, -0.75, -8.0, 3.0))]))
    return cases


def fuzz_case(seed: int):
    """A random atlas (1-6 glyphs, 0-5 contours, 1-40 points, random flags) and a random part list."""
    rng = np.random.default_rng(seed)
    atlas = [[ring(rng, int(rng.integers(1, 41))) for _ in range(int(rng.integers(0, 6)))] for _ in range(int(rng.integers(1, 7)))]
    parts = []
    for _ in range(int(rng.integers(1, 13))):
        m = IDENTITY if rng.integers(0, 2) else tuple(f2dot14(v) for v in rng.uniform(-2, 2, 4)) + tuple(float(v) for v in rng.integers(-500, 500, 2))
        parts.append((int(rng.integers(0, len(atlas))), m, float(rng.uniform(0, 8000)), float(rng.uniform(0.001, 0.1)),
                      float(rng.uniform(-0.1, 0.1))))
    return atlas, parts


# ----------------------------------------------------------------------------------------------------------------------
# the synthetic font of the tests
# ----------------------------------------------------------------------------------------------------------------------
T, F = True, False
COS, SIN = f2dot14(np.cos(0.4)), f2dot14(np.sin(0.4))
GLYPHS = [
    # 0 .notdef: a frame (lines only; every x delta of the second contour is 0 or long)
    [[(50, 0, T), (450, 0, T), (450, 700, T), (50, 700, T)], [(100, 50, T), (100, 650, T), (400, 650, T), (400, 50, T)]],
    # 1 the space
    [],
    # 2 A: lines, a hole
    [[(50, 0, T), (350, 700, T), (650, 0, T), (520, 0, T), (450, 180, T), (250, 180, T), (180, 0, T)], [(290, 300, T), (410, 300, T), (350, 470, T)]],
    # 3 o: on / off alternating outside (p[0] off, p[n-1] on), four off-curve points and nothing else inside
    [[(50, 0, F), (50, 250, T), (50, 500, F), (300, 500, T), (550, 500, F), (550, 250, T), (550, 0, F), (300, 0, T)],
     [(150, 100, F), (450, 100, F), (450, 400, F), (150, 400, F)]],
    # 4 V: short vectors of both signs, runs of equal flags
    [[(0, 700, T), (50, 700, T), (100, 700, T), (150, 700, T), (200, 700, T), (300, 100, T), (400, 700, T), (500, 700, T), (600, 700, T), (350, 0, T), (250, 0, T)]],
    # 5 an accent: two off-curve points in a row, p[0] and p[n-1] both off
    [[(0, 0, F), (60, 20, T), (160, 120, F), (140, 160, F), (100, 150, T), (20, 60, F)]],
    # 6 o with the accent: word arguments
    dict(components=[dict(glyph=3), dict(glyph=5, dx=220, dy=560)]),
    # 7 nested: glyph 6 at half size, moved (bytes), and an A turned by 0.4 rad (2 x 2)
    dict(components=[dict(glyph=6, dx=100, dy=-20, scale=0.5), dict(glyph=2, dx=-300, dy=40, scale=(COS, SIN, -SIN, COS), words=True)]),
    # 8 x and y scale, byte arguments
    dict(components=[dict(glyph=4, dx=10, dy=-100, scale=(0.75, -0.5))]),
    # 9 placed by point matching: offset (0, 0), one warning per font
    dict(components=[dict(glyph=2), dict(glyph=5, match=(1, 0))]),
    # 10 I: long vectors, a single-point contour the outline leaves out
    [[(100, 0, T), (400, 0, T), (400, 700, T), (100, 700, T)], [(250, 350, T)]],
    # 11, 12: two glyphs behind numberOfHMetrics (when the font is written so): both take the advance of glyph 10
    [[(0, 0, T), (300, 0, T), (0, 300, F)]],
    [[(0, 0, T), (0, 300, T)]],
]
ADVANCES = [500, 300, 700, 600, 600, 0, 600, 900, 480, 700, 420, 420, 420]
CMAP = {ord(" "): 1, ord("A"): 2, ord("o"): 3, ord("V"): 4, 0xF3: 6, ord("Q"): 7, ord("x"): 8, ord("P"): 9, ord("I"): 10, ord("J"): 11,
        ord("K"): 12, ord("p"): 3}
KERN = {(2, 4): -80, (4, 2): -70, (3, 4): 15}


def synthetic_ttf(**options) -> bytes:
    return build_ttf(GLYPHS, CMAP, ADVANCES, KERN, **options)
