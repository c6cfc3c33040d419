"""The inputs of the text-on-a-path tests, shared by tests/test_textpath_host.py (which checks them against the conditions of
textpath_ref's docstring and runs the header through them, on the CPU) and tests/test_gpu_textpath.py (which runs them
through the C ABI).  A case is a dict: name, path = (types, params, sizes), s (queries of svgr_path_sample) or None, inst =
(glyph, s_mid, half, dy) of svgr_path_place_glyphs or None, exact (see textpath_ref: axis-aligned integer lines, queries that
are multiples of 1/4 -- such cases may sit on joints and ends).  Every case that is not exact keeps its queries and anchors
CLEARANCE away from 0, L and every joint, relative to L, and off the slow spots of its cubics."""
import numpy as np

from tests import textpath_ref as R
from tests.dash_cases import stairs

S = 1024   # segments one workgroup of the scans covers (svgr_dash_scan_segments; the GPU test checks the value)
B = 256    # queries / output segments per workgroup of k_textpath_locate / k_textpath_emit (svgr_textpath_block; likewise)
CLEARANCE = 1e-3
FUZZ_CLEARANCE = 1e-6
FUZZ_MAY_SKIP = 0.05


# ---- glyph atlases ---------------------------------------------------------------------------------------------------------
def _line(x0, y0, x1, y1):
    return (R.LINE, [x0, y0, x1, y1, 0, 0, 0, 0])


def _box(x0, y0, x1, y1, last=R.CLOSED):
    return [_line(x0, y0, x1, y0), _line(x1, y0, x1, y1), _line(x1, y1, x0, y1), (last, [x0, y1, x0, y0, 0, 0, 0, 0])]


def atlas(glyphs):
    """(types, params (n, 8), glyph_seg_off) of glyphs given as lists of (type, 8 numbers)."""
    types = [t for g in glyphs for t, _ in g]
    params = [q for g in glyphs for _, q in g]
    off = np.concatenate([[0], np.cumsum([len(g) for g in glyphs])]).astype(np.int32)
    return np.array(types, dtype=np.int32), np.array(params, dtype=np.float64).reshape(-1, 8), off


def fixed_atlas():
    """Glyph 0: a single segment; 1: a box with a hole and a cubic bowl, y-down around the baseline; 2: B + 5 segments (a comb);
    3: no outline (a blank); advances 6, 10, 12, 4."""
    bar = [_line(1.0, -7.0, 5.0, 0.0)]
    bowl = _box(1, -8, 9, 0) + _box(3, -6, 7, -2, R.UNCLOSED) + [(R.CUBIC, [1, 0, 3, 4, 7, 4, 9, 0]), (R.UNCLOSED, [9, 0, 1, 0, 0, 0, 0, 0])]
    comb = [_line(0.5 + 11.0 * k / (B + 4), -9.0 if k % 2 else 0.0, 0.5 + 11.0 * (k + 1) / (B + 4), 0.0 if k % 2 else -9.0) for k in range(B + 4)]
    comb.append((R.UNCLOSED, [comb[-1][1][2], comb[-1][1][3], 0.5, 0.0, 0, 0, 0, 0]))
    return atlas([bar, bowl, comb, []]), np.array([6.0, 10.0, 12.0, 4.0])


# ---- paths -------------------------------------------------------------------------------------------------------------------
def chain(n, seed, kind, closed=False):
    """n segments end to end, cubics ("cubics") or lines and cubics ("mixed"): smooth, of about unit size -- but the first, the
    middle and the last one about n / 3 long, so that a query has room to keep its distance from every joint.  Returns (path, the
    indices of the long segments)."""
    rng = np.random.default_rng(seed)
    long_ones = sorted({0, n // 2, n - 1})
    segs, p = [], np.array([0.0, 0.0])
    for i in range(n):
        scale = max(4.0, n / 3.0) if i in long_ones else 1.0
        d = rng.uniform(0.4, 1.0, 2) * scale * (1.0 if i % 2 else np.array([1.0, -1.0]))
        e = p + d
        if kind == "mixed" and i % 3 == 1:
            segs.append((R.LINE, [*p, *e]))
        else:
            c1 = p + d * rng.uniform(0.2, 0.4) + rng.uniform(-0.15, 0.15, 2) * scale
            c2 = p + d * rng.uniform(0.6, 0.8) + rng.uniform(-0.15, 0.15, 2) * scale
            segs.append((R.CUBIC, [*p, *c1, *c2, *e]))
        p = e
    return R.from_segments(segs, closed), long_ones


def _in_segments(path, which, fractions):
    """Arc lengths inside the segments `which` of `path`, at `fractions` of each (by the reference's measure)."""
    m = R.Measured(*path)
    return np.array([float(m.cum[i] + f * m.lens[i]) for i in which for f in fractions])


def _instances(s_first, s_last, n, advances, dy=0.0):
    """n instances, the glyphs in turn, anchors evenly from s_first to s_last."""
    glyph = np.arange(n, dtype=np.int32) % len(advances)
    s_mid = np.linspace(s_first, s_last, n) if n > 1 else np.array([0.5 * (s_first + s_last)][:n])
    return glyph, s_mid, advances[glyph] / 2, np.full(n, float(dy))


def fixed_cases():
    (a_types, a_params, a_off), advances = fixed_atlas()
    out = []

    def add(name, path, s=None, inst=None, exact=False):
        out.append(dict(name=name, path=path, s=None if s is None else np.asarray(s, dtype=np.float64), inst=inst, exact=exact))

    # -- the scan's seams: 1, S - 1, S, S + 1, 2 S + 1 segments
    for n in (1, S - 1, S, S + 1, 2 * S + 1):
        path = stairs(n)                       # n lines of integer length and the terminating line
        m = R.Measured(*path)
        L = float(m.L)
        cum = np.asarray(m.cum[:-1], dtype=np.float64)
        picks = sorted({0, n // 3, n // 2, S - 1 if n >= S else 0, S if n > S else 0, n - 1})
        s = [cum[i] for i in picks] + [cum[i] + 0.5 for i in picks] + [0.0, L, -0.25, L + 0.25, L - 0.5]
        add(f"lines{n}", path, s[::-1] + s, _instances(-3.0, L + 3.0, 9, advances), exact=True)   # (unsorted, each value twice)
        for kind in ("cubics", "mixed"):
            path, long_ones = chain(n, 100 + n, kind)
            s = _in_segments(path, long_ones, (0.11, 0.52, 0.83))
            add(f"{kind}{n}", path, s[::-1], _instances(s.min(), s.max(), 1, advances) if n == 1 else
                (np.arange(len(s), dtype=np.int32) % 4, s, advances[np.arange(len(s)) % 4] / 2, np.full(len(s), 0.75)))
    # -- subpaths, closed subpaths, zero-length segments, the trailing unclosed line
    two = R.concat(R.polyline([(0, 0), (30, 0), (30, 40)]), R.polyline([(100, 100), (100, 60), (70, 60)]))
    three = R.concat(two, R.polyline([(5, 5), (5, 25), (20, 25)], closed=True))
    zeros = R.concat(R.polyline([(0, 0), (0, 0), (0, 0), (10, 0), (10, 0), (10, 10), (10, 10)]), R.polyline([(3, 3), (3, 3)]),
                     R.polyline([(20, 0), (20, 0), (20, 8), (20, 8)], closed=True))
    for name, path in (("two_subpaths", two), ("three_subpaths_closed", three), ("zero_length_segments", zeros)):
        L = float(R.Measured(*path).L)
        s = np.arange(-1.0, L + 1.25, 0.25)
        add(name, path, s, _instances(-2.0, L + 2.0, 13, advances, dy=-1.5), exact=True)
    curved = R.concat(chain(3, 7, "cubics")[0], chain(4, 8, "mixed", closed=True)[0])
    m = R.Measured(*curved)
    s = np.array([float(m.cum[i] + f * m.lens[i]) for i in m.real for f in (0.2, 0.7)])
    add("curved_subpaths_closed", curved, s, (np.arange(len(s), dtype=np.int32) % 4, s, advances[np.arange(len(s)) % 4] / 2, np.zeros(len(s))))
    add("no_length", R.polyline([(5, 5), (5, 5), (5, 5)]), [0.0, 1.0, -1.0], _instances(0.0, 0.0, 2, advances), exact=True)
    # -- query and instance counts at the launch seams, off both ends of the path (a negative offset, text longer than the path)
    one = R.from_segments([(R.CUBIC, [0, 0, 60, 90, 130, -70, 200, 10])])
    L = float(R.Measured(*one).L)
    for n in (0, 1, B - 1, B, B + 1):
        s = L * (-0.1165 + 1.2 * (np.arange(n) + 0.5) / max(n, 1))
        add(f"queries{n}", one, s[::-1].copy() if n else s)
        glyph = np.where(np.arange(n) % 5 == 0, 1, np.where(np.arange(n) % 5 == 3, 3, 0)).astype(np.int32)   # (5, 1 or 0 rows each)
        add(f"instances{n}", one, None, (glyph, s, advances[glyph] / 2, np.full(n, -0.5)))
    s = L * np.array([0.21, 0.48, 0.77, -0.2, 1.3])
    add("glyph_over_a_block", one, None, (np.array([0, 2, 1, 2, 2], dtype=np.int32), s, advances[[0, 2, 1, 2, 2]] / 2, np.zeros(5)))
    square = R.polyline([(0, 0), (100, 0), (100, 50), (0, 50)], closed=True)
    add("on_joints_and_ends", square, [0.0, 100.0, 150.0, 250.0, 300.0, 300.25, -0.25, 100.0, 0.0],
        (np.array([1, 1, 1], dtype=np.int32), np.array([0.0, 150.0, 300.0]), np.full(3, 5.0), np.zeros(3)), exact=True)
    return (a_types, a_params, a_off), out


def joint_cases():
    """Queries on the joints and at the end of curved paths, where the segment -- and with it the direction -- or the flag is
    a matter of rounding: the point must still agree."""
    out = []
    for n, kind in ((3, "cubics"), (S + 1, "mixed")):
        path, _long = chain(n, 300 + n, kind)
        m = R.Measured(*path)
        out.append(dict(name=f"joints_{kind}{n}", path=path, s=np.asarray(m.joints, dtype=np.float64)[:: max(1, len(m.joints) // 40)], inst=None,
                        exact=False))
    return out


def fuzz_cases(n_paths=200, seed=20260201):
    """Seeded: `n_paths` of (atlas, case): paths of <= 40 segments, lines and cubics, open and closed, one or two subpaths; atlases
    of 1 to 4 glyphs of 0 to 6 segments; up to 12 queries and 12 instances, some off the ends."""
    from tests.dash_cases import mixed_chain

    rng = np.random.default_rng(seed)
    out = []
    for i in range(n_paths):
        parts = []
        for _ in range(int(rng.integers(1, 3))):
            segs = mixed_chain(int(rng.integers(1, 21)), int(rng.integers(1 << 30)))
            parts.append(R.from_segments(segs, closed=bool(rng.random() < 0.4)))
        path = R.concat(*parts)
        L = float(R.Measured(*path).L)
        glyphs = []
        for _ in range(int(rng.integers(1, 5))):
            g = []
            for _ in range(int(rng.integers(0, 7))):
                q = rng.uniform(-6, 10, 8)
                g.append((R.CUBIC, list(q)) if rng.random() < 0.5 else (R.LINE, [*q[:4], 0, 0, 0, 0]))
            glyphs.append(g)
        n_inst = int(rng.integers(0, 13))
        glyph = rng.integers(0, len(glyphs), n_inst).astype(np.int32)
        inst = (glyph, rng.uniform(-0.15, 1.15, n_inst) * L, rng.uniform(1, 6, n_inst), rng.uniform(-3, 3, n_inst))
        out.append((atlas(glyphs), dict(name=f"fuzz{i}", path=path, s=rng.uniform(-0.15, 1.15, int(rng.integers(0, 13))) * L, inst=inst,
                                        exact=False)))
    return out


def clearance(atlas_arrays, case):
    """The case's clearance by the reference alone (over its queries and its anchors)."""
    worst = np.inf
    for s in (case["s"], None if case["inst"] is None else case["inst"][1]):
        if s is not None and len(s):
            d = {}
            R.sample(*case["path"], s, case["exact"], d)
            worst = min(worst, d["clearance"])
    return worst


# ---- documents -----------------------------------------------------------------------------------------------------------------
# A font of a few glyphs, y-up, 1000 units per em: "A" with a hole, "O" of cubics with a hole, "I", a blank; A-O kerns by 40.
FONT = """<font id="tp" horiz-adv-x="600"><font-face font-family="TP" units-per-em="1000" ascent="800" descent="-200"/>
<missing-glyph horiz-adv-x="500" d="M50,0 H450 V700 H50 Z"/>
<glyph unicode="A" horiz-adv-x="700" d="M50,0 L350,700 L650,0 L520,0 L450,180 L250,180 L180,0 Z M290,300 L410,300 L350,470 Z"/>
<glyph unicode="O" horiz-adv-x="760" d="M380,-10 C590,-10 710,150 710,350 C710,550 590,710 380,710 C170,710 50,550 50,350 C50,150 170,-10 380,-10 Z M380,110 C250,110 190,220 190,350 C190,480 250,590 380,590 C510,590 570,480 570,350 C570,220 510,110 380,110 Z"/>
<glyph unicode="I" horiz-adv-x="300" d="M100,0 H200 V700 H100 Z"/>
<glyph unicode=" " horiz-adv-x="300" d=""/>
<hkern u1="A" u2="O" k="40"/>
</font>"""


def document(body, size=256):
    return (f'<svg xmlns="http://www.w3.org/2000/svg" xmlns:xlink="http://www.w3.org/1999/xlink" width="{size}" height="{size}" '
            f'viewBox="0 0 {size} {size}"><defs>{FONT}</defs>{body}</svg>')


# The end-to-end font: 32 units per em, set at 32 user units per em, so that glyph units are user units and a glyph instance
# written out by hand is the glyph's own path data under one matrix; side bearings of 2 to 3 units keep neighbours apart.
FONT32 = """<font id="tq" horiz-adv-x="20"><font-face font-family="TQ" units-per-em="32" ascent="26" descent="-6"/>
<missing-glyph horiz-adv-x="16" d="M2,0 H14 V22 H2 Z"/>
<glyph unicode="A" horiz-adv-x="22" d="M2,0 L11,22 L20,0 L16,0 L14,6 L8,6 L6,0 Z M9,10 L13,10 L11,15 Z"/>
<glyph unicode="O" horiz-adv-x="24" d="M12,0 C19,0 22,5 22,11 C22,17 19,22 12,22 C5,22 2,17 2,11 C2,5 5,0 12,0 Z M12,4 C8,4 6,7 6,11 C6,15 8,18 12,18 C16,18 18,15 18,11 C18,7 16,4 12,4 Z"/>
<glyph unicode="I" horiz-adv-x="10" d="M3,0 H7 V22 H3 Z"/>
<glyph unicode=" " horiz-adv-x="10" d=""/>
</font>"""
