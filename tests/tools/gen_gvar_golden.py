"""Writes tests/golden/fonts/varsynth.ttf and tests/golden/gvar_kat.npz: a small variable font built with fontTools'
``FontBuilder`` (``setupFvar``, ``setupAvar``, ``setupGvar``) and, for 16 locations, the unrounded varied coordinates, component
offsets and advances computed from fontTools' own primitives -- ``normalizeLocation``, the ``avar`` map (``piecewiseLinearMap``) and
the F2Dot14 rounding, ``supportScalar``, ``iup_delta`` and an accumulation in tuple order.  The independent witness of
tests/test_truetype_var_host.py; `record` is also what that file's live test calls.

Run by hand (it needs fontTools, the suite does not run it):  python -m tests.tools.gen_gvar_golden"""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FONT = os.path.join(ROOT, "tests", "golden", "fonts", "varsynth.ttf")
KAT = os.path.join(ROOT, "tests", "golden", "gvar_kat.npz")

AXES = [("wght", 100, 400, 900), ("wdth", 75, 100, 125)]
WGHT_MAP = [(100, 100), (400, 400), (650, 525), (900, 900)]   # user -> design: normalised 0.5 goes to 0.25
ORDER = [".notdef", "space", "A", "o", "odieresis", "dot"]
ADVANCES = {".notdef": 500, "space": 300, "A": 700, "o": 600, "odieresis": 600, "dot": 250}
CMAP = {32: "space", 65: "A", 111: "o", 0xF6: "odieresis", 46: "dot"}
# contours of (x, y, on)
OUTLINES = {
    ".notdef": [[(50, 0, 1), (450, 0, 1), (450, 700, 1), (50, 700, 1)]],
    "space": [],
    "A": [[(50, 0, 1), (350, 700, 1), (650, 0, 1), (520, 0, 1), (450, 180, 1), (250, 180, 1), (180, 0, 1)], [(290, 300, 1), (410, 300, 1), (350, 470, 1)]],
    "o": [[(50, 0, 0), (50, 250, 1), (50, 500, 0), (300, 500, 1), (550, 500, 0), (550, 250, 1), (550, 0, 0), (300, 0, 1)],
          [(150, 100, 0), (450, 100, 0), (450, 400, 0), (150, 400, 0)]],
    "dot": [[(60, 0, 1), (60, 120, 1), (190, 120, 1), (190, 0, 1)]],
}
COMPONENTS = {"odieresis": [("o", 0, 0), ("dot", 110, 560), ("dot", 330, 560)]}
N = None
# per glyph: [(region {tag: (start, peak, end)}, deltas per point number: the points, then the four phantom points; None: untouched)]
VARIATIONS = {
    ".notdef": [({"wght": (0, 1, 1)}, [(-20, 0), N, (25, 10), N, N, (44, 0), N, N])],
    "space": [({"wdth": (0, 1, 1)}, [N, (60, 0), N, N]), ({"wdth": (-1, -1, 0)}, [(5, 0), (-40, 0), N, N])],
    "A": [
        ({"wght": (0, 1, 1)}, [(-30, 0), (0, 7), (30, 0), (17, 0), (10, 2), (-10, 2), (-17, 0), (-6, 4), (6, 4), (0, 6), (0, 0), (55, 0), (0, 0), (0, 0)]),
        ({"wght": (-1, -1, 0)}, [(12, 0), N, (-12, 0), N, (-9, 14), (9, 14), N, (6, -5), N, (0, 3), N, (-30, 0), N, N]),
        ({"wdth": (0, 1, 1)}, [N, (0, 0), N, (130, 0), N, N, (-10, 0), N, N, N, N, (150, 0), N, N]),
        ({"wght": (0, 1, 1), "wdth": (0, 1, 1)}, [N, (7, -3), N, N, N, N, N, N, (-300, 200), N, N, N, N, N]),
        ({"wght": (0.25, 0.5, 0.75)}, [N, (0, 33), N, N, N, N, N, N, N, (4, -17), N, N, N, N]),
    ],
    "o": [
        ({"wght": (0, 1, 1)}, [N, (-30, 0), N, N, N, (30, 0), N, N, (40, 35), N, (-40, -35), N, N, (44, 0), N, N]),
        ({"wdth": (0, 1, 1)}, [N, (0, 0), N, N, N, (140, 0), N, N, (20, 0), N, (110, 0), N, N, (150, 0), N, N]),
        ({"wdth": (-1, -1, 0)}, [N, (0, 0), N, N, N, (-130, 0), N, N, (-20, 0), N, (-100, 0), N, N, (-140, 0), N, N]),
        ({"wght": (0, 0.3, 1)}, [(3, -7), N, N, (1, 11), N, N, N, (-13, 5), N, N, N, N, N, N, N, N]),
    ],
    "odieresis": [({"wght": (0, 1, 1)}, [N, (35, 42), (-15, 42), N, (44, 0), N, N]),
                  ({"wdth": (0, 1, 1)}, [(0, 0), (40, 5), (90, 5), (0, 0), (150, 0), (0, 0), (0, 0)])],
    "dot": [({"wght": (0, 1, 1)}, [(-15, 0), N, (15, 20), N, N, (30, 0), N, N]),
            ({"wdth": (0.2, 0.6, 1.0)}, [N, (9, -4), N, (2, 8), N, (-6, 0), N, N])],
}
# per axis: the default, both ends, outside the range, inside an intermediate region (wght 775 -> 0.625, inside A's
# (0.25, 0.5, 0.75); wdth 110 -> 0.4, inside dot's (0.2, 0.6, 1)) and on a region's edge (wght 650 -> 0.25 through the avar map;
# wdth 105 -> 0.2)
LOCATIONS = [
    {"wght": 400, "wdth": 100}, {"wght": 100, "wdth": 100}, {"wght": 900, "wdth": 100}, {"wght": 400, "wdth": 75}, {"wght": 400, "wdth": 125},
    {"wght": 50, "wdth": 60}, {"wght": 1200, "wdth": 140}, {"wght": 775, "wdth": 100}, {"wght": 650, "wdth": 100}, {"wght": 837.5, "wdth": 100},
    {"wght": 650, "wdth": 80}, {"wght": 513, "wdth": 111.5}, {"wght": 233, "wdth": 88}, {"wght": 900, "wdth": 125},
    {"wght": 400, "wdth": 110}, {"wght": 400, "wdth": 105},
]


def build():
    """The TTFont."""
    from fontTools.designspaceLib import AxisDescriptor
    from fontTools.fontBuilder import FontBuilder
    from fontTools.pens.ttGlyphPen import TTGlyphPen
    from fontTools.ttLib.tables.TupleVariation import TupleVariation

    fb = FontBuilder(1000, isTTF=True)
    fb.setupGlyphOrder(ORDER)
    fb.setupCharacterMap(CMAP)
    glyphs = {}
    for name in sorted(ORDER, key=lambda name: name in COMPONENTS):   # (the simple glyphs first: a composite looks its bases up)
        pen = TTGlyphPen(glyphs)
        for contour in OUTLINES.get(name, []):   # (written point by point: the point numbers are the lists' own)
            pen.points.extend((x, y) for x, y, _on in contour)
            pen.types.extend(1 if on else 0 for _x, _y, on in contour)
            pen.endPts.append(len(pen.points) - 1)
        for base, dx, dy in COMPONENTS.get(name, []):
            pen.addComponent(base, (1, 0, 0, 1, dx, dy))
        glyphs[name] = pen.glyph(dropImpliedOnCurves=False)
    fb.setupGlyf(glyphs)
    fb.setupHorizontalMetrics({name: (ADVANCES[name], 0) for name in ORDER})
    fb.setupHorizontalHeader(ascent=800, descent=-200)
    fb.setupNameTable({"familyName": "VarGolden", "styleName": "Regular"})
    fb.setupOS2(usWeightClass=400)
    fb.setupPost()
    fb.setupFvar([(tag, lo, default, hi, tag) for tag, lo, default, hi in AXES], [])
    descriptors = []
    for tag, lo, default, hi in AXES:
        d = AxisDescriptor()
        d.tag, d.name, d.minimum, d.default, d.maximum = tag, tag, lo, default, hi
        d.map = WGHT_MAP if tag == "wght" else []
        descriptors.append(d)
    fb.setupAvar(descriptors)
    fb.setupGvar({name: [TupleVariation(dict(region), list(deltas)) for region, deltas in tuples] for name, tuples in VARIATIONS.items()})
    return fb.font


def record(font):
    """``{key: array}``: for every location of LOCATIONS the normalised coordinates, the varied points of the simple glyphs, the
    varied component offsets of the composite ones and every glyph's advance, from `font`'s own tables with fontTools' primitives."""
    from fontTools.misc.fixedTools import floatToFixedToFloat
    from fontTools.varLib.iup import iup_delta
    from fontTools.varLib.models import normalizeLocation, piecewiseLinearMap, supportScalar

    axes = {a.axisTag: (a.minValue, a.defaultValue, a.maxValue) for a in font["fvar"].axes}
    tags = [a.axisTag for a in font["fvar"].axes]
    segments = font["avar"].segments
    glyf, gvar, hmtx = font["glyf"], font["gvar"], font["hmtx"]
    order = font.getGlyphOrder()
    out = {"locations": np.array([[loc[t] for t in tags] for loc in LOCATIONS], dtype=np.float64), "normalised": [], "advances": []}
    per_glyph = {name: [] for name in order}
    for loc in LOCATIONS:
        normal = normalizeLocation(loc, axes)
        normal = {t: floatToFixedToFloat(piecewiseLinearMap(normal[t], segments[t]), 14) for t in tags}
        out["normalised"].append([normal[t] for t in tags])
        advances = []
        for name in order:
            glyph = glyf[name]
            if glyph.isComposite():
                coords = [(float(c.x), float(c.y)) for c in glyph.components]
                ends = list(range(len(coords)))
            else:
                coords = [(float(x), float(y)) for x, y in (glyph.coordinates if glyph.numberOfContours > 0 else [])]
                ends = list(glyph.endPtsOfContours) if glyph.numberOfContours > 0 else []
            n = len(coords)
            total, wider = [(0.0, 0.0)] * (n + 4), 0.0
            for tv in gvar.variations.get(name, []):
                s = supportScalar(normal, tv.axes)
                if not s:
                    continue
                # (the phantom points stand at (0, 0): each is a contour of its own to iup_delta, which only uses the count)
                full = iup_delta(tv.coordinates, coords + [(0.0, 0.0)] * 4, ends) if None in tv.coordinates else tv.coordinates
                if glyph.isComposite():   # (no interpolation between components: an untouched one takes 0)
                    full = [d if d is not None else (0, 0) for d in tv.coordinates]
                total = [(tx + s * dx, ty + s * dy) for (tx, ty), (dx, dy) in zip(total, full)]
                wider = wider + s * (float(full[n + 1][0]) - float(full[n][0]))
            per_glyph[name].append([(x + dx, y + dy) for (x, y), (dx, dy) in zip(coords, total)])
            advances.append(hmtx[name][0] + wider)
        out["advances"].append(advances)
    out["normalised"] = np.array(out["normalised"], dtype=np.float64)
    out["advances"] = np.array(out["advances"], dtype=np.float64)
    for gid, name in enumerate(order):
        out[f"points_{gid}"] = np.array(per_glyph[name], dtype=np.float64).reshape(len(LOCATIONS), -1, 2)
    return out


def main():
    font = build()
    os.makedirs(os.path.dirname(FONT), exist_ok=True)
    font.save(FONT)
    from fontTools.ttLib import TTFont

    rec = record(TTFont(FONT))
    np.savez_compressed(KAT, meta=json.dumps(dict(glyphs=ORDER, axes=[a[0] for a in AXES], source="tests/tools/gen_gvar_golden.py")), **rec)
    print(f"{FONT}: {os.path.getsize(FONT)} bytes; {KAT}: {os.path.getsize(KAT)} bytes; {len(LOCATIONS)} locations")


if __name__ == "__main__":
    main()
