"""Writes tests/golden/fonts/cffsynth.otf and tests/golden/cff_kat.npz: a small OpenType / CFF font built with fontTools'
``FontBuilder.setupCFF`` from hand-written ``T2CharString`` programs -- the glyphs of tests/cff_cases.py's synthetic font: local
and global subroutines, a ``hintmask`` with an implied ``vstem``, a ``flex`` and a fractional operand -- plus a ``kern`` table,
and for every glyph the contours fontTools' glyph set draws into a ``RecordingPen``.  The independent witness of
tests/test_cff_host.py, and the font of the end-to-end tests of tests/test_gpu_cff.py.

Per glyph g the npz holds ``xy_g`` (n, 2) float64, ``kind_g`` uint8 (0 MOVE, 1 LINE, 2 C1, 3 C2, 4 CURVE) and ``ends_g``, the last
point of each contour; and ``n_glyphs``, ``advances``, ``cmap`` (n, 2: code, glyph) and ``kern`` (n, 3: left, right, value).

Run by hand (it needs fontTools, the suite does not run it):  python -m tests.tools.gen_cff_golden"""
import io
import os

import numpy as np

from tests import cff_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FONT = os.path.join(ROOT, "tests", "golden", "fonts", "cffsynth.otf")
KAT = os.path.join(ROOT, "tests", "golden", "cff_kat.npz")

ORDER = [".notdef", "space", "A", "o", "V", "D"]
KINDS = {"moveTo": (K.MOVE,), "lineTo": (K.LINE,), "curveTo": (K.C1, K.C2, K.CURVE)}


def program(ops):
    """An operator list of tests/cff_cases.py as a fontTools program: mask bytes follow their operator as bytes."""
    return [item[1] if isinstance(item, tuple) else item for item in ops]


def build() -> bytes:
    from fontTools.cffLib import SubrsIndex
    from fontTools.fontBuilder import FontBuilder
    from fontTools.misc.psCharStrings import T2CharString
    from fontTools.ttLib import newTable
    from fontTools.ttLib.tables._k_e_r_n import KernTable_format_0

    fb = FontBuilder(1000, isTTF=False)
    fb.setupGlyphOrder(ORDER)
    fb.setupCharacterMap({code: ORDER[gid] for code, gid in K.SYNTH_CMAP.items()})
    fb.setupCFF("CFFSynth-Regular", {"FullName": "CFF Synth"}, {name: T2CharString(program=program(ops)) for name, ops in zip(ORDER, K.SYNTH)}, {})
    top = fb.font["CFF "].cff.topDictIndex[0]
    top.Private.Subrs = SubrsIndex()
    for ops in K.SYNTH_SUBRS:
        top.Private.Subrs.append(T2CharString(program=program(ops)))
    for ops in K.SYNTH_GSUBRS:
        fb.font["CFF "].cff.GlobalSubrs.append(T2CharString(program=program(ops)))
    fb.setupHorizontalMetrics({name: (advance, 0) for name, advance in zip(ORDER, K.SYNTH_ADVANCES)})
    fb.setupHorizontalHeader(ascent=800, descent=-200)
    fb.setupNameTable({"familyName": "CFF Synth", "styleName": "Regular"})
    fb.setupOS2(usWeightClass=400)
    fb.setupPost()
    kern = fb.font["kern"] = newTable("kern")
    kern.version = 0
    sub = KernTable_format_0()
    sub.apple, sub.coverage, sub.format, sub.tupleIndex = False, 1, 0, None
    sub.kernTable = {(ORDER[left], ORDER[right]): value for (left, right), value in K.SYNTH_KERN.items()}
    kern.kernTables = [sub]
    out = io.BytesIO()
    fb.save(out)
    return out.getvalue()


def record(data: bytes) -> dict:
    """The npz's arrays of the font `data`, drawn by fontTools."""
    from fontTools import ttLib
    from fontTools.pens.recordingPen import RecordingPen

    font = ttLib.TTFont(io.BytesIO(data))
    glyph_set, order = font.getGlyphSet(), font.getGlyphOrder()
    out = {"n_glyphs": np.int64(len(order)), "advances": np.array([font["hmtx"][name][0] for name in order], dtype=np.float64),
           "cmap": np.array(sorted((code, order.index(name)) for code, name in font.getBestCmap().items()), dtype=np.int64).reshape(-1, 2),
           "kern": np.array(sorted((order.index(left), order.index(right), value) for (left, right), value in font["kern"].kernTables[0].kernTable.items()),
                            dtype=np.int64).reshape(-1, 3)}
    for gid, name in enumerate(order):
        pen = RecordingPen()
        glyph_set[name].draw(pen)
        xy, kind, ends = [], [], []
        for op, args in pen.value:
            if op in KINDS:
                if op == "moveTo" and xy:
                    ends.append(len(xy) - 1)
                assert len(args) == len(KINDS[op])
                xy.extend((float(x), float(y)) for x, y in args)
                kind.extend(KINDS[op])
            else:
                assert op in ("closePath", "endPath"), op
        if xy:
            ends.append(len(xy) - 1)
        out[f"xy_{gid}"] = np.array(xy, dtype=np.float64).reshape(-1, 2)
        out[f"kind_{gid}"] = np.array(kind, dtype=np.uint8)
        out[f"ends_{gid}"] = np.array(ends, dtype=np.int32)
    return out


def main():
    data = build()
    with open(FONT, "wb") as f:
        f.write(data)
    np.savez_compressed(KAT, **record(data))
    print(f"{FONT}: {len(data)} bytes; {KAT}: {os.path.getsize(KAT)} bytes")
    assert len(data) < 65536 and os.path.getsize(KAT) < 65536


if __name__ == "__main__":
    main()
