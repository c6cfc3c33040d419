#!/usr/bin/env python3
"""Time of the OpenType / CFF outline pass (svgr_cff_outline); to be read beside profiles/bench_truetype.py's figures from the
same card.  Two figures:
  * 100 000 parts over an atlas of 64 random glyphs (1 to 4 contours of 4 to 40 segments, lines and cubics at random): per call
    the wall clock of the whole call -- the validation walk with its segment tables and the packing on the host, upload,
    k_cff_emit, download -- and the device time between two marks around it (svgr_measure_begin / _end: from the upload to the
    end of the download), each the median over `reps` calls.  `device_ms` is that span -- copies and, for the string, the host's
    work included --, not the kernel's time: k_cff_emit alone is read from a kernel trace of this script (`rocprofv3
    --kernel-trace -- python profiles/bench_cff.py --reps 3`; DESIGN.md 7m has what was measured).
  * `CFFFont.str_to_path` of a 1 000-character string: the wall clock of the call -- cmap and kerning, the atlas, the pass,
    `Path.from_segments` -- in --font FILE.otf, else, where fontTools and a DejaVuSans.ttf exist (bench_truetype.py's face), in
    that face saved as CFF in memory, else in the committed font of the tests (tests/golden/fonts/cffsynth.otf).
    python profiles/bench_cff.py [--reps 20] [--font FILE.otf]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def face(path):
    """(font bytes, what it is)."""
    if path is not None:
        with open(path, "rb") as f:
            return f.read(), path
    try:
        import fontTools  # noqa: F401
    except ImportError:
        fontTools = None
    if fontTools is not None:
        from bench_truetype import find_font
        from tests import cff_cases

        found = find_font()
        if found is not None:
            return cff_cases.truetype_as_cff(found, 600), f"the first 600 glyphs of {found} saved as CFF by fontTools"
    with open(os.path.join(ROOT, "tests", "golden", "fonts", "cffsynth.otf"), "rb") as f:
        return f.read(), "the committed font of the tests"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--font", default=None)
    args = ap.parse_args()
    import numpy as np

    import svgrasterize_amd as S
    from svgrasterize_amd import _abi

    ctx = S.Context.get(0)
    rng = np.random.default_rng(7)

    def median_ms(call):
        call()   # (warm-up: code objects, the pool's blocks, the font's glyph cache)
        ctx.sync()
        wall, device = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            ctx.measure_begin(0.0)
            out = call()
            device.append(ctx.measure_end())
            wall.append((time.perf_counter() - t0) * 1e3)
        return out, float(np.median(wall)), min(wall), float(np.median(device))

    # ---- the pass alone
    kinds, contour_off, glyph_contour_off = [], [0], [0]
    for _ in range(64):
        for _ in range(int(rng.integers(1, 5))):
            kinds.append(0)
            for _ in range(int(rng.integers(4, 41)) - 1):   # (the closing line is the contour's last segment)
                kinds.extend([1] if rng.random() < 0.5 else [2, 3, 4])
            contour_off.append(len(kinds))
        glyph_contour_off.append(len(contour_off) - 1)
    n_points, n_parts = len(kinds), 100_000
    pt_xy = rng.integers(-200 * 16, 1800 * 16, (n_points, 2)).astype(np.float64) / 16.0
    pt_kind = np.array(kinds, dtype=np.uint8)
    part_glyph = rng.integers(0, 64, n_parts).astype(np.int32)
    part_m = np.tile(np.array([1.0, 0.0, 0.0, 1.0, 0.0, 0.0]), (n_parts, 1))
    pen = np.cumsum(rng.uniform(300, 900, n_parts))
    sx, sy = np.full(n_parts, 0.012), np.full(n_parts, -0.012)
    out, wall, wall_min, device = median_ms(
        lambda: _abi.cff_outline(pt_xy, pt_kind, contour_off, glyph_contour_off, part_glyph, part_m, pen, sx, sy, ctx))
    points = np.diff(np.array(contour_off)[glyph_contour_off])[part_glyph]
    lanes = int(len(out[0]))   # one lane per output segment
    res = [dict(workload="100000 parts, atlas of 64 glyphs", parts=n_parts, points=int(points.sum()), lanes=lanes, output_segments=lanes,
                subpaths=int(len(out[2])), call_ms=round(wall, 3), call_ms_min=round(wall_min, 3), device_ms=round(device, 3),
                lanes_per_s=round(lanes / (wall * 1e-3)))]

    # ---- a string through the public API
    sys.path.insert(0, os.path.join(ROOT, "profiles"))
    data, what = face(args.font)
    font = S.read_otf(data)
    words = "The quick brown fox jumps over the lazy dog; AVATAR Typography 0123456789. "
    text = (words * (1000 // len(words) + 1))[:1000]
    (outline, _advance), wall, wall_min, device = median_ms(lambda: font.str_to_path(16.0, text))
    res.append(dict(workload="str_to_path, 1000 characters", face=what, family=font.family, subpaths=len(outline.subpaths),
                    segments=sum(len(s) for s in outline.subpaths), call_ms=round(wall, 3), call_ms_min=round(wall_min, 3),
                    device_ms=round(device, 3)))
    print(json.dumps(dict(device=ctx.name(), reps=args.reps, results=res)))


if __name__ == "__main__":
    main()
