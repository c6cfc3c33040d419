#!/usr/bin/env python3
"""Time of the TrueType outline pass (svgr_glyf_outline).  Two figures:
  * 100 000 parts over an atlas of 64 random glyphs (1 to 4 contours of 4 to 40 points): per call the wall clock of the whole
    call -- the validation walk with its slot tables and the packing on the host, upload, k_glyf_emit, download -- and the device
    time between two marks around it (svgr_measure_begin / _end: from the upload to the end of the download), each the median
    over `reps` calls.  `device_ms` is that span -- copies and, for the string, the host's work included --, not the kernel's
    time: k_glyf_emit alone is read from a kernel trace of this script (`rocprofv3 --kernel-trace -- python
    profiles/bench_truetype.py --reps 3`; DESIGN.md 7k has both).
  * `TrueTypeFont.str_to_path` of a 1 000-character string: the wall clock of the call -- cmap and kerning, the atlas, the
    pass, `Path.from_segments` -- in a TrueType face of this machine (a DejaVuSans.ttf under /usr/share/fonts or in
    matplotlib's data, or --font), else in the synthetic font of the tests.
    python profiles/bench_truetype.py [--reps 20] [--font FILE.ttf]"""
import argparse
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def find_font():
    found = sorted(glob.glob("/usr/share/fonts/**/DejaVuSans.ttf", recursive=True))
    try:
        import matplotlib

        found += glob.glob(os.path.join(matplotlib.get_data_path(), "fonts", "ttf", "DejaVuSans.ttf"))
    except ImportError:
        pass
    return found[0] if found else None


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
    contour_off, glyph_contour_off = [0], [0]
    for _ in range(64):
        for _ in range(int(rng.integers(1, 5))):
            contour_off.append(contour_off[-1] + int(rng.integers(4, 41)))
        glyph_contour_off.append(len(contour_off) - 1)
    n_points, n_parts = contour_off[-1], 100_000
    pt_xy = rng.integers(-200, 1800, (n_points, 2)).astype(np.int16)
    pt_on = (rng.random(n_points) < 0.6).astype(np.uint8)
    part_glyph = rng.integers(0, 64, n_parts).astype(np.int32)
    part_m = np.tile(np.array([1.0, 0.0, 0.0, 1.0, 0.0, 0.0]), (n_parts, 1))
    pen = np.cumsum(rng.uniform(300, 900, n_parts))
    sx, sy = np.full(n_parts, 0.012), np.full(n_parts, -0.012)
    out, wall, wall_min, device = median_ms(
        lambda: _abi.glyf_outline(pt_xy, pt_on, contour_off, glyph_contour_off, part_glyph, part_m, pen, sx, sy, ctx))
    points = np.diff(np.array(contour_off)[glyph_contour_off])[part_glyph]
    res = [dict(workload="100000 parts, atlas of 64 glyphs", parts=n_parts, lanes=int(points.sum()), output_segments=int(len(out[0])),
                subpaths=int(len(out[2])), call_ms=round(wall, 3), call_ms_min=round(wall_min, 3), device_ms=round(device, 3),
                lanes_per_s=round(int(points.sum()) / (wall * 1e-3)))]

    # ---- a string through the public API
    path = args.font or find_font()
    if path is not None:
        with open(path, "rb") as f:
            font, face = S.read_ttf(f.read()), path
    else:
        from tests import ttf_cases

        font, face = S.read_ttf(ttf_cases.synthetic_ttf()), "the synthetic font of the tests"
    words = "The quick brown fox jumps over the lazy dog; AVATAR Typography 0123456789. "
    text = (words * (1000 // len(words) + 1))[:1000]
    (outline, _advance), wall, wall_min, device = median_ms(lambda: font.str_to_path(16.0, text))
    res.append(dict(workload="str_to_path, 1000 characters", face=face, family=font.family, subpaths=len(outline.subpaths),
                    segments=sum(len(s) for s in outline.subpaths), call_ms=round(wall, 3), call_ms_min=round(wall_min, 3),
                    device_ms=round(device, 3)))
    print(json.dumps(dict(device=ctx.name(), reps=args.reps, results=res)))


if __name__ == "__main__":
    main()
