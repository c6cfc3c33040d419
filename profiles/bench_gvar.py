#!/usr/bin/env python3
"""Time of a variable font's instance against its default instance: `TrueTypeFont.str_to_path` of a 2 000-character string in
the synthetic variable font of the tests (tests/gvar_cases.py), once in the default instance (svgr_glyf_outline: k_glyf_emit)
and once at wght 650, wdth 80 (svgr_glyf_outline_var: k_gvar_delta, then k_glyf_emit).  Per workload the wall clock of the
whole call -- cmap and kerning, the atlas and the tuples' scalars on the host, upload, the kernels, download,
`Path.from_segments` -- as the median and the best of `reps` calls.  The two kernels' own device times are not in it: read
them from a kernel trace of this script (`rocprofv3 --kernel-trace --stats -- python profiles/bench_gvar.py --reps 3`;
DESIGN.md 7l has both).  No threshold is attached.
    python profiles/bench_gvar.py [--reps 20]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import numpy as np

    import svgrasterize_amd as S
    from tests import gvar_cases

    ctx = S.Context.get(0)
    font = S.read_ttf(gvar_cases.synthetic_var_ttf())
    words = "AVo \xf3Q xI oVA AVAo "   # (the characters the synthetic font maps: simple glyphs, composites, a kerning pair)
    text = (words * (2000 // len(words) + 1))[:2000]

    def median_ms(call):
        call()   # (warm-up: code objects, the pool's blocks, the glyph and tuple caches)
        ctx.sync()
        wall = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            out = call()
            wall.append((time.perf_counter() - t0) * 1e3)
        return out, float(np.median(wall)), min(wall)

    res = []
    for name, face in (("default instance", font), ("wght 650, wdth 80", font.instance(wght=650, wdth=80))):
        launches = ctx.launches()
        (outline, _advance), wall, wall_min = median_ms(lambda face=face: face.str_to_path(16.0, text))
        res.append(dict(workload=f"str_to_path, {len(text)} characters, {name}", subpaths=len(outline.subpaths),
                        segments=sum(len(s) for s in outline.subpaths), launches_per_call=(ctx.launches() - launches) // (args.reps + 1),
                        call_ms=round(wall, 3), call_ms_min=round(wall_min, 3)))
    print(json.dumps(dict(device=ctx.name(), reps=args.reps, results=res)))


if __name__ == "__main__":
    main()
