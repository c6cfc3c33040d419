#!/usr/bin/env python3
"""Time of the text-on-a-path pass (svgr_path_place_glyphs) with 100 000 glyph instances on a chain of cubics and on a polyline:
per call the wall clock of the whole call -- checking and packing the input on the host, upload, k_dash_measure, the k_scan_*
kernels, k_textpath_locate, k_textpath_emit, download -- and the device time between two marks around it (svgr_measure_begin /
_end: from the upload to the end of the download), each the median over `reps` calls, and instances per second of wall clock.
(The split per kernel is read from a kernel trace of this script: `rocprofv3 --kernel-trace --stats -- python
profiles/bench_textpath.py --reps 3`.)
    python profiles/bench_textpath.py [--reps 20]"""
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
    from svgrasterize_amd import _abi

    ctx = S.Context.get(0)
    rng = np.random.default_rng(5)

    def polyline(n):   # n vertices: n - 1 lines and the terminating line
        pts = np.cumsum(rng.uniform(-1.0, 1.5, (n, 2)), axis=0)
        params = np.zeros((n, 8))
        params[:n - 1, 0:2], params[:n - 1, 2:4] = pts[:-1], pts[1:]
        params[n - 1, 0:2], params[n - 1, 2:4] = pts[-1], pts[0]
        types = np.zeros(n, dtype=np.int32)
        types[n - 1] = 5
        return types, params, np.array([n], dtype=np.int32)

    def cubics(n):
        p0 = np.cumsum(rng.uniform(20, 40, (n + 1, 2)), axis=0)
        params = np.zeros((n + 1, 8))
        d = p0[1:] - p0[:-1]
        params[:n, 0:2], params[:n, 6:8] = p0[:-1], p0[1:]
        params[:n, 2:4] = p0[:-1] + d * 0.3 + rng.uniform(-8, 8, (n, 2))
        params[:n, 4:6] = p0[:-1] + d * 0.7 + rng.uniform(-8, 8, (n, 2))
        params[n, 0:2], params[n, 2:4] = p0[-1], p0[0]
        types = np.full(n + 1, 2, dtype=np.int32)
        types[n] = 5
        return types, params, np.array([n + 1], dtype=np.int32)

    # an atlas of 64 glyphs of 8 to 40 segments, lines and cubics, about 10 wide
    glyph_types, glyph_params, off = [], [], [0]
    for _ in range(64):
        k = int(rng.integers(8, 41))
        t = np.where(rng.random(k) < 0.5, 0, 2).astype(np.int32)
        q = rng.uniform(-2, 12, (k, 8))
        q[t == 0, 4:] = 0.0
        glyph_types.append(t)
        glyph_params.append(q)
        off.append(off[-1] + k)
    a_types, a_params, a_off = np.concatenate(glyph_types), np.concatenate(glyph_params), np.array(off, dtype=np.int32)
    n_inst = 100_000
    glyph = rng.integers(0, 64, n_inst).astype(np.int32)
    half, dy = np.full(n_inst, 5.0), np.zeros(n_inst)

    res = []
    for name, (types, params, sizes) in (("chain of 10000 cubics", cubics(10_000)), ("polyline, 10000 vertices", polyline(10_000))):
        length = _abi.path_sample(types, params, sizes, (), ctx)[3]
        s_mid = np.linspace(-0.01, 1.01, n_inst) * length          # (1 % hangs off either end)
        call = lambda: _abi.path_place_glyphs(types, params, sizes, a_types, a_params, a_off, glyph, s_mid, half, dy, ctx)   # noqa: E731
        out = call()   # (warm-up: code objects, the pool's blocks)
        ctx.sync()
        wall, device = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            ctx.measure_begin(0.0)
            out = call()
            device.append(ctx.measure_end())
            wall.append((time.perf_counter() - t0) * 1e3)
        w = float(np.median(wall))
        res.append(dict(workload=name, segments=int(len(types)), instances=n_inst, visible=int(out[1].sum()), output_segments=int(len(out[0])),
                        call_ms=round(w, 3), call_ms_min=round(min(wall), 3), device_ms=round(float(np.median(device)), 3),
                        instances_per_s=round(n_inst / (w * 1e-3))))
    print(json.dumps(dict(device=ctx.name(), reps=args.reps, results=res)))


if __name__ == "__main__":
    main()
