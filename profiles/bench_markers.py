#!/usr/bin/env python3
"""Time of the marker vertex pass (svgr_path_markers) on one 100 000-vertex polyline and on a chain of 100 000 cubics: per call
the wall clock of the whole call -- checking and packing the input on the host, upload, the k_marker_* / k_scan_* kernels,
download -- and the device time between two marks around it (svgr_measure_begin / _end: from the upload to the end of the
download), each the median over `reps` calls, and vertices per second of wall clock.  (The split per kernel is read from a kernel
trace of this script: `rocprofv3 --kernel-trace --stats -- python profiles/bench_markers.py --reps 3`.)
    python profiles/bench_markers.py [--reps 20]"""
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

    res = []
    for name, (types, params, sizes) in (("polyline, 100000 vertices", polyline(100_000)), ("chain of 100000 cubics", cubics(100_000))):
        out = _abi.path_markers(types, params, sizes, None, ctx)   # (warm-up: code objects, the pool's blocks)
        ctx.sync()
        wall, device = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            ctx.measure_begin(0.0)
            out = _abi.path_markers(types, params, sizes, None, ctx)
            device.append(ctx.measure_end())
            wall.append((time.perf_counter() - t0) * 1e3)
        n_vert = int(len(out[2]))
        w = float(np.median(wall))
        res.append(dict(workload=name, segments=int(len(types)), vertices=n_vert, call_ms=round(w, 3), call_ms_min=round(min(wall), 3),
                        device_ms=round(float(np.median(device)), 3), vertices_per_s=round(n_vert / (w * 1e-3))))
    print(json.dumps(dict(device=ctx.name(), reps=args.reps, results=res)))


if __name__ == "__main__":
    main()
