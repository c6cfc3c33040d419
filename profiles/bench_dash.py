#!/usr/bin/env python3
"""Streaming rate of the dasher (svgr_path_dash): wall clock of the whole call -- upload, the k_dash_* / k_scan_* kernels,
the read-back of the counts, download -- over `reps` calls, pieces per second, and beside it the host stroker's time on the
dasher's output.  Workloads: one 100 000-segment polyline with a period of about 3 segment lengths, and 10 000 cubics with a
period of about 1/50 of a cubic.  (The split per kernel is read from a kernel trace of this script: `rocprofv3 --kernel-trace
--stats -- python profiles/bench_dash.py --reps 3`.)
    python profiles/bench_dash.py [--reps 10]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import numpy as np

    import svgrasterize_amd as S
    from svgrasterize_amd import _abi

    ctx = S.Context.get(0)
    rng = np.random.default_rng(3)

    def polyline(n):
        pts = np.cumsum(rng.uniform(0.5, 1.5, (n + 1, 2)), axis=0)
        params = np.zeros((n + 1, 8))
        params[:n, 0:2], params[:n, 2:4] = pts[:-1], pts[1:]
        params[n, 0:2], params[n, 2:4] = pts[-1], pts[0]
        types = np.zeros(n + 1, dtype=np.int32)
        types[n] = 5
        return types, params, np.array([n + 1], dtype=np.int32), float(np.hypot(*(pts[1:] - pts[:-1]).T).mean())

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
        return types, params, np.array([n + 1], dtype=np.int32), float(np.hypot(*d.T).mean())

    res = []
    for name, (types, params, sizes, seg_len), period in (("polyline 100000 segments, period 3 segments", polyline(100_000), 3.0),
                                                            ("10000 cubics, period 1/50 cubic", cubics(10_000), 1 / 50)):
        dashes = [seg_len * period * 0.6, seg_len * period * 0.4]
        out = _abi.path_dash(types, params, sizes, dashes, 0.0, 0.0, ctx)
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            out = _abi.path_dash(types, params, sizes, dashes, 0.0, 0.0, ctx)
        dt = (time.perf_counter() - t0) / args.reps
        pieces = int(len(out[0]) - len(out[2]))
        t1 = time.perf_counter()
        _abi.path_stroke(out[0], out[1], out[2], 1.0, 0, 0)
        stroke = time.perf_counter() - t1
        res.append(dict(workload=name, segments=int(len(types)), pieces=pieces, dashes=int(len(out[2])), dash_ms=round(dt * 1e3, 3),
                        pieces_per_s=round(pieces / dt), host_stroker_ms=round(stroke * 1e3, 3)))
    print(json.dumps(dict(device=ctx.name(), reps=args.reps, results=res)))


if __name__ == "__main__":
    main()
