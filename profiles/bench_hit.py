#!/usr/bin/env python3
"""Hit testing: the rate of svgr_batch_pick on the synthetic 4096-path scene (synth.make_scene(4096, 4096), the bench scene),
drawn at `--size` / 4096 of its size.

  id map      the pixel centres of a size x size grid (the grid form: a workgroup is a 16 x 16 pixel tile)
  scattered   65 536 uniformly scattered points (the explicit form: a workgroup is 256 consecutive points, all over the canvas)
  numpy       tests/hit_ref.py's winding numbers of `--ref-points` of the scattered points, for scale

A point-edge test is one evaluation of the predicate of csrc/svgr_hit.h.  `nominal` counts points x edges, what a walk without the
cull would do (and what the numpy reference does); `walked` counts only the edges of the paths that survive the workgroup's cull,
worked out on the host from the same extents.  Times are the wall clock of the whole call -- upload of the tables, kernels,
download of the result, one wait -- the median of `--rounds` calls after a first one that also flattens; `device_ms` is the
stream's own time for the same call (svgr_measure_begin / _end).

Run alone under `timeout`.
    python profiles/bench_hit.py [--size 512] [--points 65536] [--ref-points 64] [--rounds 5] [--out PATH]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--paths", type=int, default=4096)
    ap.add_argument("--points", type=int, default=65536)
    ap.add_argument("--ref-points", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "bench_hit.json"))
    args = ap.parse_args()
    import numpy as np

    import svgrasterize_amd as S
    from svgrasterize_amd import _abi, synth
    from tests import hit_ref

    ctx = S.Context.get(0)
    block = ctx.lib.svgr_hit_block()
    tile = int(round(block ** 0.5))
    sc = synth.make_scene(4096, args.paths)
    m6 = sc["path_m6"] * (args.size / 4096.0)
    batch = _abi.Batch(ctx, sc["segs"], sc["seg_kind"], sc["path_seg_off"], m6, sc["path_rule"], sc["path_paint"], viewport=None)
    n = args.size
    rng = np.random.default_rng(1)
    scattered = rng.uniform(0.0, n, size=(args.points, 2))
    batch.pick(scattered[:block])   # (flattens and groups the edges: not timed)
    edges, edge_path = batch.all_edges()
    n_edges = len(edges)
    per_path = np.bincount(edge_path, minlength=args.paths).astype(np.int64)
    e = edges.reshape(-1, 4)
    ext = np.full((args.paths, 4), np.inf)
    ext[:, 2:] = -np.inf
    np.minimum.at(ext[:, 0], edge_path, np.minimum(e[:, 0], e[:, 2]))
    np.minimum.at(ext[:, 1], edge_path, np.minimum(e[:, 1], e[:, 3]))
    np.maximum.at(ext[:, 2], edge_path, np.maximum(e[:, 0], e[:, 2]))
    np.maximum.at(ext[:, 3], edge_path, np.maximum(e[:, 1], e[:, 3]))

    def walked(lo_a, lo_b, hi_b):
        """point-edge tests behind the cull: per workgroup (its points' extent) the edges of the paths that stay, x block lanes"""
        keep = (hi_b[:, None] >= ext[None, :, 1]) & (lo_b[:, None] < ext[None, :, 3]) & (ext[None, :, 2] > lo_a[:, None])
        return int((keep * per_path[None, :]).sum()) * block

    t0 = np.arange(0, n, tile, dtype=np.float64)
    ta, tb = np.meshgrid(t0, t0, indexing="ij")
    grid_walked = walked(ta.ravel() + 0.5, tb.ravel() + 0.5, np.minimum(tb.ravel() + tile, n) - 0.5)
    groups = scattered[: (args.points // block) * block].reshape(-1, block, 2)
    scat_walked = walked(groups[:, :, 0].min(axis=1), groups[:, :, 1].min(axis=1), groups[:, :, 1].max(axis=1))

    def timed(fn):
        fn()
        wall, dev = [], []
        for _ in range(args.rounds):
            ctx.sync()
            ctx.measure_begin(0.0)
            t = time.perf_counter()
            fn()
            wall.append((time.perf_counter() - t) * 1e3)
            dev.append(ctx.measure_end())
        return statistics.median(wall), min(wall), max(wall), statistics.median(dev)

    rows = []

    def report(name, n_points, n_walked, fn):
        wall, lo, hi, dev = timed(fn)
        nominal = n_points * n_edges
        rows.append(dict(query=name, points=n_points, paths=args.paths, edges=n_edges, wall_ms=round(wall, 3), min_ms=round(lo, 3),
                         max_ms=round(hi, 3), device_ms=round(dev, 3), nominal_tests=nominal, walked_tests=n_walked,
                         nominal_tests_per_s=round(nominal / wall * 1e3, 0), walked_tests_per_s=round(n_walked / wall * 1e3, 0)))
        print(json.dumps(rows[-1]), flush=True)

    report(f"id map {n} x {n} (grid)", n * n, grid_walked, lambda: batch.pick(grid=(0, 0, n, n)))
    report(f"{args.points} scattered points", args.points, scat_walked, lambda: batch.pick(scattered))
    sub = scattered[:args.ref_points]
    t = time.perf_counter()
    want = hit_ref.winding(edges, edge_path, args.paths, sub)
    ref_ms = (time.perf_counter() - t) * 1e3
    assert np.array_equal(batch.winding(sub), want)
    rows.append(dict(query=f"tests/hit_ref.py (numpy), {len(sub)} points", points=len(sub), edges=n_edges, wall_ms=round(ref_ms, 3),
                     nominal_tests=len(sub) * n_edges, nominal_tests_per_s=round(len(sub) * n_edges / ref_ms * 1e3, 0)))
    print(json.dumps(rows[-1]), flush=True)
    with open(args.out, "w") as f:
        json.dump(dict(device=ctx.name(), size=n, rounds=args.rounds, block=block, chunk=ctx.lib.svgr_hit_chunk(), rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
