#!/usr/bin/env python3
"""Signed distance fields: the rate of svgr_batch_distance.

  union grid   the pixel centres of a size x size grid over the synthetic 4096-path scene (synth.make_scene(4096, 4096), the bench
               scene) drawn at `--size` / 4096 of its size, as one union field: at `--spread` (the cull skips the paths out of
               reach of a tile) and at an infinite spread (every tile walks every edge)
  atlas        `--glyphs` glyphs at `--px` pixels per em from tests/golden/fonts/: the committed variable font has six glyphs, so
               the atlas holds them at `--glyphs` / 6 positions of its first axis (sdf.glyphs_sdf_atlas, what Font.sdf_atlas
               draws with); the time is the whole call -- outlines on the device, layout, batch, one union grid query

A point-edge test is one evaluation of the distance and the winding term of csrc/svgr_sdf.h.  `nominal` counts points x edges, what
a walk without the cull would do; `walked` counts only the edges of the paths that survive a workgroup's cull, worked out on the
host from the same extents and the same rule.  Times are the wall clock of the whole call -- kernels, download of the result, one
wait -- the median of `--rounds` calls after a first one that also flattens; `device_ms` is the stream's own time for the same call
(svgr_measure_begin / _end).  There is no earlier implementation to compare with; profiles/bench_hit.json has the rate of
k_hit_winding, the kernel this one is modelled on, for scale.

Run alone under `timeout`.
    python profiles/bench_sdf.py [--size 512] [--spread 8] [--glyphs 96] [--px 48] [--rounds 5] [--out PATH]"""
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
    ap.add_argument("--spread", type=float, default=8.0)
    ap.add_argument("--glyphs", type=int, default=96)
    ap.add_argument("--px", type=float, default=48.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "bench_sdf.json"))
    args = ap.parse_args()
    import numpy as np

    import svgrasterize_amd as S
    from svgrasterize_amd import _abi, sdf, synth

    ctx = S.Context.get(0)
    block = ctx.lib.svgr_hit_block()
    tile = int(round(block ** 0.5))
    rows = []

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

    def extents(edges, edge_path, n_paths):
        e = edges.reshape(-1, 4)
        ext = np.full((n_paths, 4), np.inf)
        ext[:, 2:] = -np.inf
        np.minimum.at(ext[:, 0], edge_path, np.minimum(e[:, 0], e[:, 2]))
        np.minimum.at(ext[:, 1], edge_path, np.minimum(e[:, 1], e[:, 3]))
        np.maximum.at(ext[:, 2], edge_path, np.maximum(e[:, 0], e[:, 2]))
        np.maximum.at(ext[:, 3], edge_path, np.maximum(e[:, 1], e[:, 3]))
        return ext

    def grid_walked(ext, per_path, n_rows, n_cols, spread):
        """point-edge tests behind the cull of a grid query: per tile the edges of the paths that stay, x block lanes"""
        if not np.isfinite(spread):
            return int(per_path.sum()) * block * (-(-n_rows // tile)) * (-(-n_cols // tile))
        ta, tb = np.meshgrid(np.arange(0, n_rows, tile, dtype=np.float64), np.arange(0, n_cols, tile, dtype=np.float64), indexing="ij")
        lo_a, lo_b = ta.ravel()[:, None] + 0.5, tb.ravel()[:, None] + 0.5
        hi_a, hi_b = np.minimum(ta.ravel()[:, None] + tile, n_rows) - 0.5, np.minimum(tb.ravel()[:, None] + tile, n_cols) - 0.5
        with np.errstate(invalid="ignore"):
            thr = (spread * (1.0 + 2.0 ** -40) + 2.0 ** -40 * np.abs(ext).max(axis=1))[None, :]
            gone = (ext[None, :, 1] - hi_b > thr) | (lo_b - ext[None, :, 3] > thr) | (lo_a - ext[None, :, 2] > thr) | (ext[None, :, 0] - hi_a > thr)
        return int(((~gone) * per_path[None, :]).sum()) * block

    def report(name, n_points, n_paths, n_edges, n_walked, fn, **more):
        wall, lo, hi, dev = timed(fn)
        nominal = n_points * n_edges
        rows.append(dict(query=name, points=n_points, paths=n_paths, edges=n_edges, wall_ms=round(wall, 3), min_ms=round(lo, 3),
                         max_ms=round(hi, 3), device_ms=round(dev, 3), nominal_tests=nominal, walked_tests=n_walked,
                         nominal_tests_per_s=round(nominal / wall * 1e3, 0), walked_tests_per_s=round(n_walked / wall * 1e3, 0), **more))
        print(json.dumps(rows[-1]), flush=True)

    # ---- the union grid over the synthetic scene
    sc = synth.make_scene(4096, args.paths)
    m6 = sc["path_m6"] * (args.size / 4096.0)
    batch = _abi.Batch(ctx, sc["segs"], sc["seg_kind"], sc["path_seg_off"], m6, sc["path_rule"], sc["path_paint"], viewport=None)
    n = args.size
    batch.distance(grid=(0, 0, tile, tile), spread=args.spread, union=True)   # (flattens and groups the edges: not timed)
    edges, edge_path = batch.all_edges()
    per_path = np.bincount(edge_path, minlength=args.paths).astype(np.int64)
    ext = extents(edges, edge_path, args.paths)
    for spread, out in ((args.spread, "u8"), (args.spread, "f64"), (float("inf"), "f64")):
        report(f"union grid {n} x {n}, spread {spread:g}, {out}", n * n, args.paths, len(edges), grid_walked(ext, per_path, n, n, spread),
               lambda spread=spread, out=out: batch.distance(grid=(0, 0, n, n), spread=spread, out=out, union=True))
    batch.destroy()

    # ---- the glyph atlas
    with open(os.path.join(ROOT, "tests", "golden", "fonts", "varsynth.ttf"), "rb") as f:
        font = S.read_ttf(f.read())
    axis = font.axes[0]
    per_face = font.n_glyphs
    n_faces = -(-args.glyphs // per_face)
    glyphs, keys = [], []
    for k in range(n_faces):
        face = font.instance({axis.tag: axis.minimum + (axis.maximum - axis.minimum) * (k + 0.5) / n_faces})
        for gid in range(per_face):
            if len(glyphs) < args.glyphs:
                glyphs.append(face.glyph(gid))
                keys.append((k, gid))
    spread = 4.0
    atlas = sdf.glyphs_sdf_atlas(glyphs, keys, font.units_per_em, args.px, spread)   # (the outlines are made here: not timed again below)
    drawn = [key for key in keys if atlas.cells[key].rows]
    packs = [g.path.packed() for g, key in zip(glyphs, keys) if atlas.cells[key].rows]
    offs = np.concatenate([[0], np.cumsum([len(pk[0]) for pk in packs])]).astype(np.int64)
    scale = args.px / font.units_per_em
    twin = _abi.Batch(ctx, np.concatenate([pk[0] for pk in packs]), np.concatenate([pk[1] for pk in packs]), offs,
                      np.array([sdf.cell_m6(atlas.cells[key], scale) for key in drawn]), np.zeros(len(drawn), dtype=np.uint8), np.zeros((len(drawn), 4)),
                      viewport=None)
    a_edges, a_path = twin.all_edges()
    a_rows, a_cols = atlas.image.shape
    walked = grid_walked(extents(a_edges, a_path, len(drawn)), np.bincount(a_path, minlength=len(drawn)).astype(np.int64), a_rows, a_cols, spread)
    assert np.array_equal(twin.distance(grid=(0, 0, a_rows, a_cols), spread=spread, out="u8", union=True).reshape(a_rows, a_cols), atlas.image)
    twin.destroy()
    report(f"atlas of {len(glyphs)} glyphs at {args.px:g} px, spread {spread:g}, u8 (whole call)", a_rows * a_cols, len(drawn), len(a_edges), walked,
           lambda: sdf.glyphs_sdf_atlas(glyphs, keys, font.units_per_em, args.px, spread), image=[a_rows, a_cols], glyphs=len(glyphs), drawn=len(drawn))
    with open(args.out, "w") as f:
        json.dump(dict(device=ctx.name(), size=n, rounds=args.rounds, block=block, chunk=ctx.lib.svgr_hit_chunk(), rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
