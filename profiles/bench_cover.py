#!/usr/bin/env python3
"""Differentiable coverage: the time of svgr_cover_forward and svgr_cover_backward.

  one glyph    the glyph of tests/golden/fonts/varsynth.ttf with the most segments, scaled to fill a 64 x 64 and a 256 x 256 viewport
  256 paths    that font's glyphs on a 16 x 16 grid over one 256 x 256 viewport, a plane per path (256 planes of 256 x 256)

Every array is on the device before the clock starts and stays there: a time is the call alone -- the launches of one pass on the
context's stream and one wait -- as the wall clock sees it (`wall_ms`) and as the stream does (`device_ms`, svgr_measure_begin /
_end); the median of `--rounds` calls after a first one.  float32 planes (what diff.coverage_tensor makes by default) and, for the
single glyph, float64 ones.  grad_out is standard normal.  There is no earlier implementation to compare with.

Run alone under `timeout`.
    python profiles/bench_cover.py [--rounds 7] [--out PATH]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "bench_cover.json"))
    args = ap.parse_args()
    import numpy as np

    import svgrasterize_amd as S
    from svgrasterize_amd import _abi, diff

    ctx = S.Context.get(0)
    with open(os.path.join(ROOT, "tests", "golden", "fonts", "varsynth.ttf"), "rb") as f:
        font = S.read_ttf(f.read())
    packs = [font.glyph(gid).path.packed() for gid in range(font.n_glyphs)]
    packs = [pk for pk in packs if len(pk[0])]
    big = max(packs, key=lambda pk: len(pk[0]))

    def fit(pk, r0, c0, rows, cols):
        """m6 that puts the glyph's control box into rows x cols at (r0, c0): user (x, y up) -> (row, col)."""
        pts = pk[0].reshape(-1, 4, 2)
        used = np.concatenate([pts[:, :2].reshape(-1, 2), pts[pk[1] != 0][:, 2:].reshape(-1, 2)])
        x0, y0, x1, y1 = used[:, 0].min(), used[:, 1].min(), used[:, 0].max(), used[:, 1].max()
        s = 0.9 * min(cols / max(x1 - x0, 1e-9), rows / max(y1 - y0, 1e-9))
        return [0.0, -s, r0 + 0.05 * rows + s * y1, s, 0.0, c0 + 0.05 * cols - s * x0]

    def timed(fn):
        fn()
        ctx.sync()
        wall, dev = [], []
        for _ in range(args.rounds):
            ctx.measure_begin(0.0)
            t = time.perf_counter()
            fn()
            ctx.sync()
            wall.append((time.perf_counter() - t) * 1e3)
            dev.append(ctx.measure_end())
        return statistics.median(wall), statistics.median(dev)

    results = []

    def run(name, segs, kinds, off, m6, rules, vp, dtype):
        n_paths, n_px = len(m6), len(m6) * vp[2] * vp[3]
        plane = _abi.COVER_F64 if dtype == np.float64 else _abi.COVER_F32
        d_segs, d_kinds, d_off, d_m6 = diff._upload(ctx, np.ascontiguousarray(segs, dtype=np.float64), np.ascontiguousarray(kinds, dtype=np.uint8),
                                                    np.ascontiguousarray(off, dtype=np.int32), np.ascontiguousarray(m6, dtype=np.float64))
        d_rules = ctx.from_host(np.ascontiguousarray(rules, dtype=np.uint8))
        cover, slope, status = ctx.alloc(n_px * np.dtype(dtype).itemsize), ctx.alloc(n_px), ctx.alloc(4)
        status.zero()
        grad = ctx.from_host(np.random.default_rng(1).standard_normal(n_px).astype(dtype))
        g_segs, g_m6 = ctx.alloc(len(segs) * 64), ctx.alloc(n_paths * 48)
        desc = diff._desc(len(segs), n_paths, vp, plane, diff.FLATNESS)

        def forward():
            _abi._check(ctx.lib.svgr_cover_forward(ctx.handle, C.byref(desc), d_segs.handle, d_kinds.handle, d_off.handle, d_m6.handle, d_rules.handle,
                                                   cover.handle, slope.handle, status.handle))

        def backward():
            _abi._check(ctx.lib.svgr_cover_backward(ctx.handle, C.byref(desc), d_segs.handle, d_kinds.handle, d_off.handle, d_m6.handle, slope.handle,
                                                    grad.handle, g_segs.handle, g_m6.handle, status.handle))

        fw, fd = timed(forward)
        bw, bd = timed(backward)
        assert int(status.download((1,), np.uint32)[0]) == 0
        covered = float(cover.download((n_px,), dtype).astype(np.float64).sum())
        row = dict(case=name, paths=n_paths, segments=len(segs), viewport=list(vp[2:]), plane=np.dtype(dtype).name, covered_pixels=round(covered, 1),
                   forward_wall_ms=round(fw, 4), forward_device_ms=round(fd, 4), backward_wall_ms=round(bw, 4), backward_device_ms=round(bd, 4))
        results.append(row)
        print(json.dumps(row))

    for size in (64, 256):
        for dtype in (np.float32, np.float64):
            run(f"one glyph at {size} x {size}", big[0], big[1], [0, len(big[0])], [fit(big, 0, 0, size, size)], [0], (0, 0, size, size), dtype)
    cells = [(k, packs[k % len(packs)]) for k in range(256)]
    segs = np.concatenate([pk[0] for _k, pk in cells])
    kinds = np.concatenate([pk[1] for _k, pk in cells])
    off = np.concatenate([[0], np.cumsum([len(pk[0]) for _k, pk in cells])])
    m6 = [fit(pk, 16 * (k // 16), 16 * (k % 16), 16, 16) for k, pk in cells]
    run("256 paths at 256 x 256", segs, kinds, off, m6, np.zeros(256, dtype=np.uint8), (0, 0, 256, 256), np.float32)
    with open(args.out, "w") as f:
        json.dump(dict(device=ctx.name(), rounds=args.rounds, cover_block=diff.cover_block(), cover_scan=diff.cover_scan(), results=results), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
