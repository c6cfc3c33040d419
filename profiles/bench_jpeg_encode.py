#!/usr/bin/env python3
"""JPEG output: rate of the two encode kernels (k_jpeg_planes, k_jpeg_fdct) on a 4096 x 4096 RGBA8 canvas at 4:4:4 and 4:2:0,
and the wall clock of a document's output stage as JPEG against PNG.

Kernel part: wall clock per svgr_jpeg_encode call (both kernels, the upload of the tables, the download of the coefficients and
one wait), bytes = what the two kernels must move (4 read per pixel; per sample 1 written by k_jpeg_planes, 1 read and 2 written
by k_jpeg_fdct: 16 B per pixel at 4:4:4, 10 B at 4:2:0), priced against the 6.29 TB/s copy rate.  The coefficient download
(6 or 3 B per pixel over PCIe) is inside the wall clock, so run the script alone under `rocprofv3 --kernel-trace --stats` for
the kernel times themselves (never together with counters).

Document part: tests/golden/scene_material.npz (demo/material-design.svg at 4096 x 4096) rendered as render_svg renders it
(Scene.render, on_canvas), then written as JPEG (quality 90, 4:2:0, optimised tables, over white) and as PNG at level 9 with
threads = 1 and threads = 16: wall clock of render + output, and of the output stage alone.
    python profiles/bench_jpeg_encode.py [--size 4096] [--reps 5] [--skip-png1]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-png1", action="store_true", help="leave out the single-threaded level 9 PNG (seconds per file)")
    args = ap.parse_args()
    import numpy as np

    import svgrasterize_amd as S
    from svgrasterize_amd import _abi, jpeg, scenedump

    ctx = S.Context.get(0)
    n = args.size
    rng = np.random.default_rng(1)
    yy, xx = np.mgrid[:n, :n]
    img = np.stack([(xx * 255 // n), (yy * 255 // n), ((xx + yy) * 255 // (2 * n)), np.full((n, n), 255)], axis=2).astype(np.uint8)
    img[..., :3] ^= rng.integers(0, 8, (n, n, 3), dtype=np.uint8)
    dev = ctx.from_host(img)
    quant = jpeg.quant_tables(90)[[0, 1, 1]]
    res = []

    def run(name, nbytes, fn, reps=args.reps):
        fn()
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        ctx.sync()
        dt = (time.perf_counter() - t0) / reps
        row = dict(op=name, ms=round(dt * 1e3, 3))
        if nbytes:
            row.update(gbs=round(nbytes / dt / 1e9, 1), frac_of_6290=round(nbytes / dt / 6.29e12, 3))
        res.append(row)

    for name, per_px in (("4:4:4", 16), ("4:2:0", 10)):
        frame = _abi.JpegFrame()
        frame.width = frame.height = n
        frame.n_comp, frame.colour = 3, _abi.JPEG_YCBCR
        frame.h[0], frame.v[0] = jpeg.SUBSAMPLINGS[name]
        frame.h[1] = frame.v[1] = frame.h[2] = frame.v[2] = 1
        run(f"svgr_jpeg_encode {name} {n}^2 (k_jpeg_planes + k_jpeg_fdct + coefficient download)", n * n * per_px,
            lambda f=frame: _abi.jpeg_encode(ctx, f, dev, quant))
        coef = _abi.jpeg_encode(ctx, frame, dev, quant)
        run(f"host entropy coding {name} {n}^2 (symbol counts, optimal tables, svgr_jpeg_entropy_encode)", 0,
            lambda f=frame, c=coef: jpeg.encode_frame(f, c, quant), reps=2)

    scene, info, _pins = scenedump.load_scene(os.path.join(ROOT, "tests", "golden", "scene_material.npz"))
    h, w = info["size"]
    tr = S.Transform().matrix(0, 1, 0, 1, 0, 0)

    def canvas():
        layer, _hull = scene.render(tr, viewport=[0, 0, h, w], linear_rgb=False)
        return layer.convert(pre_alpha=True, linear_rgb=False).on_canvas(h, w)

    layer = canvas()
    routes = [("JPEG q90 4:2:0", lambda l: l.write_jpeg()), ("PNG level 9 threads 16", lambda l: l.write_png(None, 9, 16))]
    if not args.skip_png1:
        routes.append(("PNG level 9 threads 1", lambda l: l.write_png(None, 9, 1)))
    for name, write in routes:
        reps = 1 if name.endswith("threads 1") else 3
        run(f"material {w}x{h}: render + {name}", 0, lambda: write(canvas()), reps=reps)
        run(f"material {w}x{h}: output stage alone, {name}", 0, lambda: write(layer), reps=reps)
    for r in res:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
