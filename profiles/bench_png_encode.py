#!/usr/bin/env python3
"""PNG output: the device encoder (svgr_png_filter + svgr_deflate: adaptive filters, one dynamic code pair) against the host
routes of canvas_to_png on the same 8-bit canvases, wall clock and file size from one run.

Canvases: the synthetic scene of bench.py (synth4096: 4096 random closed cubic paths) rendered to 4096 x 4096 and quantised, and
tests/golden/scene_material.npz (demo/material-design.svg at 4096 x 4096) rendered as render_svg renders it.  Routes, each from
the host array (the device route uploads it, as canvas_to_png(encoder="device") does): device; zlib level 9 with 1 thread (the
reference's file); level 9 with 16 threads; level 1.  For the document also Layer.write_png on the device-resident layer, both
encoders (the device route then never downloads the pixels).  Every device file is decoded and compared with the canvas.

Run alone under `timeout`; for the kernels' own times run the same command with --device-only under
`rocprofv3 --kernel-trace --stats` (never together with counters).
    python profiles/bench_png_encode.py [--size 4096] [--reps 3] [--device-only] [--skip-png1]"""
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device-only", action="store_true", help="the device route alone (for a kernel trace)")
    ap.add_argument("--skip-png1", action="store_true", help="leave out the single-threaded level 9 file (seconds per file)")
    args = ap.parse_args()
    import numpy as np

    import svgrasterize_amd as S
    from svgrasterize_amd import _abi, scenedump, synth

    ctx = S.Context.get(0)
    n = args.size
    sc = synth.make_scene(n, {4096: 4096, 8192: 10000}.get(n, n))
    batch = _abi.Batch(ctx, sc["segs"], sc["seg_kind"], sc["path_seg_off"], sc["path_m6"], sc["path_rule"], sc["path_paint"],
                       viewport=sc["viewport"])
    batch.plan()
    out = ctx.alloc(n * n * 16)
    batch.render(out, _abi.OUT_CANVAS_F32, _abi.RENDER_CLIP01)
    canvases = {f"synth{n}": np.round(out.download((n, n, 4), np.float32) * 255.0).astype(np.uint8)}
    del out, batch

    layer = None
    if n == 4096:
        scene, info, _pins = scenedump.load_scene(os.path.join(ROOT, "tests", "golden", "scene_material.npz"))
        h, w = info["size"]
        layer, _hull = scene.render(S.Transform().matrix(0, 1, 0, 1, 0, 0), viewport=[0, 0, h, w], linear_rgb=False)
        layer = layer.convert(pre_alpha=True, linear_rgb=False).on_canvas(h, w)
        canvases[f"material{w}x{h}"] = layer.to_rgba8()

    def run(name, fn, reps):
        data = fn()   # (warm: the pool's blocks, the library's first launch)
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        ctx.sync()
        row = dict(op=name, ms=round((time.perf_counter() - t0) / reps * 1e3, 2), bytes=len(data))
        print(json.dumps(row), flush=True)
        return data

    for name, img in canvases.items():
        routes = [("device (adaptive, dynamic)", lambda: S.canvas_to_png(img, encoder="device").getvalue(), args.reps)]
        if not args.device_only:
            routes += [("host level 9, 16 threads", lambda: S.canvas_to_png(img, level=9, threads=16).getvalue(), args.reps),
                       ("host level 1", lambda: S.canvas_to_png(img, level=1).getvalue(), 1)]
            if not args.skip_png1:
                routes.append(("host level 9, 1 thread (the reference's file)", lambda: S.canvas_to_png(img).getvalue(), 1))
        for route, fn, reps in routes:
            data = run(f"{name}: canvas_to_png, {route}", fn, reps)
            if route.startswith("device"):
                assert np.array_equal(S.read_png(data), img), "the device file does not decode to the canvas"
    if layer is not None:
        run("material: Layer.write_png(encoder='device') from the device-resident layer", lambda: layer.write_png(encoder="device").getvalue(),
            args.reps)
        if not args.device_only:
            run("material: Layer.write_png(level=9, threads=16) from the device-resident layer",
                lambda: layer.write_png(None, 9, 16).getvalue(), args.reps)
        for filter, huffman in (("none", "dynamic"), ("adaptive", "fixed")):
            run(f"material: Layer.write_png(encoder='device', filter={filter!r}, huffman={huffman!r})",
                lambda: layer.write_png(encoder="device", filter=filter, huffman=huffman).getvalue(), 1)


if __name__ == "__main__":
    main()
