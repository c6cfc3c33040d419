#!/usr/bin/env python3
"""Indexed PNG output: the time of each stage of Layer.write_png(palette=True) and the sizes of its files against the RGBA files
of the same pixels, from one run.

Workloads: tests/golden/scene_material.npz (demo/material-design.svg) and tests/golden/scene_icons4096.npz (demo/icons.svg), each
rendered at 4096 x 4096 as render_svg renders it and left on the device.  Stages, each timed alone between two waits for the
device: the 8-bit conversion, svgr_quant_distinct, svgr_quant_bins (with its download), the host's palette builder,
svgr_quant_index, svgr_deflate of the index rows, and the host's zlib over the downloaded rows.  Files: palette=True under both
encoders (the host one at level 9 with 1 and with 16 threads), the RGBA device file (adaptive filters, dynamic code) and the RGBA
host level 9 file.  Every indexed file is decoded and compared with palette[indices].

Run alone under `timeout`:
    python profiles/bench_png_palette.py [--reps 3] [--skip-rgba-host] [--out profiles/bench_png_palette.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-rgba-host", action="store_true", help="leave out the RGBA level 9 file of one thread (seconds per file)")
    ap.add_argument("--out", default=None, help="also write the result as one JSON document")
    args = ap.parse_args()
    import zlib

    import numpy as np

    import svgrasterize_amd as S
    from svgrasterize_amd import _abi, quant, scenedump

    ctx = S.Context.get(0)
    result = dict(device=ctx.name(), reps=args.reps, quant_block=_abi.quant_block(), workloads={})

    def timed(fn, reps=args.reps):
        out = fn()   # (warm: the pool's blocks, the first launch)
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(reps):
            out = fn()
        ctx.sync()
        return out, round((time.perf_counter() - t0) / reps * 1e3, 3)

    for name, file in (("material-design", "scene_material.npz"), ("icons", "scene_icons4096.npz")):
        scene, info, _pins = scenedump.load_scene(os.path.join(ROOT, "tests", "golden", file))
        h, w = info["size"]
        layer, _hull = scene.render(S.Transform().matrix(0, 1, 0, 1, 0, 0), viewport=[0, 0, h, w], linear_rgb=False)
        layer = layer.convert(pre_alpha=True, linear_rgb=False).on_canvas(h, w)
        row = dict(rows=h, cols=w, stages_ms={}, files={})
        (buf, rows, cols), row["stages_ms"]["to_rgba8 (device)"] = timed(layer._to_rgba8_device)
        exact, row["stages_ms"]["svgr_quant_distinct"] = timed(lambda: _abi.quant_distinct(ctx, buf, rows, cols, 256))
        (keys, bins), row["stages_ms"]["svgr_quant_bins"] = timed(lambda: _abi.quant_bins(ctx, buf, rows, cols))
        row["distinct_colours"] = None if exact is None else len(exact)
        row["bins"] = len(keys)
        lossy, row["stages_ms"]["palette builder (host, median cut + 3 Lloyd)"] = timed(lambda: quant.build_palette(bins, 256, 3), 1)
        palette = quant.order_palette(quant.colors_of_u32(exact)) if exact is not None else lossy
        row["route"] = "exact" if exact is not None else "lossy"
        row["palette_entries"] = len(palette)
        (stream, _), row["stages_ms"]["svgr_quant_index (row stream)"] = timed(lambda: _abi.quant_index(ctx, buf, rows, cols, palette))
        (_, plain), row["stages_ms"]["svgr_quant_index (plain indices)"] = timed(lambda: _abi.quant_index(ctx, buf, rows, cols, palette, False, True))
        n_bytes = rows * (1 + (cols * quant.depth_of(len(palette)) + 7) // 8)
        _, row["stages_ms"]["svgr_deflate of the index rows"] = timed(lambda: _abi.deflate(ctx, stream, n_bytes, 1))
        raw, row["stages_ms"]["download of the index rows"] = timed(lambda: stream.download((n_bytes,), np.uint8).tobytes())
        _, row["stages_ms"]["zlib level 9 of the index rows (host, 1 thread)"] = timed(lambda: zlib.compress(raw, 9), 1)
        want = palette[plain.download((rows, cols), np.uint8)]

        def file_of(label, fn, reps=args.reps):
            data, ms = timed(fn, reps)
            row["files"][label] = dict(bytes=len(data), ms=ms)
            print(json.dumps({"workload": name, "file": label, "bytes": len(data), "ms": ms}), flush=True)
            return data

        for label, kw in (("palette=True, host level 9, 1 thread", dict()), ("palette=True, host level 9, 16 threads", dict(level=9, threads=16)),
                          ("palette=True, device", dict(encoder="device")), ("palette=True, device, fixed code", dict(encoder="device", huffman="fixed"))):
            data = file_of(label, lambda: layer.write_png(palette=True, **kw).getvalue(), 1 if "1 thread" in label else args.reps)
            assert np.array_equal(S.read_png(data), want), f"{label}: the file does not decode to palette[indices]"
        file_of("RGBA, device (adaptive, dynamic)", lambda: layer.write_png(encoder="device").getvalue())
        file_of("RGBA, host level 9, 16 threads", lambda: layer.write_png(None, 9, 16).getvalue())
        if not args.skip_rgba_host:
            file_of("RGBA, host level 9, 1 thread (the reference's file)", lambda: layer.write_png().getvalue(), 1)
        if exact is not None:
            assert np.array_equal(want, quant.canonical(layer.to_rgba8())), "the exact route lost a colour"
        print(json.dumps({"workload": name, **{k: v for k, v in row.items() if k != "files"}}), flush=True)
        result["workloads"][name] = row
        del layer, buf, stream, plain
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
