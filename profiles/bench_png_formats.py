#!/usr/bin/env python3
"""PNG sample formats: the size and the write time of every (color, depth) file under both encoders against the 8-bit RGBA file
of the same encoder, from one run, and the device time of the two kernels behind them.

Workloads, each rendered at 4096 x 4096 and left on the device: tests/golden/scene_material.npz (demo/material-design.svg) as
render_svg renders it, and a linear gradient under a blurred, half-transparent disc (smooth ramps and a soft shadow: what 16 bits
are for).  Files: Layer.write_png(color=, depth=) for the four colours at both depths with encoder="device" (adaptive filters,
dynamic code) and encoder="host" (level 9, 16 threads), next to the existing 8-bit RGBA route of the same encoder (no color, no
depth: svgr_layer_to_rgba8 and k_png_filter) timed in the same run.  Every file is read back and compared with the 8-bit
conversion where the depth is 8.

Kernel times (--kernels): svgr_png_samples for every format and svgr_png_filter_bytes at every pixel size, with svgr_png_filter
beside the 4-byte one, launched in an order this script prints; run it under a kernel trace and hand the trace back with
--trace for the per-launch device times:

    python profiles/bench_png_formats.py --out profiles/bench_png_formats.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python profiles/bench_png_formats.py --kernels --plan DIR/plan.json
    python profiles/bench_png_formats.py --trace DIR --plan DIR/plan.json --out profiles/bench_png_formats.json   (merges)"""
import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COLORS = ("rgba", "rgb", "grey-alpha", "grey")
SIZE = 4096
GRADIENT = (f'<svg xmlns="http://www.w3.org/2000/svg" width="{SIZE}" height="{SIZE}"><defs>'
            '<linearGradient id="g" x1="0" y1="0" x2="1" y2="0.35"><stop offset="0" stop-color="#14203c"/>'
            '<stop offset="0.55" stop-color="#c8643c"/><stop offset="1" stop-color="#f4e8c8"/></linearGradient>'
            '<filter id="b" x="-50%" y="-50%" width="200%" height="200%"><feGaussianBlur stdDeviation="60"/></filter></defs>'
            f'<rect width="{SIZE}" height="{SIZE}" fill="url(#g)"/>'
            '<circle cx="1700" cy="2200" r="900" fill="#000000" fill-opacity="0.5" filter="url(#b)"/>'
            '<circle cx="1600" cy="2050" r="900" fill="#e8e0d0"/></svg>')


def workloads(S):
    from svgrasterize_amd import scenedump

    view = S.Transform().matrix(0, 1, 0, 1, 0, 0)
    scene, info, _pins = scenedump.load_scene(os.path.join(ROOT, "tests", "golden", "scene_material.npz"))
    h, w = info["size"]
    layer, _hull = scene.render(view, viewport=[0, 0, h, w], linear_rgb=False)
    yield "material-design", layer.convert(pre_alpha=True, linear_rgb=False).on_canvas(h, w)
    del layer, scene
    scene, _ids, _size = S.svg_scene_from_str(GRADIENT)
    layer, _hull = scene.render(view, viewport=[0, 0, SIZE, SIZE], linear_rgb=False)
    yield "gradient-blur", layer.convert(pre_alpha=True, linear_rgb=False).on_canvas(SIZE, SIZE)


def files(args):
    import numpy as np

    import svgrasterize_amd as S
    from svgrasterize_amd import _abi, png

    ctx = S.Context.get(0)
    result = dict(device=ctx.name(), reps=args.reps, filter_span=_abi.png_filter_span(), workloads={})

    def timed(fn, reps):
        out = fn()   # (warm: the pool's blocks, the first launch)
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(reps):
            out = fn()
        ctx.sync()
        return out, round((time.perf_counter() - t0) / reps * 1e3, 3)

    for name, layer in workloads(S):
        rows, cols = layer.height, layer.width
        rgba8 = layer.to_rgba8()
        row = dict(rows=rows, cols=cols, files={})
        for encoder, kw, reps in (("device", dict(encoder="device"), args.reps), ("host level 9, 16 threads", dict(level=9, threads=16), 1)):
            base, base_ms = timed(lambda: layer.write_png(**kw).getvalue(), reps)
            row["files"][f"{encoder}: existing RGBA8 route"] = dict(bytes=len(base), ms=base_ms)
            print(json.dumps({"workload": name, "encoder": encoder, "file": "existing RGBA8 route", "bytes": len(base), "ms": base_ms}), flush=True)
            for color in COLORS:
                for depth in (8, 16):
                    data, ms = timed(lambda: layer.write_png(color=color, depth=depth, **kw).getvalue(), reps)
                    got, colour_type, got_depth = png.read_samples(data)
                    assert (colour_type, got_depth) == (png.COLORS[color], depth)
                    if (color, depth) == ("rgba", 8):
                        assert np.array_equal(got, rgba8), "the new route's 8-bit RGBA samples are not to_rgba8's"
                    row["files"][f"{encoder}: {color} {depth}"] = dict(bytes=len(data), ms=ms, ms_over_rgba8_route=round(ms / base_ms, 3),
                                                                        bytes_over_rgba8_route=round(len(data) / len(base), 4))
                    print(json.dumps({"workload": name, "encoder": encoder, "file": f"{color} {depth}", "bytes": len(data), "ms": ms}), flush=True)
        result["workloads"][name] = row
        del layer
    return result


def kernels(args):
    """Every kernel `reps` times, in the order written to --plan: the trace's launches of k_png_* in order are these."""
    import svgrasterize_amd as S
    from svgrasterize_amd import _abi, png

    ctx = S.Context.get(0)
    plan = []
    for name, layer in workloads(S):
        rows, cols = layer.height, layer.width
        src = layer.convert(pre_alpha=False, linear_rgb=False)._device()
        ctx.sync()
        for color in COLORS:
            for depth in (8, 16):
                colour_type = png.COLORS[color]
                bpp = _abi.PNG_CHANNELS[colour_type] * depth // 8
                for _ in range(args.reps):
                    samples = _abi.png_samples(ctx, src, _abi.PNG_SRC_RGBA_F64, rows, cols, colour_type, depth)
                plan.append(dict(workload=name, kernel="k_png_samples", what=f"{color} {depth}", launches=args.reps,
                                 bytes_read=rows * cols * 32, bytes_written=rows * cols * bpp))
                for _ in range(args.reps):
                    _abi.png_filter_bytes(ctx, samples, rows, cols * bpp, bpp, 5)
                plan.append(dict(workload=name, kernel="k_png_filter_bytes", what=f"bpp {bpp} ({color} {depth}), adaptive", launches=args.reps,
                                 bytes_read=rows * cols * bpp, bytes_written=rows * (1 + cols * bpp)))
                if bpp == 4:
                    for _ in range(args.reps):
                        _abi.png_filter(ctx, samples, rows, cols, 5)
                    plan.append(dict(workload=name, kernel="k_png_filter", what="the existing RGBA8 kernel on the same bytes, adaptive",
                                     launches=args.reps, bytes_read=rows * cols * 4, bytes_written=rows * (1 + cols * 4)))
                ctx.sync()
                del samples
        del layer, src
    with open(args.plan, "w") as f:
        json.dump(plan, f)
    print(f"{len(plan)} steps, {sum(p['launches'] for p in plan)} launches")


def _is_kernel(name, kernel):
    if kernel == "k_png_filter":
        return "k_png_filter" in name and "k_png_filter_bytes" not in name
    return kernel in name


def merge_trace(args, result):
    with open(args.plan) as f:
        plan = json.load(f)
    path = glob.glob(os.path.join(args.trace, "**", "*kernel_trace.csv"), recursive=True)
    assert len(path) == 1, path
    with open(path[0], newline="") as f:
        launches = [r for r in csv.DictReader(f) if "k_png_samples" in r["Kernel_Name"] or "k_png_filter" in r["Kernel_Name"]]
    launches.sort(key=lambda r: int(r["Start_Timestamp"]))
    assert len(launches) == sum(p["launches"] for p in plan), (len(launches), sum(p["launches"] for p in plan))
    at, out = 0, []
    for p in plan:
        mine = launches[at:at + p["launches"]]
        at += p["launches"]
        assert all(_is_kernel(r["Kernel_Name"], p["kernel"]) for r in mine), (p, mine[0]["Kernel_Name"])
        us = sorted((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in mine)
        med = us[len(us) // 2]
        out.append(dict(p, us_median=round(med, 1), us_min=round(us[0], 1), us_max=round(us[-1], 1),
                        gb_per_s=round((p["bytes_read"] + p["bytes_written"]) / med / 1e3, 1)))
    result["kernels"] = out
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernels", action="store_true", help="launch the kernels alone, for a kernel trace")
    ap.add_argument("--plan", default=None, help="with --kernels: where the launch order goes; with --trace: where it is")
    ap.add_argument("--trace", default=None, help="the directory of a kernel trace of a --kernels run: merge its times into --out")
    ap.add_argument("--out", default=None, help="write (or, with --trace, update) the result as one JSON document")
    args = ap.parse_args()
    if args.kernels:
        return kernels(args)
    if args.trace:
        with open(args.out) as f:
            result = merge_trace(args, json.load(f))
    else:
        result = files(args)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
