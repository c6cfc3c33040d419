#!/usr/bin/env python3
"""Dithered indexed PNG output: the device time of svgr_quant_dither in both modes next to the plain svgr_quant_index, the
end-to-end time and the size of the files of every mode under both encoders, and the device's diffusion against the host
build's sequential loop -- equal bit for bit, and timed.

Images: tests/golden/scene_icons4096.npz (demo/icons.svg at 4096 x 1051, the lossy route), and a synthetic 4096 x 4096 image
built here: a two-axis colour gradient under a blurred translucent shadow, opaque.  Device times are between two events on the
context's stream (svgr_measure_begin / _end), warm, the median of --reps runs; they include the wrapper's upload of the palette.
End-to-end times are a host clock around write_png, which ends in a wait.  The sequential loop is tests/dither_harness.cpp
(csrc/svgr_dither.h compiled for the host, -O2), one thread, on the 4096 x 1051 image.

Run alone under `timeout`:
    python profiles/bench_png_dither.py [--reps 5] [--out profiles/bench_png_dither.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic(n=4096):
    import numpy as np

    y, x = np.mgrid[0:n, 0:n].astype(np.float32) / np.float32(n - 1)
    img = np.empty((n, n, 4), dtype=np.uint8)
    shadow = np.exp(-(((x - 0.55) / 0.22) ** 2 + ((y - 0.6) / 0.16) ** 2)) * 0.7   # a soft drop shadow
    img[..., 0] = np.rint(255 * x * (1 - shadow))
    img[..., 1] = np.rint(255 * y * (1 - shadow))
    img[..., 2] = np.rint(255 * (1 - 0.5 * (x + y)) * (1 - shadow))
    img[..., 3] = 255
    return img


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the result as one JSON document")
    args = ap.parse_args()
    import numpy as np

    import svgrasterize_amd as S
    from svgrasterize_amd import _abi, quant, scenedump
    from tests import dither_ref

    ctx = S.Context.get(0)
    harness = dither_ref.harness()
    result = dict(device=ctx.name(), reps=args.reps, tile=_abi.dither_tile(), quant_block=_abi.quant_block(), workloads={})

    def device_ms(fn):
        fn()   # (warm: the pool's blocks, the first launch)
        times = []
        for _ in range(args.reps):
            ctx.sync()
            ctx.measure_begin()
            out = fn()
            times.append(ctx.measure_end())
        return out, round(statistics.median(times), 3)

    def wall_ms(fn, reps):
        fn()
        times = []
        for _ in range(reps):
            ctx.sync()
            t0 = time.perf_counter()
            out = fn()
            ctx.sync()
            times.append((time.perf_counter() - t0) * 1e3)
        return out, round(statistics.median(times), 3)

    scene, info, _pins = scenedump.load_scene(os.path.join(ROOT, "tests", "golden", "scene_icons4096.npz"))
    h, w = info["size"]
    layer, _hull = scene.render(S.Transform().matrix(0, 1, 0, 1, 0, 0), viewport=[0, 0, h, w], linear_rgb=False)
    icons = layer.convert(pre_alpha=True, linear_rgb=False).on_canvas(h, w).to_rgba8()
    del layer, scene
    for name, img in (("icons", icons), ("synthetic gradient and shadow", synthetic())):
        rows, cols = img.shape[:2]
        buf = ctx.from_host(img)
        palette, exact = quant.palette_and_route(buf, rows, cols, 256, 3)
        assert not exact, f"{name}: the image fits its palette, there is nothing to dither"
        amp = quant.ordered_amplitude(palette)
        row = dict(rows=rows, cols=cols, palette_entries=len(palette), ordered_amplitude=amp, device_ms={}, files={})
        (_, plain), row["device_ms"]["svgr_quant_index"] = device_ms(lambda: _abi.quant_index(ctx, buf, rows, cols, palette, True, True))
        n0 = ctx.launches()
        (_, ordered), row["device_ms"]["svgr_quant_dither, ordered"] = device_ms(lambda: _abi.quant_dither(ctx, buf, rows, cols, palette, "ordered", amp, True, True))
        n1 = ctx.launches()
        (_, diffused), row["device_ms"]["svgr_quant_dither, diffusion"] = device_ms(lambda: _abi.quant_dither(ctx, buf, rows, cols, palette, "diffusion", 0, True, True))
        row["diffusion_launches"] = (ctx.launches() - n1) // (args.reps + 1)
        assert (n1 - n0) // (args.reps + 1) == 1
        row["ordered_over_plain"] = round(row["device_ms"]["svgr_quant_dither, ordered"] / row["device_ms"]["svgr_quant_index"], 3)
        indices = {None: plain.download((rows, cols), np.uint8), "ordered": ordered.download((rows, cols), np.uint8),
                   "diffusion": diffused.download((rows, cols), np.uint8)}
        if rows * cols <= 4096 * 1051:
            t0 = time.perf_counter()
            _, host = dither_ref.harness_dither(harness, img, palette, "diffusion")
            row["host_sequential_diffusion_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
            assert np.array_equal(host, indices["diffusion"]), f"{name}: the device's diffusion is not the sequential loop's"
            assert np.array_equal(dither_ref.harness_dither(harness, img, palette, "ordered", amp)[1], indices["ordered"]), f"{name}: ordered differs"
            row["device_equals_host_bit_for_bit"] = True
            row["host_over_device"] = round(row["host_sequential_diffusion_ms"] / row["device_ms"]["svgr_quant_dither, diffusion"], 1)
        for mode in (None, "ordered", "diffusion"):
            for label, kw, reps in (("host level 9, 1 thread", dict(), 1), ("host level 9, 16 threads", dict(level=9, threads=16), args.reps),
                                    ("device", dict(encoder="device"), args.reps)):
                data, ms = wall_ms(lambda: S.canvas_to_png(img, palette=True, dither=mode, **kw).getvalue(), reps)
                assert np.array_equal(S.read_png(data), palette[indices[mode]]), f"{name}, {mode}, {label}: the file does not decode to palette[indices]"
                row["files"][f"dither={mode!r}, {label}"] = dict(bytes=len(data), ms=ms)
                print(json.dumps({"workload": name, "dither": mode, "file": label, "bytes": len(data), "ms": ms}), flush=True)
        print(json.dumps({"workload": name, **{k: v for k, v in row.items() if k != "files"}}), flush=True)
        result["workloads"][name] = row
        del buf, plain, ordered, diffused
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
