#!/usr/bin/env python3
"""Tensor output: device time of svgr_layer_to_tensor at size x size against the kernel that has moved the same bytes all along,
and the wall clock of getting a layer to the host through it.

  yardstick   svgr_layer_to_f32 (k_to_f32: float64 RGBA in, float32 out, a lane per value) -- of this build and, with
              --parent-lib, of a libsvgr_hip.so built from the parent commit, loaded beside it
  hwc/f32     the new kernel moving the same bytes (32 in, 16 out per pixel)
  chw         planar, every element type, RGBA and RGB
  wall        Layer.image (float64 HWC, 32 bytes per pixel over PCIe) against Layer.to_array(dtype=float16) (8)

Device times are svgr_measure_begin / _end around `--reps` launches queued behind a hold (the stream's own time, no host in it),
taken `--rounds` times with the routes alternating; the median and the spread of the rounds are reported.  Bytes are what the
algorithm needs (source pixels read once, elements written once), so GB/s is a rate over that, not a counter.

Run alone under `timeout`.
    python profiles/bench_tensor_out.py [--size 4096] [--reps 20] [--rounds 5] [--parent-lib PATH] [--out PATH]"""
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
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="a libsvgr_hip.so built from the parent commit: its svgr_layer_to_f32 is timed too")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "bench_tensor_out.json"))
    args = ap.parse_args()
    import numpy as np

    import svgrasterize_amd as S
    from svgrasterize_amd import _abi, tensor

    ctx = S.Context.get(0)
    lib = ctx.lib
    n = args.size
    px = n * n
    rng = np.random.default_rng(1)
    tile = rng.uniform(0, 1, (256, n, 4))
    tile[..., :3] *= tile[..., 3:]
    src = ctx.alloc(px * 32)
    for r0 in range(0, n, 256):
        src.upload(tile[:min(256, n - r0)], offset=r0 * n * 32)
    dst = ctx.alloc(px * 16)
    bbox = (C.c_int64 * 4)(0, 0, n, n)

    def device_ms(enqueue):
        enqueue()
        ctx.sync()
        ctx.measure_begin(20.0)
        for _ in range(args.reps):
            enqueue()
        return ctx.measure_end() / args.reps

    routes = {}

    def yardstick():
        _abi._check(lib.svgr_layer_to_f32(ctx.handle, dst.handle, src.handle, px * 4, 0))

    routes["svgr_layer_to_f32 (yardstick, this build)"] = (yardstick, px * 48)

    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        P = C.c_void_p
        parent.svgr_layer_to_f32.argtypes = [P, P, P, C.c_int64, C.c_int]
        parent.svgr_init.argtypes = [C.c_int, C.POINTER(P)]
        parent.svgr_buf_wrap.argtypes = [P, P, C.c_size_t, C.POINTER(P)]
        parent.svgr_measure_begin.argtypes = [P, C.c_double]
        parent.svgr_measure_end.argtypes = [P, C.POINTER(C.c_double)]
        parent.svgr_sync.argtypes = [P]
        pctx, psrc, pdst = P(), P(), P()
        assert parent.svgr_init(0, C.byref(pctx)) == 0
        assert parent.svgr_buf_wrap(pctx, P(src.ptr), px * 32, C.byref(psrc)) == 0
        assert parent.svgr_buf_wrap(pctx, P(dst.ptr), px * 16, C.byref(pdst)) == 0

        def parent_ms():
            assert parent.svgr_layer_to_f32(pctx, pdst, psrc, px * 4, 0) == 0
            parent.svgr_sync(pctx)
            assert parent.svgr_measure_begin(pctx, 20.0) == 0
            for _ in range(args.reps):
                parent.svgr_layer_to_f32(pctx, pdst, psrc, px * 4, 0)
            ms = C.c_double()
            assert parent.svgr_measure_end(pctx, C.byref(ms)) == 0
            return ms.value / args.reps

        routes["svgr_layer_to_f32 (yardstick, parent build)"] = (parent_ms, px * 48)

    def pack(dtype, layout, channels):
        nch = tensor.N_CHANNELS[channels]
        d = tensor._desc(dtype, channels, n, n, tensor._dense_strides(layout, nch, n, n))

        def enqueue():
            _abi._check(lib.svgr_layer_to_tensor(ctx.handle, C.byref(d), src.handle, bbox, dst.handle))
        return enqueue, px * (32 + nch * tensor._ELEM_BYTES[dtype])

    names = {_abi.TENSOR_F32: "f32", _abi.TENSOR_F16: "f16", _abi.TENSOR_BF16: "bf16", _abi.TENSOR_U8: "u8"}
    routes["svgr_layer_to_tensor hwc/f32/rgba"] = pack(_abi.TENSOR_F32, "hwc", "rgba")
    for dtype, name in names.items():
        for channels in ("rgba", "rgb"):
            routes[f"svgr_layer_to_tensor chw/{name}/{channels}"] = pack(dtype, "chw", channels)
    routes["svgr_layer_to_tensor hwc/u8/rgba"] = pack(_abi.TENSOR_U8, "hwc", "rgba")

    samples = {name: [] for name in routes}
    for _ in range(args.rounds):
        for name, (fn, _bytes) in routes.items():
            samples[name].append(fn() if "parent build" in name else device_ms(fn))
    rows = []
    for name, (fn, nbytes) in routes.items():
        ms = statistics.median(samples[name])
        rows.append(dict(route=name, device_ms=round(ms, 4), min_ms=round(min(samples[name]), 4), max_ms=round(max(samples[name]), 4),
                         gb_per_s=round(nbytes / ms / 1e6, 1), mb=round(nbytes / 1e6, 1)))
        print(json.dumps(rows[-1]), flush=True)

    def wall(name, fn, reps=3):
        fn()
        ctx.sync()
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            times.append((time.perf_counter() - t0) * 1e3)
        rows.append(dict(route=name, wall_ms=round(statistics.median(times), 2), min_ms=round(min(times), 2), max_ms=round(max(times), 2)))
        print(json.dumps(rows[-1]), flush=True)

    def layer():
        return S.Layer._from_device(src, (n, n, 4), (0, 0), True, False)

    wall("Layer.image (float64 hwc to the host)", lambda: layer().image)
    wall("Layer.to_array(dtype=float16) (chw to the host)", lambda: layer().to_array(dtype=np.float16))
    wall("Layer.to_array(dtype=uint8, layout='hwc')", lambda: layer().to_array(dtype=np.uint8, layout="hwc"))
    result = dict(device=ctx.name(), size=n, reps=args.reps, rounds=args.rounds, rows=rows)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
