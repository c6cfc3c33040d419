#!/usr/bin/env python3
"""Rate of the SVG <image> kernels at a 4096 x 4096 output: k_image_fill for a 512^2 image upscaled, a 2048^2 image
rotated by 30 degrees, an 8192^2 image shrunk to 4096^2 (trilinear) and nearest mode; and the upload + mip build of each
image.  Wall clock per call (host clock around work that ends in a synchronise); bytes = what the op must move: the fill
reads the mask (8 B / pixel) and writes the premultiplied double result (32 B / pixel), the texel reads are not counted;
the upload's device work reads 4 B and writes 16 B per level-0 texel, then every level is read once (16 B / texel) to write
the next (16 B / texel); its wall clock also holds the host-to-device copy of the bytes.
Run it under `rocprofv3 --kernel-trace --stats` for the kernel times alone.
    python profiles/bench_image_ops.py [--size 4096] [--reps 5]"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import numpy as np

    import svgrasterize_amd as S
    from svgrasterize_amd import _abi, paint

    ctx = S.Context.get(0)
    n = args.size
    swap = S.Transform().matrix(0, 1, 0, 1, 0, 0)
    mask = ctx.from_host(np.ones((n, n)))
    out = ctx.alloc(n * n * 32)
    bbox = (C.c_int64 * 4)(0, 0, n, n)
    rng = np.random.default_rng(1)
    res = []

    def timed(fn):
        fn()
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            fn()
        ctx.sync()
        return (time.perf_counter() - t0) / args.reps

    def row(name, nbytes, dt):
        res.append(dict(op=name, ms=round(dt * 1e3, 3), gbs=round(nbytes / dt / 1e9, 1), frac_of_6290=round(nbytes / dt / 6.29e12, 3)))

    cases = [
        ("upscale 512^2 -> 4096^2", 512, swap.scale(n / 512), True),
        ("rotate 30 deg 2048^2 (x 1.4)", 2048, swap.translate(n / 2, -n * 0.15).rotate(math.radians(30)).scale(1.4), True),
        ("shrink 8192^2 -> 3686^2 (trilinear)", 8192, swap.scale(0.45), True),
        ("nearest, rotate 30 deg 2048^2 (x 1.4)", 2048, swap.translate(n / 2, -n * 0.15).rotate(math.radians(30)).scale(1.4), False),
    ]
    images = {}
    for name, size, fwd, smooth in cases:
        if size not in images:
            px = rng.integers(0, 256, (size, size, 4), dtype=np.uint8)
            levels = _abi.image_levels(size, size)
            texels = levels[-1][0] + 1
            mip_bytes = size * size * 20 + 16 * (texels - 1) + 16 * (texels - size * size)
            dt = timed(lambda px=px: _abi.image_upload(ctx, px, True))
            row(f"svgr_image_upload {size}^2 (host copy + k_image_prepare + k_image_downsample x {len(levels) - 1})", mip_bytes, dt)
            images[size] = _abi.image_upload(ctx, px, True)
        inv = fwd.invert.m
        im = _abi.ImageArgs()
        im.inv_m6 = (C.c_double * 6)(*np.asarray(inv, dtype=np.float64)[:2].ravel())
        im.height = im.width = size
        im.smooth = int(smooth)
        im.lod = paint.image_lod(inv, len(_abi.image_levels(size, size))) if smooth else 0.0
        buf = images[size]
        dt = timed(lambda im=im, buf=buf: _abi._check(ctx.lib.svgr_image_fill(ctx.handle, C.byref(im), buf.handle, mask.handle, bbox, out.handle)))
        row(f"k_image_fill {name} (lod {im.lod:.2f})", n * n * 40, dt)
    for r in res:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
