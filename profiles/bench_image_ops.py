#!/usr/bin/env python3
"""Rate of the SVG <image> kernels at a 4096 x 4096 output: k_image_fill for a 512^2 image upscaled, a 2048^2 image
rotated by 30 degrees, an 8192^2 image shrunk to 4096^2 (trilinear) and nearest mode; and the upload + mip build of each
image.  Wall clock per call (host clock around work that ends in a synchronise); bytes = what the op must move: the fill
reads the mask (8 B / pixel) and writes the premultiplied double result (32 B / pixel), the texel reads are not counted;
the upload's device work reads 4 B and writes 16 B per level-0 texel, then every level is read once (16 B / texel) to write
the next (16 B / texel); its wall clock also holds the host-to-device copy of the bytes.
The JPEG case decodes a size x size 4:2:0 baseline image (written by Pillow from a synthetic picture when Pillow is there, else
the coefficients of tests/golden/jpeg/ycc420_photo.jpg tiled): the host's marker + entropy time, then svgr_jpeg_decode, whose
wall clock holds the host-to-device copy of the coefficients; its kernels (k_jpeg_idct, k_jpeg_colour) must read the int16
coefficients (2 B each, 1.5 per pixel at 4:2:0) and write 4 B / pixel; the planes of 8-bit samples between the two kernels
(1.5 B / pixel written, then read) are not counted.
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
    jpeg_case(ctx, n, timed, row, res)
    for r in res:
        print(json.dumps(r))


def jpeg_case(ctx, n, timed, row, res):
    import ctypes as C
    import io

    import numpy as np

    from svgrasterize_amd import _abi, jpeg

    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        rng = np.random.default_rng(3)
        y, x = np.mgrid[0:n, 0:n].astype(np.float32)
        img = np.stack([255 * x / n, 255 * y / n, 128 + 100 * np.sin(x / 37) * np.cos(y / 53)], axis=-1)
        img += rng.normal(0.0, 10.0, img.shape).astype(np.float32)
        buf = io.BytesIO()
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(buf, "JPEG", quality=85, subsampling=2)
        data = buf.getvalue()
        t0 = time.perf_counter()
        frame, coef, quant = jpeg.decode_coefficients(data)
        host = time.perf_counter() - t0
        source = f"{len(data)} bytes from Pillow"
    else:   # the photo-like fixture's blocks repeated over the frame
        with open(os.path.join(ROOT, "tests", "golden", "jpeg", "ycc420_photo.jpg"), "rb") as f:
            data = f.read()
        t0 = time.perf_counter()
        small, scoef, quant = jpeg.decode_coefficients(data)
        host = (time.perf_counter() - t0) * (n * n) / (small.width * small.height)
        frame = _abi.JpegFrame.from_buffer_copy(small)
        frame.width = frame.height = n
        parts = []
        for (sb, sbh, sbw), (_b, bh, bw) in zip(jpeg.coefficient_layout(small)[0], jpeg.coefficient_layout(frame)[0]):
            blocks = scoef[64 * sb:64 * (sb + sbh * sbw)].reshape(sbh, sbw, 64)
            parts.append(np.tile(blocks, (-(-bh // sbh), -(-bw // sbw), 1))[:bh, :bw].reshape(-1))
        coef = np.concatenate(parts)
        source = "tests/golden/jpeg/ycc420_photo.jpg tiled; the host time is the fixture's, scaled by the pixel count"
    res.append(dict(op=f"read_jpeg {n}^2 4:2:0 baseline, host: markers + svgr_jpeg_entropy ({source})", ms=round(host * 1e3, 3)))
    out = ctx.alloc(n * n * 4)
    call = lambda: _abi._check(ctx.lib.svgr_jpeg_decode(ctx.handle, C.byref(frame), _abi.ptr(coef), coef.size, _abi.ptr(quant), out.handle))
    row(f"svgr_jpeg_decode {n}^2 4:2:0 (host copy of {coef.nbytes >> 20} MiB + k_jpeg_idct + k_jpeg_colour)", coef.nbytes + n * n * 4, timed(call))


if __name__ == "__main__":
    main()
