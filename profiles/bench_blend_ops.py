#!/usr/bin/env python3
"""Rate of the mix-blend-mode kernel (k_layer_mix_blend) on 4096 x 4096 RGBA float64 layers (537 MB each): wall clock per
call, bytes = what the blend must read + write (backdrop 32 + source 32 read, 32 written per pixel it touches).  Run it under
`rocprofv3 --kernel-trace --stats` for the kernel times alone.
    python profiles/bench_blend_ops.py [--size 4096] [--small 512] [--reps 5]"""
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
    ap.add_argument("--small", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import numpy as np

    import svgrasterize_amd as S

    ctx = S.Context.get(0)
    n, m = args.size, args.small
    px = n * n * 32
    rng = np.random.default_rng(1)

    def premul(rows, cols, offset):
        img = rng.random((rows, cols, 4))
        img[..., :3] *= img[..., 3:4]
        return S.Layer._from_device(ctx.from_host(img), img.shape, offset, True, False)

    back = premul(n, n, (0, 0))
    src = premul(n, n, (0, 0))
    small = premul(m, m, (n // 3, n // 5))
    res = []

    def run(name, nbytes, fn):
        fn()
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            fn()
        ctx.sync()
        dt = (time.perf_counter() - t0) / args.reps
        row = dict(op=name, ms=round(dt * 1e3, 3))
        if nbytes:
            row.update(gbs=round(nbytes / dt / 1e9, 1), frac_of_6290=round(nbytes / dt / 6.29e12, 3))
        res.append(row)

    run("copy (svgr_buf_copy, the yardstick)", 2 * px, lambda: back._copy_device())
    run("k_layer_mix_blend normal (full overlap, out of place)", 3 * px, lambda: S.Layer.mix_blend(back, src, S.BLEND_MODES["normal"]))
    for name in ("multiply", "soft-light", "color-dodge", "color", "hue"):
        run(f"k_layer_mix_blend {name} (full overlap, out of place)", 3 * px, lambda k=S.BLEND_MODES[name]: S.Layer.mix_blend(back, src, k))
    # the cost rule: a small source over a large backdrop the caller owns touches the source's rectangle alone ...
    acc = S.Layer._from_device(back._copy_device(), back._shape, back.offset, True, False)
    run(f"k_layer_mix_blend multiply, {m}^2 source in place in a {n}^2 backdrop", 3 * m * m * 32,
        lambda: S.Layer.mix_blend(acc, small, S.BLEND_MODES["multiply"], reuse_backdrop=True))
    run(f"k_layer_mix_blend color, {m}^2 source in place in a {n}^2 backdrop", 3 * m * m * 32,
        lambda: S.Layer.mix_blend(acc, small, S.BLEND_MODES["color"], reuse_backdrop=True))
    # ... and out of place it is one pass over the union (the backdrop copied, the source's rectangle blended)
    run(f"k_layer_mix_blend multiply, {m}^2 source out of place over a {n}^2 backdrop", 2 * px + 2 * m * m * 32,
        lambda: S.Layer.mix_blend(back, small, S.BLEND_MODES["multiply"]))
    for r in res:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
