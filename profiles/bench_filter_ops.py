#!/usr/bin/env python3
"""Rate of the filter-primitive kernels beyond the reference on a 4096 x 4096 RGBA float64 layer (537 MB): wall clock per
call (each entry point uploads its host-side set-up and synchronises), bytes = what the op must read + write.  Run it under
`rocprofv3 --kernel-trace --stats` for the kernel times alone.
    python profiles/bench_filter_ops.py [--size 4096] [--reps 3]"""
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
    args = ap.parse_args()
    import numpy as np

    import svgrasterize_amd as S

    ctx = S.Context.get(0)
    n = args.size
    npx = n * n
    px = npx * 32
    tr = S.Transform().matrix(0, 1, 0, 1, 0, 0).rotate(0.3)
    rng = np.random.default_rng(1)
    host = rng.random((n, n, 4))
    straight = S.Layer(host, (0, 0), pre_alpha=False, linear_rgb=True)
    straight._device()
    layer = S.Layer._from_device(straight._device(), (n, n, 4), (0, 0), False, True)
    pre = S.Layer._from_device(layer._copy_device(), (n, n, 4), (0, 0), True, True)
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

    for octaves in (1, 4, 8):
        run(f"k_layer_turbulence fractalNoise, {octaves} octaves", px,
            lambda o=octaves: S.Layer.turbulence(tr, (0, 0), (n, n), (0.01, 0.02), o, 5, None, True))
    run("k_layer_turbulence turbulence, stitch, 4 octaves", px,
        lambda: S.Layer.turbulence(tr, (0, 0), (n, n), (0.01, 0.02), 4, 5, (0.0, 0.0, 300.0, 200.0), False))
    funcs = [("table", tuple(np.linspace(0, 1, 17) ** 2)), ("discrete", (0.1, 0.5, 0.9)), ("linear", 0.8, 0.1), None]
    run("k_layer_component_transfer (table, discrete, linear, identity; copy + in place)", 4 * px, lambda: layer.component_transfer(funcs))
    gamma = [("gamma", 1.0, 2.2, 0.0)] * 3 + [None]
    run("k_layer_component_transfer (gamma x 3; copy + in place)", 4 * px, lambda: layer.component_transfer(gamma))
    for order in (3, 5, 9):
        k = rng.random((order, order))
        run(f"k_layer_convolve_matrix {order}x{order}", 2 * px, lambda k=k: pre.convolve_matrix(k, None, 0.0, None, "duplicate", False))
    run("k_layer_displacement_map (scale 20)", 3 * px, lambda: pre.displacement_map(layer, tr, 20.0, "R", "G"))
    # lighting over the layer's own extent: 32 B read (alpha, one double of each pixel, whole lines) + 32 B written per pixel
    from svgrasterize_amd.filters import DistantLight, PointLight, SpotLight

    cx, cy = tr.invert(np.array([n / 2, n / 2]))
    lx, ly = tr.invert(np.array([n / 4, n / 3]))
    white = (1.0, 1.0, 1.0)
    run("k_layer_lighting diffuse, distant", 2 * px,
        lambda: pre.lighting(tr, (0, 0), (n, n), DistantLight(45.0, 30.0), white, 2.0, 1.0))
    run("k_layer_lighting specular, point, exponent 20", 2 * px,
        lambda: pre.lighting(tr, (0, 0), (n, n), PointLight(lx, ly, 500.0), white, 2.0, 1.0, 20.0))
    run("k_layer_lighting specular, spot with a cone, exponent 20", 2 * px,
        lambda: pre.lighting(tr, (0, 0), (n, n), SpotLight(lx, ly, 2000.0, cx, cy, 0.0, 8.0, 40.0), white, 2.0, 1.0, 20.0))
    # feTile over the whole layer's box: 32 B written per pixel; what is read is the tile, over and over (64 x 64: 131 KB, from
    # cache; 1024 x 1024: 33.5 MB).  The window (a result cut to its subregion) next to it: svgr_layer_compose_over with one source
    for t in (64, 1024):
        run(f"k_layer_tile {t}x{t} tile", px, lambda t=t: pre.tile((0, 0), (n, n), (17, 29), (t, t)))
    run("k_layer_tile tile = output (a crop by one pixel)", 2 * px, lambda: pre.tile((1, 1), (n, n), (1, 1), (n, n)))
    run("k_layer_compose_over, one source (window, a crop by one pixel)", 2 * px, lambda: pre.window((1, 1), (n, n)))
    for r in res:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
