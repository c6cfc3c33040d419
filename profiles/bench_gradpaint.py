#!/usr/bin/env python3
"""Gradient paints in differentiable compositing: diff.compose_painted_tensor against the same composition written as a torch
loop over the planes, by the method of bench_compose.py.

  8 paths      8 soft discs of radius 40 to 100 pixels spread over a 256 x 256 viewport
  256 paths    256 soft discs of radius 12 on a 16 x 16 grid over a 256 x 256 viewport: most planes are zero on most pixels

Every path is a gradient: linear and radial in turn, pad, repeat and reflect in turn, 2 to 4 stops in turn, each under its own
transform.  The baseline evaluates the gradient with torch operations per path (the affine map, the offset, the spread, the
three tests of the stops with torch.where), multiplies by the plane and composites `C = s + C * (1 - s[..., 3:])` in paint order,
differentiated by torch autograd, on the same device and in the planes' own type; compose_painted_tensor computes in double
whatever the planes' type.

Everything is on the device before the clock starts.  A time is per call: `--reps` calls between two events on torch's stream,
the median, the least and the most of `--rounds` such windows after one untimed window of each; the two implementations take
turns round after round.  `forward_ms` is the image alone, `both_ms` the image and the six gradients (planes, paints, transforms,
geometry, stop positions, stop colours).  `peak_bytes` is torch.cuda.max_memory_allocated over one image-and-gradients run,
minus what was allocated before it; compose_painted_tensor's scratch comes from the library's own pool, which torch does not see,
so `library_scratch_bytes` states it (the workgroups' partial sums; for float32 planes the double T_p plane as well).

Run alone under `timeout`.
    python profiles/bench_gradpaint.py [--rounds 7] [--out PATH]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "bench_gradpaint.json"))
    args = ap.parse_args()
    import torch

    torch.cuda.init()   # (torch first: tensor.IMPORT_ORDER)
    import numpy as np

    import svgrasterize_amd as S
    from svgrasterize_amd import diff

    dev = torch.device("cuda", 0)
    size = 256
    bg = (0.1, 0.2, 0.3, 0.5)

    def discs(centres, radii):
        r, c = np.mgrid[0:size, 0:size] + 0.5
        d = np.sqrt((r[None] - centres[:, 0, None, None]) ** 2 + (c[None] - centres[:, 1, None, None]) ** 2)
        return np.clip(radii[:, None, None] - d + 0.5, 0.0, 1.0)   # a one-pixel ramp at the rim

    rng = np.random.default_rng(3)
    grid = np.stack(np.meshgrid(np.arange(16), np.arange(16), indexing="ij"), axis=-1).reshape(-1, 2) * 16.0 + 8.0
    c8, r8 = rng.uniform(40, 216, (8, 2)), rng.uniform(40, 100, 8)
    scenes = {
        "8 paths at 256 x 256": (discs(c8, r8), c8, r8),
        "256 paths at 256 x 256": (discs(grid, np.full(256, 12.0)), grid, np.full(256, 12.0)),
    }

    def gradients(centres, radii):
        """GradientPaints (host) over the discs: linear across the disc or radial from near its centre."""
        n = len(centres)
        kind = np.array([1 + p % 2 for p in range(n)], dtype=np.int32)
        spread = np.array([p % 3 for p in range(n)], dtype=np.int32)
        count = np.array([2 + p % 3 for p in range(n)])
        off = np.concatenate([[0], np.cumsum(count)]).astype(np.int32)
        m6 = np.tile([1.0, 0.0, 0.0, 0.0, 1.0, 0.0], (n, 1)) + rng.uniform(-0.05, 0.05, (n, 6)) * [1, 1, 20, 1, 1, 20]
        geom = np.zeros((n, 4))
        for p in range(n):
            c, r = centres[p], radii[p]
            geom[p] = (c[0] - 0.6 * r, c[1] - 0.5 * r, c[0] + 0.7 * r, c[1] + 0.4 * r) if kind[p] == 1 else (c[0] + 0.1 * r, c[1] - 0.1 * r, 0.8 * r, 0.0)
        pos = np.concatenate([np.sort(rng.uniform(0.0, 1.0, k)) for k in count])
        alpha = rng.uniform(0.3, 1.0, len(pos))
        rgba = np.concatenate([rng.uniform(0, 1, (len(pos), 3)) * alpha[:, None], alpha[:, None]], axis=1)
        return diff.GradientPaints(kind, spread, off, m6, geom, pos, rgba)

    def torch_loop(planes, paints, gp, bg_t, px, py):
        C = bg_t.expand(size, size, 4)
        for p in range(planes.shape[0]):
            m6, geom = gp.m6[p], gp.geom[p]
            x = py * m6[1] + px * m6[0] + m6[2]
            y = py * m6[4] + px * m6[3] + m6[5]
            if gp.kind[p] == 1:
                v0, v1 = geom[2] - geom[0], geom[3] - geom[1]
                t = ((x - geom[0]) * v0 + (y - geom[1]) * v1) / (v0 * v0 + v1 * v1)
            else:
                o0, o1 = (x - geom[0]) / geom[2], (y - geom[1]) / geom[2]
                t = torch.sqrt(o0 * o0 + o1 * o1)
            if gp.spread[p] == 1:
                t = t - torch.trunc(t)
            elif gp.spread[p] == 2:
                a = t + 1.0
                t = torch.abs((a - 2.0 * torch.floor(a * 0.5)) - 1.0)
            s0, s1 = int(gp.path_stop_off[p]), int(gp.path_stop_off[p + 1])
            pos, rgba = gp.stop_pos[s0:s1], gp.stop_rgba[s0:s1]
            u = t[..., None]
            col = torch.where(u <= pos[0], rgba[0], 0.0) + torch.where(u > pos[-1], rgba[-1], 0.0)
            for s in range(s1 - s0 - 1):
                ratio = (u - pos[s]) / (pos[s + 1] - pos[s])
                col = col + torch.where((u > pos[s]) & (u <= pos[s + 1]), (1 - ratio) * rgba[s] + ratio * rgba[s + 1], 0.0)
            s = (col * planes[p][..., None]) * paints[p]
            C = s + C * (1 - s[..., 3:])
        return C

    def timed(fns):
        """{name: (median, least, most) ms per call}: the functions take turns, round after round, `--reps` calls between two events."""
        for fn in fns.values():   # (a window's worth of each first: code objects, the allocators' blocks, the clocks)
            for _ in range(args.reps):
                fn()
        torch.cuda.synchronize()
        ms = {name: [] for name in fns}
        for _ in range(args.rounds):
            for name, fn in fns.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.reps):
                    fn()
                b.record()
                torch.cuda.synchronize()
                ms[name].append(a.elapsed_time(b) / args.reps)
        return {name: (round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)) for name, v in ms.items()}

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        del out
        return int(torch.cuda.max_memory_allocated() - before)

    results = []
    for name, (cover, centres, radii) in scenes.items():
        n_paths = len(cover)
        hgp = gradients(centres, radii)
        paints_np = np.ones((n_paths, 4)) * rng.uniform(0.5, 1.0, (n_paths, 1))
        for dtype in (torch.float32, torch.float64):
            def dt(a, t=torch.float64):
                return torch.tensor(a, dtype=t, device=dev, requires_grad=True)

            planes, paints = dt(cover, dtype), dt(paints_np)
            gp = diff.GradientPaints(hgp.kind, hgp.spread, hgp.path_stop_off, dt(hgp.m6), dt(hgp.geom), dt(hgp.stop_pos), dt(hgp.stop_rgba))
            leaves = (planes, paints, gp.m6, gp.geom, gp.stop_pos, gp.stop_rgba)
            g = torch.randn((size, size, 4), dtype=dtype, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
            bg_t = torch.tensor(bg, dtype=dtype, device=dev)
            px = (torch.arange(size, dtype=dtype, device=dev) + 0.5)[:, None].expand(size, size)
            py = (torch.arange(size, dtype=dtype, device=dev) + 0.5)[None, :].expand(size, size)

            def cast():
                return paints.to(dtype), gp._replace(m6=gp.m6.to(dtype), geom=gp.geom.to(dtype), stop_pos=gp.stop_pos.to(dtype), stop_rgba=gp.stop_rgba.to(dtype))

            def ours_forward():
                with torch.no_grad():
                    return diff.compose_painted_tensor(planes, paints, gp, bg=bg)

            def ours_both():
                return torch.autograd.grad(diff.compose_painted_tensor(planes, paints, gp, bg=bg), leaves, g)

            def loop_forward():
                with torch.no_grad():
                    return torch_loop(planes, *cast(), bg_t, px, py)

            def loop_both():
                return torch.autograd.grad(torch_loop(planes, *cast(), bg_t, px, py), leaves, g)

            a, b = ours_both(), loop_both()
            agree = {k: float(f"{float((x - y).abs().max()) / max(float(y.abs().max()), 1e-300):.3e}")   # (float32 planes: the loop's own arithmetic shows)
                     for k, x, y in zip(("planes", "paints", "m6", "geom", "stop_pos", "stop_rgba"), a, b)}
            n_all = n_paths * size * size
            groups = min(diff.compose_groups(), -(-size * size // diff.compose_block()))
            n_params = 14 * n_paths + 5 * len(hgp.stop_pos)
            t = timed(dict(painted_forward=ours_forward, loop_forward=loop_forward, painted_both=ours_both, loop_both=loop_both))
            row = dict(case=name, paths=n_paths, stops=len(hgp.stop_pos), plane=str(dtype).split(".")[-1], zero_share=round(float((cover == 0.0).mean()), 4),
                       **{f"{k}_ms": v[0] for k, v in t.items()}, **{f"{k}_min_ms": v[1] for k, v in t.items()}, **{f"{k}_max_ms": v[2] for k, v in t.items()},
                       painted_peak_bytes=peak(ours_both), library_scratch_bytes=groups * n_params * 8 + n_paths * 16 + (n_all * 8 if dtype == torch.float32 else 0),
                       loop_peak_bytes=peak(loop_both), grad_rel_diff=agree)
            results.append(row)
            print(json.dumps(row), flush=True)
    with open(args.out, "w") as f:
        json.dump(dict(device=S.Context.get(0).name(), rounds=args.rounds, reps=args.reps, compose_block=diff.compose_block(), compose_groups=diff.compose_groups(),
                       results=results), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
