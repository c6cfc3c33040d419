#!/usr/bin/env python3
"""Differentiable compositing: diff.compose_tensor against the same composition written as a torch loop over the planes.

  8 paths      8 soft discs of radius 40 to 100 pixels spread over a 256 x 256 viewport
  256 paths    256 soft discs of radius 12 on a 16 x 16 grid over a 256 x 256 viewport: most planes are zero on most pixels

The baseline is what the README recommended before this pass existed: `C = s + C * (1 - s[..., 3:])` with `s = m[..., None] * paint`
for every plane in paint order, differentiated by torch autograd, on the same device.  It runs in the planes' own type (float32
planes: float32 arithmetic, the paints cast once); compose_tensor computes in double whatever the planes' type.

Planes, paints and grad_image are on the device before the clock starts.  A time is per call: `--reps` calls between two events
on torch's stream (compose_tensor's kernels run on the library's stream, ordered behind and in front of torch's by events, so they
are inside), the median and the least of `--rounds` such windows after one untimed window of each; the two implementations take
turns round after round.  `forward_ms` is the image alone, `both_ms` the image and the two gradients.  `peak_bytes`
is torch.cuda.max_memory_allocated over one image-and-gradients run, minus what was allocated before it; compose_tensor's scratch
comes from the library's own pool, which torch does not see, so `library_scratch_bytes` states it (the workgroups' partial paint
sums; for float32 planes the double T_p plane as well).

Run alone under `timeout`.
    python profiles/bench_compose.py [--rounds 7] [--out PATH]"""
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
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "bench_compose.json"))
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
    scenes = {
        "8 paths at 256 x 256": discs(rng.uniform(40, 216, (8, 2)), rng.uniform(40, 100, 8)),
        "256 paths at 256 x 256": discs(grid, np.full(256, 12.0)),
    }

    def torch_loop(planes, paints, bg_t):
        C = bg_t.expand(size, size, 4)
        for p in range(planes.shape[0]):
            s = planes[p][..., None] * paints[p]
            C = s + C * (1 - s[..., 3:])
        return C

    def timed(fns):
        """{name: (median, least) ms per call}: the functions take turns, round after round, `--reps` calls between two events."""
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
        return {name: (round(statistics.median(v), 4), round(min(v), 4)) for name, v in ms.items()}

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        del out
        return int(torch.cuda.max_memory_allocated() - before)

    results = []
    for name, cover in scenes.items():
        n_paths = len(cover)
        alpha = rng.uniform(0.3, 1.0, n_paths)
        paints_np = np.concatenate([rng.uniform(0, 1, (n_paths, 3)) * alpha[:, None], alpha[:, None]], axis=1)
        for dtype in (torch.float32, torch.float64):
            planes = torch.tensor(cover, dtype=dtype, device=dev, requires_grad=True)
            paints = torch.tensor(paints_np, dtype=torch.float64, device=dev, requires_grad=True)
            g = torch.randn((size, size, 4), dtype=dtype, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
            bg_t = torch.tensor(bg, dtype=dtype, device=dev)

            def ours_forward():
                with torch.no_grad():
                    return diff.compose_tensor(planes, paints, bg=bg)

            def ours_both():
                return torch.autograd.grad(diff.compose_tensor(planes, paints, bg=bg), (planes, paints), g)

            def loop_forward():
                with torch.no_grad():
                    return torch_loop(planes, paints.to(dtype), bg_t)

            def loop_both():
                return torch.autograd.grad(torch_loop(planes, paints.to(dtype), bg_t), (planes, paints), g)

            a, b = ours_both(), loop_both()
            scale = float(b[1].abs().max())
            agree = float((a[1] - b[1]).abs().max()) / scale   # (float32 planes: the loop's own float32 arithmetic shows here)
            n_all = n_paths * size * size
            groups = min(diff.compose_groups(), -(-size * size // diff.compose_block()))
            t = timed(dict(compose_forward=ours_forward, loop_forward=loop_forward, compose_both=ours_both, loop_both=loop_both))
            row = dict(case=name, paths=n_paths, plane=str(dtype).split(".")[-1], zero_share=round(float((cover == 0.0).mean()), 4),
                       **{f"{k}_ms": v[0] for k, v in t.items()}, **{f"{k}_min_ms": v[1] for k, v in t.items()},
                       compose_peak_bytes=peak(ours_both), library_scratch_bytes=groups * n_paths * 32 + (n_all * 8 if dtype == torch.float32 else 0),
                       loop_peak_bytes=peak(loop_both), grad_paints_rel_diff=float(f"{agree:.3e}"))
            results.append(row)
            print(json.dumps(row), flush=True)
    with open(args.out, "w") as f:
        json.dump(dict(device=S.Context.get(0).name(), rounds=args.rounds, reps=args.reps, compose_block=diff.compose_block(), compose_groups=diff.compose_groups(),
                       results=results), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
