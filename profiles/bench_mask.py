#!/usr/bin/env python3
"""Luminance masks in differentiable compositing: diff.compose_masked_tensor against the same composition written as a torch
loop under autograd, by the method and on the scenes of bench_group.py:

  8 paths      8 soft discs of radius 40 to 100 pixels spread over a 256 x 256 viewport
  256 paths    256 soft discs of radius 12 on a 16 x 16 grid over a 256 x 256 viewport: most planes are zero on most pixels

Every path is a gradient (linear and radial, the three spreads and 2 to 4 stops in turn).  Four consecutive paths make a group with
an opacity; every group is clipped by one more plane, a soft disc about the four (so there are n_paths / 4 more planes), and every
second pair of groups sits in an outer group with an opacity of its own: two levels.  ONE group, the first, has a mask: one more
plane, a soft disc about the group filled by a gradient like the others.  The baseline is bench_group.py's loop with the mask
written out (the mask's group composited on zeros, divided by its alpha where that is above 1e-4, clamped, luminance times
alpha, the group multiplied by it), differentiated by torch autograd, on the same device and in the planes' own type.

The second pair of rows has NO mask: bench_group.py's grouped program through compose_masked_tensor beside
compose_grouped_tensor of the same build on the same inputs, which is what the two more ops and walk 0's test cost when nothing
is masked.

Times, windows and peak memory are bench_gradpaint.py's: `--reps` calls between two events, the median, the least and the most of
`--rounds` windows after one untimed window of each, the implementations taking turns.  `library_scratch_bytes` is what the
library's own pool holds besides: partial sums, the program, a double plane per group (T_end), four per masked pair (the mask's
canvas, parked by walk 0) and, for float32 planes, the double T_p plane.

Run alone under `timeout`.
    python profiles/bench_mask.py [--rounds 7] [--out PATH]"""
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
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "bench_mask.json"))
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
    scenes = {"8 paths at 256 x 256": (c8, r8), "256 paths at 256 x 256": (grid, np.full(256, 12.0))}

    def gradients(centres, radii, n_clip):
        """GradientPaints (host) over the discs, as bench_gradpaint.py's; the clip planes after them are solid."""
        n = len(centres)
        kind = np.array([1 + p % 2 for p in range(n)] + [0] * n_clip, dtype=np.int32)
        spread = np.array([p % 3 for p in range(n)] + [0] * n_clip, dtype=np.int32)
        count = np.array([2 + p % 3 for p in range(n)] + [0] * n_clip)
        off = np.concatenate([[0], np.cumsum(count)]).astype(np.int32)
        m6 = np.tile([1.0, 0.0, 0.0, 0.0, 1.0, 0.0], (n + n_clip, 1))
        m6[:n] += rng.uniform(-0.05, 0.05, (n, 6)) * [1, 1, 20, 1, 1, 20]
        geom = np.zeros((n + n_clip, 4))
        for p in range(n):
            c, r = centres[p], radii[p]
            geom[p] = (c[0] - 0.6 * r, c[1] - 0.5 * r, c[0] + 0.7 * r, c[1] + 0.4 * r) if kind[p] == 1 else (c[0] + 0.1 * r, c[1] - 0.1 * r, 0.8 * r, 0.0)
        pos = np.concatenate([np.sort(rng.uniform(0.0, 1.0, k)) for k in count[:n]])
        alpha = rng.uniform(0.3, 1.0, len(pos))
        rgba = np.concatenate([rng.uniform(0, 1, (len(pos), 3)) * alpha[:, None], alpha[:, None]], axis=1)
        return diff.GradientPaints(kind, spread, off, m6, geom, pos, rgba)

    def fill(C, p, planes, paints, gp, px, py):
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
        return s + C * (1 - s[..., 3:])

    def torch_loop(tree, planes, paints, gp, opacity, bg_t, px, py):
        slot = [0]
        lum_w = torch.tensor([0.2125, 0.7154, 0.072], dtype=planes.dtype, device=dev)

        def draw(children, C):
            for child in children:
                if isinstance(child, diff.Group):
                    G = draw(child.children, torch.zeros_like(C))
                    if child.opacity is not None:
                        G = G * opacity[slot[0]]
                        slot[0] += 1
                    if child.clip is not None:
                        G = G * planes[child.clip[0]][..., None]
                    if child.mask is not None:
                        M = draw(child.mask, torch.zeros_like(C))
                        al = M[..., 3:]
                        divide = al > 1e-4
                        x = torch.where(divide, M[..., :3] / torch.where(divide, al, 1.0), M[..., :3]).clamp(0.0, 1.0)
                        G = G * ((x * lum_w).sum(dim=-1, keepdim=True) * al.clamp(0.0, 1.0))
                    C = G + C * (1 - G[..., 3:])
                else:
                    C = fill(C, child, planes, paints, gp, px, py)
            return C

        return draw(tree, bg_t.expand(size, size, 4))

    def timed(fns):
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
    groups_cap = min(diff.compose_groups(), -(-size * size // diff.compose_block()))
    for name, (centres, radii) in scenes.items():
        n_fill = len(centres)
        n_inner = n_fill // 4
        clip_c = np.stack([centres[4 * q:4 * q + 4].mean(axis=0) for q in range(n_inner)])
        clip_r = np.array([1.2 * radii[4 * q:4 * q + 4].max() for q in range(n_inner)])
        # planes: the fills, the mask's disc (a gradient fill like them), the clips
        mask_c, mask_r = clip_c[:1], 1.5 * clip_r[:1]
        cover = np.concatenate([discs(centres, radii), discs(mask_c, mask_r), discs(clip_c, clip_r)])

        def tree_of(masked):
            inner = [diff.Group(list(range(4 * q, 4 * q + 4)), opacity=0.5 + 0.4 * (q % 3) / 2, clip=[n_fill + 1 + q], mask=[n_fill] if masked and q == 0 else None)
                     for q in range(n_inner)]
            tree = []
            for q in range(0, n_inner, 2):   # every second pair in an outer group
                tree += [diff.Group(inner[q:q + 2], opacity=0.9)] if (q // 2) % 2 == 0 else inner[q:q + 2]
            return tree

        hgp = gradients(np.concatenate([centres, mask_c]), np.concatenate([radii, mask_r]), n_inner)
        paints_np = np.ones((len(cover), 4)) * rng.uniform(0.5, 1.0, (len(cover), 1))
        for grouped in (True, False):   # (with the mask; without it)
            for dtype in (torch.float32, torch.float64):
                def dt(a, t=torch.float64):
                    return torch.tensor(a, dtype=t, device=dev, requires_grad=True)

                keep = np.arange(len(cover)) if grouped else np.delete(np.arange(len(cover)), n_fill)   # (without the mask: without its plane)
                n_paths = len(keep)
                if grouped:
                    the_tree, sub = tree_of(True), hgp
                    prog = diff.mask_program(the_tree)
                else:
                    the_tree = tree_of(False)
                    for child in the_tree:   # the clips move down by the plane that left
                        for gr in (child.children if isinstance(child.children[0], diff.Group) else [child]):
                            gr.clip = [gr.clip[0] - 1]
                    prog = diff.group_program(the_tree)
                    n_mask_stops = int(hgp.path_stop_off[n_fill + 1] - hgp.path_stop_off[n_fill])
                    off = np.concatenate([hgp.path_stop_off[:n_fill + 1], hgp.path_stop_off[n_fill + 2:] - n_mask_stops]).astype(np.int32)
                    stops = np.delete(np.arange(len(hgp.stop_pos)), np.arange(hgp.path_stop_off[n_fill], hgp.path_stop_off[n_fill + 1]))
                    sub = hgp._replace(kind=hgp.kind[keep], spread=hgp.spread[keep], path_stop_off=off, m6=hgp.m6[keep], geom=hgp.geom[keep],
                                       stop_pos=hgp.stop_pos[stops], stop_rgba=hgp.stop_rgba[stops])
                planes, paints, opacity = dt(cover[keep], dtype), dt(paints_np[keep]), dt(prog.opacity)
                gp = diff.GradientPaints(sub.kind, sub.spread, sub.path_stop_off, dt(sub.m6), dt(sub.geom), dt(sub.stop_pos), dt(sub.stop_rgba))
                leaves = (planes, paints, gp.m6, gp.geom, gp.stop_pos, gp.stop_rgba, opacity)
                g = torch.randn((size, size, 4), dtype=dtype, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
                bg_t = torch.tensor(bg, dtype=dtype, device=dev)
                px = (torch.arange(size, dtype=dtype, device=dev) + 0.5)[:, None].expand(size, size)
                py = (torch.arange(size, dtype=dtype, device=dev) + 0.5)[None, :].expand(size, size)

                def cast():
                    return (paints.to(dtype), gp._replace(m6=gp.m6.to(dtype), geom=gp.geom.to(dtype), stop_pos=gp.stop_pos.to(dtype), stop_rgba=gp.stop_rgba.to(dtype)),
                            opacity.to(dtype))

                def ours_forward():
                    with torch.no_grad():
                        return diff.compose_masked_tensor(planes, paints, gp, prog, opacity, bg=bg)

                def ours_both():
                    return torch.autograd.grad(diff.compose_masked_tensor(planes, paints, gp, prog, opacity, bg=bg), leaves, g)

                def other_forward():
                    with torch.no_grad():
                        if grouped:
                            return torch_loop(the_tree, planes, *cast(), bg_t, px, py)
                        return diff.compose_grouped_tensor(planes, paints, gp, prog, opacity, bg=bg)

                def other_both():
                    if grouped:
                        return torch.autograd.grad(torch_loop(the_tree, planes, *cast(), bg_t, px, py), leaves, g)
                    return torch.autograd.grad(diff.compose_grouped_tensor(planes, paints, gp, prog, opacity, bg=bg), leaves, g)

                a, b = ours_both(), other_both()
                names = ("planes", "paints", "m6", "geom", "stop_pos", "stop_rgba", "opacity")
                agree = {k: float(f"{float((x - y).abs().max()) / max(float(y.abs().max()), 1e-300):.3e}") for k, x, y in zip(names, a, b)}
                other = "loop" if grouped else "grouped"
                t = timed({"masked_forward": ours_forward, f"{other}_forward": other_forward, "masked_both": ours_both, f"{other}_both": other_both})
                n_groups = int((prog.items[:, 0] == diff.OP_BEGIN).sum())
                n_params = 14 * n_paths + 5 * len(sub.stop_pos) + len(prog.opacity)
                n_pairs = int((prog.items[:, 0] == diff.OP_HOLD).sum())
                scratch = groups_cap * n_params * 8 + n_paths * 16 + prog.items.size * 4 + max(n_groups, 1) * size * size * 8 \
                    + max(n_pairs, 1) * 4 * size * size * 8 + (n_paths * size * size * 8 if dtype == torch.float32 else 0)
                row = dict(case=name, program="one mask" if grouped else "no mask", planes=n_paths, pairs=n_pairs, groups=n_groups, stops=len(sub.stop_pos), plane=str(dtype).split(".")[-1],
                           **{f"{k}_ms": v[0] for k, v in t.items()}, **{f"{k}_min_ms": v[1] for k, v in t.items()}, **{f"{k}_max_ms": v[2] for k, v in t.items()},
                           masked_peak_bytes=peak(ours_both), library_scratch_bytes=scratch, **{f"{other}_peak_bytes": peak(other_both)}, grad_rel_diff=agree)
                results.append(row)
                print(json.dumps(row), flush=True)
    with open(args.out, "w") as f:
        json.dump(dict(device=S.Context.get(0).name(), rounds=args.rounds, reps=args.reps, compose_block=diff.compose_block(), compose_groups=diff.compose_groups(),
                       group_depth=diff.group_depth(), results=results), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
