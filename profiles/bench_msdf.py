#!/usr/bin/env python3
"""Multi-channel distance fields: k_msdf_distance against k_sdf_distance on the same glyph atlas.

  atlas    `--glyphs` glyphs at `--px` pixels per em from tests/golden/fonts/varsynth.ttf, as profiles/bench_sdf.py builds its atlas: the
           committed variable font has six glyphs, so the atlas holds them at `--glyphs` / 6 positions of its first axis.  Both
           fields are taken over the same cells (sdf.atlas_layout) at the same spread, uint8:
             sdf    one path per glyph, one union grid query          (svgr_batch_distance, k_sdf_distance)
             msdf   up to four paths per glyph, a group per glyph     (svgr_batch_msdf, k_msdf_group_extent + k_msdf_distance)
           The batches are built, flattened and queried once before anything is timed.

Every figure is the time of one query on a resident batch -- kernels, download of the result, one wait.  `device_ms` is the
stream's own time between two HIP events around the call (svgr_measure_begin / _end), `wall_ms` the host clock around the same
call; both are medians over `--rounds` rounds, and in every round the two queries run one after the other, alternating, so that
what else the machine does falls on both.  `ratio` is msdf over sdf; `ratio_per_round` its spread.  The whole calls
(Font.sdf_atlas and Font.msdf_atlas do the layout, the colouring and the batch on the host as well) are timed the same way.

`edge_tests` counts points x edges behind the cull of a grid query, per tile the edges of the groups (paths, for sdf) that stay,
worked out on the host from the same extents and the same rule: both kernels walk the same edges, so the ratio of the times is the
ratio of the cost per point-edge pair, but for the tables.

Run alone under `timeout`.
    python profiles/bench_msdf.py [--glyphs 384] [--px 64] [--spread 4] [--rounds 30] [--out PATH]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--glyphs", type=int, default=384)
    ap.add_argument("--px", type=float, default=64.0)
    ap.add_argument("--spread", type=float, default=4.0)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "bench_msdf.json"))
    args = ap.parse_args()
    import numpy as np

    import svgrasterize_amd as S
    from svgrasterize_amd import _abi, msdf, sdf

    ctx = S.Context.get(0)
    block = ctx.lib.svgr_hit_block()
    tile = int(round(block ** 0.5))

    def once(fn):
        ctx.sync()
        ctx.measure_begin(0.0)
        t = time.perf_counter()
        fn()
        wall = (time.perf_counter() - t) * 1e3
        return wall, ctx.measure_end()

    def alternate(first, second):
        """[(wall, device)] per round for each of two calls, run one after the other in every round, the order swapped each round"""
        first(), second()
        a, b = [], []
        for k in range(args.rounds):
            if k % 2:
                b.append(once(second)), a.append(once(first))
            else:
                a.append(once(first)), b.append(once(second))
        return a, b

    def summary(name, runs, **more):
        wall, dev = [r[0] for r in runs], [r[1] for r in runs]
        return dict(query=name, wall_ms=round(statistics.median(wall), 4), device_ms=round(statistics.median(dev), 4), device_min_ms=round(min(dev), 4),
                    device_max_ms=round(max(dev), 4), **more)

    def ratios(a, b, k=1):
        """msdf over sdf in column k (0 wall, 1 device): of the medians, and the smallest and largest of the rounds' own"""
        per = sorted(y[k] / x[k] for x, y in zip(a, b))
        return dict(ratio=round(statistics.median(y[k] for y in b) / statistics.median(x[k] for x in a), 3), ratio_per_round=[round(per[0], 3), round(per[-1], 3)],
                    ratio_of="wall_ms" if k == 0 else "device_ms")

    def walked(edges, edge_path, unit_of_path, n_units, n_rows, n_cols, spread):
        """point-edge pairs behind the cull: per tile the edges of the units (paths or groups) that stay, x block lanes"""
        e = edges.reshape(-1, 4)
        unit = np.asarray(unit_of_path)[edge_path]
        ext = np.full((n_units, 4), np.inf)
        ext[:, 2:] = -np.inf
        np.minimum.at(ext[:, 0], unit, np.minimum(e[:, 0], e[:, 2]))
        np.minimum.at(ext[:, 1], unit, np.minimum(e[:, 1], e[:, 3]))
        np.maximum.at(ext[:, 2], unit, np.maximum(e[:, 0], e[:, 2]))
        np.maximum.at(ext[:, 3], unit, np.maximum(e[:, 1], e[:, 3]))
        per_unit = np.bincount(unit, minlength=n_units).astype(np.int64)
        ta, tb = np.meshgrid(np.arange(0, n_rows, tile, dtype=np.float64), np.arange(0, n_cols, tile, dtype=np.float64), indexing="ij")
        lo_a, lo_b = ta.ravel()[:, None] + 0.5, tb.ravel()[:, None] + 0.5
        hi_a, hi_b = np.minimum(ta.ravel()[:, None] + tile, n_rows) - 0.5, np.minimum(tb.ravel()[:, None] + tile, n_cols) - 0.5
        thr = (spread * (1.0 + 2.0 ** -40) + 2.0 ** -40 * np.abs(ext).max(axis=1))[None, :]
        gone = (ext[None, :, 1] - hi_b > thr) | (lo_b - ext[None, :, 3] > thr) | (lo_a - ext[None, :, 2] > thr) | (ext[None, :, 0] - hi_a > thr)
        return int(((~gone) * per_unit[None, :]).sum()) * block

    with open(os.path.join(ROOT, "tests", "golden", "fonts", "varsynth.ttf"), "rb") as f:
        font = S.read_ttf(f.read())
    axis = font.axes[0]
    per_face = font.n_glyphs
    n_faces = -(-args.glyphs // per_face)
    glyphs, keys = [], []
    for k in range(n_faces):
        face = font.instance({axis.tag: axis.minimum + (axis.maximum - axis.minimum) * (k + 0.5) / n_faces})
        for gid in range(per_face):
            if len(glyphs) < args.glyphs:
                glyphs.append(face.glyph(gid))
                keys.append((k, gid))
    spread, scale = args.spread, args.px / font.units_per_em
    paths = [g.path for g in glyphs]
    cells, rows, cols = sdf.atlas_layout(keys, [p.user_box() for p in paths], [g.advance for g in glyphs], args.px, font.units_per_em, spread, 1024)
    drawn = [(path, sdf.cell_m6(cells[key], scale)) for key, path in zip(keys, paths) if cells[key].rows]
    grid = (0, 0, rows, cols)

    packs = [path.packed() for path, _m6 in drawn]
    offs = np.concatenate([[0], np.cumsum([len(pk[0]) for pk in packs])]).astype(np.int64)
    plain = _abi.Batch(ctx, np.concatenate([pk[0] for pk in packs]), np.concatenate([pk[1] for pk in packs]), offs, np.array([m6 for _p, m6 in drawn]),
                       np.zeros(len(drawn), dtype=np.uint8), np.zeros((len(drawn), 4)), viewport=None)
    multi, colour, group_off, orient = msdf.shapes_batch([(path, m6, 0) for path, m6 in drawn])

    def q_sdf():
        return plain.distance(grid=grid, spread=spread, out="u8", union=True)

    def q_msdf():
        return multi.msdf(colour, group_off, orient, grid=grid, spread=spread, out="u8")

    a_img, m_img = q_sdf().reshape(rows, cols), q_msdf().reshape(rows, cols, 4)
    assert np.array_equal(m_img[..., 3], a_img), "the alpha plane is not the single-channel field"
    exact = multi.msdf(colour, group_off, orient, grid=grid, spread=spread).reshape(rows, cols, 4)
    assert np.array_equal(sdf.median(exact) < 0, exact[..., 3] < 0), "the median's side is not the alpha plane's"
    # (in uint8 a median of exactly 0 -- a pixel centre on the line of an edge -- is code 128 like the outline itself, whatever A is)
    codes_differ = int(((sdf.median(m_img) >= 128) != (a_img >= 128)).sum())
    p_edges, p_path = plain.all_edges()
    m_edges, m_path = multi.all_edges()
    group_of = np.repeat(np.arange(len(orient)), np.diff(group_off))
    tests_sdf = walked(p_edges, p_path, np.arange(len(drawn)), len(drawn), rows, cols, spread)
    tests_msdf = walked(m_edges, m_path, group_of, len(orient), rows, cols, spread)
    result = dict(device=ctx.name(), rounds=args.rounds, block=block, chunk=ctx.lib.svgr_hit_chunk(), glyphs=len(glyphs), drawn=len(drawn), px=args.px,
                  spread=spread, image=[rows, cols], sdf_paths=plain.n_paths, msdf_paths=multi.n_paths, msdf_groups=len(orient), edges=len(p_edges),
                  msdf_edges=len(m_edges), median_128_side_differs=codes_differ, corner_share=round(float((m_img[..., :3] != m_img[..., 3:]).any(axis=-1).mean()), 4), rows=[])
    a, b = alternate(q_sdf, q_msdf)
    result["rows"].append(summary("sdf query, u8", a, edge_tests=tests_sdf, edge_tests_per_s=round(tests_sdf / statistics.median(x[1] for x in a) * 1e3, 0)))
    result["rows"].append(summary("msdf query, u8", b, edge_tests=tests_msdf, edge_tests_per_s=round(tests_msdf / statistics.median(x[1] for x in b) * 1e3, 0),
                                  **ratios(a, b)))
    plain.destroy()
    multi.destroy()
    a, b = alternate(lambda: sdf.glyphs_sdf_atlas(glyphs, keys, font.units_per_em, args.px, spread),
                     lambda: msdf.glyphs_msdf_atlas(glyphs, keys, font.units_per_em, args.px, spread))
    result["rows"].append(summary("sdf_atlas, whole call", a))
    result["rows"].append(summary("msdf_atlas, whole call", b, **ratios(a, b, 0)))
    for row in result["rows"]:
        print(json.dumps(row), flush=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
