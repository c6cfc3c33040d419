#!/usr/bin/env python3
"""One digest per case of every entry whose kernel takes a Box (csrc/svgr_box.h): seeded inputs through the C ABI, the output
downloaded and hashed with svgr_hash_buffers, the launches the call made next to it.  Two builds compute the same thing exactly
when their listings are identical line for line.
    python profiles/layer_boxes/digest.py > listing.txt"""
import ctypes as C
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

D_BIG, D_ROW = (-7, 11, 300, 517), (3, -5, 1, 1025)
PAIRS = [(D_BIG, (-50, 100, 100, 200)), (D_BIG, (250, 100, 100, 200)), (D_BIG, (50, -80, 100, 200)), (D_BIG, (50, 400, 100, 200)),
         (D_BIG, (400, 600, 20, 30)), (D_BIG, (-10, 5, 310, 530)), (D_BIG, (10, 20, 33, 300)), (D_BIG, D_BIG),
         (D_ROW, (3, -20, 1, 1100)), (D_ROW, (0, 500, 5, 700)), (D_ROW, (2, -100, 3, 300)), (D_ROW, (10, 0, 2, 50)), (D_ROW, D_ROW),
         (D_BIG, D_ROW), (D_ROW, D_BIG)]   # tests/test_gpu_layer_kernels.py
STOPS = [(0.0, (0.9, 0.1, 0.05, 1.0)), (0.35, (0.1, 0.6, 0.2, 0.7)), (1.0, (0.05, 0.15, 0.8, 0.9))]


def main():
    import svgrasterize_amd as S
    from svgrasterize_amd import _abi

    ctx = S.Context.get(0)
    lib, check, ptr = ctx.lib, _abi._check, _abi.ptr

    def rng(name):
        return np.random.default_rng(zlib.crc32(name.encode()))

    def bb(b):
        return (C.c_int64 * 4)(*[int(v) for v in b])

    def layer(name, box, ch=4):
        img = rng(name).random((box[2], box[3], ch))
        if ch == 4:
            img[..., :3] *= img[..., 3:]
        return img

    def report(name, buf, shape, n0):
        got = np.ascontiguousarray(buf.download(shape, np.float64))
        h = _abi.hash_buffers(np.array([got.ctypes.data], dtype=np.uint64), np.array([got.nbytes], dtype=np.int64))
        print(f"{name}: {h:016x} launches {ctx.launches() - n0}")

    def poisoned(shape):
        return ctx.from_host(np.full(shape, np.nan))

    # ---- the two-layer entries on PAIRS, 1 and 4 channels
    k4 = np.array([0.3, 0.5, 0.7, 0.1])
    for op in ("over", "over_first", "in", "crop4", "blend1", "blend3", "blend4", "blend5"):
        for n, (db, sb) in enumerate(PAIRS):
            for ch in (1, 4):
                dst, src = layer("dst", db), layer(f"src{ch}", sb, ch)
                s_dev = ctx.from_host(src)
                d_dev = poisoned(dst.shape) if op == "crop4" else ctx.from_host(dst)
                a = (ctx.handle, d_dev.handle, bb(db), s_dev.handle, bb(sb), ch)
                n0 = ctx.launches()
                if op in ("over", "over_first"):
                    check(lib.svgr_layer_over(*a, int(op == "over_first")))
                elif op == "in":
                    check(lib.svgr_layer_in(*a))
                elif op == "crop4":
                    check(lib.svgr_layer_crop4(*a))
                else:
                    check(lib.svgr_layer_blend(*a, int(op[-1]), ptr(k4)))
                report(f"{op} pair {n} ch {ch}", d_dev, dst.shape, n0)

    # ---- one 25-source compose of each mode (two launches: 24 sources, then one more onto what is there)
    for mode in ("over", "in"):
        r = rng(f"compose {mode}")
        specs = []
        for i in range(25):
            if mode == "over":
                box = (int(r.integers(-25, 25)), int(r.integers(-160, 160)), int(r.integers(3, 40)), int(r.integers(5, 200)))
            else:
                box = (int(r.integers(-8, 8)), int(r.integers(-12, 12)), int(r.integers(30, 50)), int(r.integers(280, 330)))
            ch = 1 if i % 5 == 3 else 4
            specs.append((r.random((box[2], box[3], ch)), box, 0 if ch == 1 else int(r.choice([0, 8, 1, 4 | 8, 1 | 2, 1 | 2 | 8]))))
        lo = [f(s[1][k] for s in specs) for k, f in ((0, min), (1, min))] if mode == "over" else [max(s[1][k] for s in specs) for k in (0, 1)]
        ends = [(max if mode == "over" else min)(s[1][k] + s[1][2 + k] for s in specs) for k in (0, 1)]
        ob = (lo[0], lo[1], ends[0] - lo[0], ends[1] - lo[1])
        srcs = [ctx.from_host(s[0]) for s in specs]
        out = poisoned((ob[2], ob[3], 4))
        fn = lib.svgr_layer_compose_over if mode == "over" else lib.svgr_layer_compose_in
        n0 = ctx.launches()
        check(fn(ctx.handle, out.handle, bb(ob), 25, (_abi._P * 25)(*[b.handle for b in srcs]), (C.c_int64 * 100)(*[v for s in specs for v in s[1]]),
                 (C.c_int32 * 25)(*[s[0].shape[2] for s in specs]), (C.c_uint32 * 25)(*[s[2] for s in specs])))
        report(f"compose_{mode} of 25 over {ob}", out, (ob[2], ob[3], 4), n0)

    # ---- the filter primitives
    box = (-9, 14, 70, 333)
    inv = np.array([0.7, -0.2, 3.0, 0.15, 0.9, -8.0])
    tile = np.array([5.0, -3.0, 40.0, 25.0])
    out = poisoned((box[2], box[3], 4))
    n0 = ctx.launches()
    check(lib.svgr_layer_turbulence(ctx.handle, out.handle, bb(box), ptr(inv), 0.04, 0.07, ptr(tile), 11, 3, 1, 1))
    report("turbulence", out, (box[2], box[3], 4), n0)

    src_box, map_box = (-20, 0, 60, 200), (-9, 14, 70, 333)   # (the source covers part of the map's box)
    src, disp = layer("dm src", src_box), rng("dm map").random((map_box[2], map_box[3], 4))
    lin = np.array([0.9, -0.5, 0.4, 1.1])
    sbuf, dbuf = ctx.from_host(src), ctx.from_host(disp)
    out = poisoned((map_box[2], map_box[3], 4))
    n0 = ctx.launches()
    check(lib.svgr_layer_displacement_map(ctx.handle, out.handle, bb(map_box), dbuf.handle, sbuf.handle, bb(src_box), ptr(lin), 14.5, 0, 1))
    report("displacement_map", out, (map_box[2], map_box[3], 4), n0)

    params = np.array([9.5, 30.25, 21.0, 0.0, 0.0, 0.0, 3.0, 0.55])
    d = np.array([8.0, 120.0, 0.0]) - params[0:3]
    params[3:6] = d / np.sqrt((d * d).sum())
    color = np.array([0.95, 0.7, 0.35])
    for specular in (0, 1):
        out = poisoned((map_box[2], map_box[3], 4))
        n0 = ctx.launches()
        check(lib.svgr_layer_lighting(ctx.handle, out.handle, bb(map_box), sbuf.handle, bb(src_box), 2, ptr(params), ptr(color), 2.0, 0.9,
                                      17.0 if specular else 1.0, specular))
        report("lighting " + ("specular" if specular else "diffuse"), out, (map_box[2], map_box[3], 4), n0)

    tile_box = (-15, 30, 17, 23)   # (reaches beyond the source on one side)
    out = poisoned((map_box[2], map_box[3], 4))
    n0 = ctx.launches()
    check(lib.svgr_layer_tile(ctx.handle, out.handle, bb(map_box), sbuf.handle, bb(src_box), bb(tile_box)))
    report("tile", out, (map_box[2], map_box[3], 4), n0)

    # ---- every mix-blend mode: out of place over the union (a 1-channel source, then a 1-channel backdrop), in place with the
    #      source inside the backdrop and with the source partly outside it (a clipped window)
    b_box, s_box, s_out = (-4, 6, 37, 301), (3, 10, 12, 270), (30, 290, 20, 40)
    union = (-4, 6, 37, 301)
    b_img, s_img, s1_img, b1_img, so_img = layer("mb b", b_box), layer("mb s", s_box), layer("mb s1", s_box, 1), layer("mb b1", b_box, 1), layer("mb so", s_out)
    bufs = {k: ctx.from_host(v) for k, v in dict(b=b_img, s=s_img, s1=s1_img, b1=b1_img, so=so_img).items()}
    for mode in range(16):
        for name, bk, bch, sk, sch, sbox in (("4 over 4", "b", 4, "s", 4, s_box), ("1 over 4", "b", 4, "s1", 1, s_box), ("4 over 1", "b1", 1, "s", 4, s_box)):
            out = poisoned((union[2], union[3], 4))
            n0 = ctx.launches()
            check(lib.svgr_layer_mix_blend(ctx.handle, out.handle, bb(union), bufs[bk].handle, bb(b_box), bch, bufs[sk].handle, bb(sbox), sch, mode))
            report(f"mix_blend mode {mode} out of place {name}", out, (union[2], union[3], 4), n0)
        for name, sk, sbox in (("inside", "s", s_box), ("clipped", "so", s_out)):
            acc = ctx.from_host(b_img)
            n0 = ctx.launches()
            check(lib.svgr_layer_mix_blend(ctx.handle, acc.handle, bb(b_box), acc.handle, bb(b_box), 4, bufs[sk].handle, bb(sbox), 4, mode))
            report(f"mix_blend mode {mode} in place {name}", acc, b_img.shape, n0)

    # ---- the paint servers
    g_box = (-3, 11, 130, 300)
    user = S.Transform(np.array([[1.0 / 2, 0.0, 1.5], [0.0, 0.25, -2.25], [0.0, 0.0, 1.0]]))
    stops = [(o, np.array(c)) for o, c in STOPS]
    paints = {
        "linear": S.GradLinear(np.array([2.0, 1.0]), np.array([60.0, 70.0]), stops, None, "reflect", False, True),
        "radial": S.GradRadial(np.array([30.0, 40.0]), 35.0, None, None, stops, None, "repeat", False, True),
        "focal": S.GradRadial(np.array([30.0, 40.0]), 35.0, np.array([40.0, 30.0]), 4.0, stops, None, "pad", False, True),
        "focal outside": S.GradRadial(np.array([30.0, 40.0]), 12.0, np.array([70.0, 10.0]), 2.0, stops, None, "pad", False, True),
    }
    mask = rng("mask").random(g_box[2:])
    mbuf = ctx.from_host(mask)
    for name, paint in paints.items():
        g, keep = paint.abi(user, True)
        out = poisoned((g_box[2], g_box[3], 4))
        n0 = ctx.launches()
        check(lib.svgr_gradient_fill(ctx.handle, C.byref(g), mbuf.handle, bb(g_box), out.handle))
        report(f"gradient {name} (kind {g.kind})", out, (g_box[2], g_box[3], 4), n0)

    c, s = np.cos(0.5), np.sin(0.5)
    lin2 = np.array([[c, -s], [s, c]]) @ np.diag([1.7, 1.3])
    cell = (1.5, 0.25, 9.0, 6.0)
    corners = np.array([[0, 0], [cell[2], 0], [0, cell[3]], [cell[2], cell[3]]]) @ lin2.T
    mx, my = corners.max(axis=0).astype(int)
    nx, ny = corners.min(axis=0).astype(int)
    inv2 = np.linalg.inv(lin2)
    t = -inv2 @ np.array([3.25, -1.5])
    pa = _abi.PatternArgs()
    pa.inv_m6 = (C.c_double * 6)(inv2[0, 0], inv2[0, 1], t[0], inv2[1, 0], inv2[1, 1], t[1])
    pa.fwd_m6 = (C.c_double * 6)(lin2[0, 0], lin2[0, 1], 0.0, lin2[1, 0], lin2[1, 1], 0.0)
    pa.cell = (C.c_double * 4)(*cell)
    pa.min_xy = (C.c_int64 * 2)(int(nx), int(ny))
    pa.pat_shape = (C.c_int64 * 2)(int(mx - nx) + 1, int(my - ny) + 1)
    pa.tile_bbox = (C.c_int64 * 4)(-3 - int(nx), 2 - int(ny), 11, 9)
    tbuf = ctx.from_host(rng("pattern tile").uniform(-0.2, 1.2, (11, 9, 4)))
    out = poisoned((g_box[2], g_box[3], 4))
    n0 = ctx.launches()
    check(lib.svgr_pattern_fill(ctx.handle, C.byref(pa), tbuf.handle, mbuf.handle, bb(g_box), out.handle))
    report("pattern", out, (g_box[2], g_box[3], 4), n0)

    px = rng("image").integers(0, 256, (37, 53, 4), dtype=np.uint8)
    levels = _abi.image_upload(ctx, px, True)
    for smooth, lod in ((0, 0.0), (1, 0.0), (1, 1.4)):
        im = _abi.ImageArgs()
        im.inv_m6 = (C.c_double * 6)(0.2, 0.05, 1.0, -0.04, 0.15, -0.5)
        im.height, im.width = px.shape[:2]
        im.smooth, im.lod = smooth, lod
        out = poisoned((g_box[2], g_box[3], 4))
        n0 = ctx.launches()
        check(lib.svgr_image_fill(ctx.handle, C.byref(im), levels.handle, mbuf.handle, bb(g_box), out.handle))
        report(f"image smooth {smooth} lod {lod}", out, (g_box[2], g_box[3], 4), n0)


if __name__ == "__main__":
    main()
