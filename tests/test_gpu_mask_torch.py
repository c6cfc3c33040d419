"""diff.compose_masked_tensor and diff.render_masked_tensor with torch, in ONE fresh child process that imports torch and
initialises CUDA before it touches the library (the import-order rule of svgrasterize_amd/tensor.py).  The child runs its checks
in order, stops at the first that fails and records each in a JSON file; this process asserts on that file and on the child's exit
status."""
import json
import multiprocessing
import os
import traceback

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H = 1e-6            # the step of the differences through the geometry (tests/cover_cases.py's)
NAMES = ["equals the numpy route", "refusals", "gradcheck compose_masked", "gradcheck render_masked", "fitting loop"]


def _checks():
    """(name, callable) in the order they run.  Everything is made inside: torch comes first."""
    import torch

    torch.cuda.init()
    from svgrasterize_amd import diff
    from tests import cover_ref as CR
    from tests import group_cases as GK
    from tests import mask_cases as K

    dev = torch.device("cuda", 0)

    def dt(a, grad=False, dtype=torch.float64):
        return torch.tensor(np.asarray(a), dtype=dtype, device=dev, requires_grad=grad)

    def gpt(gp, grad=False):
        return diff.GradientPaints(gp.kind, gp.spread, gp.path_stop_off, *(dt(getattr(gp, k), grad) for k in ("m6", "geom", "stop_pos", "stop_rgba")))

    def topo(c):
        return dict(kinds=c["kinds"], path_seg_off=c["off"], rules=c["rules"], viewport=c["viewport"])

    def equals_numpy_route():
        c = K.case("mask_generic", True)
        rows, cols = c["cover"].shape[1:]
        hgp, hgr = diff.GradientPaints(*c["gp"]), diff.Groups(*c["gr"])
        s = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(s):
            for dtype, npt in ((torch.float64, np.float64), (torch.float32, np.float32)):
                cover, g = c["cover"].astype(npt), c["g"].astype(npt)
                want = diff.compose_masked(cover, c["paints"], hgp, hgr, bg=c["bg"], origin=c["origin"])
                want_cover, want_paints, want_gp, want_op = diff.compose_masked_backward(cover, c["paints"], hgp, hgr, g, bg=c["bg"], origin=c["origin"])
                planes, paints, gp, opacity = dt(cover, True, dtype), dt(c["paints"], True), gpt(c["gp"], True), dt(c["gr"].opacity, True)
                out = torch.full((rows, cols, 4), 7.0, dtype=dtype, device=dev)
                got = diff.compose_masked_tensor(planes, paints, gp, hgr, opacity, bg=c["bg"], origin=c["origin"], out=out)
                assert got.data_ptr() == out.data_ptr() and got.dtype == dtype and tuple(got.shape) == (rows, cols, 4)   # out= is written in place
                (got * dt(g, dtype=dtype)).sum().backward()
                assert np.array_equal(out.detach().cpu().numpy(), want)
                assert np.array_equal(planes.grad.cpu().numpy(), want_cover) and np.array_equal(paints.grad.cpu().numpy(), want_paints)
                assert np.array_equal(opacity.grad.cpu().numpy(), want_op) and opacity.grad.dtype == torch.float64
                for k in ("m6", "geom", "stop_pos", "stop_rgba"):
                    assert np.array_equal(getattr(gp, k).grad.cpu().numpy(), getattr(want_gp, k)), k
                assert planes.grad.dtype == dtype
        plain = diff.compose_masked_tensor(dt(c["cover"]), dt(c["paints"]), gpt(c["gp"]), hgr, dt(c["gr"].opacity))   # the defaults
        assert not plain.requires_grad and np.array_equal(plain.cpu().numpy(), diff.compose_masked(c["cover"], c["paints"], hgp, hgr))
        flat = K.case("plain", False)   # no opacity at all: an empty tensor
        image = diff.compose_masked_tensor(dt(flat["cover"], True), dt(flat["paints"]), gpt(flat["gp"]), diff.Groups(*flat["gr"]), dt(np.zeros(0), True))
        image.sum().backward()
        assert np.array_equal(image.detach().cpu().numpy(), diff.compose_masked(flat["cover"], flat["paints"], diff.GradientPaints(*flat["gp"]), diff.Groups(*flat["gr"])))
        g = GK.case("nested3", True)   # a program without masks: compose_grouped_tensor's bits
        args = (dt(g["cover"]), dt(g["paints"]), gpt(g["gp"]), diff.Groups(*g["gr"]), dt(g["gr"].opacity))
        assert torch.equal(diff.compose_masked_tensor(*args, bg=g["bg"]), diff.compose_grouped_tensor(*args, bg=g["bg"]))
        r, paints_np, rgp, rgr = K.render_case()
        image = diff.render_masked_tensor(dt(r["segs"]), dt(r["m6"]), dt(paints_np), gpt(rgp), dt(rgr.opacity), groups=diff.Groups(*rgr), bg=r["bg"],
                                          dtype=torch.float64, check=True, **topo(r))
        want = K.reference_render(r, r["segs"], r["m6"], paints_np, rgp, rgr)
        assert tuple(image.shape) == (12, 11, 4) and np.abs(image.cpu().numpy() - want).max() <= 1e-11   # the mask KATs' tolerance
        assert diff.render_masked_tensor(dt(r["segs"]), dt(r["m6"]), dt(paints_np), gpt(rgp), dt(rgr.opacity), groups=diff.Groups(*rgr), **topo(r)).dtype == torch.float32
        # a loaded document with a <mask>: the renderer's picture, and a gradient to the mask's outline, gradient and the opacity
        import svgrasterize_amd as S
        from tests.test_gpu_mask import VIEWPORT, document_picture

        scene, want = document_picture()
        low = diff.lower_scene(scene, S.Transform(), masks=True)
        segs, lgp, opacity = dt(low.segs, True), gpt(low.gp, True), dt(low.groups.opacity, True)
        image = diff.render_masked_tensor(segs, dt(low.m6), dt(low.paints), lgp, opacity, groups=low.groups, kinds=low.kinds, path_seg_off=low.path_seg_off,
                                          rules=low.rules, viewport=VIEWPORT, dtype=torch.float64)
        assert np.abs(image.detach().cpu().numpy() - want).max() <= 1e-11   # (test_gpu_mask.py has the reason for the bound)
        (image * dt(np.random.default_rng(2).standard_normal((20, 20, 4)))).sum().backward()
        mine = slice(int(low.path_seg_off[2]), int(low.path_seg_off[3]))
        assert float(segs.grad[mine].abs().max()) > 1e-3 and float(lgp.geom.grad[2, :3].abs().min()) > 1e-4 and float(lgp.stop_rgba.grad.abs().max()) > 1e-3
        assert float(opacity.grad.abs().max()) > 1e-2

    def refusals():
        c = K.case("opacity_clip", False)
        planes, paints, gp, gr, opacity = dt(c["cover"]), dt(c["paints"]), gpt(c["gp"]), diff.Groups(*c["gr"]), dt(c["gr"].opacity)
        items = np.array(gr.items)
        assert items[4].tolist() == [3, 1, 0, 0]
        items[4, 0] = 2   # the target closed by END: its mask's group does not follow a HOLD
        for args, kw, exc in (((planes.half(), paints, gp, gr, opacity), {}, TypeError), ((planes, paints, gp, gr, opacity.float()), {}, TypeError),
                              ((planes, paints, gp, gr, opacity.cpu()), {}, TypeError), ((planes, paints, gp, gr, c["gr"].opacity), {}, TypeError),
                              ((planes, paints, gp, tuple(gr), opacity), {}, TypeError), ((planes, paints, tuple(gp)[:6], gr, opacity), {}, TypeError),
                              ((planes, paints, gp, gr._replace(items=torch.tensor(gr.items, device=dev)), opacity), {}, TypeError),
                              ((planes, paints, gp, gr, opacity[None]), {}, ValueError), ((planes, paints, gp, gr, torch.cat([opacity, opacity])), {}, ValueError),
                              ((planes, paints, gp, gr, opacity[:0]), {}, ValueError), ((planes, paints, gp, gr._replace(items=items), opacity), {}, ValueError),
                              ((planes, paints, gp, gr._replace(clip_planes=[3, 3]), opacity), {}, ValueError),
                              ((planes[:4], paints[:4], gpt(K.G.make_gp([None] * 4)), gr, opacity), {}, ValueError),
                              ((planes, paints, gp, gr, opacity), dict(bg=(0.0, 1.0)), ValueError), ((planes, paints, gp, gr, opacity), dict(origin=(1, 2, 3)), ValueError),
                              ((planes, paints, gp, gr, opacity), dict(out=torch.empty((12, 11, 3), dtype=torch.float64, device=dev)), ValueError)):
            with pytest.raises(exc):
                diff.compose_masked_tensor(*args, **kw)
        with pytest.raises(ValueError):   # and the grouped form refuses the masked program
            diff.compose_grouped_tensor(planes, paints, gp, gr, opacity)

    def gradcheck_compose_masked():
        cover, paints_np, hgp, hgr = K.small_case()
        assert cover.shape == (6, 6, 5) and hgr.items[:, 0].tolist() == [0, 1, 0, 1, 0, 2, 3, 1, 0, 0, 4] and hgp.kind.tolist() == [0, 0, 0, 0, 0, 1]
        groups = diff.Groups(*hgr)
        for bg in (None, K.BG):
            args = (dt(cover, True), dt(paints_np, True), dt(hgp.m6, True), dt(hgp.geom, True), dt(hgp.stop_pos, True), dt(hgp.stop_rgba, True),
                    dt(hgr.opacity, True))

            def f(planes, paints, m6, geom, pos, rgba, opacity):
                return diff.compose_masked_tensor(planes, paints, diff.GradientPaints(hgp.kind, hgp.spread, hgp.path_stop_off, m6, geom, pos, rgba), groups,
                                                  opacity, bg=bg)

            assert torch.autograd.gradcheck(f, args, fast_mode=False)   # torch's defaults: eps 1e-6, atol 1e-5, rtol 1e-3

    def gradcheck_render_masked():
        c, paints_np, hgp, hgr = K.render_case()
        groups = diff.Groups(*hgr)
        points, index = GK.point_index(c)
        idx = torch.tensor(index, device=dev)
        sizes = [points.size, 12, 8, hgp.m6.size, hgp.geom.size, hgp.stop_pos.size, hgp.stop_rgba.size, 1]
        cuts = np.cumsum([0] + sizes)

        def image_of(flat):
            pts, m6, paints, gm6, geom, pos, rgba, opacity = (flat[a:b] for a, b in zip(cuts, cuts[1:]))
            gp = hgp._replace(m6=gm6.reshape(2, 6), geom=geom.reshape(2, 4), stop_pos=pos, stop_rgba=rgba.reshape(-1, 4))
            return K.reference_render(c, pts.reshape(-1, 2)[index], m6.reshape(2, 6), paints.reshape(2, 4), gp, hgr._replace(opacity=opacity))

        # atol from the reference alone: per pixel and component 4 |FD_h - FD_2h|, plus the rounding of a difference of values <= 2
        trunc, scale = 0.0, 0.0
        flat = np.concatenate([points.ravel(), c["m6"].ravel(), paints_np.ravel(), hgp.m6.ravel(), hgp.geom.ravel(), hgp.stop_pos, hgp.stop_rgba.ravel(), hgr.opacity])
        for j in range(len(flat)):
            d = []
            for h in (H, 2 * H):
                lo, hi = flat.copy(), flat.copy()
                lo[j] -= h
                hi[j] += h
                d.append((image_of(hi) - image_of(lo)) / (2 * h))
            trunc, scale = max(trunc, float(np.abs(d[0] - d[1]).max())), max(scale, float(np.abs(d[0]).max()))
        atol = 4.0 * trunc + 2.0 ** -49 / H
        assert atol <= 1e-5 * scale, (atol, scale)
        _cover, _slope, _A, tol = CR.forward(c["segs"], c["kinds"], c["off"], c["m6"], c["rules"], c["viewport"])

        def f(pts, m6, paints, gm6, geom, pos, rgba, opacity):
            gp = diff.GradientPaints(hgp.kind, hgp.spread, hgp.path_stop_off, gm6, geom, pos, rgba)
            return diff.render_masked_tensor(pts[idx], m6, paints, gp, opacity, groups=groups, bg=c["bg"], dtype=torch.float64, **topo(c))

        args = tuple(dt(a, True) for a in (points, c["m6"], paints_np, hgp.m6, hgp.geom, hgp.stop_pos, hgp.stop_rgba, hgr.opacity))
        # the mask outline's control points do get a gradient, and so do its gradient's geometry and stops
        image = f(*args)
        (image * dt(np.random.default_rng(5).standard_normal(tuple(image.shape)))).sum().backward()
        mine = K.mask_points(c, index)
        assert float(args[0].grad[torch.tensor(mine, device=dev)].abs().max()) > 1e-2
        assert float(args[4].grad[0].abs().max()) > 1e-4 and float(args[5].grad.abs().max()) > 1e-4 and float(args[6].grad.abs().max()) > 1e-4
        for a in args:
            a.grad = None
        # (the coverage forward's atomic adds land in any order: two runs differ by the rounding of its sums, which a paint scales by <= 1)
        assert torch.autograd.gradcheck(f, args, eps=H, atol=atol, rtol=0.0, nondet_tol=4.0 * float(tol.max()) + 1e-15, fast_mode=False)

    def fitting_loop():
        c, paints_np, hgp, hgr = K.render_case()
        groups = diff.Groups(*hgr)
        losses = K.host_fit()
        assert losses[-1] < 0.1 * losses[0] and all(b < a for a, b in zip(losses, losses[1:])), losses
        segs, m6, paints, rest = dt(c["segs"]), dt(c["m6"]), dt(paints_np), dt(hgp.geom[1:])
        m6g, rgba = dt(hgp.m6), dt(hgp.stop_rgba)
        pos0 = hgp.stop_pos

        def render(opacity, stop, end):
            pos = torch.cat([dt(pos0[:1]), stop, dt(pos0[2:])])
            geom = torch.cat([torch.cat([dt(hgp.geom[0, :2]), end])[None], rest])
            gp = diff.GradientPaints(hgp.kind, hgp.spread, hgp.path_stop_off, m6g, geom, pos, rgba)
            return diff.render_masked_tensor(segs, m6, paints, gp, opacity, groups=groups, bg=c["bg"], dtype=torch.float64, **topo(c))

        tgp, topacity = K.fit_target(hgp, hgr.opacity)
        with torch.no_grad():
            target = render(dt(topacity), dt(tgp.stop_pos[1:2]), dt(tgp.geom[0, 2:]))
        opacity, stop, end = dt(hgr.opacity, True), dt(pos0[1:2], True), dt(hgp.geom[0, 2:], True)

        def loss_of():
            return 0.5 * ((render(opacity, stop, end) - target) ** 2).sum()

        for _ in range(K.FIT_STEPS):
            go, gs, ge = torch.autograd.grad(loss_of(), (opacity, stop, end))
            with torch.no_grad():
                opacity -= K.FIT_RATE_OPACITY * go
                stop -= K.FIT_RATE_STOP * gs
                end -= K.FIT_RATE_END * ge
        final = float(loss_of().item())
        assert abs(final - losses[-1]) <= 1e-6 * losses[-1], (final, losses[-1])
        assert abs(float(opacity) - K.FIT_OPACITY) < abs(float(hgr.opacity[0]) - K.FIT_OPACITY)   # and the parameters moved towards the target's

    checks = [equals_numpy_route, refusals, gradcheck_compose_masked, gradcheck_render_masked, fitting_loop]
    return list(zip(NAMES, checks))


def _child(path):
    results = []

    def record():
        with open(path, "w") as f:
            json.dump(results, f)

    try:
        checks = _checks()
    except BaseException:  # noqa: BLE001
        results.append({"name": "set-up", "ok": False, "error": traceback.format_exc()})
        record()
        raise SystemExit(1)
    for name, check in checks:
        results.append({"name": name, "ok": False, "error": "did not finish"})
        record()
        try:
            check()
        except BaseException:  # noqa: BLE001
            results[-1]["error"] = traceback.format_exc()
            record()
            raise SystemExit(1)
        results[-1].update(ok=True, error=None)
        record()


@pytest.mark.timeout(300)
def test_compose_masked_tensor_in_a_torch_first_child(tmp_path):
    path = str(tmp_path / "results.json")
    ctx = multiprocessing.get_context("spawn")
    child = ctx.Process(target=_child, args=(path,))
    child.start()
    child.join(240)
    if child.is_alive():
        child.kill()
        child.join()
        pytest.fail("the child did not finish")
    results = json.load(open(path)) if os.path.exists(path) else []
    for r in results:
        assert r["ok"], f"{r['name']}:\n{r['error']}"
    assert child.exitcode == 0, child.exitcode
    assert [r["name"] for r in results] == NAMES
