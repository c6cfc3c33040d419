"""diff.compose_grouped_tensor and diff.render_grouped_tensor with torch, in ONE fresh child process that imports torch and
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
NAMES = ["equals the numpy route", "refusals", "gradcheck compose_grouped", "gradcheck render_grouped", "fitting loop"]


def _checks():
    """(name, callable) in the order they run.  Everything is made inside: torch comes first."""
    import torch

    torch.cuda.init()
    from svgrasterize_amd import diff
    from tests import cover_ref as CR
    from tests import group_cases as K

    dev = torch.device("cuda", 0)

    def dt(a, grad=False, dtype=torch.float64):
        return torch.tensor(np.asarray(a), dtype=dtype, device=dev, requires_grad=grad)

    def gpt(gp, grad=False):
        return diff.GradientPaints(gp.kind, gp.spread, gp.path_stop_off, *(dt(getattr(gp, k), grad) for k in ("m6", "geom", "stop_pos", "stop_rgba")))

    def topo(c):
        return dict(kinds=c["kinds"], path_seg_off=c["off"], rules=c["rules"], viewport=c["viewport"])

    def equals_numpy_route():
        c = K.case("gradient_generic", True)
        rows, cols = c["cover"].shape[1:]
        hgp, hgr = diff.GradientPaints(*c["gp"]), diff.Groups(*c["gr"])
        s = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(s):
            for dtype, npt in ((torch.float64, np.float64), (torch.float32, np.float32)):
                cover, g = c["cover"].astype(npt), c["g"].astype(npt)
                want = diff.compose_grouped(cover, c["paints"], hgp, hgr, bg=c["bg"], origin=c["origin"])
                want_cover, want_paints, want_gp, want_op = diff.compose_grouped_backward(cover, c["paints"], hgp, hgr, g, bg=c["bg"], origin=c["origin"])
                planes, paints, gp, opacity = dt(cover, True, dtype), dt(c["paints"], True), gpt(c["gp"], True), dt(c["gr"].opacity, True)
                out = torch.full((rows, cols, 4), 7.0, dtype=dtype, device=dev)
                got = diff.compose_grouped_tensor(planes, paints, gp, hgr, opacity, bg=c["bg"], origin=c["origin"], out=out)
                assert got.data_ptr() == out.data_ptr() and got.dtype == dtype and tuple(got.shape) == (rows, cols, 4)   # out= is written in place
                (got * dt(g, dtype=dtype)).sum().backward()
                assert np.array_equal(out.detach().cpu().numpy(), want)
                assert np.array_equal(planes.grad.cpu().numpy(), want_cover) and np.array_equal(paints.grad.cpu().numpy(), want_paints)
                assert np.array_equal(opacity.grad.cpu().numpy(), want_op) and opacity.grad.dtype == torch.float64
                for k in ("m6", "geom", "stop_pos", "stop_rgba"):
                    assert np.array_equal(getattr(gp, k).grad.cpu().numpy(), getattr(want_gp, k)), k
                assert planes.grad.dtype == dtype
        plain = diff.compose_grouped_tensor(dt(c["cover"]), dt(c["paints"]), gpt(c["gp"]), hgr, dt(c["gr"].opacity))   # the defaults
        assert not plain.requires_grad and np.array_equal(plain.cpu().numpy(), diff.compose_grouped(c["cover"], c["paints"], hgp, hgr))
        only = dt(c["gr"].opacity, True)
        diff.compose_grouped_tensor(dt(c["cover"]), dt(c["paints"]), gpt(c["gp"]), hgr, only, bg=c["bg"], origin=c["origin"]).sum().backward()
        want = diff.compose_grouped_backward(c["cover"], c["paints"], hgp, hgr, np.ones((rows, cols, 4)), bg=c["bg"], origin=c["origin"])[3]
        assert np.array_equal(only.grad.cpu().numpy(), want)
        flat = K.case("clip1", False)   # no opacity at all: an empty tensor
        image = diff.compose_grouped_tensor(dt(flat["cover"], True), dt(flat["paints"]), gpt(flat["gp"]), diff.Groups(*flat["gr"]), dt(np.zeros(0), True))
        image.sum().backward()
        assert np.array_equal(image.detach().cpu().numpy(), diff.compose_grouped(flat["cover"], flat["paints"], diff.GradientPaints(*flat["gp"]), diff.Groups(*flat["gr"])))
        r, paints_np, rgp, rgr = K.render_case()
        image = diff.render_grouped_tensor(dt(r["segs"]), dt(r["m6"]), dt(paints_np), gpt(rgp), dt(rgr.opacity), groups=diff.Groups(*rgr), bg=r["bg"],
                                           dtype=torch.float64, check=True, **topo(r))
        want = K.reference_render(r, r["segs"], r["m6"], paints_np, rgp, rgr)
        assert tuple(image.shape) == (12, 11, 4) and np.abs(image.cpu().numpy() - want).max() <= 1e-11   # the mask KATs' tolerance
        assert diff.render_grouped_tensor(dt(r["segs"]), dt(r["m6"]), dt(paints_np), gpt(rgp), dt(rgr.opacity), groups=diff.Groups(*rgr), **topo(r)).dtype == torch.float32

    def refusals():
        c = K.case("both", False)
        planes, paints, gp, gr, opacity = dt(c["cover"]), dt(c["paints"]), gpt(c["gp"]), diff.Groups(*c["gr"]), dt(c["gr"].opacity)
        items = np.array(gr.items)
        items[1, 1] = 3
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
                diff.compose_grouped_tensor(*args, **kw)

    def gradcheck_compose_grouped():
        cover, paints_np, hgp, hgr = K.small_case()
        levels = np.cumsum(np.where(hgr.items[:, 0] == 1, 1, np.where(hgr.items[:, 0] == 2, -1, 0)))
        assert cover.shape == (6, 6, 5) and levels.max() == 2 and np.diff(hgr.clip_off).tolist() == [2] and hgp.kind.tolist() == [0, 0, 1, 0, 0, 0]
        groups = diff.Groups(*hgr)
        for bg in (None, K.BG):
            args = (dt(cover, True), dt(paints_np, True), dt(hgp.m6, True), dt(hgp.geom, True), dt(hgp.stop_pos, True), dt(hgp.stop_rgba, True),
                    dt(hgr.opacity, True))

            def f(planes, paints, m6, geom, pos, rgba, opacity):
                return diff.compose_grouped_tensor(planes, paints, diff.GradientPaints(hgp.kind, hgp.spread, hgp.path_stop_off, m6, geom, pos, rgba), groups,
                                                   opacity, bg=bg)

            assert torch.autograd.gradcheck(f, args, fast_mode=False)   # torch's defaults: eps 1e-6, atol 1e-5, rtol 1e-3

    def gradcheck_render_grouped():
        c, paints_np, hgp, hgr = K.render_case()
        groups = diff.Groups(*hgr)
        points, index = K.point_index(c)
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
            return diff.render_grouped_tensor(pts[idx], m6, paints, gp, opacity, groups=groups, bg=c["bg"], dtype=torch.float64, **topo(c))

        args = tuple(dt(a, True) for a in (points, c["m6"], paints_np, hgp.m6, hgp.geom, hgp.stop_pos, hgp.stop_rgba, hgr.opacity))
        # the clip outline's control points do get a gradient
        image = f(*args)
        (image * dt(np.random.default_rng(5).standard_normal(tuple(image.shape)))).sum().backward()
        mine = K.clip_points(c, index)
        assert float(args[0].grad[torch.tensor(mine, device=dev)].abs().max()) > 1e-2
        for a in args:
            a.grad = None
        # (the coverage forward's atomic adds land in any order: two runs differ by the rounding of its sums, which a paint scales by <= 1)
        assert torch.autograd.gradcheck(f, args, eps=H, atol=atol, rtol=0.0, nondet_tol=4.0 * float(tol.max()) + 1e-15, fast_mode=False)

    def fitting_loop():
        c, paints_np, hgp, hgr = K.render_case()
        groups = diff.Groups(*hgr)
        losses = K.host_fit()
        assert losses[-1] < 0.1 * losses[0] and all(b < a for a, b in zip(losses, losses[1:])), losses
        points, index = K.point_index(c)
        idx = torch.tensor(index, device=dev)
        mine = dt(K.clip_points(c, index)[:, None].astype(np.float64))
        m6, gp, rest = dt(c["m6"]), gpt(hgp), dt(paints_np[1:])

        def render(pts, opacity, paint0):
            return diff.render_grouped_tensor(pts[idx], m6, torch.cat([paint0[None], rest]), gp, opacity, groups=groups, bg=c["bg"], dtype=torch.float64, **topo(c))

        with torch.no_grad():
            target = render(dt(points) + mine * dt(K.FIT_SHIFT), dt([K.FIT_OPACITY]), dt(K.FIT_PAINT))
        pts, opacity, paint0 = dt(points, True), dt(hgr.opacity, True), dt(paints_np[0], True)

        def loss_of():
            return 0.5 * ((render(pts, opacity, paint0) - target) ** 2).sum()

        for _ in range(K.FIT_STEPS):
            gpts, go, gpaint = torch.autograd.grad(loss_of(), (pts, opacity, paint0))
            with torch.no_grad():
                pts -= K.FIT_RATE_POINTS * mine * gpts
                opacity -= K.FIT_RATE_OPACITY * go
                paint0 -= K.FIT_RATE_PAINT * gpaint
        final = float(loss_of().item())
        assert abs(final - losses[-1]) <= 1e-6 * losses[-1], (final, losses[-1])

    checks = [equals_numpy_route, refusals, gradcheck_compose_grouped, gradcheck_render_grouped, fitting_loop]
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
def test_compose_grouped_tensor_in_a_torch_first_child(tmp_path):
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
