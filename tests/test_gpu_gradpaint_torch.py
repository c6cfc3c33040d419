"""diff.compose_painted_tensor and diff.render_painted_tensor with torch, in ONE fresh child process that imports torch and
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
NAMES = ["equals the numpy route", "refusals", "gradcheck compose_painted", "gradcheck render_painted", "fitting loop"]


def _checks():
    """(name, callable) in the order they run.  Everything is made inside: torch comes first."""
    import torch

    torch.cuda.init()
    from svgrasterize_amd import diff
    from tests import cover_ref as CR
    from tests import gradpaint_cases as G
    from tests.test_gpu_compose_torch import _point_index

    dev = torch.device("cuda", 0)

    def dt(a, grad=False, dtype=torch.float64):
        return torch.tensor(np.asarray(a), dtype=dtype, device=dev, requires_grad=grad)

    def gpt(gp, grad=False, **over):
        """GradientPaints of tensors from a host one."""
        t = {k: over.get(k, dt(getattr(gp, k), grad)) for k in ("m6", "geom", "stop_pos", "stop_rgba")}
        return diff.GradientPaints(gp.kind, gp.spread, gp.path_stop_off, **t)

    def topo(c):
        return dict(kinds=c["kinds"], path_seg_off=c["off"], rules=c["rules"], viewport=c["viewport"])

    def equals_numpy_route():
        c = G.case("mixed", True)
        rows, cols = c["cover"].shape[1:]
        hgp = diff.GradientPaints(*c["gp"])
        s = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(s):
            for dtype, npt in ((torch.float64, np.float64), (torch.float32, np.float32)):
                cover, g = c["cover"].astype(npt), c["g"].astype(npt)
                want = diff.compose_painted(cover, c["paints"], hgp, bg=c["bg"], origin=c["origin"])
                want_cover, want_paints, want_gp = diff.compose_painted_backward(cover, c["paints"], hgp, g, bg=c["bg"], origin=c["origin"])
                planes, paints, gp = dt(cover, True, dtype), dt(c["paints"], True), gpt(c["gp"], True)
                out = torch.full((rows, cols, 4), 7.0, dtype=dtype, device=dev)
                got = diff.compose_painted_tensor(planes, paints, gp, bg=c["bg"], origin=c["origin"], out=out)
                assert got.data_ptr() == out.data_ptr() and got.dtype == dtype and tuple(got.shape) == (rows, cols, 4)   # out= is written in place
                (got * dt(g, dtype=dtype)).sum().backward()
                assert np.array_equal(out.detach().cpu().numpy(), want)
                assert np.array_equal(planes.grad.cpu().numpy(), want_cover) and np.array_equal(paints.grad.cpu().numpy(), want_paints)
                for k in ("m6", "geom", "stop_pos", "stop_rgba"):
                    assert np.array_equal(getattr(gp, k).grad.cpu().numpy(), getattr(want_gp, k)), k
                assert planes.grad.dtype == dtype and gp.geom.grad.dtype == torch.float64
        plain = diff.compose_painted_tensor(dt(c["cover"]), dt(c["paints"]), gpt(c["gp"]))   # the defaults: no bg, origin (0, 0), a new image
        assert not plain.requires_grad and np.array_equal(plain.cpu().numpy(), diff.compose_painted(c["cover"], c["paints"], hgp))
        only = dt(c["gp"].geom, True)
        diff.compose_painted_tensor(dt(c["cover"]), dt(c["paints"]), gpt(c["gp"], geom=only), bg=c["bg"], origin=c["origin"]).sum().backward()
        want = diff.compose_painted_backward(c["cover"], c["paints"], hgp, np.ones((rows, cols, 4)), bg=c["bg"], origin=c["origin"])[2].geom
        assert np.array_equal(only.grad.cpu().numpy(), want)
        solid = G.make_gp([None] * len(c["cover"]))   # no stops at all: empty tensors
        image = diff.compose_painted_tensor(dt(c["cover"], True), dt(c["paints"]), gpt(solid, True), bg=c["bg"])
        image.sum().backward()
        assert np.array_equal(image.detach().cpu().numpy(), diff.compose(c["cover"], c["paints"], bg=c["bg"]))
        r, paints_np, rgp = G.render_case()
        image = diff.render_painted_tensor(dt(r["segs"]), dt(r["m6"]), dt(paints_np), gpt(rgp), bg=r["bg"], dtype=torch.float64, check=True, **topo(r))
        want = G.reference_render(r, r["segs"], r["m6"], paints_np, rgp)
        assert tuple(image.shape) == (12, 11, 4) and np.abs(image.cpu().numpy() - want).max() <= 1e-11   # the mask KATs' tolerance
        assert diff.render_painted_tensor(dt(r["segs"]), dt(r["m6"]), dt(paints_np), gpt(rgp), **topo(r)).dtype == torch.float32

    def refusals():
        c = G.case("mixed", False)
        planes, paints, gp = dt(c["cover"]), dt(c["paints"]), gpt(c["gp"])
        kind = np.array(c["gp"].kind)
        kind[1] = 3
        for args, kw, exc in (((planes.half(), paints, gp), {}, TypeError), ((planes, paints.float(), gp), {}, TypeError),
                              ((planes.cpu(), paints, gp), {}, TypeError), ((c["cover"], paints, gp), {}, TypeError),
                              ((planes, paints, diff.GradientPaints(*c["gp"])), {}, TypeError), ((planes, paints, gp._replace(geom=gp.geom.float())), {}, TypeError),
                              ((planes, paints, gp._replace(stop_pos=gp.stop_pos.cpu())), {}, TypeError), ((planes, paints, tuple(gp)[:6]), {}, TypeError),
                              ((planes, paints, gp._replace(kind=torch.tensor(kind, device=dev))), {}, TypeError),
                              ((planes[0], paints, gp), {}, ValueError), ((planes, paints[:2], gp), {}, ValueError),
                              ((planes, paints, gp._replace(m6=gp.m6[:, :5])), {}, ValueError), ((planes, paints, gp._replace(geom=gp.geom[:3])), {}, ValueError),
                              ((planes, paints, gp._replace(stop_rgba=gp.stop_rgba[:6])), {}, ValueError),
                              ((planes, paints, gp._replace(stop_pos=gp.stop_pos[:6])), {}, ValueError),
                              ((planes, paints, gp._replace(kind=kind)), {}, ValueError), ((planes, paints, gp._replace(path_stop_off=[0, 0, 3, 6, 7])), {}, ValueError),
                              ((planes, paints, gp), dict(bg=(0.0, 1.0)), ValueError), ((planes, paints, gp), dict(origin=(1, 2, 3)), ValueError),
                              ((planes, paints, gp), dict(out=torch.empty((12, 11, 3), dtype=torch.float64, device=dev)), ValueError),
                              ((planes, paints, gp), dict(out=torch.empty((12, 11, 4), dtype=torch.float32, device=dev)), ValueError)):
            with pytest.raises(exc):
                diff.compose_painted_tensor(*args, **kw)

    def gradcheck_compose_painted():
        cover, paints_np, hgp = G.small_case()
        assert hgp.kind.tolist() == [0, 1, 2] and hgp.spread.tolist() == [0, 2, 1] and cover.shape == (3, 6, 5)
        for bg in (None, G.BG):
            args = (dt(cover, True), dt(paints_np, True), dt(hgp.m6, True), dt(hgp.geom, True), dt(hgp.stop_pos, True), dt(hgp.stop_rgba, True))

            def f(planes, paints, m6, geom, pos, rgba):
                return diff.compose_painted_tensor(planes, paints, diff.GradientPaints(hgp.kind, hgp.spread, hgp.path_stop_off, m6, geom, pos, rgba), bg=bg)

            assert torch.autograd.gradcheck(f, args, fast_mode=False)   # torch's defaults: eps 1e-6, atol 1e-5, rtol 1e-3

    def gradcheck_render_painted():
        c, paints_np, hgp = G.render_case()
        points, index = _point_index(c)
        idx = torch.tensor(index, device=dev)
        sizes = [points.size, 12, 8, hgp.m6.size, hgp.geom.size, hgp.stop_pos.size, hgp.stop_rgba.size]
        cuts = np.cumsum([0] + sizes)

        def image_of(flat):
            pts, m6, paints, gm6, geom, pos, rgba = (flat[a:b] for a, b in zip(cuts, cuts[1:]))
            gp = hgp._replace(m6=gm6.reshape(2, 6), geom=geom.reshape(2, 4), stop_pos=pos, stop_rgba=rgba.reshape(-1, 4))
            return G.reference_render(c, pts.reshape(-1, 2)[index], m6.reshape(2, 6), paints.reshape(2, 4), gp)

        # atol from the reference alone: per pixel and component 4 |FD_h - FD_2h|, plus the rounding of a difference of values <= 2
        trunc, scale = 0.0, 0.0
        flat = np.concatenate([points.ravel(), c["m6"].ravel(), paints_np.ravel(), hgp.m6.ravel(), hgp.geom.ravel(), hgp.stop_pos, hgp.stop_rgba.ravel()])
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

        def f(pts, m6, paints, gm6, geom, pos, rgba):
            gp = diff.GradientPaints(hgp.kind, hgp.spread, hgp.path_stop_off, gm6, geom, pos, rgba)
            return diff.render_painted_tensor(pts[idx], m6, paints, gp, bg=c["bg"], dtype=torch.float64, **topo(c))

        args = tuple(dt(a, True) for a in (points, c["m6"], paints_np, hgp.m6, hgp.geom, hgp.stop_pos, hgp.stop_rgba))
        # (the coverage forward's atomic adds land in any order: two runs differ by the rounding of its sums, which a paint scales by <= 1)
        assert torch.autograd.gradcheck(f, args, eps=H, atol=atol, rtol=0.0, nondet_tol=4.0 * float(tol.max()) + 1e-15, fast_mode=False)

    def fitting_loop():
        c, paints_np, hgp = G.render_case()
        losses = G.host_fit()
        assert losses[-1] < 0.05 * losses[0] and all(b < a for a, b in zip(losses, losses[1:])), losses
        segs, m6 = dt(c["segs"]), dt(c["m6"])
        gm6, pos = dt(hgp.m6), dt(hgp.stop_pos)
        ones = dt(paints_np[:1])   # path 0 keeps its multiplier of ones; path 1 is the solid paint

        def render(solid, geom0, rgba):
            paints = torch.cat([ones, solid[None]])
            geom = torch.cat([geom0[None], dt(hgp.geom[1:])])
            gp = diff.GradientPaints(hgp.kind, hgp.spread, hgp.path_stop_off, gm6, geom, pos, rgba)
            return diff.render_painted_tensor(segs, m6, paints, gp, bg=c["bg"], dtype=torch.float64, **topo(c))

        with torch.no_grad():
            target = render(dt(G.FIT_SOLID), dt(G.FIT_GEOM), dt(G.fit_target_rgba(hgp.stop_rgba)))
        solid, geom0, rgba = dt(paints_np[1], True), dt(hgp.geom[0], True), dt(hgp.stop_rgba, True)

        def loss_of():
            return 0.5 * ((render(solid, geom0, rgba) - target) ** 2).sum()

        for _ in range(G.FIT_STEPS):
            gs, gg, gr = torch.autograd.grad(loss_of(), (solid, geom0, rgba))
            with torch.no_grad():
                solid -= G.FIT_RATE_COLOUR * gs
                rgba -= G.FIT_RATE_COLOUR * gr
                geom0 -= G.FIT_RATE_GEOM * gg
        final = float(loss_of().item())
        assert abs(final - losses[-1]) <= 1e-6 * losses[-1], (final, losses[-1])

    checks = [equals_numpy_route, refusals, gradcheck_compose_painted, gradcheck_render_painted, fitting_loop]
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
def test_compose_painted_tensor_in_a_torch_first_child(tmp_path):
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
