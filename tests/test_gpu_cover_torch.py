"""diff.coverage_tensor with torch, in ONE fresh child process that imports torch and initialises CUDA before it touches the
library (the import-order rule of svgrasterize_amd/tensor.py).  The child runs its checks in order, stops at the first that fails
and records each in a JSON file; this process asserts on that file and on the child's exit status."""
import json
import multiprocessing
import os
import traceback

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H = 1e-6
FIT_STEPS, FIT_RATE = 12, 0.02   # fixed on the CPU with the harness: the host loop ends below a tenth of its initial loss (checked below)
FIT_SHIFT = (1.2, -0.9)


def _point_index(c):
    """(points (n, 2), index (n_segs, 4)): the distinct control points of a case and where each segment's points are among them
    (an unused slot of a line points at point 0: its gradient is 0)."""
    index = np.zeros((len(c["segs"]), 4), dtype=np.int64)
    points = np.zeros((len(c["groups"]), 2))
    for i, grp in enumerate(c["groups"]):
        for s, k in grp:
            index[s, k] = i
        points[i] = c["segs"][grp[0][0], grp[0][1]]
    return points, index


def _host_fit(K, c):
    """Plain gradient descent with the harness: the losses of every step, the last one after the final update."""
    segs, m6 = c["segs"].copy(), np.array([K.IDENTITY], dtype=np.float64)
    target = K.harness_forward(segs, c["kinds"], c["off"], [[1.0, 0.0, FIT_SHIFT[0], 0.0, 1.0, FIT_SHIFT[1]]], c["rules"], c["viewport"])[0]
    losses = []
    for step in range(FIT_STEPS + 1):
        cover, slope, _acc, _st = K.harness_forward(segs, c["kinds"], c["off"], m6, c["rules"], c["viewport"])
        r = cover - target
        losses.append(0.5 * float((r * r).sum()))
        if step == FIT_STEPS:
            break
        gs, gm, _st = K.harness_backward(segs, c["kinds"], c["off"], m6, c["viewport"], slope, r)
        for grp in c["groups"]:
            g = sum(gs[s, k] for s, k in grp)
            for s, k in grp:
                segs[s, k] = segs[s, k] - FIT_RATE * g
        m6[0, 2] -= FIT_RATE * gm[0, 2]
        m6[0, 5] -= FIT_RATE * gm[0, 5]
    return target, losses


def _checks():
    """(name, callable) in the order they run.  Everything is made inside: torch comes first."""
    import torch

    torch.cuda.init()
    from oracle import oracle
    from svgrasterize_amd import diff
    from tests import cover_cases as K
    from tests import cover_ref as R

    dev = torch.device("cuda", 0)

    def tensors(c, grad=False):
        segs = torch.tensor(c["segs"], dtype=torch.float64, device=dev, requires_grad=grad)
        m6 = torch.tensor(c["m6"], dtype=torch.float64, device=dev, requires_grad=grad)
        return segs, m6

    def topo(c):
        return dict(kinds=c["kinds"], path_seg_off=c["off"], rules=c["rules"], viewport=c["viewport"])

    def equals_numpy_route():
        c = K.case("mixed", 1, "rotated")
        want, want_slope = diff.coverage(c["segs"], c["kinds"], c["off"], c["m6"], c["rules"], c["viewport"])
        g = torch.tensor(c["g"], dtype=torch.float64, device=dev)
        s = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(s):
            for dtype, tol in ((torch.float64, 1e-12), (torch.float32, 2.0 ** -24)):
                segs, m6 = tensors(c, grad=True)
                out = torch.full((1, 24, 21), 7.0, dtype=dtype, device=dev)
                got = diff.coverage_tensor(segs, m6, out=out, check=True, **topo(c))
                assert got.data_ptr() == out.data_ptr() and got.dtype == dtype and tuple(got.shape) == (1, 24, 21)
                (got * g.to(dtype)).sum().backward()
                host = got.detach().double().cpu().numpy()   # (a host wait)
                assert np.abs(host - want).max() <= tol, float(np.abs(host - want).max())
                ws, wm = diff.coverage_backward(c["segs"], c["kinds"], c["off"], c["m6"], c["rules"], c["viewport"], want_slope,
                                                c["g"].astype(np.float64 if dtype == torch.float64 else np.float32))
                assert np.array_equal(segs.grad.cpu().numpy(), ws) and np.array_equal(m6.grad.cpu().numpy(), wm)
        plain = diff.coverage_tensor(*tensors(c), **topo(c))   # the defaults: float32, no status read
        assert plain.dtype == torch.float32 and not plain.requires_grad
        assert np.abs(plain.double().cpu().numpy() - want).max() <= 2.0 ** -24
        on_device = dict(kinds=torch.tensor(c["kinds"], device=dev), path_seg_off=torch.tensor(c["off"], device=dev),
                         rules=torch.tensor(c["rules"], device=dev), viewport=c["viewport"])
        again = diff.coverage_tensor(*tensors(c), dtype=torch.float64, **on_device)
        assert np.abs(again.cpu().numpy() - want).max() <= 1e-12

    def refusals():
        c = K.case("polygon", 0, "identity")
        segs, m6 = tensors(c)
        for kw, exc in ((dict(dtype=torch.float16), TypeError), (dict(viewport=(0, 0, 0, 3)), ValueError), (dict(rules=[3]), ValueError),
                        (dict(kinds=c["kinds"][:-1]), ValueError), (dict(out=torch.empty((1, 3, 3), device=dev)), ValueError)):
            with pytest.raises(exc):
                diff.coverage_tensor(segs, m6, **{**topo(c), **kw})
        with pytest.raises(TypeError):
            diff.coverage_tensor(segs.float(), m6, **topo(c))
        with pytest.raises(TypeError):
            diff.coverage_tensor(segs.cpu(), m6, **topo(c))
        bad = segs.clone()
        bad[0, 0, 0] = float("nan")
        diff.coverage_tensor(bad, m6, **topo(c))   # not read: nothing raised, nothing waited for
        with pytest.raises(RuntimeError):
            diff.coverage_tensor(bad, m6, check=True, **topo(c))

    def gradcheck_case(name, rule):
        c = K.case(name, rule, "rotated")
        points, index = _point_index(c)
        idx = torch.tensor(index, device=dev)

        def planes(pts, m):
            segs = pts[index]
            ln, cb = K.lines_cubics(segs, c["kinds"])
            return oracle.mask(oracle.path_edges(ln, cb, R.m3(m)), c["viewport"], ("nonzero", "evenodd")[rule])

        # atol from the oracle alone: per pixel and component 4 |FD_h - FD_2h|, plus the rounding of a difference of values <= 1
        trunc, scale = 0.0, 0.0
        flat = np.concatenate([points.ravel(), c["m6"][0]])
        for j in range(len(flat)):
            d = []
            for h in (H, 2 * H):
                lo, hi = flat.copy(), flat.copy()
                lo[j] -= h
                hi[j] += h
                d.append((planes(hi[:-6].reshape(-1, 2), hi[-6:]) - planes(lo[:-6].reshape(-1, 2), lo[-6:])) / (2 * h))
            trunc, scale = max(trunc, float(np.abs(d[0] - d[1]).max())), max(scale, float(np.abs(d[0]).max()))
        atol = 4.0 * trunc + 2.0 ** -50 / H
        assert atol <= 1e-5 * scale, (atol, scale)
        _cover, _slope, _A, tol = R.forward(c["segs"], c["kinds"], c["off"], c["m6"], c["rules"], c["viewport"])

        def f(pts, m6):
            return diff.coverage_tensor(pts[idx], m6, dtype=torch.float64, **topo(c))

        pts = torch.tensor(points, dtype=torch.float64, device=dev, requires_grad=True)
        m6 = torch.tensor(c["m6"], dtype=torch.float64, device=dev, requires_grad=True)
        # (the forward's atomic adds land in any order: two runs differ by the rounding of the sums)
        assert torch.autograd.gradcheck(f, (pts, m6), eps=H, atol=atol, rtol=0.0, nondet_tol=float(tol.max()) + 1e-15, fast_mode=False)

    def fitting_loop():
        c = K.case("blob", 0, "identity")
        target_np, losses = _host_fit(K, c)
        assert losses[-1] < 0.1 * losses[0], losses
        points, index = _point_index(c)
        idx = torch.tensor(index, device=dev)
        target = torch.tensor(target_np, dtype=torch.float64, device=dev)
        pts = torch.tensor(points, dtype=torch.float64, device=dev, requires_grad=True)
        shift = torch.zeros(2, dtype=torch.float64, device=dev, requires_grad=True)
        base = torch.tensor([K.IDENTITY], dtype=torch.float64, device=dev)
        place = torch.zeros((2, 6), dtype=torch.float64, device=dev)
        place[0, 2] = place[1, 5] = 1.0

        def loss_of():
            m6 = base + (shift @ place)[None]
            cover = diff.coverage_tensor(pts[idx], m6, dtype=torch.float64, **topo(c))
            return 0.5 * ((cover - target) ** 2).sum()

        for _ in range(FIT_STEPS):
            loss = loss_of()
            gp, gs = torch.autograd.grad(loss, (pts, shift))
            with torch.no_grad():
                pts -= FIT_RATE * gp
                shift -= FIT_RATE * gs
        final = float(loss_of().item())
        assert abs(final - losses[-1]) <= 1e-6 * losses[-1], (final, losses[-1])

    return [("equals the numpy route", equals_numpy_route), ("refusals", refusals), ("gradcheck star", lambda: gradcheck_case("star", 0)),
            ("gradcheck blob", lambda: gradcheck_case("blob", 1)), ("fitting loop", fitting_loop)]


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
def test_coverage_tensor_in_a_torch_first_child(tmp_path):
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
    assert [r["name"] for r in results] == ["equals the numpy route", "refusals", "gradcheck star", "gradcheck blob", "fitting loop"]
