"""Layer.to_tensor, Layer.from_tensor and render_svgs_to_tensor with torch, in ONE fresh child process that imports torch and
initialises CUDA before it touches the library (the import-order rule of svgrasterize_amd/tensor.py: the other order leaves torch
without a device).  The child runs its checks in order, stops at the first that fails and records each in a JSON file; this
process asserts on that file and on the child's exit status, then checks that the wrong order -- its own -- is reported as a
RuntimeError."""
import json
import multiprocessing
import os
import traceback

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DOCS = [
    """<svg xmlns="http://www.w3.org/2000/svg" width="100" height="100"><circle cx="50" cy="50" r="40" fill="#c03"/>
    <rect x="10" y="10" width="30" height="20" fill="#369" fill-opacity="0.6"/></svg>""",
    """<svg xmlns="http://www.w3.org/2000/svg" width="200" height="50"><rect x="5" y="5" width="190" height="40" rx="8" fill="orange"
    stroke="navy" stroke-width="3"/></svg>""",
    """<svg xmlns="http://www.w3.org/2000/svg" width="30" height="90"><polygon points="15,5 28,85 2,85" fill="#0a0"/>
    <line x1="2" y1="45" x2="28" y2="45" stroke="black" stroke-width="4" stroke-opacity="0.5"/></svg>""",
]
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _bits(t):
    """A tensor's elements as integers (bfloat16 has no numpy type: compared through its bits)."""
    import torch

    view = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.uint8: torch.uint8}[t.dtype]
    return t.contiguous().view(view).cpu().numpy()


def _checks():
    """(name, callable) in the order they run.  Everything is made inside: torch comes first."""
    import torch

    torch.cuda.init()
    import svgrasterize_amd as S
    from svgrasterize_amd import tensor
    from tests import tensor_ref as R

    rng = np.random.default_rng(81)
    dev = torch.device("cuda", 0)
    small = rng.uniform(0, 1, (5, 7, 4))
    small[..., :3] *= small[..., 3:]
    image = R.random_layer(rng, 9, 300)
    DT = {torch.float32: R.F32, torch.float16: R.F16, torch.bfloat16: R.BF16, torch.uint8: R.U8}

    def ref_chw(img, bbox, rows, cols, dtype, channels=R.RGBA, **kw):
        return np.ascontiguousarray(R.pack_ref(img, bbox, rows, cols, DT[dtype], channels, **kw).transpose(2, 0, 1))

    def same(t, ref):
        got = _bits(t)
        assert got.shape == ref.shape and np.array_equal(got.view(ref.dtype), ref), "elements differ"

    def first_call():
        layer = S.Layer(small, (0, 0), True, False)
        out = layer.to_tensor()
        assert out.dtype == torch.float32 and tuple(out.shape) == (4, 5, 7) and out.device == dev
        same(out, ref_chw(small, (0, 0, 5, 7), 5, 7, torch.float32))

    def slices_and_windows():
        layer = S.Layer(image, (0, 0), True, False)
        batch = torch.full((4, 3, 9, 300), -3.0, dtype=torch.float16, device=dev)
        ret = layer.to_tensor(out=batch[2], channels="rgb")
        assert ret.data_ptr() == batch[2].data_ptr()
        want_batch = np.full((4, 3, 9, 300), np.float16(-3.0)).view(np.uint16)
        want_batch[2] = ref_chw(image, (0, 0, 9, 300), 9, 300, torch.float16, R.RGB)
        same(batch, want_batch)
        big = torch.full((4, 20, 333), 9.0, dtype=torch.float32, device=dev)
        layer.to_tensor(out=big[:, 1:10, 3:303])
        want = np.full((4, 20, 333), np.float32(9.0)).view(np.uint32)
        want[:, 1:10, 3:303] = ref_chw(image, (0, 0, 9, 300), 9, 300, torch.float32)
        same(big, want)
        hwc = torch.full((2, 12, 310, 4), 77, dtype=torch.uint8, device=dev)
        layer.to_tensor(out=hwc[1, 2:11, 5:305], layout="hwc")
        want = np.full((2, 12, 310, 4), 77, dtype=np.uint8)
        want[1, 2:11, 5:305] = R.pack_ref(image, (0, 0, 9, 300), 9, 300, R.U8)
        same(hwc, want)
        nhwc = torch.zeros((9, 300, 4), dtype=torch.float16, device=dev).permute(2, 0, 1)   # (C, rows, cols) in interleaved memory
        layer.to_tensor(out=nhwc)
        same(nhwc, ref_chw(image, (0, 0, 9, 300), 9, 300, torch.float16))
        for bad, exc in ((dict(out=batch[2]), ValueError), (dict(out=batch[2], channels="rgb", dtype=torch.float32), TypeError),
                         (dict(out=batch[2].cpu(), channels="rgb"), ValueError),
                         (dict(out=torch.zeros((3, 9, 600), dtype=torch.float16, device=dev)[:, :, ::2], channels="rgb"), ValueError)):
            try:
                layer.to_tensor(**bad)
            except exc:
                continue
            raise AssertionError(f"{bad} was not refused")
        same(batch, want_batch)

    def every_dtype():
        layer = S.Layer(image, (2, -5), True, False)
        for dtype in DT:
            for layout in ("chw", "hwc"):
                for channels, name in ((R.RGBA, "rgba"), (R.LUMA, "luma")):
                    out = layer.to_tensor(size=(12, 290), dtype=dtype, layout=layout, channels=name, bg=(0.5, 0.25, 1.0), mean=0.5, std=0.25)
                    n = R.N_CH[channels]
                    ref = R.pack_ref(image, (2, -5, 9, 300), 12, 290, DT[dtype], channels, (0.5, 0.25, 1.0), [4.0] * n, [-2.0] * n)
                    same(out, ref if layout == "hwc" else np.ascontiguousarray(ref.transpose(2, 0, 1)))

    def side_stream():
        clean = rng.uniform(0, 1, (9, 300, 4))   # (no NaN: the sum is compared)
        layer = S.Layer(clean, (0, 0), True, False)
        s = torch.cuda.Stream(device=dev)
        out = torch.empty((4, 9, 300), dtype=torch.float16, device=dev)
        with torch.cuda.stream(s):
            for _ in range(3):
                out.fill_(7)
                layer.to_tensor(out=out)
                total = out.double().sum()
            got = total.item()   # the only host wait
        # float16 values below 2 are multiples of 2^-24 and there are 10800 of them: the double sum is exact in any order
        want = float(R.decode_ref(R.F16, ref_chw(clean, (0, 0, 9, 300), 9, 300, torch.float16)).sum())
        assert got == want, (got, want)

    def from_tensor_composes():
        rows, cols = 24, 40
        y, x = torch.meshgrid(torch.arange(rows, device=dev), torch.arange(cols, device=dev), indexing="ij")
        grad = torch.stack([x / (cols - 1), y / (rows - 1), torch.full_like(x, 0.25, dtype=torch.float32), torch.ones_like(x, dtype=torch.float32)]).to(torch.float32)
        over = S.Layer(small, (3, 4), True, False)
        a = S.Layer.compose([S.Layer.from_tensor(grad, offset=(1, 2), linear_rgb=False), over], S.COMPOSE_OVER, linear_rgb=False)
        host = grad.cpu().numpy()
        b = S.Layer.compose([S.Layer.from_tensor(host, offset=(1, 2), linear_rgb=False), over], S.COMPOSE_OVER, linear_rgb=False)
        c = S.Layer.compose([S.Layer(np.ascontiguousarray(host.transpose(1, 2, 0)).astype(np.float64), (1, 2), True, False), over], S.COMPOSE_OVER, linear_rgb=False)
        assert a.on_device and tuple(a.offset) == tuple(c.offset)
        ia, ib, ic = a.image, b.image, c.image
        assert np.array_equal(ia, ib) and np.array_equal(ia, ic) and ia.shape == (rows, cols, 4)
        h = S.Layer.from_tensor(grad.to(torch.bfloat16)[:3].permute(1, 2, 0))   # (rows, cols, 3) view of planar memory, bfloat16
        want = grad.to(torch.bfloat16)[:3].to(torch.float64).permute(1, 2, 0).cpu().numpy()
        assert h.channels == 4 and np.array_equal(h.image[..., :3], want) and (h.image[..., 3] == 1).all()

    def svg_batch():
        out = torch.full((3, 3, 32, 48), 5.0, dtype=torch.float16, device=dev)
        ret = S.render_svgs_to_tensor(DOCS, (32, 48), out=out, dtype=torch.float16, channels="rgb", bg=(1, 1, 1), mean=MEAN, std=STD)
        assert ret is out
        got = _bits(out)
        for n, doc in enumerate(DOCS):
            layer = tensor._svg_layer(doc, (32, 48), None, None, False)
            alone = layer.to_array((32, 48), dtype=np.float16, channels="rgb", bg=(1, 1, 1), mean=MEAN, std=STD)
            assert np.array_equal(got[n].view(np.uint16), alone.view(np.uint16)), n
            white = np.float16(1.0 * (1.0 / STD[0]) + (-MEAN[0] / STD[0]))   # (the kernel's own order)
            assert (alone[0] == white).any() and (alone[0] != white).any(), "the document and the background around it"
        fresh = S.render_svgs_to_tensor(DOCS[:2], (16, 16), layout="hwc", dtype=torch.uint8, alpha="straight")
        assert tuple(fresh.shape) == (2, 16, 16, 4) and fresh.dtype == torch.uint8 and int(fresh[..., 3].max()) == 255

    return [("first call", first_call), ("slices and windows", slices_and_windows), ("every dtype", every_dtype),
            ("side stream", side_stream), ("from_tensor composes", from_tensor_composes), ("svg batch", svg_batch)]


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
def test_torch_first_child_and_the_wrong_order_here(tmp_path):
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
    assert [r["name"] for r in results] == ["first call", "slices and windows", "every dtype", "side stream", "from_tensor composes", "svg batch"]

    # this process: the library first, torch afterwards
    import svgrasterize_amd as S
    from svgrasterize_amd import tensor

    S.Context.get()
    import torch

    layer = S.Layer(np.zeros((2, 3, 4)), (0, 0), True, False)
    assert layer.to_array(dtype=np.float16).shape == (4, 2, 3), "to_array needs no torch and no order"
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="before the first svgrasterize_amd call"):
            layer.to_tensor()
        with pytest.raises(RuntimeError, match="before the first svgrasterize_amd call"):
            S.Layer.from_tensor(torch.zeros((4, 2, 3)))
        assert tensor.IMPORT_ORDER.startswith("torch finds no device")
