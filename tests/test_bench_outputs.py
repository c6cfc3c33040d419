"""bench.py's plain run and `--dump-outputs DIR`: the plain line carries the contract fields and nothing that needs runs of its
own (those are `--full`), `--steps` is the number of timed steps, and the dump is float32 / float64 .npy files within 64 MB
whose sample does not depend on the run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def test_image_outputs_whole_or_fixed_sample():
    import bench

    small = np.arange(64 * 32 * 4, dtype=np.float32).reshape(64, 32, 4)
    out = bench.image_outputs("canvas", small)
    assert list(out) == ["canvas"] and np.array_equal(out["canvas"], small)

    big = np.random.default_rng(1).random((4096, 2048, 4))   # 256 MB of float64: sampled
    a = bench.image_outputs("layer", big)
    b = bench.image_outputs("layer", np.zeros_like(big))
    assert sorted(a) == ["layer_row_sums", "layer_sample", "layer_sample_pixels"]
    assert np.array_equal(a["layer_sample_pixels"], b["layer_sample_pixels"])   # same pixels whatever the data
    pix = a["layer_sample_pixels"].astype(np.int64)
    assert np.array_equal(a["layer_sample"], big.reshape(-1, 4)[pix])
    assert np.allclose(a["layer_row_sums"], big.reshape(4096, -1).sum(axis=1))
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_LIMIT_BYTES


def test_dump_outputs_writes_npy_and_refuses_too_much(tmp_path):
    import bench

    bench.dump_outputs(str(tmp_path / "d"), {"x": np.ones((3, 4), np.float32), "y": np.zeros(2)})
    assert sorted(os.listdir(tmp_path / "d")) == ["x.npy", "y.npy"]
    assert np.load(tmp_path / "d" / "x.npy").dtype == np.float32
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "e"), {"x": np.zeros(bench.DUMP_LIMIT_BYTES // 8 + 1)})


@pytest.mark.gpu
def test_plain_run_and_dump(tmp_path):
    d = tmp_path / "out"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(d)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 3 and line["warmup"] == 1 and line["value"] > 0 and line["ms_per_step"] > 0
    for k in ("cpu_baseline", "parity", "configs", "roofline", "cold_ms"):
        assert k not in line, k
    files = sorted(os.listdir(d))
    assert files == ["canvas_row_sums.npy", "canvas_sample.npy", "canvas_sample_pixels.npy"], files
    assert sum(os.path.getsize(d / f) for f in files) <= 64 << 20
    sample = np.load(d / "canvas_sample.npy")
    rows = np.load(d / "canvas_row_sums.npy")
    assert sample.dtype == np.float32 and sample.shape[1] == 4 and rows.shape == (4096,)
    assert np.isfinite(sample).all() and 0.0 <= sample.min() and sample.max() <= 1.0 and rows.max() > 0
