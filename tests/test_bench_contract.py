"""bench.py output contract on CPU: one JSON line from rank 0, whole-job value.

The driver launches ``bench.py`` directly for N=1 and through
``torch.distributed.run`` for N>1; these tests run both launch shapes on the
16^3 plumbing config with the gloo backend and check the JSON keys the driver
and judge read.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
        "scaling", "vs_baseline", "dtype", "data", "config"}


def _run(cmd, timeout=300):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def _check(r, n, steps, warmup):
    assert KEYS <= set(r)
    assert r["n_gpus"] == n and r["steps"] == steps and r["warmup"] == warmup
    assert r["value"] > 0 and r["ms_per_step"] > 0
    assert r["higher_is_better"] is True and r["scaling"] == "weak"
    assert "16^3" in r["data"] and r["data"].startswith("synthetic")
    cfg = r["config"]
    assert cfg["global_batch"] == cfg["per_gpu_batch"] * n
    assert cfg["parallelism"] == f"dp{n}"
    # value is the whole-job aggregate: global samples over the max-rank step time
    assert r["value"] == pytest.approx(cfg["global_batch"] / (r["ms_per_step"] / 1e3), rel=0.02)


def test_bench_single_process_json():
    r = _run([sys.executable, "bench.py", "--device", "cpu", "--tiny", "--steps", "2", "--warmup", "1",
              "--batch", "16"])
    _check(r, 1, 2, 1)


def test_bench_dump_outputs_and_full(tmp_path):
    """--dump-outputs writes the last timed step's loss / gradients / parameters as float32 .npy,
    identically from run to run; --full runs and keeps the plain keys."""
    import numpy as np

    base = [sys.executable, "bench.py", "--device", "cpu", "--tiny", "--steps", "2", "--warmup", "1", "--batch", "16"]
    a, b = tmp_path / "a", tmp_path / "b"
    r = _run(base + ["--dump-outputs", str(a)])
    _check(_run(base + ["--full", "--dump-outputs", str(b)]), 1, 2, 1)
    assert sorted(p.name for p in a.iterdir()) == ["grads.npy", "loss.npy", "params.npy"]
    total = 0
    for name in ("loss", "grads", "params"):
        x, y = np.load(a / f"{name}.npy"), np.load(b / f"{name}.npy")
        assert x.dtype == np.float32 and np.isfinite(x).all() and x.size > 0
        assert np.array_equal(x, y), name
        total += x.nbytes
    assert total <= 64 << 20
    assert np.load(a / "loss.npy").item() == pytest.approx(r["final_loss"], abs=1e-4)
    assert np.abs(np.load(a / "grads.npy")).max() > 0


@pytest.mark.slow
def test_bench_two_ranks_gloo_json():
    r = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
              "--master-addr", "127.0.0.1", "--master-port", "29561", "bench.py", "--gpus", "2",
              "--device", "cpu", "--dist-backend", "gloo", "--tiny", "--steps", "2", "--warmup", "1",
              "--batch", "16"])
    _check(r, 2, 2, 1)
