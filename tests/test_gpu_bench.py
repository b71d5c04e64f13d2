"""bench.py on one GPU: a plain run prints the headline only, and --dump-outputs writes what the last timed step computed, identically
for two runs with the same arguments (a small workload)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(outdir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "2", "--frames", "4",
           "--size", "64", "--dump-outputs", str(outdir), *extra]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=280)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = [l for l in r.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_dumps_the_last_step_reproducibly(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    d = _run(a)
    _run(b)
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "clips/s" and d["higher_is_better"] is True and d["dtype"] == "bf16"
    assert abs(d["value"] - 2 * 3 / (d["ms_per_step"] * 3 / 1e3)) < 1e-6 * d["value"]
    assert not any(k in d for k in ("fwd_bwd_only", "pcie_inclusive", "roofline", "kernel_table", "cpu_baseline", "logits_check"))
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and len(names) == d["outputs"]["arrays"]
    assert {"loss.npy", "logits.npy", "grad.head.weight.npy", "param.head.weight.npy", "buffer.encoder1.enc1norm1.running_mean.npy"} <= set(names)
    assert sum(os.path.getsize(a / n) for n in names) <= 64 * 1000 * 1000
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype == np.float32 and np.isfinite(x).all(), n
        assert np.array_equal(x, y), n
    assert np.load(a / "logits.npy").shape == (2, 8)
    assert np.load(a / "loss.npy") == np.float32(d["final_loss"])


def test_eager_run_dumps_the_same_arrays(tmp_path):
    """--eager (no graph replay): the step's logits come from the Python-issued forward; the same set of arrays is written."""
    a, e = tmp_path / "a", tmp_path / "e"
    _run(a)
    d = _run(e, "--eager")
    assert d["steps"] == 3 and "eager" in d["config"]["launch"]
    assert sorted(os.listdir(e)) == sorted(os.listdir(a))
    for n in os.listdir(e):
        x = np.load(e / n)
        assert x.dtype == np.float32 and x.shape == np.load(a / n).shape and np.isfinite(x).all(), n
    assert np.load(e / "loss.npy") == np.float32(d["final_loss"])
