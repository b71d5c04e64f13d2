"""Gradient accumulation with data parallelism on a one-GPU box: two gloo ranks sharing cuda:0 (the pattern of
tests/test_gpu_dp.py::test_graph_and_eager_dp_steps_end_bit_equal)."""
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_accumulated_dp_steps_equal_the_eager_reference_and_reduce_once_per_optimizer_step():
    """GraphedTrainStep(accumulation_steps=2) on two ranks against an eager reference that forms the accumulated gradient with torch ops,
    all-reduces it once and takes a plain device-path step on acc * inv_k: parameters and BatchNorm buffers bit-equal on every rank and equal
    across ranks; exactly two all-reduces (one per bucket) per optimizer step, not per micro-step; both buckets all zero after the update
    (tests/accum_dp_worker.py)."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "accum_dp_worker.py")]
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=280)
    lines = [l for l in r.stdout.decode().splitlines() if l.startswith("ACDP")]
    assert r.returncode == 0, "\n".join(lines) + "\n" + r.stderr.decode()[-2000:]
    assert len(lines) == 2, lines
    for l in lines:
        assert "mismatching tensors []" in l and "all ranks equal True" in l, l
        assert "all-reduces per optimizer step [2, 2]" in l and "buckets zero after update [True, True]" in l, l
        assert "update flags ok True" in l and "fwd_bwd refused True" in l, l
