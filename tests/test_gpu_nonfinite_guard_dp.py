"""The non-finite guard with data parallelism: two ranks, only rank 1's batch is poisoned, both ranks skip the step
(tests/nonfinite_guard_dp_worker.py, after tests/test_gpu_accum_dp.py).  Needs two GPUs."""
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
@pytest.mark.parametrize("k", [1, 2])
def test_a_batch_poisoned_on_one_rank_skips_the_step_on_both(k):
    """The norm is taken over the all-reduced buckets: both ranks report the skip, the parameters stay bit-equal to what they were and across
    the ranks, the buckets are zero afterwards when they are the accumulators (k = 2), and the next clean step applies on both ranks."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "nonfinite_guard_dp_worker.py"), str(k)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=280)
    lines = [l for l in r.stdout.decode().splitlines() if l.startswith("NFDP")]
    assert r.returncode == 0, "\n".join(lines) + "\n" + r.stderr.decode()[-2000:]
    assert len(lines) == 2, lines
    for l in lines:
        assert "skipped (1, 1)" in l and "parameters unchanged True" in l and "norm finite False" in l, l
        assert "ranks equal after the skip True" in l and "clean step applied True" in l and "ranks equal after it True" in l, l
        assert "steps done 2" in l and "step counts [2]" in l, l
        if k == 2:
            assert "buckets zero True" in l, l
