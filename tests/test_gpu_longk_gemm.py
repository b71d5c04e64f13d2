"""The long-K token GEMM (HYB_GEMM_LONGK, gemm_nt_longk_kernel in csrc/linear.hip) against gemm_nt_splitk_kernel, which it replaces for the
encoder's products with R >= 1024: one encoder forward + backward (bf16, no dropout) must give the same output, dx and parameter
gradients BIT FOR BIT under HYB_GEMM_LONGK=1 and =0.  Both kernels give wave w the k-steps w, w + 8, ... in that order and add the eight
partials as ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)); only the tile shape and the number of loads in flight differ, and neither
enters an element's value: nothing to tolerate.

The switch is read once per process: tests/longk_worker.py runs every case once under each value (two child processes for the whole
file) and the tests compare what they saved."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import longk_worker as worker      # noqa: E402  (the case tables; importing it starts nothing)


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    return worker.run_both(tmp_path_factory, "gemm", "HYB_GEMM_LONGK")


@pytest.mark.parametrize("name", list(worker.ENCODERS))
def test_encoder_is_the_same_bit_for_bit_on_the_long_k_kernel(both, name):
    on, off = both["1"][name], both["0"][name]
    B, S, D, Hid, H = worker.ENCODERS[name]
    # the comparison is not one of the old kernel with itself: the dispatcher's own rule takes the FFN products (R = Hid) in every case, the
    # Q|K|V dX (R = 3 D) where 3 D reaches 1024, the R = D products (the second Linear's dX with its Cmask epilogue) where D does -- and
    # none with the switch off
    rules = ("rule_ffn", "rule_qkv", "rule_d")
    assert [int(on[r]) for r in rules] == [1, int(3 * D >= 1024), int(D >= 1024)]
    assert [int(off[r]) for r in rules] == [0, 0, 0]
    tensors = sorted(k for k in on if k not in rules)
    assert len(tensors) == 2 + 14 * worker.LAYERS and set(on) == set(off)
    for k in tensors:
        assert on[k].dtype == off[k].dtype and on[k].shape == off[k].shape, k
        assert torch.isfinite(on[k].float()).all(), k
        assert torch.equal(on[k], off[k]), f"{k}: {(on[k].float() != off[k].float()).sum().item()} of {on[k].numel()} values differ"
    assert tuple(on["out"].shape) == (B, S, D) and on["out"].float().abs().mean() > 0.1 and on["dx"].float().abs().mean() > 0
