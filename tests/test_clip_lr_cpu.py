"""CPU-only tests of gradient-norm clipping / device hyper-parameters: the new C-ABI entry points are declared, exported by both builds and
refuse bad arguments without touching a device; HybridAdamW validates max_grad_norm and its state dict still interchanges with
torch.optim.AdamW in both directions."""
import ctypes

import pytest
import torch

import transformer_cnn_hybrid_network_for_video_processing_amd as P
from transformer_cnn_hybrid_network_for_video_processing_amd import _lib

NEW = ("hyb_adamw_hyper_set", "hyb_grad_norm_workspace", "hyb_grad_norm", "hyb_adamw_step_dev")


@pytest.fixture(scope="module")
def built():
    from transformer_cnn_hybrid_network_for_video_processing_amd import build
    build.build()
    return _lib.lib


def test_new_prototypes_are_parsed():
    protos = _lib.parse_header()
    assert protos["hyb_adamw_hyper_set"] == ("int", ["ptr"] + ["double"] * 6 + ["ptr"])
    assert protos["hyb_grad_norm_workspace"] == ("size_t", ["int", "ptr"])
    assert protos["hyb_grad_norm"] == ("int", ["int"] + ["ptr"] * 6)
    assert protos["hyb_adamw_step_dev"] == ("int", ["int"] + ["ptr"] * 6 + ["long long"] + ["ptr"] * 4)
    # the old entry point keeps its 15 arguments
    assert protos["hyb_adamw_step"] == ("int", ["int"] + ["ptr"] * 5 + ["double"] * 5 + ["long long"] + ["ptr"] * 3)


def test_both_builds_export_the_new_symbols_and_the_abi_version_stays(built):
    for name in NEW:
        built.raw(name)
        built.x3.raw(name)
    assert built.query("hyb_abi_version") == 9 and built.x3.query("hyb_abi_version") == 9


def test_argument_checks_fail_without_a_device(built):
    one = (ctypes.c_longlong * 1)(5)
    fake = ctypes.c_void_p(16)                     # never dereferenced: every check below fails before any HIP call
    ptrs = (ctypes.c_void_p * 1)(16)
    assert built.raw("hyb_adamw_hyper_set")(None, 1e-3, 0.9, 0.999, 1e-8, 0.01, 0.0, None) == -1
    assert built.raw("hyb_adamw_hyper_set")(fake, -1.0, 0.9, 0.999, 1e-8, 0.01, 0.0, None) == -1
    assert built.raw("hyb_adamw_hyper_set")(fake, 1e-3, 1.0, 0.999, 1e-8, 0.01, 0.0, None) == -1
    assert built.raw("hyb_adamw_hyper_set")(fake, 1e-3, 0.9, 0.999, 1e-8, 0.01, float("nan"), None) == -1
    assert built.raw("hyb_grad_norm")(0, None, None, None, None, None, None) == -1
    assert built.raw("hyb_grad_norm")(1, ptrs, one, None, fake, fake, None) == -1                # no partials
    assert built.raw("hyb_grad_norm")(1, ptrs, one, fake, fake, None, None) == -1                # no norm_out
    assert built.raw("hyb_grad_norm")(1, ptrs, (ctypes.c_longlong * 1)(0), fake, fake, fake, None) == -1
    assert built.raw("hyb_adamw_step_dev")(0, None, None, None, None, None, None, 1, None, None, None, None) == -1
    assert built.raw("hyb_adamw_step_dev")(1, ptrs, ptrs, ptrs, ptrs, one, None, 1, None, None, None, None) == -1    # no hyper block
    assert built.raw("hyb_adamw_step_dev")(1, ptrs, ptrs, ptrs, ptrs, one, fake, 0, None, None, None, None) == -1    # step is 1-based
    assert built.raw("hyb_adamw_step_dev")(1, ptrs, ptrs, ptrs, ptrs, one, fake, 1, None, fake, None, None) == -1    # ticket without counter
    with pytest.raises(RuntimeError, match="argument check"):
        built.call("hyb_grad_norm", 0, None, None, None, None, None, None)


def test_grad_norm_workspace_counts_4096_element_chunks(built):
    numel = [1, 4095, 4096, 4097, 262144, 1048576 + 3, 27]
    arr = (ctypes.c_longlong * len(numel))(*numel)
    assert built.query("hyb_grad_norm_workspace", len(numel), arr) == sum(-(-n // 4096) for n in numel)
    assert built.x3.query("hyb_grad_norm_workspace", len(numel), arr) == sum(-(-n // 4096) for n in numel)
    assert built.query("hyb_grad_norm_workspace", 0, arr) == 0 and built.query("hyb_grad_norm_workspace", 3, None) == 0
    assert built.query("hyb_grad_norm_workspace", 1, (ctypes.c_longlong * 1)(0)) == 0


def test_constructor_validates_max_grad_norm():
    p = [torch.nn.Parameter(torch.zeros(3))]
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="max_grad_norm"):
            P.HybridAdamW(p, max_grad_norm=bad)
    assert P.HybridAdamW(p).param_groups[0]["max_grad_norm"] is None
    assert P.HybridAdamW(p).uses_device_hyper() is False
    o = P.HybridAdamW(p, max_grad_norm=2.5)
    assert o.param_groups[0]["max_grad_norm"] == 2.5 and o.uses_device_hyper()
    o = P.HybridAdamW(p)
    o.set_dynamic_hyper(True)
    assert o.uses_device_hyper()
    two = P.HybridAdamW([{"params": [torch.nn.Parameter(torch.zeros(3))], "max_grad_norm": 1.0}, {"params": [torch.nn.Parameter(torch.zeros(2))]}])
    with pytest.raises(RuntimeError, match="same max_grad_norm"):
        two._clip_value()


def test_state_dict_interchanges_with_torch_adamw_in_both_directions():
    def params():
        return [torch.nn.Parameter(torch.arange(6, dtype=torch.float32).reshape(2, 3)), torch.nn.Parameter(torch.ones(4))]
    # torch -> Hybrid: the loaded groups lack max_grad_norm, which reads as "no clipping"
    pt = params()
    ot = torch.optim.AdamW(pt, lr=3e-4, weight_decay=0.1)
    for p in pt:
        p.grad = torch.ones_like(p)
    ot.step()
    oh = P.HybridAdamW(params(), lr=1.0, max_grad_norm=4.0)
    oh.load_state_dict(ot.state_dict())
    assert oh.param_groups[0]["lr"] == 3e-4 and oh.param_groups[0].get("max_grad_norm") is None
    assert oh._clip_value() is None and not oh.uses_device_hyper()
    st = oh.state[oh.param_groups[0]["params"][0]]
    assert st["step"] == 1 and torch.equal(st["exp_avg"], ot.state[pt[0]]["exp_avg"])
    # Hybrid -> torch: the extra group key is inert there, torch steps on
    oh2 = P.HybridAdamW(params(), lr=2e-3, max_grad_norm=4.0)
    sd = oh2.state_dict()
    assert sd["param_groups"][0]["max_grad_norm"] == 4.0
    pt2 = params()
    ot2 = torch.optim.AdamW(pt2, lr=1.0)
    ot2.load_state_dict(sd)
    assert ot2.param_groups[0]["lr"] == 2e-3
    for p in pt2:
        p.grad = torch.ones_like(p)
    ot2.step()
    assert all(torch.isfinite(p).all() for p in pt2)
    # Hybrid -> Hybrid keeps the value
    oh3 = P.HybridAdamW(params())
    oh3.load_state_dict(sd)
    assert oh3._clip_value() == 4.0 and oh3.uses_device_hyper()


def test_graphed_step_signature_has_dynamic_hyper():
    import inspect
    assert inspect.signature(P.GraphedTrainStep.__init__).parameters["dynamic_hyper"].default is False
