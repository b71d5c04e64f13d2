"""CPU-only tests of the weight average kept by HybridAdamW: the two new C-ABI entry points are declared, exported by both builds and refuse
bad arguments without touching a device; the constructor validates ema_decay, the defaults change nothing, and a state dict that carries
averages still interchanges with torch.optim.AdamW in both directions."""
import ctypes

import pytest
import torch

import transformer_cnn_hybrid_network_for_video_processing_amd as P
from transformer_cnn_hybrid_network_for_video_processing_amd import _lib

NEW = ("hyb_adamw_ema_set", "hyb_adamw_step_dev_ema")


@pytest.fixture(scope="module")
def built():
    from transformer_cnn_hybrid_network_for_video_processing_amd import build
    build.build()
    return _lib.lib


def test_new_prototypes_are_parsed_and_the_old_ones_unchanged():
    protos = _lib.parse_header()
    assert protos["hyb_adamw_ema_set"] == ("int", ["ptr", "double", "double", "ptr"])
    assert protos["hyb_adamw_step_dev_ema"] == ("int", ["int"] + ["ptr"] * 8 + ["long long"] + ["ptr"] * 4)
    assert protos["hyb_adamw_step"] == ("int", ["int"] + ["ptr"] * 5 + ["double"] * 5 + ["long long"] + ["ptr"] * 3)
    assert protos["hyb_adamw_step_dev"] == ("int", ["int"] + ["ptr"] * 6 + ["long long"] + ["ptr"] * 4)
    assert protos["hyb_adamw_hyper_set"] == ("int", ["ptr"] + ["double"] * 6 + ["ptr"])


def test_both_builds_export_the_new_symbols_and_the_abi_version_stays(built):
    for name in NEW:
        built.raw(name)
        built.x3.raw(name)
    assert built.query("hyb_abi_version") == 9 and built.x3.query("hyb_abi_version") == 9


def test_argument_checks_fail_without_a_device(built):
    one = (ctypes.c_longlong * 1)(5)
    fake = ctypes.c_void_p(16)                     # never dereferenced: every check below fails before any HIP call
    ptrs = (ctypes.c_void_p * 1)(16)
    other = (ctypes.c_void_p * 1)(32)
    null = (ctypes.c_void_p * 1)(None)
    for dll in (built, built.x3):
        ema_set, step = dll.raw("hyb_adamw_ema_set"), dll.raw("hyb_adamw_step_dev_ema")
        assert ema_set(None, 0.9, 0.0, None) == -1                                                   # NULL block
        for decay in (1.0, -0.1, float("nan")):
            assert ema_set(fake, decay, 0.0, None) == -1
        assert ema_set(fake, 0.9, 0.5, None) == -1                                                   # warmup is a flag: 0 or 1
        assert step(0, None, None, None, None, None, None, None, None, 1, None, None, None, None) == -1
        assert step(1, ptrs, ptrs, ptrs, ptrs, None, one, fake, fake, 1, None, None, None, None) == -1     # no ema array
        assert step(1, ptrs, ptrs, ptrs, ptrs, null, one, fake, fake, 1, None, None, None, None) == -1     # an ema entry that is NULL
        assert step(1, ptrs, ptrs, ptrs, ptrs, ptrs, one, fake, fake, 1, None, None, None, None) == -1     # the average IS the parameter
        assert step(1, ptrs, ptrs, ptrs, ptrs, other, one, fake, None, 1, None, None, None, None) == -1    # no ema_hyper block
        assert step(1, ptrs, ptrs, ptrs, ptrs, other, one, None, fake, 1, None, None, None, None) == -1    # no hyper block
        assert step(1, ptrs, ptrs, ptrs, ptrs, other, one, fake, fake, 0, None, None, None, None) == -1    # step is 1-based
        assert step(1, ptrs, ptrs, ptrs, ptrs, other, one, fake, fake, 1, None, fake, None, None) == -1    # ticket without counter
    with pytest.raises(RuntimeError, match="argument check"):
        built.call("hyb_adamw_ema_set", None, 0.9, 0.0, None)


def test_constructor_validates_ema_decay_and_the_defaults_change_nothing():
    p = [torch.nn.Parameter(torch.zeros(3))]
    for bad in (1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="ema_decay"):
            P.HybridAdamW(p, ema_decay=bad)
    o = P.HybridAdamW(p)
    assert o.param_groups[0]["ema_decay"] is None and o.param_groups[0]["ema_warmup"] is False
    assert o.uses_device_hyper() is False
    o = P.HybridAdamW(p, ema_decay=0.999)
    assert o.param_groups[0]["ema_decay"] == 0.999 and o.param_groups[0]["ema_warmup"] is False and o.uses_device_hyper() is True
    o = P.HybridAdamW(p, ema_decay=0.0, ema_warmup=True)                 # 0 is a decay (the average equals the weights), not "off"
    assert o.param_groups[0]["ema_warmup"] is True and o.uses_device_hyper() is True
    # groups may differ
    two = P.HybridAdamW([{"params": [torch.nn.Parameter(torch.zeros(3))], "ema_decay": 0.9}, {"params": [torch.nn.Parameter(torch.zeros(2))]}])
    assert [g["ema_decay"] for g in two.param_groups] == [0.9, None] and two.uses_device_hyper()
    # a value put into a group later is validated where it is used
    two.param_groups[1]["ema_decay"] = 1.0
    with pytest.raises(ValueError, match="ema_decay"):
        two._group_ema(two.param_groups[1])


def test_ema_model_needs_the_averages():
    lin = torch.nn.Linear(3, 2)
    o = P.HybridAdamW(lin.parameters(), ema_decay=0.9)
    with pytest.raises(RuntimeError, match="no average yet"):
        o.ema_model(lin)
    o.ema_init()
    twin = o.ema_model(lin)
    for (n, a), (_, b) in zip(lin.named_parameters(), twin.named_parameters()):
        assert b.data_ptr() == o.state[a]["ema"].data_ptr() != a.data_ptr() and not b.requires_grad and torch.equal(a, b), n
    # without an ema_decay the twin's parameters are the live ones
    o2 = P.HybridAdamW(lin.parameters())
    assert all(b.data_ptr() == a.data_ptr() and not b.requires_grad for a, b in zip(lin.parameters(), o2.ema_model(lin).parameters()))


def _params():
    return [torch.nn.Parameter(torch.arange(6, dtype=torch.float32).reshape(2, 3)), torch.nn.Parameter(torch.ones(4))]


def _with_state(opt):
    """A state as one step on the device would leave it (the step itself needs the GPU)."""
    for i, p in enumerate(opt.param_groups[0]["params"]):
        opt.state[p] = {"step": 1, "exp_avg": torch.full_like(p, 0.1), "exp_avg_sq": torch.full_like(p, 0.01), "ema": p.detach().clone() + (i + 1)}
    return opt


def test_state_dict_with_averages_interchanges_with_torch_adamw_in_both_directions():
    # torch -> Hybrid: no `ema` in the state, no key in the groups: reads as "off"
    pt = _params()
    ot = torch.optim.AdamW(pt, lr=3e-4, weight_decay=0.1)
    for p in pt:
        p.grad = torch.ones_like(p)
    ot.step()
    oh = P.HybridAdamW(_params(), lr=1.0, ema_decay=0.99, ema_warmup=True)
    oh.load_state_dict(ot.state_dict())
    g = oh.param_groups[0]
    assert g["lr"] == 3e-4 and g.get("ema_decay") is None and not g.get("ema_warmup")
    assert oh._group_ema(g) is None and not oh.uses_device_hyper()
    st = oh.state[g["params"][0]]
    assert st["step"] == 1 and "ema" not in st and torch.equal(st["exp_avg"], ot.state[pt[0]]["exp_avg"])
    # Hybrid -> torch: the extra state entry and the two group keys are inert there, torch steps on from the loaded moments
    oh2 = _with_state(P.HybridAdamW(_params(), lr=2e-3, ema_decay=0.99, ema_warmup=True))
    sd = oh2.state_dict()
    assert sd["param_groups"][0]["ema_decay"] == 0.99 and sd["param_groups"][0]["ema_warmup"] is True
    assert all("ema" in s for s in sd["state"].values())
    pt2 = _params()
    ot2 = torch.optim.AdamW(pt2, lr=1.0)
    ot2.load_state_dict(sd)
    assert ot2.param_groups[0]["lr"] == 2e-3
    assert torch.equal(ot2.state[pt2[0]]["exp_avg"], torch.full_like(pt2[0], 0.1))
    for p in pt2:
        p.grad = torch.ones_like(p)
    ot2.step()
    assert all(torch.isfinite(p).all() for p in pt2) and int(ot2.state[pt2[0]]["step"]) == 2


def test_hybrid_to_hybrid_keeps_the_average_and_its_settings():
    src = _with_state(P.HybridAdamW(_params(), ema_decay=0.99, ema_warmup=True))
    sd = src.state_dict()
    dst = P.HybridAdamW(_params())
    assert not dst.uses_device_hyper()
    dst.load_state_dict(sd)
    g = dst.param_groups[0]
    assert g["ema_decay"] == 0.99 and g["ema_warmup"] is True and dst._group_ema(g) == (0.99, 1.0) and dst.uses_device_hyper()
    for ps, pd in zip(src.param_groups[0]["params"], g["params"]):
        e = dst.state[pd]["ema"]
        assert e.dtype == torch.float32 and e.is_contiguous() and torch.equal(e, src.state[ps]["ema"])
        assert dst.state[pd]["step"] == 1
    # fp64 state in the file comes back as fp32
    sd64 = src.state_dict()
    sd64["state"] = {k: {n: (v.double() if torch.is_tensor(v) else v) for n, v in s.items()} for k, s in sd64["state"].items()}
    dst2 = P.HybridAdamW(_params())
    dst2.load_state_dict(sd64)
    assert all(dst2.state[p]["ema"].dtype == torch.float32 for p in dst2.param_groups[0]["params"])


def test_graphed_step_refuses_switching_the_average_after_capture():
    """(The decision only: _check_hyper on an object whose capture-time record says "no average".)"""
    lin = torch.nn.Linear(3, 2)
    opt = P.HybridAdamW(lin.parameters())
    tr = object.__new__(P.GraphedTrainStep)
    tr.optimizer, tr.criterion = opt, None
    tr._captured_loss_opts, tr._dev_hyper, tr._clipping = None, False, False
    tr._ema_on, tr._captured_hyper = [False], tr._hyper_now()
    tr._check_hyper()
    opt.param_groups[0]["ema_decay"] = 0.9
    with pytest.raises(RuntimeError, match="ema_decay was switched on or off"):
        tr._check_hyper()
