"""CPU-only: the C ABI of the LAMB entry points (prototypes, argument refusals on the built libraries -- fake addresses, never dereferenced:
-1 is the argument check's answer, before any HIP call), the reference rule of tests/lamb_ref.py against torch.optim.AdamW and a case worked
by hand, and HybridLAMB's constructor."""
import ctypes
import math

import pytest
import torch

from lamb_ref import LambRef
from transformer_cnn_hybrid_network_for_video_processing_amd import _lib

FAKE = ctypes.c_void_p(16)
A, B, C, D, E, F = ((ctypes.c_void_p * 1)(16 * (i + 1)) for i in range(6))
NULL_ENTRY = (ctypes.c_void_p * 1)(None)
ONE, ZERO = (ctypes.c_longlong * 1)(5), (ctypes.c_longlong * 1)(0)
GROUP0, GROUP1 = (ctypes.c_ubyte * 1)(0), (ctypes.c_ubyte * 1)(1)

TRUST_ORDER = "count params grads exp_avg exp_avg_sq acc numel group groups hyper k step step_inc clip guard always_adapt partials trust_out".split()
STEP_ORDER = "count params grads exp_avg exp_avg_sq acc ema numel group groups hyper ema_hyper k step step_inc ticket clip guard trust".split()
TABLE = dict(count=1, params=A, grads=B, exp_avg=C, exp_avg_sq=D, acc=E, numel=ONE, group=GROUP0, groups=1, hyper=FAKE, k=2, step=1, step_inc=None,
             clip=FAKE, guard=FAKE)
VALID = {"hyb_lamb_trust": (TRUST_ORDER, dict(TABLE, always_adapt=0, partials=FAKE, trust_out=FAKE)),
         "hyb_lamb_step_dev": (STEP_ORDER, dict(TABLE, ema=F, ema_hyper=FAKE, ticket=None, trust=FAKE))}


def mutations(name):
    valid = VALID[name][1]
    for a in ("params", "exp_avg", "exp_avg_sq", "numel", "hyper", "partials", "trust_out", "trust", "ema", "ema_hyper"):
        if a in valid:
            yield f"{a} NULL", {a: None}
    for a in ("params", "grads", "exp_avg", "exp_avg_sq", "acc", "ema"):
        if a in valid:
            yield f"{a} with a NULL entry", {a: NULL_ENTRY}
    yield "count 0", dict(count=0)
    yield "count negative", dict(count=-1)
    yield "numel 0", dict(numel=ZERO)
    yield "step 0", dict(step=0)
    yield "k 0", dict(k=0)
    yield "acc == param", dict(acc=valid["params"])
    yield "acc NULL with grads NULL", dict(acc=None, grads=None, k=1)
    yield "acc NULL with k = 2", dict(acc=None)
    yield "guard without clip", dict(clip=None)
    yield "a group index >= groups", dict(group=GROUP1)
    yield "groups 0", dict(groups=0)
    yield "groups 256", dict(groups=256)
    yield "a table of 2^31 chunks", dict(numel=(ctypes.c_longlong * 1)(1 << 43))
    if name == "hyb_lamb_trust":
        yield "always_adapt 2", dict(always_adapt=2)
        yield "always_adapt negative", dict(always_adapt=-1)
    else:
        yield "ema == param", dict(ema=valid["params"])
        yield "a ticket without a counter", dict(ticket=FAKE, step_inc=None)


@pytest.fixture(scope="module")
def builds():
    from transformer_cnn_hybrid_network_for_video_processing_amd import build
    build.build()
    return (("libhybrid_hip", _lib.lib), ("libhybrid_hip_x3", _lib.lib.x3))


def status(dll, name, args):
    order = VALID[name][0]
    assert set(args) == set(order)
    return dll.raw(name)(*[args[p] for p in order], None)


def test_header_prototypes():
    protos = _lib.parse_header()
    assert protos["hyb_lamb_trust_workspace"] == ("size_t", ["int", "ptr"])
    assert protos["hyb_lamb_trust"] == ("int", ["int"] + ["ptr"] * 7 + ["int", "ptr", "long long", "long long", "ptr", "ptr", "ptr", "int", "ptr", "ptr", "ptr"])
    assert protos["hyb_lamb_step_dev"] == ("int", ["int"] + ["ptr"] * 8 + ["int", "ptr", "ptr", "long long", "long long"] + ["ptr"] * 6)
    # hyb_lamb_step_dev takes hyb_adamw_step_dev_groups' parameters, the trust block, the stream
    groups = protos["hyb_adamw_step_dev_groups"][1]
    assert protos["hyb_lamb_step_dev"][1] == groups[:-1] + ["ptr", "ptr"]
    for name, (order, valid) in VALID.items():
        assert len(protos[name][1]) == len(order) + 1 and set(valid) == set(order), name


def test_built_libraries_export_the_symbols_and_size_the_workspace(builds):
    numel = [1, 4096, 4097, 3 * 4096 + 1]
    arr = (ctypes.c_longlong * len(numel))(*numel)
    for _, dll in builds:
        assert dll.query("hyb_abi_version") == 9
        for name in ("hyb_lamb_trust_workspace", "hyb_lamb_trust", "hyb_lamb_step_dev"):
            dll.raw(name)
        assert dll.query("hyb_lamb_trust_workspace", len(numel), arr) == 2 * sum(-(-n // 4096) for n in numel)
        assert dll.query("hyb_lamb_trust_workspace", len(numel), arr) == 2 * dll.query("hyb_grad_norm_workspace", len(numel), arr)
        assert dll.query("hyb_lamb_trust_workspace", 0, arr) == 0 and dll.query("hyb_lamb_trust_workspace", 3, None) == 0
        assert dll.query("hyb_lamb_trust_workspace", 1, (ctypes.c_longlong * 1)(0)) == 0


@pytest.mark.parametrize("name", list(VALID))
def test_every_mutation_of_a_valid_call_is_refused_before_any_hip_call(builds, name):
    valid = VALID[name][1]
    labels = [label for label, _ in mutations(name)]
    assert len(set(labels)) == len(labels) and len(labels) >= 25
    for label, change in mutations(name):
        assert set(change) <= set(valid), label
        for lib_name, dll in builds:
            assert status(dll, name, dict(valid, **change)) == -1, f"{name}: {label} ({lib_name})"


@pytest.mark.parametrize("name", list(VALID))
def test_a_bad_entry_in_a_later_slice_is_refused_before_the_first_launch(builds, name):
    """81 tensors whose entry 80 is NULL: behind the first slice of every variant's table.  A launch of the first slice, here without a
    device, would have answered with a HIP error, not -1."""
    tables = [(ctypes.c_void_p * 81)(*[4096 * (j + 1) + 16 * (i + 1) for i in range(81)]) for j in range(6)]
    tables[2][80] = None                                              # exp_avg
    big = dict(count=81, params=tables[0], grads=tables[1], exp_avg=tables[2], exp_avg_sq=tables[3], acc=tables[4], ema=tables[5],
               numel=(ctypes.c_longlong * 81)(*[5] * 81), group=(ctypes.c_ubyte * 81)(*[0] * 81))
    valid = VALID[name][1]
    for lib_name, dll in builds:
        assert status(dll, name, dict(valid, **{k: v for k, v in big.items() if k in valid})) == -1, lib_name


# ---- the reference -----------------------------------------------------------------------------------------------------------------------------
def test_reference_without_weight_decay_is_adamw():
    g = torch.Generator().manual_seed(0)
    init = [torch.randn(n, generator=g, dtype=torch.float64) for n in (1, 7, 300)]
    hyper = dict(lr=3e-2, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.0)
    ref = LambRef([dict(params=init, **hyper)], torch.float64, always_adapt=False, max_grad_norm=None)
    ps = [torch.nn.Parameter(t.clone()) for t in init]
    opt = torch.optim.AdamW(ps, **hyper)
    for _ in range(5):
        grads = [torch.randn(t.shape, generator=g, dtype=torch.float64) for t in init]
        for p, gr in zip(ps, grads):
            p.grad = gr.clone()
        opt.step()
        ref.step(grads)
        assert all(t[2] == 1.0 for t in ref.trust)
        for a, b in zip(ref.params, ps):
            assert (a - b.detach()).abs().max().item() <= 1e-12 * max(1.0, b.detach().abs().max().item())
    # with always_adapt the ratios are no longer 1 and the run leaves AdamW's
    ada = LambRef([dict(params=init, **hyper)], torch.float64, always_adapt=True)
    ada.step([torch.ones_like(t) for t in init])
    assert all(t[2] != 1.0 for t in ada.trust)


def test_reference_on_a_case_worked_by_hand():
    """p = (3, 4), g = (1, -1), step 1 from zero moments, eps = 0: m_hat = g and v_hat = g^2, so q = sign(g) = (1, -1); wd = 0.5 gives
    u = (2.5, 1), |p| = 5, |u| = sqrt(7.25), r = 5 / sqrt(7.25); lr = 0.1: p' = p - 0.1 r u."""
    p, g = torch.tensor([3.0, 4.0], dtype=torch.float64), torch.tensor([1.0, -1.0], dtype=torch.float64)
    ref = LambRef([dict(params=[p], lr=0.1, betas=(0.9, 0.999), eps=0.0, weight_decay=0.5)], torch.float64)
    ref.step([g])
    r = 5.0 / math.sqrt(7.25)
    w_norm, u_norm, got_r = ref.trust[0]
    assert abs(w_norm - 5.0) <= 1e-12 and abs(u_norm - math.sqrt(7.25)) <= 1e-12 and abs(got_r - r) <= 1e-12
    want = torch.tensor([3.0 - 0.1 * r * 2.5, 4.0 - 0.1 * r * 1.0], dtype=torch.float64)
    assert (ref.params[0] - want).abs().max().item() <= 1e-12
    # clipping: max_grad_norm = 1 scales g by 1 / (sqrt(2) + 1e-6); q = sign(g) all the same at eps = 0, so the step is the same
    clipped = LambRef([dict(params=[p], lr=0.1, betas=(0.9, 0.999), eps=0.0, weight_decay=0.5)], torch.float64, max_grad_norm=1.0)
    total, coef = clipped.step([g])
    assert abs(total - math.sqrt(2.0)) <= 1e-12 and abs(coef - 1.0 / (math.sqrt(2.0) + 1e-6)) <= 1e-12
    assert (clipped.params[0] - want).abs().max().item() <= 1e-12
    # weight_decay = 0 without always_adapt: r = 1; a zero tensor: r = 1 whatever the flag
    plain = LambRef([dict(params=[p], lr=0.1, betas=(0.9, 0.999), eps=0.0, weight_decay=0.0)], torch.float64)
    plain.step([g])
    assert plain.trust[0][2] == 1.0 and (plain.params[0] - torch.tensor([2.9, 4.1], dtype=torch.float64)).abs().max().item() <= 1e-12
    zero = LambRef([dict(params=[torch.zeros(2, dtype=torch.float64)], lr=0.1, betas=(0.9, 0.999), eps=0.0, weight_decay=0.5)], torch.float64, always_adapt=True)
    zero.step([g])
    assert zero.trust[0] == (0.0, math.sqrt(2.0), 1.0)


# ---- the constructor ---------------------------------------------------------------------------------------------------------------------------
def test_constructor():
    from transformer_cnn_hybrid_network_for_video_processing_amd import HybridAdamW, HybridLAMB
    ps = [torch.nn.Parameter(torch.zeros(3))]
    opt = HybridLAMB(ps)
    assert isinstance(opt, HybridAdamW) and opt.uses_device_hyper() and opt.always_adapt is False and opt.trust_ratios() == {}
    g = opt.param_groups[0]
    assert (g["lr"], g["betas"], g["eps"], g["weight_decay"], g["max_grad_norm"]) == (1e-3, (0.9, 0.999), 1e-6, 1e-2, 1.0)
    assert set(opt.state_dict()["param_groups"][0]) == set(HybridAdamW(ps).state_dict()["param_groups"][0])
    assert HybridLAMB(ps, always_adapt=True, max_grad_norm=None).uses_device_hyper()
    for bad in (dict(lr=-1.0), dict(eps=-1.0), dict(betas=(1.0, 0.9)), dict(betas=(0.9, 1.0)), dict(weight_decay=-0.1), dict(always_adapt=1),
                dict(always_adapt=None), dict(max_grad_norm=0.0), dict(ema_decay=1.0), dict(accumulation_steps=0), dict(skip_nonfinite=1),
                dict(merge_groups="yes")):
        with pytest.raises(ValueError):
            HybridLAMB(ps, **bad)
