"""CPU-only tests of HybridAdamW's non-finite guard (skip_nonfinite): the three new C-ABI entry points are declared, exported by both builds
and refuse bad arguments without touching a device; the default changes nothing in `defaults`, the group keys or the state dict; the flag
is validated and takes the device path; state dicts still interchange with torch.optim.AdamW in both directions; and GraphedTrainStep
refuses a toggle after capture."""
import ctypes

import pytest
import torch

import transformer_cnn_hybrid_network_for_video_processing_amd as P
from transformer_cnn_hybrid_network_for_video_processing_amd import _lib

NEW = ("hyb_grad_norm_guard", "hyb_grad_norm_acc_guard", "hyb_adamw_step_dev_guard")


@pytest.fixture(scope="module")
def built():
    from transformer_cnn_hybrid_network_for_video_processing_amd import build
    build.build()
    return _lib.lib


def test_new_prototypes_are_parsed_and_the_old_ones_unchanged():
    protos = _lib.parse_header()
    # the unguarded twin's arguments, then guard, then stream
    assert protos["hyb_grad_norm_guard"] == ("int", ["int"] + ["ptr"] * 7)
    assert protos["hyb_grad_norm_acc_guard"] == ("int", ["int"] + ["ptr"] * 3 + ["long long"] + ["ptr"] * 5)
    assert protos["hyb_adamw_step_dev_guard"] == ("int", ["int"] + ["ptr"] * 9 + ["long long"] * 2 + ["ptr"] * 5)
    assert protos["hyb_grad_accumulate"] == ("int", ["int"] + ["ptr"] * 4)
    assert protos["hyb_adamw_step_dev_acc"] == ("int", ["int"] + ["ptr"] * 9 + ["long long"] * 2 + ["ptr"] * 4)
    assert protos["hyb_grad_norm_acc"] == ("int", ["int"] + ["ptr"] * 3 + ["long long"] + ["ptr"] * 4)
    assert protos["hyb_adamw_step"] == ("int", ["int"] + ["ptr"] * 5 + ["double"] * 5 + ["long long"] + ["ptr"] * 3)
    assert protos["hyb_adamw_step_dev"] == ("int", ["int"] + ["ptr"] * 6 + ["long long"] + ["ptr"] * 4)
    assert protos["hyb_adamw_step_dev_ema"] == ("int", ["int"] + ["ptr"] * 8 + ["long long"] + ["ptr"] * 4)
    assert protos["hyb_adamw_hyper_set"] == ("int", ["ptr"] + ["double"] * 6 + ["ptr"])
    assert protos["hyb_adamw_ema_set"] == ("int", ["ptr", "double", "double", "ptr"])
    assert protos["hyb_grad_norm"] == ("int", ["int"] + ["ptr"] * 6)
    assert protos["hyb_grad_norm_workspace"] == ("size_t", ["int", "ptr"])


def test_both_builds_export_the_new_symbols_and_the_abi_version_stays(built):
    for name in NEW:
        built.raw(name)
        built.x3.raw(name)
    assert built.query("hyb_abi_version") == 9 and built.x3.query("hyb_abi_version") == 9


def test_argument_checks_fail_without_a_device(built):
    one = (ctypes.c_longlong * 1)(5)
    zero = (ctypes.c_longlong * 1)(0)
    fake = ctypes.c_void_p(16)                     # never dereferenced: every check below fails before any HIP call
    ptrs = (ctypes.c_void_p * 1)(16)
    other = (ctypes.c_void_p * 1)(32)
    third = (ctypes.c_void_p * 1)(48)
    null = (ctypes.c_void_p * 1)(None)
    for dll in (built, built.x3):
        norm, norm_acc, step = dll.raw("hyb_grad_norm_guard"), dll.raw("hyb_grad_norm_acc_guard"), dll.raw("hyb_adamw_step_dev_guard")

        # hyb_grad_norm_guard(count, grads, numel, partials, hyper, norm_out, guard, stream)
        def n(count=1, grads=ptrs, numel=one, partials=fake, hyper=fake, out=fake, guard=fake):
            return norm(count, grads, numel, partials, hyper, out, guard, None)
        assert n(guard=None) == -1                                                                   # no guard block
        assert n(count=0) == -1 and n(count=-1) == -1 and n(grads=None) == -1 and n(grads=null) == -1 and n(numel=None) == -1
        assert n(numel=zero) == -1 and n(partials=None) == -1 and n(hyper=None) == -1 and n(out=None) == -1

        # hyb_grad_norm_acc_guard(count, acc, grads, numel, k, partials, hyper, norm_out, guard, stream)
        def na(count=1, acc=other, grads=ptrs, numel=one, k=2, partials=fake, hyper=fake, out=fake, guard=fake):
            return norm_acc(count, acc, grads, numel, k, partials, hyper, out, guard, None)
        assert na(guard=None) == -1
        assert na(count=0) == -1 and na(acc=None) == -1 and na(acc=null) == -1 and na(grads=null) == -1 and na(numel=None) == -1
        assert na(numel=zero) == -1 and na(k=0) == -1 and na(partials=None) == -1 and na(hyper=None) == -1 and na(out=None) == -1

        # hyb_adamw_step_dev_guard(count, params, grads, exp_avg, exp_avg_sq, acc, ema, numel, hyper, ema_hyper, k, step, step_inc, ticket, clip, guard, stream)
        def s(count=1, params=ptrs, grads=ptrs, m=ptrs, v=ptrs, acc=other, ema=None, numel=one, hyper=fake, ema_hyper=None, k=2, step_no=1,
              step_inc=None, ticket=None, clip=fake, guard=fake):
            return step(count, params, grads, m, v, acc, ema, numel, hyper, ema_hyper, k, step_no, step_inc, ticket, clip, guard, None)
        assert s(guard=None) == -1                                                                   # no guard block
        assert s(clip=None) == -1                                                                    # the guarded step always follows a norm call
        assert s(k=0) == -1 and s(k=-3) == -1                                                        # k < 1
        assert s(acc=None, k=2) == -1                                                                # no accumulators: the plain step, k == 1 ...
        assert s(acc=None, k=1, grads=None) == -1                                                    # ... which needs the gradients
        assert s(acc=null) == -1                                                                     # a NULL accumulator entry
        assert s(acc=ptrs) == -1                                                                     # the accumulator IS the parameter
        assert s(grads=null) == -1 and s(acc=None, k=1, grads=null) == -1                            # grads given: every entry non-NULL
        assert s(ema=third, ema_hyper=None) == -1 and s(ema=None, ema_hyper=fake) == -1              # both or neither
        assert s(ema=null, ema_hyper=fake) == -1                                                     # an ema entry that is NULL
        assert s(ema=ptrs, ema_hyper=fake) == -1                                                     # the average IS the parameter
        assert s(count=0) == -1 and s(params=None) == -1 and s(m=None) == -1 and s(v=None) == -1 and s(numel=None) == -1
        assert s(params=null) == -1 and s(m=null) == -1 and s(v=null) == -1 and s(numel=zero) == -1
        assert s(hyper=None) == -1                                                                   # no hyper block
        assert s(step_no=0) == -1                                                                    # step is 1-based
        assert s(ticket=fake) == -1                                                                  # ticket without counter
    with pytest.raises(RuntimeError, match="argument check"):
        built.call("hyb_grad_norm_guard", 1, ptrs, one, fake, fake, fake, None, None)


def test_the_default_changes_nothing_and_the_flag_is_validated():
    p = [torch.nn.Parameter(torch.zeros(3))]
    o = P.HybridAdamW(p)
    assert o.skip_nonfinite is False and o.uses_device_hyper() is False
    assert set(o.defaults) == {"lr", "betas", "eps", "weight_decay", "max_grad_norm", "ema_decay", "ema_warmup"}
    sd = o.state_dict()
    assert set(sd) == {"state", "param_groups"}
    assert set(sd["param_groups"][0]) == {"lr", "betas", "eps", "weight_decay", "max_grad_norm", "ema_decay", "ema_warmup", "params"}
    assert set(o.param_groups[0]) == set(sd["param_groups"][0])
    g = P.HybridAdamW(p, skip_nonfinite=True)
    assert g.skip_nonfinite is True and g.uses_device_hyper() is True
    assert g.defaults == o.defaults and set(g.param_groups[0]) == set(o.param_groups[0])           # neither a default nor a group key
    gsd = g.state_dict()                                                                             # (no device block yet: nothing to fold)
    assert set(gsd) == {"state", "param_groups"} and set(gsd["param_groups"][0]) == set(sd["param_groups"][0])
    for bad in (1, 0, None, "yes", 1.0):
        with pytest.raises(ValueError, match="skip_nonfinite must be a bool"):
            P.HybridAdamW(p, skip_nonfinite=bad)
        with pytest.raises(ValueError, match="skip_nonfinite must be a bool"):
            g.set_skip_nonfinite(bad)
    assert g.skip_nonfinite is True
    g.set_skip_nonfinite(False)
    assert g.skip_nonfinite is False and g.uses_device_hyper() is False and g.fold_skipped() == 0
    o.set_skip_nonfinite(True)
    assert o.uses_device_hyper() is True


def _params():
    return [torch.nn.Parameter(torch.arange(6, dtype=torch.float32).reshape(2, 3)), torch.nn.Parameter(torch.ones(4))]


def test_state_dicts_interchange_with_torch_adamw_in_both_directions():
    # torch -> Hybrid (guarded): the groups and the state load as ever, the flag is untouched by the load
    pt = _params()
    ot = torch.optim.AdamW(pt, lr=3e-4, weight_decay=0.1)
    for p in pt:
        p.grad = torch.ones_like(p)
    ot.step()
    oh = P.HybridAdamW(_params(), lr=1.0, skip_nonfinite=True)
    oh.load_state_dict(ot.state_dict())
    g = oh.param_groups[0]
    assert g["lr"] == 3e-4 and oh.skip_nonfinite is True and "skip_nonfinite" not in g
    st = oh.state[g["params"][0]]
    assert st["step"] == 1 and set(st) == {"step", "exp_avg", "exp_avg_sq"} and torch.equal(st["exp_avg"], ot.state[pt[0]]["exp_avg"])
    # Hybrid (guarded) -> torch: nothing new in the file, torch steps on from the loaded moments
    oh2 = P.HybridAdamW(_params(), lr=2e-3, skip_nonfinite=True)
    for p in oh2.param_groups[0]["params"]:
        oh2.state[p] = {"step": 1, "exp_avg": torch.full_like(p, 0.1), "exp_avg_sq": torch.full_like(p, 0.01)}
    sd = oh2.state_dict()
    assert all(set(s) == {"step", "exp_avg", "exp_avg_sq"} for s in sd["state"].values())
    assert "skip_nonfinite" not in sd["param_groups"][0] and set(sd) == {"state", "param_groups"}
    pt2 = _params()
    ot2 = torch.optim.AdamW(pt2, lr=1.0)
    ot2.load_state_dict(sd)
    assert ot2.param_groups[0]["lr"] == 2e-3 and torch.equal(ot2.state[pt2[0]]["exp_avg"], torch.full_like(pt2[0], 0.1))
    for p in pt2:
        p.grad = torch.ones_like(p)
    ot2.step()
    assert all(torch.isfinite(p).all() for p in pt2) and int(ot2.state[pt2[0]]["step"]) == 2
    # Hybrid -> Hybrid: a plain optimizer loads a guarded one's file and stays plain
    oh3 = P.HybridAdamW(_params())
    oh3.load_state_dict(sd)
    assert oh3.skip_nonfinite is False and not oh3.uses_device_hyper()


def test_graphed_step_refuses_a_toggle_after_capture():
    """(The decision only: _check_hyper on an object that never captured.)"""
    lin = torch.nn.Linear(3, 2)
    opt = P.HybridAdamW(lin.parameters())
    tr = object.__new__(P.GraphedTrainStep)
    tr.optimizer, tr.criterion = opt, None
    tr._captured_loss_opts, tr._dev_hyper, tr._clipping = None, False, False
    tr._ema_on, tr._captured_hyper, tr._guard_on = [False], tr._hyper_now(), False
    tr._check_hyper()
    opt.set_skip_nonfinite(True)
    with pytest.raises(RuntimeError, match="skip_nonfinite was switched on or off after capture"):
        tr._check_hyper()
    opt.set_skip_nonfinite(False)
    tr._check_hyper()
    tr._guard_on = True                                # ... and captured with the guard, switched off afterwards
    with pytest.raises(RuntimeError, match="skip_nonfinite was switched on or off after capture"):
        tr._check_hyper()
