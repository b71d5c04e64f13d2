"""HybridAdamW(skip_nonfinite=True) on the device: with finite gradients every step is bit-identical to the unguarded optimizer's; one
poisoned gradient element (an infinity, a NaN, or a finite 1e20 whose square overflows fp32) anywhere in the tensor table makes the step
leave parameters, moments and the weight average bit for bit as they were, counts it, zeroes the accumulators and advances the counter;
afterwards the run has the parameters of a run that never saw the batch; several groups skip together and are counted once; the skipped
count folds into `step` and through a state dict; GraphedTrainStep replays through a poisoned batch; and the refusals.

Every comparison is bitwise.  The tensor sets and the small model (SMALL) are those of tests/test_gpu_accum.py."""
import copy

import pytest
import torch

from test_gpu_accum import _all_plus_zero, _bind, _init, _model, _new_grads, _params

pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")
POISONS = {"+inf": INF, "-inf": -INF, "nan": NAN, "1e20": 1e20}
# (tensor set, tensor, element): the first element of the first tensor; index 4096 of the 4097-element tensor (its tail chunk); inside the
# 1025-element tensor at a 4-byte offset (the scalar path); tensor 85 of the 90 (the second norm launch, and the second AdamW launch)
POSITIONS = {"first": (False, 0, 0), "tail_chunk": (False, 4, 4096), "misaligned": (False, 6, 500), "tensor85of90": (True, 85, 2)}


def P():
    import transformer_cnn_hybrid_network_for_video_processing_amd as pkg
    return pkg


def _opt(ps, guard, clip=None, ema=None, k=1, **kw):
    return P().HybridAdamW(ps, lr=1e-3, max_grad_norm=clip, ema_decay=ema, accumulation_steps=k, skip_nonfinite=guard, **kw)


def _state(ps, opt, ema):
    keys = ("exp_avg", "exp_avg_sq") + (("ema",) if ema is not None else ())
    return [[p.detach().clone()] + [opt.state[p][key].clone() for key in keys] for p in ps]


def _same(a, b, tag):
    for i, (ta, tb) in enumerate(zip(a, b)):
        for j, (x, y) in enumerate(zip(ta, tb)):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (tag, i, j)       # bit for bit (a NaN equals itself here)


def _one_step(opts_params, micro_grads, counters=()):
    """One optimizer step of every (optimizer, parameters) pair on the same k micro-batches of gradients."""
    k = len(micro_grads)
    for j, grads in enumerate(micro_grads):
        for opt, ps in opts_params:
            _bind(ps, grads)                                # (shared: the launches only read them)
            if j < k - 1:
                opt.accumulate()
            else:
                opt.step()
        if j < k - 1:
            for c in counters:
                c.add_(1)                                   # what ends a micro-step that is no update in GraphedTrainStep


def _micro_grads(ps, gen, k, many):
    return [_new_grads(ps, gen, many) for _ in range(k)]


# ---- 1. finite gradients: the guard changes nothing ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("many", [False, True])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("ema", [None, 0.9])
@pytest.mark.parametrize("clip", [None, 3.0])
def test_finite_gradients_are_bit_identical_to_the_unguarded_optimizer(clip, ema, k, many):
    init = _init(2, many)
    a, b, c = _params(init, many), _params(init, many), _params(init, many)
    oa, ob = _opt(a, True, clip, ema, k), _opt(b, False, clip, ema, k)
    oc = _opt(c, False, 3.0, None, k)                # clip is None: the unguarded optimizer takes no norm; this one's norm is the reference
    gen = torch.Generator().manual_seed(3)
    for s in range(3):
        _one_step([(oa, a), (ob, b), (oc, c)], _micro_grads(a, gen, k, many))
        _same(_state(a, oa, ema), _state(b, ob, ema), (clip, ema, k, many, s))
        assert torch.equal(oa.grad_norm, oc.grad_norm) and bool(torch.isfinite(oa.grad_norm))
        if clip is not None:
            assert oa.clip_coef.item() < 1.0 and torch.equal(oa._norm_out, ob._norm_out)
        else:
            assert oa.clip_coef.item() == 1.0
        if k > 1:
            assert all(_all_plus_zero(oa._acc[p]) for p in a)
    assert int(oa.skipped_steps.item()) == 0 and int(oa.last_step_skipped.item()) == 0
    assert oa.skipped_steps.dtype == torch.int64 and oa.skipped_steps.dim() == 0 and oa.last_step_skipped.dtype == torch.int64
    assert all(int(oa.state[p]["step"]) == 3 for p in a)


# ---- 2. one poisoned step -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("position", list(POSITIONS))
@pytest.mark.parametrize("poison", list(POISONS))
def test_one_poisoned_element_skips_the_step(poison, position, k):
    """One clean step, then one whose gradients carry the poison (k = 3: in the second micro-batch), guarded and unguarded, with clipping
    and the weight average.

    The control: the same step unguarded destroys the model -- an infinity or a NaN leaves non-finite parameters (inf * 0 = NaN under the
    clip coefficient 0).  A finite 1e20 cannot do that to the unguarded launch: its norm overflows to +inf, the coefficient
    max_norm / (inf + 1e-6) is 0 and 1e20 * 0 = 0, so the unguarded step is a finite but wrong one (every gradient zeroed, the moments
    decayed, the weights moved by momentum and weight decay); for that value the control asserts the infinite norm, the zero coefficient
    and that the unguarded model did move, all of which the guarded step is spared."""
    many, ti, ei = POSITIONS[position]
    value = POISONS[poison]
    clip, ema = 3.0, 0.9
    init = _init(4, many)
    a, b = _params(init, many), _params(init, many)
    oa, ob = _opt(a, True, clip, ema, k), _opt(b, False, clip, ema, k)
    gen = torch.Generator().manual_seed(5)
    _one_step([(oa, a), (ob, b)], _micro_grads(a, gen, k, many))
    before = _state(a, oa, ema)
    _same(before, _state(b, ob, ema), "clean step")
    skipped0 = int(oa.skipped_steps.item())
    micro = _micro_grads(a, gen, k, many)
    micro[k // 2][ti].view(-1)[ei] = value
    _one_step([(oa, a), (ob, b)], micro)
    _same(_state(a, oa, ema), before, (poison, position, k))                       # p, m, v and the average: untouched
    assert int(oa.last_step_skipped.item()) == 1 and int(oa.skipped_steps.item()) == skipped0 + 1
    assert not bool(torch.isfinite(oa.grad_norm))
    if k > 1:
        assert all(_all_plus_zero(oa._acc[p]) for p in a)
    # the control
    if poison == "1e20":
        assert ob.grad_norm.item() == INF and ob.clip_coef.item() == 0.0
        assert all(not torch.equal(p.detach(), s[0]) for p, s in zip(b, before))
    else:
        assert not all(bool(torch.isfinite(p).all()) for p in b)
    # and the next clean step applies
    _one_step([(oa, a)], _micro_grads(a, gen, k, many))
    assert int(oa.last_step_skipped.item()) == 0 and int(oa.skipped_steps.item()) == skipped0 + 1
    assert all(bool(torch.isfinite(p).all()) and not torch.equal(p.detach(), s[0]) for p, s in zip(a, before))


# ---- 3. a skipped step is a batch never seen ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["by_value", "counter_k1", "counter_k3", "ema_warmup"])
def test_a_skipped_step_equals_never_having_seen_the_batch(case):
    """Guarded: g1, g2 (poisoned), g3, g4.  Unguarded twin: g1, g3, g4.  Bit-equal after every applied step -- for the last three cases
    only if bias correction and the average's warm-up use the number of applied updates (step + counter / k - skipped)."""
    k = 3 if case == "counter_k3" else 1
    many = case == "counter_k3"                     # 90 tensors: several AdamW launches, only the last advances the counter
    counter = case.startswith("counter")
    ema = None if case == "by_value" else 0.9
    init = _init(6, many)
    a, b = _params(init, many), _params(init, many)
    kw = dict(ema_warmup=True) if case == "ema_warmup" else {}
    oa, ob = _opt(a, True, None, ema, k, **kw), _opt(b, False, None, ema, k, **kw)
    ka = kb = None
    if counter:
        ka, kb = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
        oa.set_step_counter(ka, advance=True)
        ob.set_step_counter(kb, advance=True)
    gen = torch.Generator().manual_seed(7)
    g1, g2, g3, g4 = (_micro_grads(a, gen, k, many) for _ in range(4))
    g2[k // 2][len(a) // 2].view(-1)[0] = NAN        # (k = 3: micro-batch 1 of 0 .. 2)
    _one_step([(oa, a)], g1, [ka] if counter else [])
    _one_step([(ob, b)], g1, [kb] if counter else [])
    _same(_state(a, oa, ema), _state(b, ob, ema), (case, "g1"))
    _one_step([(oa, a)], g2, [ka] if counter else [])
    _same(_state(a, oa, ema), _state(b, ob, ema), (case, "g2 skipped"))
    assert int(oa.skipped_steps.item()) == 1
    for name, g in (("g3", g3), ("g4", g4)):
        _one_step([(oa, a)], g, [ka] if counter else [])
        _one_step([(ob, b)], g, [kb] if counter else [])
        _same(_state(a, oa, ema), _state(b, ob, ema), (case, name))
        assert int(oa.last_step_skipped.item()) == 0
    assert int(oa.skipped_steps.item()) == 1
    if counter:                                      # the skipped step advanced the counter like an applied one
        assert int(ka.item()) == 4 * k and int(kb.item()) == 3 * k and int(oa._ticket.item()) == 0
    else:
        assert all(int(oa.state[p]["step"]) == 4 for p in a)        # attempted steps, until folded
        assert oa.fold_skipped() == 1 and all(int(oa.state[p]["step"]) == 3 for p in a)


# ---- 4. several groups --------------------------------------------------------------------------------------------------------------------
def test_several_groups_skip_together_and_are_counted_once():
    init = _init(8)
    a, b = _params(init), _params(init)
    groups = lambda ps: [{"params": ps[:3]}, {"params": ps[3:], "lr": 3e-4}]
    oa, ob = _opt(groups(a), True, 3.0, 0.9), _opt(groups(b), False, 3.0, 0.9)
    gen = torch.Generator().manual_seed(9)
    _one_step([(oa, a), (ob, b)], _micro_grads(a, gen, 1, False))
    before = _state(a, oa, 0.9)
    micro = _micro_grads(a, gen, 1, False)
    micro[0][5].view(-1)[7] = NAN                    # in the second group
    _one_step([(oa, a), (ob, b)], micro)
    _same(_state(a, oa, 0.9), before, "both groups")
    assert int(oa.skipped_steps.item()) == 1 and int(oa.last_step_skipped.item()) == 1          # once, not once per group
    assert not any(bool(torch.isfinite(p).all()) for p in b)                                     # the control: the NaN coefficient reaches both groups
    _one_step([(oa, a)], _micro_grads(a, gen, 1, False))
    assert int(oa.skipped_steps.item()) == 1 and int(oa.last_step_skipped.item()) == 0
    assert all(bool(torch.isfinite(p).all()) and not torch.equal(p.detach(), s[0]) for p, s in zip(a, before))


# ---- 5. folding and state dicts -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["fold_skipped", "state_dict"])
def test_the_skipped_count_folds_into_step_and_through_a_state_dict(how):
    init = _init(10)
    a = _params(init)
    oa = _opt(a, True, 3.0, 0.9)
    gen = torch.Generator().manual_seed(11)
    steps = [_micro_grads(a, gen, 1, False) for _ in range(4)]
    steps[1][0][2].view(-1)[1] = -INF
    for g in steps[:3]:                              # applied, skipped, applied
        _one_step([(oa, a)], g)
    assert all(int(oa.state[p]["step"]) == 3 for p in a) and int(oa.skipped_steps.item()) == 1
    if how == "fold_skipped":
        assert oa.fold_skipped() == 1
        assert all(int(oa.state[p]["step"]) == 2 for p in a) and int(oa.skipped_steps.item()) == 0
        assert oa.fold_skipped() == 0
    sd = copy.deepcopy(oa.state_dict())              # (as a file would hold it: state_dict() returns the live tensors)
    assert all(int(s["step"]) == 2 for s in sd["state"].values()) and int(oa.skipped_steps.item()) == 0
    assert all(int(oa.state[p]["step"]) == 2 for p in a)
    b = _params([p.detach() for p in a])             # (the last one at a 4-byte offset again)
    ob = _opt(b, True, 3.0, 0.9)
    ob.load_state_dict(sd)
    assert all(int(ob.state[p]["step"]) == 2 for p in b)
    _one_step([(oa, a), (ob, b)], steps[3])          # stepping on == loading into a fresh guarded optimizer and stepping
    for pa, pb in zip(a, b):
        for key in ("exp_avg", "exp_avg_sq", "ema"):
            assert torch.equal(oa.state[pa][key], ob.state[pb][key]), key
        assert torch.equal(pa.detach(), pb.detach())
    assert int(ob.skipped_steps.item()) == 0 and all(int(ob.state[p]["step"]) == 3 for p in b)


# ---- 6. GraphedTrainStep ------------------------------------------------------------------------------------------------------------------
def _mix_batches(n):
    g = torch.Generator().manual_seed(13)
    out = []
    for _ in range(n):
        x = torch.rand(2, 2, 3, 32, 32, generator=g).cuda()
        y = P().MixTarget(torch.randint(0, 8, (2,), generator=g).cuda(), torch.randint(0, 8, (2,), generator=g).cuda(),
                          torch.rand(2, generator=g).cuda())
        out.append((x, y))
    return out


def _poisoned(batch):
    """The same clip and labels with a NaN mixing weight: read at replay time, and the forward pass never sees it."""
    x, y = batch
    lam = y.lam.clone()
    lam[1] = NAN
    return x, P().MixTarget(y.y_a, y.y_b, lam)


@pytest.mark.parametrize("k", [1, 2])
def test_graphed_step_replays_through_a_poisoned_batch(k):
    pkg = P()
    clip = 0.5 if k == 2 else None
    batches = _mix_batches(k)
    crit = pkg.HybridCrossEntropyLoss()

    def build(guard):
        m = _model()
        o = pkg.HybridAdamW(m.parameters(), lr=1e-3, max_grad_norm=clip, ema_decay=0.9, skip_nonfinite=guard)
        return m, o, pkg.GraphedTrainStep(m, crit, o, *batches[0], warmup=k, accumulation_steps=k)

    def optimizer_step(tr, first_poisoned):
        losses = []
        for j, b in enumerate(batches):
            tr.load(*(_poisoned(b) if first_poisoned and j == 0 else b))
            losses.append(tr.step())
        assert tr.is_update_step
        return losses

    # the control: the same replay unguarded ends with non-finite parameters
    mc, oc, trc = build(False)
    try:
        optimizer_step(trc, True)
        assert not all(bool(torch.isfinite(p).all()) for p in mc.parameters())
    finally:
        trc.close()

    m, o, tr = build(True)
    try:
        assert tr.steps_done() == 1 and int(tr.skipped_steps.item()) == 0             # the warm-up step applied
        params = list(m.parameters())
        before = _state(params, o, 0.9)
        micro0 = tr.micro_steps_done()
        losses = optimizer_step(tr, True)
        assert not bool(torch.isfinite(losses[0]))
        _same(_state(params, o, 0.9), before, "poisoned replay")
        assert int(tr.skipped_steps.item()) == 1 and int(o.last_step_skipped.item()) == 1
        assert not bool(torch.isfinite(tr.grad_norm))
        assert tr.micro_steps_done() == micro0 + k and tr.steps_done() == 2           # the counter advanced
        if k > 1:
            assert all(_all_plus_zero(o._acc[p]) for p in params)
        for s in range(2):                                                            # the clean replays train on
            prev = [p.detach().clone() for p in params]
            losses = optimizer_step(tr, False)
            assert all(bool(torch.isfinite(l)) for l in losses) and int(o.last_step_skipped.item()) == 0
            assert all(bool(torch.isfinite(p).all()) for p in params)
            assert any(not torch.equal(p.detach(), q) for p, q in zip(params, prev))
        assert int(tr.skipped_steps.item()) == 1 and tr.steps_done() == 4
        tr.sync_optimizer_state()
        assert all(int(o.state[p]["step"]) == 3 for p in params)                      # 1 warm-up + 2 clean; the skipped one is not counted
        assert tr.micro_steps_done() == 0 and int(tr.skipped_steps.item()) == 0
        o.set_skip_nonfinite(False)                                                   # a toggle after capture
        with pytest.raises(RuntimeError, match="skip_nonfinite was switched on or off after capture"):
            tr.step()
        o.set_skip_nonfinite(True)
        optimizer_step(tr, False)
        assert tr.steps_done() == 1
    finally:
        tr.close()


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------------
def test_a_missing_guard_block_is_refused_under_capture(monkeypatch):
    """(No real capture: only the decisions are under test.)"""
    from transformer_cnn_hybrid_network_for_video_processing_amd._lib import lib
    ps = [torch.nn.Parameter(torch.randn(5000, device="cuda"))]
    ps[0].grad = torch.randn(5000, device="cuda")
    opt = P().HybridAdamW(ps, lr=1e-3, max_grad_norm=1.0)
    opt.step()                                       # the hyper block and the norm workspace exist; the guard block does not
    opt.set_skip_nonfinite(True)
    calls = []
    orig = lib.call
    monkeypatch.setattr(lib, "call", lambda name, *a: (calls.append(name), orig(name, *a))[1])
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    for f in (opt.step, lambda: opt.skipped_steps, lambda: opt.last_step_skipped):
        with pytest.raises(RuntimeError, match="non-finite guard's device block does not exist yet"):
            f()
    assert calls == [] and opt._guard is None and int(opt.state[ps[0]]["step"]) == 1
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    assert int(opt.skipped_steps.item()) == 0        # created eagerly, zeroed
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    opt.step()
    assert calls == ["hyb_grad_norm_guard", "hyb_adamw_step_dev_guard"], calls
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert int(opt.state[ps[0]]["step"]) == 2 and int(opt.skipped_steps.item()) == 0
