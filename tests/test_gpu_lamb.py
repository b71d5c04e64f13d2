"""HybridLAMB on the device: against the fp64 rule of tests/lamb_ref.py, its bit identities (AdamW where every ratio is 1, merged groups
against per-group launches, run to run), tables of more than one slice, the non-finite guard, the accumulator-only gradient mode through the
C ABI, and GraphedTrainStep replaying it with layer-wise groups under a scheduler.

Tensors, groups and hyper-parameters are those of tests/test_gpu_param_groups.py: sizes 1, 3, 4, 4095, 4096, 4097, 2 * 4096 + 5 and a
1025-element view at a 4-byte offset, in three groups with grossly different hyper-parameters of which the first has weight_decay = 0 -- so
both branches of the trust rule occur (r = 1 there unless always_adapt).

Gate against fp64 (test_against_fp64, test_tables_of_more_than_one_slice): per tensor and per quantity x in (p, exp_avg, exp_avg_sq), after
`steps` steps, max|x - x64| <= 4 max|x32 - x64| + steps 2^-23 max|x64|, x32 the same rule in torch float32 on the CPU (the error yardstick);
the ratios and both norms within 1e-5 relative of fp64's."""
import ctypes
import functools

import pytest
import torch

from lamb_ref import LambRef
from test_gpu_clip_lr import _sched_step, _setup, _warmup_lambda
from test_gpu_param_groups import HYPER, LAYOUT, VARIANTS, Recorder, _assert_same, _bind, _grads, _groups, _init, _params, _state

pytestmark = pytest.mark.gpu
STEPS = 5
LAMB_CALLS = ("hyb_lamb_trust", "hyb_lamb_step_dev")


def P():
    import transformer_cnn_hybrid_network_for_video_processing_amd as pkg
    return pkg


def _lamb(ps, merge=True, layout=LAYOUT, no_decay=False, **kw):
    groups = _groups(ps, layout)
    if no_decay:
        for g in groups:
            g["weight_decay"] = 0.0
    return P().HybridLAMB(groups, merge_groups=merge, **kw)


def _trust(opt, ps):
    t = opt.trust_ratios()
    return torch.stack([t[p] for p in ps]).cpu()


def _gate(name, i, steps, got, ref32, ref64):
    """the file's gate; prints each figure before it asserts"""
    err, yard, big = (got.double().cpu().flatten() - ref64.flatten()).abs().max().item(), (ref32.double().flatten() - ref64.flatten()).abs().max().item(), ref64.abs().max().item()
    bound = 4 * yard + steps * 2.0 ** -23 * big
    print(f"{name} tensor {i} ({ref64.numel()} elements) after {steps} steps: error {err:.3e}, fp32 restatement {yard:.3e}, gate {bound:.3e}, ratio {err / bound:.3f}")
    assert err <= bound, (name, i, steps, err, bound)


def _check_trust(got, ref, tag):
    """got: [n, 3] fp32 from the device; ref: the reference's (|p|, |u|, r) tuples"""
    want = torch.tensor(ref, dtype=torch.float64)
    rel = ((got.double() - want).abs() / want.abs().clamp_min(1e-300))
    rel[want == 0] = (got.double() - want).abs()[want == 0]                # a zero norm must come out as zero
    print(f"{tag}: worst relative error of (|p|, |u|, r) {rel.max(dim=0).values.tolist()}")
    assert rel.max().item() <= 1e-5, (tag, rel.max(dim=0))


# ---- 1. against fp64 ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _references(always_adapt):
    """The fp64 and fp32 runs of the five steps, computed once: per step (p, m, v per tensor in both precisions, the fp64 trust tuples)."""
    init = _init(11)
    views = init[:-1] + [init[-1][1:1026]]
    gen = torch.Generator().manual_seed(12)
    grads = [[torch.randn(t.shape, generator=gen) for t in views] for _ in range(STEPS)]
    refs = {dt: LambRef(_groups(views), dt, always_adapt=always_adapt, max_grad_norm=1.0) for dt in (torch.float64, torch.float32)}
    out = []
    for gs in grads:
        for r in refs.values():
            r.step(gs)
        snap = {dt: [[x.clone() for x in col] for col in (r.params, r.exp_avg, r.exp_avg_sq)] for dt, r in refs.items()}
        out.append((snap, list(refs[torch.float64].trust)))
    return init, grads, out


@pytest.mark.parametrize("always_adapt", [False, True])
def test_against_fp64(always_adapt):
    init, grads, ref = _references(always_adapt)
    ps = _params(init)
    opt = _lamb(ps, always_adapt=always_adapt, max_grad_norm=1.0)
    for s in range(STEPS):
        _bind(ps, [g.cuda() for g in grads[s]])
        opt.step()
        snap, trust64 = ref[s]
        assert opt.clip_coef.item() < 1.0                                 # clipping was active
        for i, p in enumerate(ps):
            st = opt.state[p]
            for j, (name, x) in enumerate((("p", p.detach()), ("exp_avg", st["exp_avg"]), ("exp_avg_sq", st["exp_avg_sq"]))):
                _gate(name, i, s + 1, x, snap[torch.float32][j][i], snap[torch.float64][j][i])
        _check_trust(_trust(opt, ps), trust64, f"always_adapt={always_adapt}, step {s + 1}")
    r = _trust(opt, ps)[:, 2]
    if always_adapt:
        assert all(x != 1.0 for x in r.tolist())
    else:                                                                 # the first group has weight_decay = 0: not adapted, exactly
        assert all(x == 1.0 for x in r[:LAYOUT[0]].tolist()) and all(x != 1.0 for x in r[LAYOUT[0]:].tolist())


# ---- 2. bit identities ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_no_decay_lamb_is_adamw_on_the_device_path_bit_for_bit(variant):
    """All groups weight_decay = 0, always_adapt = False: every ratio is exactly 1 and the step is HybridAdamW's, in every variant."""
    kw = dict(VARIANTS[variant])
    k = kw.get("accumulation_steps", 1)
    kw.setdefault("max_grad_norm", None)
    init = _init(13)
    a, b = _params(init), _params(init)
    groups = _groups(b)
    for g in groups:
        g["weight_decay"] = 0.0
    oa = _lamb(a, no_decay=True, **kw)
    ob = P().HybridAdamW(groups, **kw)
    ob.set_dynamic_hyper(True)
    gen = torch.Generator().manual_seed(14)
    for s in range(STEPS):
        for j in range(k):
            gs = _grads(a, gen)
            _bind(a, gs); _bind(b, gs)
            if j < k - 1:
                oa.accumulate(); ob.accumulate()
            else:
                oa.step(); ob.step()
        _assert_same(_state(a, oa), _state(b, ob), (variant, "step", s))
        assert bool((_trust(oa, a)[:, 2] == 1.0).all())
    if "ema_decay" in kw:
        assert all("ema" in oa.state[p] for p in a)
    if kw["max_grad_norm"] is not None:
        assert torch.equal(oa._norm_out, ob._norm_out) and oa.clip_coef.item() < 1.0


def test_merged_equals_per_group_and_runs_repeat_bit_for_bit(monkeypatch):
    init = _init(15)
    runs = []
    for merge in (True, False, True):
        ps = _params(init)
        opt = _lamb(ps, merge, ema_decay=0.9, always_adapt=True)
        rec = Recorder(monkeypatch)
        gen = torch.Generator().manual_seed(16)
        trusts = []
        for s in range(STEPS):
            _bind(ps, _grads(ps, gen))
            opt.step()
            trusts.append(_trust(opt, ps))
        names = rec.take()
        monkeypatch.undo()
        units = 1 if merge else len(LAYOUT)
        assert [names.count(n) for n in LAMB_CALLS] == [STEPS * units] * 2 and names.count("hyb_grad_norm") == STEPS, names
        assert not any(n.startswith("hyb_adamw_step") for n in names), names
        runs.append((_state(ps, opt), trusts))
    for other, tag in ((1, "merged against per group"), (2, "merged, run to run")):
        _assert_same(runs[0][0], runs[other][0], tag)
        assert all(torch.equal(x, y) for x, y in zip(runs[0][1], runs[other][1])), tag
    assert not bool((runs[0][1][-1][:, 2] == 1.0).any())


def test_a_tensor_of_zeros_has_ratio_one():
    init = _init(17)
    init[5].zero_()                                                       # the second group's first tensor: weight_decay = 0.5
    ps = _params(init)
    opt = _lamb(ps, always_adapt=True)
    _bind(ps, _grads(ps, torch.Generator().manual_seed(18)))
    opt.step()
    t = _trust(opt, ps)
    assert t[5].tolist()[0] == 0.0 and t[5].tolist()[1] > 0.0 and t[5].tolist()[2] == 1.0
    assert all(x != 1.0 for i, x in enumerate(t[:, 2].tolist()) if i != 5)
    assert bool(ps[5].detach().abs().max() > 0)                           # it was stepped, at the plain rate


# ---- 3. more than one slice ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count,ema", [(83, None), (67, 0.9)], ids=["83 tensors", "67 tensors with the average"])
def test_tables_of_more_than_one_slice(count, ema, monkeypatch):
    """Five-element tensors, one of 4097 at index 80 (64 with the average: the first tensor of the second slice), and tensor 81 (65) with 100 x
    its neighbours' norm.  Without clipping a tensor's step depends on no other tensor, so the long table must give, bit for bit, what two
    optimizers over its halves give; and every ratio must be the tensor's own by the fp64 rule."""
    cap = 80 if ema is None else 64
    sizes = [5] * count
    sizes[cap] = 4097
    g = torch.Generator().manual_seed(count)
    init = [torch.randn(n, generator=g) for n in sizes]
    init[cap + 1] *= 100.0
    hyper = [dict(lr=1e-2, weight_decay=1e-2, eps=1e-6, betas=(0.9, 0.999)), dict(lr=3e-3, weight_decay=0.1, eps=1e-6, betas=(0.8, 0.95))]
    h = count // 2                                                        # two groups, the table's halves: the table's order is the list's
    groups = lambda ps: [dict(params=ps[:h], **hyper[0]), dict(params=ps[h:], **hyper[1])]            # noqa: E731
    a = [torch.nn.Parameter(t.clone().cuda()) for t in init]
    oa = P().HybridLAMB(groups(a), max_grad_norm=None, ema_decay=ema)
    assert oa.merges_groups()
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    oa.set_step_counter(counter, advance=True)
    b = [torch.nn.Parameter(t.clone().cuda()) for t in init]
    obs = [P().HybridLAMB([gr], max_grad_norm=None, ema_decay=ema) for gr in groups(b)]               # each a single slice, ungrouped calls
    refs = {dt: LambRef(groups(init), dt) for dt in (torch.float64, torch.float32)}
    rec = Recorder(monkeypatch)
    for s in range(2):
        gs = [torch.randn(n, generator=g) for n in sizes]
        _bind(a, [x.cuda() for x in gs]); _bind(b, [x.cuda() for x in gs])
        oa.step()
        for ob in obs:
            ob.step()
        for r in refs.values():
            r.step(gs)
        assert int(counter.item()) == s + 1 and int(oa._ticket.item()) == 0
        ta, tb = oa.trust_ratios(), {k: v for ob in obs for k, v in ob.trust_ratios().items()}
        for i in range(count):
            assert torch.equal(a[i], b[i]) and torch.equal(ta[a[i]], tb[b[i]]), (s, i)
            if ema is not None:
                assert torch.equal(oa.state[a[i]]["ema"], obs[0 if i < h else 1].state[b[i]]["ema"]), (s, i)
        for i in (0, cap - 1, cap, cap + 1, count - 1):
            st = oa.state[a[i]]
            for j, (name, x) in enumerate((("p", a[i].detach()), ("exp_avg", st["exp_avg"]), ("exp_avg_sq", st["exp_avg_sq"]))):
                r32, r64 = ((r.params, r.exp_avg, r.exp_avg_sq)[j][i] for r in (refs[torch.float32], refs[torch.float64]))
                _gate(name, i, s + 1, x, r32, r64)
        _check_trust(torch.stack([ta[p] for p in a]).cpu(), refs[torch.float64].trust, f"{count} tensors, step {s + 1}")
    names = rec.take()
    assert [names.count(n) for n in LAMB_CALLS] == [2 * 3] * 2, names     # one pair per optimizer and step, whatever the number of slices
    w = oa.trust_ratios()
    big, near = w[a[cap + 1]][0].item(), [w[a[i]][0].item() for i in (cap - 1, cap + 2)]
    assert big > 10 * max(near), (big, near)                              # the row of the tensor behind the slice boundary holds its own norm


# ---- 4. the guard -----------------------------------------------------------------------------------------------------------------------------------
def test_a_skipped_step_changes_nothing_and_the_run_continues_as_if_never_seen():
    init = _init(19)
    kw = dict(skip_nonfinite=True, ema_decay=0.9, accumulation_steps=2)
    a, b = _params(init), _params(init)
    oa, ob = _lamb(a, **kw), _lamb(b, **kw)
    gen = torch.Generator().manual_seed(20)
    batches = [[_grads(a, gen) for _ in range(2)] for _ in range(3)]      # three optimizer steps of two micro-batches
    poisoned = [_grads(a, gen), _grads(a, gen, poison=True)]

    def run(opt, ps, micro):
        _bind(ps, micro[0]); opt.accumulate()
        _bind(ps, micro[1]); opt.step()
    run(oa, a, batches[0]); run(ob, b, batches[0])
    before = _state(a, oa)
    run(oa, a, poisoned)
    assert int(oa.last_step_skipped.item()) == 1 and int(oa.skipped_steps.item()) == 1
    _assert_same(before, _state(a, oa), "the skipped step")               # p, exp_avg, exp_avg_sq, ema as they were; the accumulators zero again
    assert all(not bool(oa._acc[p].view(torch.int32).any()) for p in a)
    for s in (1, 2):
        run(oa, a, batches[s]); run(ob, b, batches[s])
        _assert_same(_state(a, oa), _state(b, ob), ("after the skipped step", s))
        assert torch.equal(_trust(oa, a), _trust(ob, b))
    assert int(oa.skipped_steps.item()) == 1 and int(ob.skipped_steps.item()) == 0
    assert torch.isfinite(torch.cat([p.detach().flatten() for p in a])).all()


# ---- 5. the accumulators as the only gradient, through the C ABI -----------------------------------------------------------------------------------------
def test_grad_acc_through_the_abi_equals_the_plain_calls():
    """grads = NULL, acc = 2 G, k = 2: the effective gradient acc * 0.5 is G exactly, so both calls must give the plain calls' bits."""
    from transformer_cnn_hybrid_network_for_video_processing_amd._lib import lib
    init = _init(21)
    gen = torch.Generator().manual_seed(22)
    stream = torch.cuda.current_stream().cuda_stream
    hyper = torch.zeros(6, dtype=torch.float64, device="cuda")
    lib.call("hyb_adamw_hyper_set", hyper, 1e-1, 0.8, 0.95, 1e-6, 0.5, 0.0, stream)
    results = []
    for mode in ("plain", "acc"):
        ps = [p.detach() for p in _params(init)]
        ms, vs = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
        n = len(ps)
        numel = (ctypes.c_longlong * n)(*[p.numel() for p in ps])
        partials = torch.zeros(lib.query("hyb_lamb_trust_workspace", n, numel), device="cuda")
        trust = torch.zeros(n, 3, device="cuda")
        g2 = torch.Generator().manual_seed(23)
        for step in (1, 2):
            gs = [torch.randn(p.shape, generator=g2).cuda() for p in ps]
            accs = [2.0 * g for g in gs] if mode == "acc" else None
            grads, k = (None, 2) if mode == "acc" else (gs, 1)
            lib.call("hyb_lamb_trust", n, ps, grads, ms, vs, accs, numel, None, 0, hyper, k, step, None, None, None, 0, partials, trust, stream)
            lib.call("hyb_lamb_step_dev", n, ps, grads, ms, vs, accs, None, numel, None, 0, hyper, None, k, step, None, None, None, None, trust, stream)
            torch.cuda.synchronize()
            if accs is not None:
                assert all(not bool(a.view(torch.int32).any()) for a in accs)     # left zeroed
        results.append(([p.clone() for p in ps], ms, vs, trust.clone()))
    for x, y in zip(results[0][:3], results[1][:3]):
        assert all(torch.equal(s, t) for s, t in zip(x, y))
    assert torch.equal(results[0][3], results[1][3]) and not bool((results[0][3][:, 2] == 1.0).any())
    assert all(not torch.equal(p, t.cuda().view_as(p)) for p, t in zip(results[0][0][:-1], init[:-1]))          # and the steps were taken


# ---- 6. under replay ------------------------------------------------------------------------------------------------------------------------------------
def test_replay_with_layerwise_groups_equals_eager_steps(monkeypatch):
    WARM, K = 2, 4
    crit = P().HybridCrossEntropyLoss()
    m1, x, y = _setup()
    m2, _, _ = _setup()
    o1 = P().HybridLAMB(m1.param_groups(lr=1e-3, layer_decay=0.75))
    o2 = P().HybridLAMB(m2.param_groups(lr=1e-3, layer_decay=0.75))
    assert len(o1.param_groups) == 12 and o1.merges_groups()
    s1 = torch.optim.lr_scheduler.LambdaLR(o1, _warmup_lambda)
    s2 = torch.optim.lr_scheduler.LambdaLR(o2, _warmup_lambda)
    rec = Recorder(monkeypatch)
    eager_losses, rates = [], []
    for k in range(WARM + K):
        o1.zero_grad(set_to_none=True)
        loss = crit(m1(x), y)
        loss.backward()
        rec.take()
        o1.step()
        names = [n for n in rec.take() if not n.startswith("hyb_adamw_hyper_set")]
        assert names == ["hyb_grad_norm", "hyb_lamb_trust", "hyb_lamb_step_dev"], names
        eager_losses.append(loss.item())
        rates.append([g["lr"] for g in o1.param_groups])
        if k >= WARM:
            s1.step()
    assert all(len({r[i] for r in rates[WARM:]}) == K for i in range(12))      # every group's rate moved on every compared step
    rec.take()
    tr = P().GraphedTrainStep(m2, crit, o2, x, y, warmup=WARM, dynamic_hyper=True)
    try:
        names = rec.take()                                               # WARM eager steps and the capture
        assert [names.count(n) for n in ("hyb_grad_norm",) + LAMB_CALLS] == [WARM + 1] * 3, names
        assert not any(n.startswith("hyb_adamw_step") for n in names) and tr._advancing
        graph_losses = []
        for _ in range(K):
            graph_losses.append(tr.step().item())
            _sched_step(s2)
        assert not any(n in LAMB_CALLS for n in rec.take())              # replays make no library call for the step
        assert graph_losses == eager_losses[WARM:], (graph_losses, eager_losses)
        assert int(tr.counter.item()) == WARM + K
        for (n, pa), (_, pb) in zip(m1.named_parameters(), m2.named_parameters()):
            assert torch.equal(pa, pb), n
        t1, t2 = o1.trust_ratios(), o2.trust_ratios()
        for pa, pb in zip(m1.parameters(), m2.parameters()):
            assert torch.equal(t1[pa], t2[pb])
        # weight_decay is read on the device: a decaying group set to 0 between replays is not adapted by the next one
        gi = next(i for i, g in enumerate(o2.param_groups) if g["weight_decay"] != 0 and all(t2[p][2].item() != 1.0 for p in g["params"]))
        o2.param_groups[gi]["weight_decay"] = 0.0
        tr.step()
        t2 = o2.trust_ratios()
        assert all(t2[p][2].item() == 1.0 for p in o2.param_groups[gi]["params"])
        others = [t2[p][2].item() for i, g in enumerate(o2.param_groups) if i != gi and g["weight_decay"] != 0 for p in g["params"]]
        assert others and all(r != 1.0 for r in others)
        assert int(tr.counter.item()) == WARM + K + 1
    finally:
        tr.close()
