"""Gradient accumulation in HybridAdamW and GraphedTrainStep: the accumulate launch against torch's own `acc += g`; the accumulated step
against the plain device step on a mean formed with torch ops, bit for bit (k a power of two or not, clipped or not, with the weight average,
through an advancing device counter that counts micro-steps); accumulation_steps == 1 is today's launch sequence; the refusals under
capture; GraphedTrainStep with k = 3 against the eager accumulate() / step() sequence; and a new dropout mask for every micro-batch."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4095, 4096, 4097, 3 * 4096 + 5]
SMALL = dict(cnn_channels=(32, 64), d_model=64, num_heads=4, num_layers=1, hidden_dim=128, dropout=0.0)      # tests/test_gpu_ema.py


def P():
    import transformer_cnn_hybrid_network_for_video_processing_amd as pkg
    return pkg


def _offset_copy(t):
    """The values of t in a contiguous view 4 bytes into a flat buffer: 16-byte accesses are impossible, the kernels take their scalar path."""
    base = torch.empty(t.numel() + 1, device="cuda")
    v = base[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _init(seed, many=False):
    g = torch.Generator().manual_seed(seed)
    if many:                                        # 90 tensors: more than any launch's table holds (80, 76, 64)
        return [torch.randn(5, generator=g).cuda() for _ in range(90)]
    return [torch.randn(n, generator=g).cuda() for n in SIZES] + [torch.randn(1025, generator=g).cuda()]


def _params(init, many=False):
    """Fresh parameters holding `init`: the sizes of SIZES, 16-byte aligned, and a last one (1025 elements) at a 4-byte offset."""
    if many:
        return [torch.nn.Parameter(t.clone()) for t in init]
    return [torch.nn.Parameter(t.clone()) for t in init[:-1]] + [torch.nn.Parameter(_offset_copy(init[-1]))]


def _new_grads(ps, g, many=False):
    """One gradient per parameter, 16-byte aligned except (the SIZES set) the last, which sits at a 4-byte offset like its parameter."""
    gs = [torch.randn(p.shape, generator=g).cuda() for p in ps]
    if not many:
        gs[-1] = _offset_copy(gs[-1])
    return gs


def _bind(ps, grads):
    for p, g in zip(ps, grads):
        p.grad = g


def _all_plus_zero(t):
    return not bool(t.view(torch.int32).any())       # every element's bits are those of +0.0f


@pytest.mark.parametrize("many", [False, True])
def test_accumulate_launch_equals_torch_add(many):
    ps = _params(_init(0, many), many)
    opt = P().HybridAdamW(ps, lr=1e-3, accumulation_steps=4)
    ref = [torch.zeros_like(p) for p in ps]
    g = torch.Generator().manual_seed(1)
    for j in range(1, 4):
        grads = _new_grads(ps, g, many)
        keep = [t.clone() for t in grads]
        _bind(ps, grads)
        opt.accumulate()
        for r, t in zip(ref, keep):
            r += t
        for i, (p, r, t, t0) in enumerate(zip(ps, ref, grads, keep)):
            acc = opt._acc[p]
            assert acc.dtype == torch.float32 and acc.data_ptr() % 16 == 0 and acc.shape == p.shape, (j, i)
            assert torch.equal(acc, r), (j, i)
            assert torch.equal(t, t0), (j, i)                     # g is only read
    assert all(not torch.equal(opt._acc[p], torch.zeros_like(p)) for p in ps)
    assert all("acc" not in st for st in opt.state.values()) and len(opt.state) == 0         # the accumulators are no state


def _compare(a, oa, b, ob, ema, tag):
    for i, (pa, pb) in enumerate(zip(a, b)):
        assert torch.equal(pa.data, pb.data), (tag, i)
        assert torch.equal(oa.state[pa]["exp_avg"], ob.state[pb]["exp_avg"]), (tag, i)
        assert torch.equal(oa.state[pa]["exp_avg_sq"], ob.state[pb]["exp_avg_sq"]), (tag, i)
        if ema is not None:
            assert torch.equal(oa.state[pa]["ema"], ob.state[pb]["ema"]), (tag, i)
        assert _all_plus_zero(oa._acc[pa]), (tag, i)


def _accumulated_against_plain(k, clip, ema, steps, many=False, counters=False):
    """`steps` optimizer steps of a: k micro-batches each, accumulate() k - 1 times, then step().  b: the plain device-path optimizer on
    G = (acc + g_k) * inv_k with acc = 0; acc += g_j, all torch ops on the device.  Everything is compared after every optimizer step."""
    init = _init(2, many)
    a, b = _params(init, many), _params(init, many)
    kw = dict(lr=1e-3, max_grad_norm=clip, ema_decay=ema, ema_warmup=counters)
    oa = P().HybridAdamW(a, accumulation_steps=k, **kw)
    ob = P().HybridAdamW(b, accumulation_steps=1, **kw)
    ob.set_dynamic_hyper(True)
    if counters:                                    # a's counter counts micro-steps, b's optimizer steps
        ka, kb = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
        oa.set_step_counter(ka, advance=True)
        ob.set_step_counter(kb, advance=True)
    inv_k = float(torch.tensor(1.0 / k, dtype=torch.float64).float())      # (float)(1.0 / (double)k)
    g = torch.Generator().manual_seed(3)
    for s in range(steps):
        acc = [torch.zeros_like(p) for p in b]
        for j in range(k):
            grads = _new_grads(a, g, many)
            _bind(a, grads)
            if j < k - 1:
                oa.accumulate()
                if counters:
                    ka.add_(1)                      # what ends a micro-step that is no update in GraphedTrainStep
                for r, t in zip(acc, grads):
                    r += t
            else:
                _bind(b, [(r + t) * inv_k for r, t in zip(acc, grads)])
                oa.step(); ob.step()
        if clip is not None:
            assert oa.clip_coef.item() < 1.0
            assert torch.equal(oa.clip_coef, ob.clip_coef) and torch.equal(oa.grad_norm, ob.grad_norm)
        _compare(a, oa, b, ob, ema, (k, clip, ema, s))
    if counters:
        assert int(ka.item()) == steps * k and int(kb.item()) == steps
        assert int(oa._ticket.item()) == 0
        assert all(int(oa.state[p]["step"]) == 0 for p in a)       # the device counter carries the step number


@pytest.mark.parametrize("ema", [None, 0.9])
@pytest.mark.parametrize("clip", [None, 3.0])
@pytest.mark.parametrize("k", [2, 3, 4])
def test_accumulated_step_equals_the_plain_step_on_a_torch_formed_mean(k, clip, ema):
    _accumulated_against_plain(k, clip, ema, steps=3)


@pytest.mark.parametrize("ema", [None, 0.9])
def test_step_number_is_the_micro_step_counter_divided_by_k(ema):
    """90 tensors (several launches, only the last advances), k = 3, an advancing device counter: after K optimizer steps it holds K * k, the
    bias corrections and the average's warm-up value used counter / k."""
    _accumulated_against_plain(3, None, ema, steps=4, many=True, counters=True)


def test_one_accumulation_step_is_todays_launch_sequence(monkeypatch):
    from transformer_cnn_hybrid_network_for_video_processing_amd._lib import lib
    calls = []
    orig = lib.call
    monkeypatch.setattr(lib, "call", lambda name, *a: (calls.append(name), orig(name, *a))[1])

    def two_steps(**kw):
        ps = [torch.nn.Parameter(torch.randn(5000, device="cuda"))]
        ps[0].grad = torch.randn(5000, device="cuda")
        opt = P().HybridAdamW(ps, lr=1e-3, **kw)
        del calls[:]
        opt.step()
        first = list(calls)
        del calls[:]
        opt.step()
        assert not opt._acc                          # nothing was created
        return first, list(calls)
    assert two_steps(accumulation_steps=1) == (["hyb_adamw_step"], ["hyb_adamw_step"])
    assert two_steps(accumulation_steps=1, max_grad_norm=1.0) == (["hyb_adamw_hyper_set", "hyb_grad_norm", "hyb_adamw_step_dev"],
                                                                  ["hyb_grad_norm", "hyb_adamw_step_dev"])
    assert two_steps(accumulation_steps=1, ema_decay=0.9) == (["hyb_adamw_hyper_set", "hyb_adamw_ema_set", "hyb_adamw_step_dev_ema"],
                                                              ["hyb_adamw_step_dev_ema"])
    assert two_steps() == (["hyb_adamw_step"], ["hyb_adamw_step"])
    monkeypatch.undo()
    torch.cuda.synchronize()


def test_missing_accumulators_are_refused_under_capture(monkeypatch):
    """(No real capture: only the decisions are under test.)"""
    from transformer_cnn_hybrid_network_for_video_processing_amd._lib import lib
    ps = [torch.nn.Parameter(torch.randn(5000, device="cuda"))]
    ps[0].grad = torch.randn(5000, device="cuda")
    opt = P().HybridAdamW(ps, lr=1e-3, accumulation_steps=2)
    calls = []
    orig = lib.call
    monkeypatch.setattr(lib, "call", lambda name, *a: (calls.append(name), orig(name, *a))[1])
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    for f in (opt.accumulate, opt.step, opt.accum_init):
        with pytest.raises(RuntimeError, match=r"accum_init\(\)"):
            f()
    assert calls == [] and not opt._acc and len(opt.state) == 0
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    opt.accum_init()
    assert _all_plus_zero(opt._acc[ps[0]])
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    opt.accumulate()
    assert calls == ["hyb_grad_accumulate"], calls
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert torch.equal(opt._acc[ps[0]], ps[0].grad)


# ---- the model ----------------------------------------------------------------------------------------------------------------------------
K = 3


def _model(seed=0, attention_dropout=False):
    torch.manual_seed(seed)
    m = P().TransformerCNNHybrid(compute_dtype="bf16", **SMALL).cuda().train()
    if not attention_dropout:
        for a in m.encoder.attention_layers:
            a.dropoutLayer.p = 0.0
    return m


def _batches(mix):
    """K distinct micro-batches."""
    g = torch.Generator().manual_seed(3)
    out = []
    for _ in range(K):
        x = torch.rand(2, 4, 3, 32, 32, generator=g).cuda()
        y = torch.randint(0, 8, (2,), generator=g).cuda()
        if mix:
            y = P().MixTarget(y, torch.randint(0, 8, (2,), generator=g).cuda(), torch.rand(2, generator=g).cuda())
        out.append((x, y))
    return out


@pytest.mark.parametrize("variant", ["plain", "clip_lr", "mix"])
def test_graph_equals_eager_with_accumulation(variant):
    """GraphedTrainStep(accumulation_steps=3, warmup=3) against the eager sequence zero_grad / backward / accumulate() ... step(), from the
    same weights on the same micro-batches: one warm-up optimizer step on the construction batch, then two through load() + step()."""
    _graph_against_eager(variant, single=True)


def test_three_graph_form_on_one_rank_accumulates_too(monkeypatch):
    """HYB_GRAPH_SINGLE=0 (the A/B switch): graphs A and B, then either graph C or the captured accumulate launch + counter += 1."""
    monkeypatch.setenv("HYB_GRAPH_SINGLE", "0")
    _graph_against_eager("clip_lr", single=False)


def _graph_against_eager(variant, single):
    pkg = P()
    clip = variant == "clip_lr"
    batches = _batches(variant == "mix")
    crit = pkg.HybridCrossEntropyLoss()
    kw = dict(lr=1e-3, max_grad_norm=0.5 if clip else None)
    with pytest.raises(ValueError, match="multiple of accumulation_steps"):
        m0 = _model()
        pkg.GraphedTrainStep(m0, crit, pkg.HybridAdamW(m0.parameters(), **kw), *batches[0], warmup=4, accumulation_steps=K)

    # the eager run first (as the other graph tests do): a snapshot after each of its three optimizer steps
    m1 = _model()
    o1 = pkg.HybridAdamW(m1.parameters(), accumulation_steps=K, **kw)
    eager_losses, snaps = [], []
    for s, data in enumerate([[batches[0]] * K, batches, batches]):          # the warm-up step, then the two that are compared
        if clip and s == 2:                                               # a schedule moves lr between optimizer steps
            o1.param_groups[0]["lr"] = 4e-4
        for j, (x, y) in enumerate(data):
            o1.zero_grad(set_to_none=True)
            loss = crit(m1(x), y)
            loss.backward()
            eager_losses.append(loss.item())
            if j < K - 1:
                o1.accumulate()
            else:
                o1.step()
        snaps.append(({n: t.detach().clone() for n, t in list(m1.named_parameters()) + list(m1.named_buffers())},
                      (o1.clip_coef.clone(), o1.grad_norm.clone()) if clip else None))

    m2 = _model()
    o2 = pkg.HybridAdamW(m2.parameters(), **kw)
    tr = pkg.GraphedTrainStep(m2, crit, o2, *batches[0], warmup=K, dynamic_hyper=clip, accumulation_steps=K)
    try:
        assert (tr.gs is not None) == single and tr.gm is not None and o2.accumulation_steps == K and tr.is_update_step
        assert tr.micro_steps_done() == K and tr.steps_done() == 1
        graph_losses = []
        for s in (1, 2):
            if clip and s == 2:
                o2.param_groups[0]["lr"] = 4e-4
            for j, (x, y) in enumerate(batches):
                tr.load(x, y)
                graph_losses.append(tr.step().item())
                assert tr.is_update_step == (j == K - 1)
            want, norms = snaps[s]
            if clip:
                assert o2.clip_coef.item() < 1.0 and torch.equal(norms[0], o2.clip_coef) and torch.equal(norms[1], tr.grad_norm)
            for n, t in list(m2.named_parameters()) + list(m2.named_buffers()):
                assert torch.equal(t, want[n]), (s, n)
        assert graph_losses == eager_losses[K:], (graph_losses, eager_losses)
        assert len(set(graph_losses[:K])) == K                            # the micro-batches are distinct
        assert tr.micro_steps_done() == 3 * K and tr.steps_done() == tr.micro_steps_done() // K == 3
        assert all(_all_plus_zero(o2._acc[p]) for p in m2.parameters())
        for pa, pb in zip(m1.parameters(), m2.parameters()):
            assert torch.equal(o1.state[pa]["exp_avg"], o2.state[pb]["exp_avg"])
        tr.step()                                                         # one further micro-step: in the middle of an optimizer step
        assert not tr.is_update_step and tr.micro_steps_done() == 3 * K + 1 and tr.steps_done() == 3
        with pytest.raises(RuntimeError, match="middle of an accumulated step"):
            tr.sync_optimizer_state()
        with pytest.raises(RuntimeError, match="middle of an accumulated step"):
            tr.fwd_bwd()
        o2.set_accumulation(2)
        with pytest.raises(RuntimeError, match="accumulation_steps changed after capture"):
            tr.step()
        o2.set_accumulation(K)
        tr.step(); tr.step()
        assert tr.is_update_step
        tr.sync_optimizer_state()
        assert tr.micro_steps_done() == 0 and all(int(o2.state[p]["step"]) == 4 for p in m2.parameters())
    finally:
        tr.close()


@pytest.mark.parametrize("attention_dropout", [True, False])
def test_every_micro_batch_draws_its_own_masks(attention_dropout):
    """The same (x, y) for every micro-batch of one optimizer step: the weights do not change between them and train-mode BatchNorm uses batch
    statistics, so without dropout the logits are equal (the control) and with the attention dropout they differ only through the masks."""
    pkg = P()
    m = _model(attention_dropout=attention_dropout)
    (x, y), = _batches(False)[:1]
    tr = pkg.GraphedTrainStep(m, pkg.HybridCrossEntropyLoss(), pkg.HybridAdamW(m.parameters(), lr=1e-3), x, y, warmup=K, accumulation_steps=K)
    try:
        logits = []
        for j in range(K):
            tr.step()
            logits.append(tr.logits.clone())
        assert tr.is_update_step
        for i in range(K):
            for j in range(i + 1, K):
                assert torch.equal(logits[i], logits[j]) == (not attention_dropout), (i, j)
    finally:
        tr.close()
