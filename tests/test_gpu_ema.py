"""The weight average HybridAdamW keeps inside the AdamW launch (hyb_adamw_step_dev_ema): the optimizer itself is untouched bit for bit, the
average follows an fp64 evaluation of the same recurrence, a decay of 0 copies the weights, the first use starts from the weights before the
step, more tensors than one launch's table holds, GraphedTrainStep == eager with a decay changed between replays, the refusals under
capture, the twin module for predict / GraphedPredict, and a checkpoint round trip."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4095, 4096, 4097, 3 * 4096 + 5]
U = 2.0 ** -24                                      # one fp32 rounding, relative
SMALL = dict(cnn_channels=(32, 64), d_model=64, num_heads=4, num_layers=1, hidden_dim=128, dropout=0.0)      # tests/test_gpu_optim.py


def P():
    import transformer_cnn_hybrid_network_for_video_processing_amd as pkg
    return pkg


def _offset_copy(t):
    """The values of t in a contiguous view 4 bytes into a flat buffer: 16-byte loads are impossible, the kernel takes its scalar path."""
    base = torch.empty(t.numel() + 1, device="cuda")
    v = base[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _init(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g).cuda() for n in SIZES] + [torch.randn(1025, generator=g)]


def _params(init):
    """Fresh parameters holding `init`: the sizes of SIZES, 16-byte aligned, and a last one (1025 elements) at a 4-byte offset."""
    return [torch.nn.Parameter(t.clone()) for t in init[:-1]] + [torch.nn.Parameter(_offset_copy(init[-1].cuda()))]


def _set_grads(lists, g, scale=1.0):
    for group in zip(*lists):
        gr = torch.randn(group[0].shape, generator=g).cuda() * scale
        for p in group:
            p.grad = gr.clone()


def _d_pair(decay, warmup, t):
    """(d32, omd32) as doubles, formed as the kernel forms them at step t (1-based): d in double, then d and 1 - d rounded to fp32 once each."""
    n = t - 1
    d = min(decay, (1 + n) / (10 + n)) if warmup else decay
    return (torch.tensor(d, dtype=torch.float64).float().double().item(), torch.tensor(1.0 - d, dtype=torch.float64).float().double().item())


def _track(opt, ps, k, decay, warmup, g, scale=1.0, first_step=1):
    """k steps; the average of every parameter against e <- d32 * e + omd32 * p in float64 on the DEVICE's parameter trajectory, starting from
    the parameters before the first step.  -> per parameter (worst |e_dev - e_ref|, M = largest |p| or |e| seen)."""
    ref = [p.detach().double().cpu() for p in ps]
    big = [r.abs().max().item() for r in ref]
    worst = [0.0] * len(ps)
    for s in range(k):
        _set_grads([ps], g, scale)
        opt.step()
        d32, omd32 = _d_pair(decay, warmup, first_step + s)
        for i, p in enumerate(ps):
            pn = p.detach().double().cpu()
            ref[i] = d32 * ref[i] + omd32 * pn
            e = opt.state[p]["ema"].double().cpu()
            big[i] = max(big[i], pn.abs().max().item(), ref[i].abs().max().item(), e.abs().max().item())
            worst[i] = max(worst[i], (e - ref[i]).abs().max().item())
    return worst, big


@pytest.mark.parametrize("clip", [None, 3.0])
def test_the_optimizer_is_untouched_by_the_average(clip):
    init = _init(0)
    a, b = _params(init), _params(init)
    oa = P().HybridAdamW(a, lr=1e-3, max_grad_norm=clip, ema_decay=0.9)
    ob = P().HybridAdamW(b, lr=1e-3, max_grad_norm=clip)
    ob.set_dynamic_hyper(True)
    g = torch.Generator().manual_seed(1)
    for _ in range(5):
        _set_grads([a, b], g)
        oa.step(); ob.step()
        if clip is not None:
            assert oa.clip_coef.item() < 1.0 and torch.equal(oa.clip_coef, ob.clip_coef)
        for pa, pb in zip(a, b):
            assert torch.equal(pa.data, pb.data)
            assert torch.equal(oa.state[pa]["exp_avg"], ob.state[pb]["exp_avg"]) and torch.equal(oa.state[pa]["exp_avg_sq"], ob.state[pb]["exp_avg_sq"])
            assert "ema" in oa.state[pa] and "ema" not in ob.state[pb]


@pytest.mark.parametrize("decay,warmup", [(0.9, False), (0.999, True)])
def test_average_against_fp64(decay, warmup):
    """Gate, elementwise: |e_dev - e_ref| <= 3 k 2^-24 M, M the largest |p| or |e| of that tensor on the trajectory.  Each step makes two
    roundings (the product omd32 * p, the fused multiply-add), each at most 2^-24 relative on quantities bounded by M; the error carried from
    earlier steps is multiplied by d <= 1: 2k, and a third unit for second-order terms.  With warmup and k = 6 every step is in the warm-up
    branch: d = 0.1, 2/11, ..., 6/15."""
    K = 6
    if warmup:
        assert all((1 + n) / (10 + n) < decay for n in range(K))
    ps = _params(_init(2))
    opt = P().HybridAdamW(ps, lr=1e-2, ema_decay=decay, ema_warmup=warmup)
    worst, big = _track(opt, ps, K, decay, warmup, torch.Generator().manual_seed(3))
    for i, (w, m) in enumerate(zip(worst, big)):
        print(f"decay {decay} warmup {warmup} tensor {i} ({ps[i].numel()} elements): worst error {w:.3e}, gate {3 * K * U * m:.3e} (M {m:.4g})")
    for w, m in zip(worst, big):
        assert w <= 3 * K * U * m, (w, m)
    # the average did move away from both the start and the weights
    assert all(not torch.equal(opt.state[p]["ema"], p.data) for p in ps)


def test_decay_zero_copies_the_weights():
    ps = _params(_init(4))
    opt = P().HybridAdamW(ps, lr=1e-2, ema_decay=0.0)
    g = torch.Generator().manual_seed(5)
    for _ in range(3):
        _set_grads([ps], g)
        before = [p.detach().clone() for p in ps]
        opt.step()
        for p, old in zip(ps, before):
            assert torch.equal(opt.state[p]["ema"], p.data) and not torch.equal(p.data, old)


def test_first_use_starts_from_the_weights_before_the_step():
    """One step with decay d: e = d32 * p_old + omd32 * p_new within 2 * 2^-24 * M (two roundings) -- the clone was taken BEFORE the step;
    ema_init() and then the step gives the same bits."""
    d = 0.75
    init = _init(6)
    a, b = _params(init), _params(init)
    oa, ob = P().HybridAdamW(a, lr=1e-1, ema_decay=d), P().HybridAdamW(b, lr=1e-1, ema_decay=d)
    ob.ema_init()
    for p, t in zip(b, init):
        assert torch.equal(ob.state[p]["ema"], t.cuda()) and ob.state[p]["ema"].data_ptr() != p.data_ptr()
    old = [p.detach().double().cpu() for p in a]
    _set_grads([a, b], torch.Generator().manual_seed(7))
    oa.step(); ob.step()
    d32, omd32 = _d_pair(d, False, 1)
    for pa, pb, po in zip(a, b, old):
        pn = pa.detach().double().cpu()
        want = d32 * po + omd32 * pn
        e = oa.state[pa]["ema"].double().cpu()
        m = max(po.abs().max().item(), pn.abs().max().item(), e.abs().max().item())
        assert (pn - po).abs().max().item() > 0.05                    # lr 0.1: the step is large against the gate, old and new are told apart
        assert (e - want).abs().max().item() <= 2 * U * m
        assert torch.equal(oa.state[pa]["ema"], ob.state[pb]["ema"]) and torch.equal(pa.data, pb.data)


def test_more_tensors_than_one_launch_holds():
    """70 parameters: two launches with the average (64 per launch), one without (80); only the last launch advances the counter."""
    K = 3
    g0 = torch.Generator().manual_seed(8)
    init = [torch.randn(5, generator=g0).cuda() for _ in range(70)]
    a = [torch.nn.Parameter(t.clone()) for t in init]
    b = [torch.nn.Parameter(t.clone()) for t in init]
    oa = P().HybridAdamW(a, lr=1e-2, ema_decay=0.9)
    ob = P().HybridAdamW(b, lr=1e-2)
    ob.set_dynamic_hyper(True)
    ka, kb = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    oa.set_step_counter(ka, advance=True)
    ob.set_step_counter(kb, advance=True)
    ref = [t.double().cpu() for t in init]
    big = [r.abs().max().item() for r in ref]
    g = torch.Generator().manual_seed(9)
    d32, omd32 = _d_pair(0.9, False, 1)
    for s in range(K):
        _set_grads([a, b], g)
        oa.step(); ob.step()
        for i, (pa, pb) in enumerate(zip(a, b)):
            assert torch.equal(pa.data, pb.data), i
            ref[i] = d32 * ref[i] + omd32 * pa.detach().double().cpu()
            big[i] = max(big[i], pa.detach().abs().max().item(), ref[i].abs().max().item())
    assert int(ka.item()) == K and int(kb.item()) == K
    assert int(oa._ticket.item()) == 0
    for i, p in enumerate(a):
        err = (oa.state[p]["ema"].double().cpu() - ref[i]).abs().max().item()
        assert err <= 3 * K * U * big[i], (i, err)
        assert int(oa.state[p]["step"]) == 0                          # the device counter carries the step number


# ---- the model ----------------------------------------------------------------------------------------------------------------------------
def _model(seed=0, mode="bf16"):
    torch.manual_seed(seed)
    m = P().TransformerCNNHybrid(compute_dtype=mode, **SMALL).cuda().train()
    for a in m.encoder.attention_layers:
        a.dropoutLayer.p = 0.0
    g = torch.Generator().manual_seed(3)
    x = torch.rand(2, 4, 3, 32, 32, generator=g).cuda()
    y = torch.randint(0, 8, (2,), generator=g).cuda()
    return m, x, y


def _eager_step(m, opt, crit, x, y):
    opt.zero_grad(set_to_none=True)
    crit(m(x), y).backward()
    opt.step()


def _assert_same(m1, o1, m2, o2):
    for (n, a), (_, b) in zip(m1.named_parameters(), m2.named_parameters()):
        assert torch.equal(a, b), n
        assert torch.equal(o1.state[a]["ema"], o2.state[b]["ema"]), n


def test_graph_equals_eager_and_follows_a_changed_decay():
    """WARM = 6, so that the step after the three compared replays is step 10: the first at which the warm-up value (10/19) is above 0.5 and
    a decay of 0.5 and one of 0.99 give different averages; steps 7 .. 9 are in the warm-up branch."""
    WARM, K = 6, 3
    crit = P().HybridCrossEntropyLoss()
    kw = dict(lr=1e-3, ema_decay=0.99, ema_warmup=True)
    m1, x, y = _model()
    o1 = P().HybridAdamW(m1.parameters(), **kw)
    for _ in range(WARM + K):
        _eager_step(m1, o1, crit, x, y)
    m2, _, _ = _model()
    o2 = P().HybridAdamW(m2.parameters(), **kw)
    tr = P().GraphedTrainStep(m2, crit, o2, x, y, warmup=WARM)
    try:
        assert tr.gs is not None
        bound = [o2.state[p]["ema"].data_ptr() for p in m2.parameters()]
        for _ in range(K):
            tr.step()
        _assert_same(m1, o1, m2, o2)
        assert bound == [o2.state[p]["ema"].data_ptr() for p in m2.parameters()]         # the averages of the warm-up steps are the bound ones
        o1.param_groups[0]["ema_decay"] = 0.5
        o2.param_groups[0]["ema_decay"] = 0.5
        _eager_step(m1, o1, crit, x, y)
        tr.step()
        _assert_same(m1, o1, m2, o2)
        changed = [o2.state[p]["ema"].clone() for p in m2.parameters()]
        o2.param_groups[0]["ema_decay"] = None
        with pytest.raises(RuntimeError, match="switched on or off"):
            tr.step()
        o2.param_groups[0]["ema_decay"] = 0.5
    finally:
        tr.close()
    m3, _, _ = _model()
    o3 = P().HybridAdamW(m3.parameters(), **kw)
    tr = P().GraphedTrainStep(m3, crit, o3, x, y, warmup=WARM)
    try:
        for _ in range(K + 1):
            tr.step()
        for (n, a), b, e2 in zip(m2.named_parameters(), m3.parameters(), changed):
            assert torch.equal(a, b), n                                                  # the weights do not depend on the decay
        differ = sum(1 for b, e2 in zip(m3.parameters(), changed) if not torch.equal(o3.state[b]["ema"], e2))
        assert differ > 10, differ
    finally:
        tr.close()


def test_averages_and_blocks_are_refused_under_capture(monkeypatch):
    """A first step under capture whose averages, or whose device blocks, do not exist raises before any launch is recorded; with both in place a
    capturing step() records the one launch and no upload.  (No real capture: only the decisions are under test.)"""
    from transformer_cnn_hybrid_network_for_video_processing_amd._lib import lib
    ps = [torch.nn.Parameter(torch.randn(5000, device="cuda"))]
    ps[0].grad = torch.randn(5000, device="cuda")
    opt = P().HybridAdamW(ps, lr=1e-3, ema_decay=0.9)
    calls = []
    orig = lib.call
    monkeypatch.setattr(lib, "call", lambda name, *a: (calls.append(name), orig(name, *a))[1])
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="weight average does not exist yet and cannot be created under stream capture"):
        opt.step()
    with pytest.raises(RuntimeError, match="under stream capture"):
        opt.ema_init()
    assert calls == [] and "ema" not in opt.state[ps[0]]
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    opt.ema_init()
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="device hyper-parameter block does not exist yet"):
        opt.step()
    assert calls == []
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    opt.step()                                            # eager: creates the blocks, uploads both
    assert calls == ["hyb_adamw_hyper_set", "hyb_adamw_ema_set", "hyb_adamw_step_dev_ema"], calls
    del calls[:]
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    opt.param_groups[0]["ema_decay"] = 0.5                # a change nobody uploaded: the "captured" step still must not upload it
    opt.step()
    assert calls == ["hyb_adamw_step_dev_ema"], calls
    with pytest.raises(RuntimeError, match="under stream capture"):
        opt.sync_hyper()
    monkeypatch.undo()
    torch.cuda.synchronize()


def _reference_predict(m, opt, x):
    """predict of a fresh model that loaded the live state dict with every parameter replaced by a clone of its average."""
    sd = m.state_dict()
    for n, p in m.named_parameters():
        sd[n] = opt.state[p]["ema"].clone()
    torch.manual_seed(99)
    ref = P().TransformerCNNHybrid(**SMALL).cuda()
    ref.load_state_dict(sd)
    return ref.predict(x)


def test_twin_module_reads_the_averages_in_place():
    torch.manual_seed(0)
    m = P().TransformerCNNHybrid(**SMALL).cuda().train()
    for a in m.encoder.attention_layers:
        a.dropoutLayer.p = 0.0
    g = torch.Generator().manual_seed(3)
    x = torch.rand(2, 4, 3, 32, 32, generator=g).cuda()
    y = torch.randint(0, 8, (2,), generator=g).cuda()
    crit = P().HybridCrossEntropyLoss()
    opt = P().HybridAdamW(m.parameters(), lr=1e-2, ema_decay=0.5)
    with pytest.raises(RuntimeError, match="no average yet"):
        opt.ema_model(m)
    for _ in range(3):
        _eager_step(m, opt, crit, x, y)
    twin = opt.ema_model(m)
    assert type(twin) is type(m)
    for (n, p), (n2, q) in zip(m.named_parameters(), twin.named_parameters()):
        assert n == n2 and q.data_ptr() == opt.state[p]["ema"].data_ptr() and q.data_ptr() != p.data_ptr() and not q.requires_grad, n
    for (n, b), (n2, c) in zip(m.named_buffers(), twin.named_buffers()):
        assert n == n2 and c.data_ptr() == b.data_ptr(), n
    assert all(p.requires_grad for p in m.parameters())
    out = twin.predict(x).clone()
    assert torch.equal(out, _reference_predict(m, opt, x))
    assert not torch.equal(out, m.predict(x))                             # the averaged weights are not the live ones
    gp = P().GraphedPredict(twin, x)
    try:
        assert torch.equal(gp(x), out)
        _eager_step(m, opt, crit, x, y)                                   # the averages (and the running statistics) move under the twin
        out2 = twin.predict(x).clone()
        assert torch.equal(out2, _reference_predict(m, opt, x)) and not torch.equal(out2, out)
        assert torch.equal(gp(x), out2)                                   # the replay reads what the averages hold now
    finally:
        gp.close()


def test_checkpoint_round_trip_and_the_tables_follow_the_new_averages():
    """a: steps, reloads its own state dict midrun (new state tensors; the freed ones are poisoned), steps on.  b: a fresh optimizer that loaded
    the same state dict.  c: never interrupted.  All three agree bit for bit, averages included."""
    init = _init(10)
    a, b, c = _params(init), _params(init), _params(init)
    kw = dict(lr=1e-2, ema_decay=0.9, ema_warmup=True)
    oa, oc = P().HybridAdamW(a, **kw), P().HybridAdamW(c, **kw)
    g = torch.Generator().manual_seed(11)
    for _ in range(2):
        _set_grads([a, c], g)
        oa.step(); oc.step()
    sd = copy.deepcopy(oa.state_dict())
    ob = P().HybridAdamW(b, lr=1.0)
    ob.load_state_dict(copy.deepcopy(sd))
    assert ob.param_groups[0]["ema_decay"] == 0.9 and ob.param_groups[0]["ema_warmup"] is True
    with torch.no_grad():
        for pb, pa in zip(b, a):
            pb.copy_(pa)
    old = [oa.state[p]["ema"].data_ptr() for p in a]
    oa.load_state_dict(copy.deepcopy(sd))
    assert all(oa.state[p]["ema"].data_ptr() != o for p, o in zip(a, old))
    junk = [torch.full((1 << 20,), float("nan"), device="cuda") for _ in range(8)]     # recycle freed blocks with poison
    junk += [torch.full((n,), float("nan"), device="cuda") for n in SIZES + [1025] for _ in range(4)]
    del junk
    _set_grads([a, b, c], g)
    oa.step(); ob.step(); oc.step()
    for pa, pb, pc in zip(a, b, c):
        assert torch.equal(pa.data, pc.data) and torch.equal(pb.data, pc.data)
        ea, eb, ec = oa.state[pa]["ema"], ob.state[pb]["ema"], oc.state[pc]["ema"]
        assert eb.dtype == torch.float32 and eb.is_contiguous()
        assert torch.isfinite(ec).all() and torch.equal(ea, ec) and torch.equal(eb, ec)
        assert int(oa.state[pa]["step"]) == int(ob.state[pb]["step"]) == 3
