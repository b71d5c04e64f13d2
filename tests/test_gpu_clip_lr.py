"""Gradient-norm clipping fused into HybridAdamW and hyper-parameters that live on the device (learning-rate schedules under hipGraph replay):
hyb_grad_norm against fp64 and bit-reproducible, the clipped update against an fp64 optimizer with torch's own fp32 chain as the arbiter,
"unclipped == no clipping" bit for bit, and GraphedTrainStep following a torch.optim.lr_scheduler / clipping exactly like the eager step."""
import ctypes
import math
import os
import socket
import subprocess
import sys
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KW = dict(cnn_channels=(32, 64), d_model=64, num_heads=4, num_layers=2, hidden_dim=128)      # the small model of tests/test_gpu_graph.py


def P():
    import transformer_cnn_hybrid_network_for_video_processing_amd as pkg
    return pkg


def _lib():
    from transformer_cnn_hybrid_network_for_video_processing_amd._lib import lib, ptr_array
    return lib, ptr_array


def _params(seed):
    """The tensor set of tests/test_gpu_optim.py::_params: odd sizes, and one view that is only 4-byte aligned."""
    g = torch.Generator().manual_seed(seed)
    shapes = [(512, 512), (2048, 512), (8,), (3,), (1000,), (4097,), (32, 3, 3, 3), (1,)]
    ps = [torch.randn(s, generator=g).cuda() for s in shapes]
    base = torch.randn(1030, generator=g).cuda()
    ps.append(base[1:1026])
    return ps


def _hundred(seed):
    """100 tensors: more than one launch's tensor table holds (tests/test_gpu_optim.py, the two-launch case)."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(int(n), generator=g).cuda() for n in torch.randint(1, 5000, (100,), generator=g)]


class NormCall:
    """hyb_grad_norm through the raw C ABI with buffers of its own."""

    def __init__(self, tensors, max_norm):
        lib, ptr_array = _lib()
        self.tensors = tensors
        self.numel = (ctypes.c_longlong * len(tensors))(*[t.numel() for t in tensors])
        self.ptrs = ptr_array([t.data_ptr() for t in tensors])
        chunks = lib.query("hyb_grad_norm_workspace", len(tensors), self.numel)
        assert chunks == sum(-(-t.numel() // 4096) for t in tensors)
        self.partials = torch.zeros(chunks, device="cuda")
        self.out = torch.zeros(2, device="cuda")
        self.hyper = torch.zeros(6, dtype=torch.float64, device="cuda")
        lib.call("hyb_adamw_hyper_set", self.hyper.data_ptr(), 1e-3, 0.9, 0.999, 1e-8, 1e-2, float(max_norm), torch.cuda.current_stream().cuda_stream)

    def __call__(self):
        lib, _ = _lib()
        lib.call("hyb_grad_norm", len(self.tensors), self.ptrs, self.numel, self.partials.data_ptr(), self.hyper.data_ptr(), self.out.data_ptr(),
                 torch.cuda.current_stream().cuda_stream)
        return self.out


@pytest.mark.parametrize("which", ["params", "hundred"])
def test_norm_against_fp64(which):
    """norm_out[0]^2 against the fp64 sum of squares: relative error <= 26 * 2^-24 = 1.6e-6.  Derivation: every term is non-negative, so the
    relative error of the sum is at most (depth of fp32 roundings on any path) * 2^-24.  The kernel's depth: 16 (a thread's 16 fused
    multiply-adds: ONE rounding each -- the square is not rounded by itself, fewer than the 1 + 16 of a separate square and add) + 6 (wave_sum: four
    row rotations, two levels over the four rows) + 2 (four waves pairwise) = 24; everything after that is double, and the final rounding of the
    norm to fp32 is 2^-24 on the norm = 2 * 2^-24 on its square: 26 in all."""
    ts = _params(0) if which == "params" else _hundred(7)
    exact = sum((t.double() ** 2).sum().item() for t in ts)
    for c in (0.5 * math.sqrt(exact), 3.0 * math.sqrt(exact), 0.0, float("inf")):
        call = NormCall(ts, c)
        out = call().cpu().double()
        norm, coef = out[0].item(), out[1].item()
        err = abs(norm * norm - exact) / exact
        print(f"[{which}] max_norm {c:.6g}: norm {norm!r} (fp64 {math.sqrt(exact)!r}), norm^2 rel err {err:.3e}, coef {coef!r}")
        assert err <= 1.6e-6, err
        want = 1.0 if (c <= 0.0 or math.isinf(c)) else min(1.0, c / (norm + 1e-6))
        assert abs(coef - want) <= 2.0 ** -24 * want, (coef, want)               # one fp32 rounding
        if c > math.sqrt(exact) or c == 0.0 or math.isinf(c):
            assert coef == 1.0
        else:
            assert coef < 0.51


def test_norm_is_deterministic_and_independent_of_alignment():
    """(The norm's hand-off between workgroups is a second launch, so there is no ticket word whose rest state could be checked.)"""
    ts = _params(1) + _hundred(2)
    call = NormCall(ts, 1.0)
    torch.cuda.synchronize()
    o0, p0 = call().clone(), call.partials.clone()
    o1, p1 = call().clone(), call.partials.clone()
    busy = torch.randn(4096, 4096, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for _ in range(4):
        busy = busy @ busy * 1e-3                                   # keeps the device busy on the default stream meanwhile
    with torch.cuda.stream(side):
        o2, p2 = call().clone(), call.partials.clone()
    torch.cuda.synchronize()
    assert torch.equal(o0, o1) and torch.equal(o0, o2)
    assert torch.equal(p0, p1) and torch.equal(p0, p2)
    # the same values in a 16-byte-aligned tensor and in a view at a 4-byte offset
    n = 3 * 4096 + 1234
    aligned = torch.randn(n, device="cuda")
    base = torch.empty(n + 1, device="cuda")
    view = base[1:]
    view.copy_(aligned)
    assert aligned.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4
    ca, cv = NormCall([aligned], 1.0), NormCall([view], 1.0)
    oa, ov = ca().clone(), cv().clone()
    torch.cuda.synchronize()
    assert torch.equal(oa, ov) and torch.equal(ca.partials, cv.partials)


def _rel(a, ref):
    return ((a.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


def test_clipped_adamw_against_an_fp64_optimizer():
    """Reference: torch.optim.AdamW on double copies with clip_grad_norm_ on double gradients.  Arbiter: torch's fp32 clip_grad_norm_ +
    torch.optim.AdamW on the GPU, same inputs.  Gate: for parameters and both moments, the worst (over tensors and steps) relative error
    max|x - ref| / max|ref| of HybridAdamW(max_grad_norm) is at most 2 x the arbiter's worst."""
    C = 1000.0
    init = _params(0)
    ref = [torch.nn.Parameter(t.double().clone()) for t in init]
    arb = [torch.nn.Parameter(t.clone()) for t in init]
    hyb = [torch.nn.Parameter(t.clone()) for t in init]
    o_ref = torch.optim.AdamW(ref, lr=1e-3, weight_decay=1e-2)
    o_arb = torch.optim.AdamW(arb, lr=1e-3, weight_decay=1e-2)
    o_hyb = P().HybridAdamW(hyb, lr=1e-3, weight_decay=1e-2, max_grad_norm=C)
    g = torch.Generator().manual_seed(1)
    worst = {k: [0.0, 0.0] for k in ("param", "exp_avg", "exp_avg_sq")}
    ref_norms = []
    for step in range(5):
        for pr, pa, ph in zip(ref, arb, hyb):
            gr = torch.randn(pr.shape, generator=g).cuda() * (10.0 ** (step - 2))
            pr.grad = gr.double(); pa.grad = gr.clone(); ph.grad = gr.clone()
        ref_norms.append(torch.nn.utils.clip_grad_norm_(ref, C).item())
        arb_norm = torch.nn.utils.clip_grad_norm_(arb, C).item()
        o_ref.step(); o_arb.step(); o_hyb.step()
        got = o_hyb.grad_norm.item()
        print(f"step {step}: fp64 norm {ref_norms[-1]:.9g}, HybridAdamW {got:.9g} (rel {abs(got - ref_norms[-1]) / ref_norms[-1]:.2e}), "
              f"torch fp32 {arb_norm:.9g} (rel {abs(arb_norm - ref_norms[-1]) / ref_norms[-1]:.2e}), coef {o_hyb.clip_coef.item():.6g}")
        for pr, pa, ph in zip(ref, arb, hyb):
            for k, xr, xa, xh in (("param", pr.data, pa.data, ph.data),
                                  ("exp_avg", o_ref.state[pr]["exp_avg"], o_arb.state[pa]["exp_avg"], o_hyb.state[ph]["exp_avg"]),
                                  ("exp_avg_sq", o_ref.state[pr]["exp_avg_sq"], o_arb.state[pa]["exp_avg_sq"], o_hyb.state[ph]["exp_avg_sq"])):
                worst[k][0] = max(worst[k][0], _rel(xh, xr))
                worst[k][1] = max(worst[k][1], _rel(xa, xr))
    # the inputs do exercise both branches -- decided on the REFERENCE norms
    assert any(n < C for n in ref_norms) and any(C / n < 0.5 for n in ref_norms), ref_norms
    for k, (e_hyb, e_arb) in worst.items():
        print(f"{k}: worst error against fp64 -- HybridAdamW {e_hyb:.3e}, torch fp32 (arbiter) {e_arb:.3e}")
    for k, (e_hyb, e_arb) in worst.items():
        assert e_hyb <= 2.0 * e_arb, (k, e_hyb, e_arb)


def _grads(ps_lists, g, scale=1.0):
    for group in zip(*ps_lists):
        gr = torch.randn(group[0].shape, generator=g).cuda() * scale
        for p in group:
            p.grad = gr.clone()


def test_unclipped_equals_no_clipping_bit_for_bit():
    init = _params(3)
    a = [torch.nn.Parameter(t.clone()) for t in init]
    b = [torch.nn.Parameter(t.clone()) for t in init]
    oa = P().HybridAdamW(a, lr=1e-3, max_grad_norm=1e30)
    ob = P().HybridAdamW(b, lr=1e-3)
    ob.set_dynamic_hyper(True)
    g = torch.Generator().manual_seed(4)
    for _ in range(3):
        _grads([a, b], g)
        oa.step(); ob.step()
        assert oa.clip_coef.item() == 1.0 and oa.grad_norm.item() > 0
        for pa, pb in zip(a, b):
            assert torch.equal(pa.data, pb.data)
            assert torch.equal(oa.state[pa]["exp_avg"], ob.state[pb]["exp_avg"]) and torch.equal(oa.state[pa]["exp_avg_sq"], ob.state[pb]["exp_avg_sq"])
    # the device path against the plain launch with a device step counter (which already forms its bias corrections with the device pow()):
    # the same arithmetic, only the source of lr / betas / eps / weight_decay differs
    c = [torch.nn.Parameter(t.clone()) for t in init]
    d = [torch.nn.Parameter(t.clone()) for t in init]
    oc = P().HybridAdamW(c, lr=3e-4, weight_decay=0.1, betas=(0.8, 0.99))
    od = P().HybridAdamW(d, lr=3e-4, weight_decay=0.1, betas=(0.8, 0.99), max_grad_norm=1e30)
    kc, kd = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    oc.set_step_counter(kc, advance=True)
    od.set_step_counter(kd, advance=True)
    for step in range(4):
        _grads([c, d], g)
        oc.step(); od.step()
        assert int(kc.item()) == int(kd.item()) == step + 1
        for pc, pd in zip(c, d):
            assert torch.equal(pc.data, pd.data)
            assert torch.equal(oc.state[pc]["exp_avg"], od.state[pd]["exp_avg"]) and torch.equal(oc.state[pc]["exp_avg_sq"], od.state[pd]["exp_avg_sq"])
    assert int(od._ticket.item()) == 0


def test_one_norm_over_all_param_groups():
    init = _params(5)
    C = 20.0
    two = [torch.nn.Parameter(t.clone()) for t in init]
    one_a = [torch.nn.Parameter(t.clone()) for t in init]
    one_b = [torch.nn.Parameter(t.clone()) for t in init]
    o2 = P().HybridAdamW([{"params": two[:4], "lr": 1e-3}, {"params": two[4:], "lr": 5e-3}], max_grad_norm=C)
    oa = P().HybridAdamW(one_a, lr=1e-3, max_grad_norm=C)
    ob = P().HybridAdamW(one_b, lr=5e-3, max_grad_norm=C)
    g = torch.Generator().manual_seed(6)
    for _ in range(3):
        _grads([two, one_a, one_b], g)
        exact = math.sqrt(sum((p.grad.double() ** 2).sum().item() for p in two))
        o2.step(); oa.step(); ob.step()
        assert torch.equal(o2.grad_norm, oa.grad_norm) and torch.equal(o2.clip_coef, oa.clip_coef)
        assert abs(o2.grad_norm.item() - exact) <= 1.6e-6 * exact and o2.clip_coef.item() < 1.0
        for i, p in enumerate(two):                       # each group moved as the single-group optimizer with its learning rate did
            assert torch.equal(p.data, (one_a if i < 4 else one_b)[i].data), i
    bad = P().HybridAdamW([{"params": [torch.nn.Parameter(init[0].clone())], "max_grad_norm": 1.0}, {"params": [torch.nn.Parameter(init[2].clone())]}])
    for grp in bad.param_groups:
        for p in grp["params"]:
            p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError, match="same max_grad_norm"):
        bad.step()


# ---- under replay -------------------------------------------------------------------------------------------------------------------------
def _setup(seed=0, mode="bf16"):
    torch.manual_seed(seed)
    m = P().TransformerCNNHybrid(dropout=0.0, compute_dtype=mode, **KW).cuda().train()
    for a in m.encoder.attention_layers:
        a.dropoutLayer.p = 0.0
    g = torch.Generator().manual_seed(3)
    x = torch.rand(3, 4, 3, 32, 32, generator=g).cuda()
    y = torch.randint(0, 8, (3,), generator=g).cuda()
    return m, x, y


def _sched_step(s):
    with warnings.catch_warnings():                       # a replay is not an optimizer.step() call torch's scheduler could count
        warnings.simplefilter("ignore")
        s.step()


def _warmup_lambda(e):
    return min(1.0, (e + 1) / 6.0)


def _first_step_norm():
    m, x, y = _setup()
    P().HybridCrossEntropyLoss()(m(x), y).backward()
    return math.sqrt(sum((p.grad.double() ** 2).sum().item() for p in m.parameters() if p.grad is not None))


def _graph_against_eager(max_grad_norm, K=6, WARM=2, lr=1e-3):
    """K scheduled steps through GraphedTrainStep against the eager loop with HybridAdamW on the device path and the same scheduler.  The
    constructor's WARM real steps run at the construction-time rate, so the eager loop takes WARM steps at that rate before its scheduler starts."""
    m1, x, y = _setup()
    m2, _, _ = _setup()
    crit = P().HybridCrossEntropyLoss()
    o1 = P().HybridAdamW(m1.parameters(), lr=lr, max_grad_norm=max_grad_norm)
    o2 = P().HybridAdamW(m2.parameters(), lr=lr, max_grad_norm=max_grad_norm)
    o1.set_dynamic_hyper(True)
    s1 = torch.optim.lr_scheduler.LambdaLR(o1, _warmup_lambda)
    s2 = torch.optim.lr_scheduler.LambdaLR(o2, _warmup_lambda)
    eager_losses, eager_norms, rates = [], [], []
    for k in range(WARM + K):
        o1.zero_grad(set_to_none=True)
        loss = crit(m1(x), y)
        loss.backward()
        o1.step()
        eager_losses.append(loss.item())
        eager_norms.append(o1.grad_norm.item())
        rates.append(o1.param_groups[0]["lr"])
        if k >= WARM:
            s1.step()
    assert len(set(rates[WARM:])) == K                    # the schedule did move the rate on every compared step
    tr = P().GraphedTrainStep(m2, crit, o2, x, y, warmup=WARM, dynamic_hyper=True)
    try:
        graph_losses, graph_norms = [], []
        for _ in range(K):
            graph_losses.append(tr.step().item())
            graph_norms.append(tr.grad_norm.item())
            _sched_step(s2)
        assert graph_losses == eager_losses[WARM:], (graph_losses, eager_losses)
        if max_grad_norm is not None:
            print(f"max_grad_norm {max_grad_norm:.6g}, unclipped norms of the compared steps {graph_norms}")
            assert graph_norms == eager_norms[WARM:], (graph_norms, eager_norms)
            assert all(n > max_grad_norm for n in graph_norms), (graph_norms, max_grad_norm)        # coef < 1: clipping was active on every step
        for (n, a), (_, b) in zip(m1.named_parameters(), m2.named_parameters()):
            assert torch.equal(a, b), n
        for (n, a), (_, b) in zip(m1.named_buffers(), m2.named_buffers()):
            assert torch.equal(a, b), n
        tr.sync_optimizer_state()
        for pa, pb in zip(m1.parameters(), m2.parameters()):
            assert int(o1.state[pa]["step"]) == int(o2.state[pb]["step"]) == WARM + K
            assert torch.equal(o1.state[pa]["exp_avg"], o2.state[pb]["exp_avg"])
            assert torch.equal(o1.state[pa]["exp_avg_sq"], o2.state[pb]["exp_avg_sq"])
    finally:
        tr.close()


def test_schedule_under_replay():
    crit = P().HybridCrossEntropyLoss()
    m, x, y = _setup()
    opt = P().HybridAdamW(m.parameters(), lr=1e-3, weight_decay=0.0)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda e: 0.0 if e < 1 else 1.0)
    assert opt.param_groups[0]["lr"] == 0.0               # the rate the step is captured at
    start = [p.detach().clone() for p in m.parameters()]
    tr = P().GraphedTrainStep(m, crit, opt, x, y, warmup=1, dynamic_hyper=True)
    try:
        tr.step(); tr.step()
        torch.cuda.synchronize()
        for p, s in zip(m.parameters(), start):
            assert torch.equal(p, s)
        _sched_step(sched)
        assert opt.param_groups[0]["lr"] == 1e-3
        tr.step()
        torch.cuda.synchronize()
        moved = 0
        for (n, p), s in zip(m.named_parameters(), start):
            if p.grad is not None and bool((p.grad != 0).any()):
                assert not torch.equal(p, s), n
                moved += 1
        assert moved > 10
    finally:
        tr.close()
    _graph_against_eager(None)
    # without dynamic_hyper a changed rate would be lost silently: step() refuses it
    m, x, y = _setup()
    opt = P().HybridAdamW(m.parameters(), lr=1e-3)
    tr = P().GraphedTrainStep(m, crit, opt, x, y, warmup=1)
    try:
        tr.step()
        opt.param_groups[0]["lr"] = 5e-4
        with pytest.raises(RuntimeError, match="dynamic_hyper=True"):
            tr.step()
        opt.param_groups[0]["lr"] = 1e-3
        tr.step()
    finally:
        tr.close()


def test_clipping_under_replay():
    """max_grad_norm = half of the first step's unclipped norm; clipping must be active (coef < 1) on every compared step.  On this one fixed
    batch the gradient norm falls quickly while the model fits it (at a peak rate of 1e-3: 21 -> 17.5 -> 14.8 -> 10.0 -> 5.7 over the first
    steps, measured), so the comparison runs at a peak rate of 1e-5, where the norm stays well above that half for all eight steps."""
    c = 0.5 * _first_step_norm()
    _graph_against_eager(c, lr=1e-5)
    # against stock torch: clip_grad_norm_ + torch.optim.AdamW + the same scheduler (eval mode: no dropout streams to align), 2 steps
    torch.manual_seed(0)
    kw = dict(cnn_channels=(32, 64), d_model=64, num_heads=4, num_layers=1, hidden_dim=128, dropout=0.0)
    m1, m2 = P().TransformerCNNHybrid(**kw).cuda().eval(), P().TransformerCNNHybrid(**kw).cuda().eval()
    m2.load_state_dict(m1.state_dict())
    x = torch.rand(2, 4, 3, 32, 32, device="cuda"); y = torch.tensor([1, 3], device="cuda")
    P().HybridCrossEntropyLoss()(m1(x), y).backward()
    c = 0.5 * math.sqrt(sum((p.grad.double() ** 2).sum().item() for p in m1.parameters()))
    o1, o2 = torch.optim.AdamW(m1.parameters(), lr=1e-3), P().HybridAdamW(m2.parameters(), lr=1e-3, max_grad_norm=c)
    s1, s2 = torch.optim.lr_scheduler.LambdaLR(o1, _warmup_lambda), torch.optim.lr_scheduler.LambdaLR(o2, _warmup_lambda)
    for _ in range(2):
        for m, o, s in ((m1, o1, s1), (m2, o2, s2)):
            o.zero_grad(set_to_none=True)
            P().HybridCrossEntropyLoss()(m(x), y).backward()
            if o is o1:
                n1 = torch.nn.utils.clip_grad_norm_(m.parameters(), c)
            o.step()
            s.step()
        assert o2.clip_coef.item() < 1.0
        torch.testing.assert_close(o2.grad_norm, n1.float().reshape(()), rtol=1e-3, atol=0)
    for (n, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        torch.testing.assert_close(p2, p1, rtol=1e-3, atol=2e-5, msg=n)


def test_constructed_on_dirty_memory():
    """The hyper blocks, partials and norm_out are created and zeroed eagerly, never inside a capture: built on freshly
    poisoned allocator blocks, with only step() ever called, the first replays must be the eager steps."""
    WARM, K = 1, 3
    m1, x, y = _setup()
    m2, _, _ = _setup()
    crit = P().HybridCrossEntropyLoss()
    c = 0.5 * _first_step_norm()
    o1 = P().HybridAdamW(m1.parameters(), lr=1e-3, max_grad_norm=c)
    eager = []
    for _ in range(WARM + K):
        o1.zero_grad(set_to_none=True)
        loss = crit(m1(x), y)
        loss.backward()
        o1.step()
        eager.append((loss.item(), o1.grad_norm.item()))
    torch.cuda.synchronize()
    junk = [torch.full((16 << 20,), -1, dtype=torch.int32, device="cuda") for _ in range(4)]      # 256 MB of 0xFF.. in blocks of several sizes
    junk += [torch.full((n,), -1, dtype=torch.int32, device="cuda") for n in (1, 2, 6, 12, 64, 128, 512, 2048) for _ in range(8)]
    torch.cuda.synchronize()
    del junk
    o2 = P().HybridAdamW(m2.parameters(), lr=1e-3, max_grad_norm=c)
    tr = P().GraphedTrainStep(m2, crit, o2, x, y, warmup=WARM, dynamic_hyper=True)
    try:
        assert tr.gs is not None
        for k in range(K):
            got = tr.step().item()
            norm = tr.grad_norm.item()
            assert math.isfinite(got) and math.isfinite(norm)
            assert (got, norm) == eager[WARM + k], (k, got, norm, eager)
            assert int(o2._ticket.item()) == 0                 # (the advancing AdamW launch's; the norm keeps no state between calls)
    finally:
        tr.close()


def test_buffers_are_refused_under_capture(monkeypatch):
    """A HybridAdamW whose device buffers do not exist yet must not create them while its stream captures (they would be zeroed by that one
    graph only); with the buffers in place and the hyper-parameters uploaded, a capturing step() enqueues no upload."""
    from transformer_cnn_hybrid_network_for_video_processing_amd._lib import lib
    ps = [torch.nn.Parameter(torch.randn(5000, device="cuda"))]
    ps[0].grad = torch.randn(5000, device="cuda")
    opt = P().HybridAdamW(ps, lr=1e-3, max_grad_norm=1.0)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)       # (no real capture: only the decision is under test)
    with pytest.raises(RuntimeError, match="under stream capture"):
        opt.step()
    monkeypatch.undo()
    opt.step()                                            # eager: creates the buffers, uploads the hyper-parameters
    calls = []
    orig = lib.call
    monkeypatch.setattr(lib, "call", lambda name, *a: (calls.append(name), orig(name, *a))[1])
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    opt.param_groups[0]["lr"] = 5e-4                      # a change nobody uploaded: the "captured" step still must not upload it
    opt.step()
    assert calls == ["hyb_grad_norm", "hyb_adamw_step_dev"], calls
    with pytest.raises(RuntimeError, match="under stream capture"):
        opt.sync_hyper()
    monkeypatch.undo()
    torch.cuda.synchronize()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_data_parallel_clipping_and_schedule_graph_equals_eager():
    """Two gloo ranks sharing cuda:0 (tests/dp_clip_worker.py): the graphed DP step with clipping + warm-up schedule against the eager
    GradAllReducer step with the same optimizer -- parameters bit-equal between the two and across ranks, clipping active."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "dp_clip_worker.py")]
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=280)
    lines = [l for l in r.stdout.decode().splitlines() if l.startswith("DPCLIP")]
    assert r.returncode == 0, "\n".join(lines) + "\n" + r.stderr.decode()[-2000:]
    assert len(lines) == 2 and all("mismatching tensors []" in l and "all ranks equal True" in l and "clipped every step True" in l for l in lines), lines
