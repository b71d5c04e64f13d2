"""HybridCrossEntropyLoss with a MixTarget (two targets per clip and their mixing weight, the labels of a Mixup / CutMix batch) on the
GPU: the criterion alone against tests/mix_ref.py in float64, the edge semantics (lam == 1 is the one-target criterion bit for bit, bad
lam, nothing kept, a side that must not be looked at), the loss inside the temporal part's launches against the separate criterion bit
for bit, the graphed training step with a MixTarget, and opcheck of the four new operators.

Grid and gates are those of tests/test_gpu_loss_options.py: (B, C) in its SHAPES x eps {0, 0.1, 1} x weighted / unweighted x
ignore_index {None, 1, -100}, 108 cases, none skipped; loss error <= 1e-5 * max(1, |ref|); gradient error <= 4 * (the fp32 CPU arbiter's
error against the same float64 reference) + 1e-6 * max|g_ref|.  lam is per clip: random values plus one exact 1 and one exact 0 when
B > 2; with an ignore_index and B > 1 the last clip's first target is ignored, and so is the second target of whichever clip has the last
clip as its partner.  Every case prints its figures before it asserts (pytest -s); profiles/mix_loss_errors.txt (scripts/mix_loss_errors.py,
from measure() below) lists the measured worst figures per option combination."""
import functools
import math

import pytest
import torch

from mix_ref import mix_ce_ref
from test_gpu_loss_options import DLOSS, EPS, IGNORE, KW, OPCHECK_TESTS, SHAPES, _option_criterion, _setup

pytestmark = pytest.mark.gpu


def P():
    import transformer_cnn_hybrid_network_for_video_processing_amd as pkg
    return pkg


def ops():
    from transformer_cnn_hybrid_network_for_video_processing_amd import ops as o
    return o


@functools.lru_cache(maxsize=None)
def case(B, C, eps, use_w, ign):
    """One grid case, on the CPU, computed once: (logits, y_a, y_b, lam, weight or None, float64 loss, float64 gradient for dloss = 1.5, the
    fp32 CPU arbiter's loss and gradient errors)."""
    g = torch.Generator().manual_seed(100 * B + C)
    logits = 3.0 * torch.randn(B, C, generator=g)
    ya = torch.randint(0, C, (B,), generator=g)
    w = None
    if use_w:
        w = torch.rand(C, generator=g) + 0.25
        if C > 2:
            w[1] = 0.0
    ya[0] = 0                                                       # clip 0's first target is kept and its class carries weight
    perm = torch.randperm(B, generator=g)
    lam = torch.rand(B, generator=g)
    if B > 2:
        lam[1], lam[2] = 1.0, 0.0
    if ign is not None and B > 1:
        ya[B - 1] = ign                                             # ignored on the a side (last clip) and, through the partner, on the c side
    yb = ya[perm]

    def run(dtype):
        lg = logits.clone().to(dtype).requires_grad_(True)
        loss = mix_ce_ref(lg, ya, yb, lam, w, ign, eps)
        (loss * DLOSS).backward()
        return loss.detach(), lg.grad
    l64, g64 = run(torch.float64)
    l32, g32 = run(torch.float32)
    assert math.isfinite(float(l64)) and bool(torch.isfinite(g64).all())            # no case is skipped: the reference is finite on this grid
    return logits, ya, yb, lam, w, float(l64), g64, abs(float(l32) - float(l64)), float((g32.double() - g64).abs().max())


def _target(ya, yb, lam):
    return P().MixTarget(ya.cuda(), yb.cuda(), lam.cuda())


def measure(B, C, eps, use_w, ign):
    """-> (loss error, loss bound, gradient error, gradient bound, arbiter's gradient error) of the criterion on the GPU for one case."""
    logits, ya, yb, lam, w, l64, g64, _, arb = case(B, C, eps, use_w, ign)
    crit = P().HybridCrossEntropyLoss(weight=w, ignore_index=ign, label_smoothing=eps).cuda()
    lg = logits.cuda().requires_grad_(True)
    loss = crit(lg, _target(ya, yb, lam))
    (loss * DLOSS).backward()
    gerr = float((lg.grad.double().cpu() - g64).abs().max())
    return abs(float(loss.detach()) - l64), 1e-5 * max(1.0, abs(l64)), gerr, 4.0 * arb + 1e-6 * float(g64.abs().max()), arb


@pytest.mark.parametrize("ign", IGNORE, ids=["keepall", "ignore1", "ignore-100"])
@pytest.mark.parametrize("use_w", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("eps", EPS, ids=["eps0", "eps0.1", "eps1"])
def test_mix_criterion_against_the_float64_definition(eps, use_w, ign):
    """Six shapes per option combination, 108 cases in all.  Measured on the MI355X (profiles/mix_loss_errors.txt): worst loss error 0.014
    of its bound, worst gradient error 0.14 of its gate; the gates are those of tests/test_gpu_loss_options.py, unchanged."""
    bad = []
    for B, C in SHAPES:
        lerr, lbound, gerr, gbound, arb = measure(B, C, eps, use_w, ign)
        print(f"B={B} C={C} eps={eps} weighted={use_w} ignore={ign}: loss err {lerr:.3e} (<= {lbound:.1e})  grad err {gerr:.3e} "
              f"(<= {gbound:.3e}, arbiter {arb:.3e})")
        if not (lerr <= lbound and gerr <= gbound):
            bad.append((B, C, lerr, lbound, gerr, gbound))
    assert not bad, bad


def _run(crit, logits, y):
    lg = logits.clone().requires_grad_(True)
    loss = crit(lg, y)
    (loss * DLOSS).backward()
    return loss.detach(), lg.grad


@pytest.mark.parametrize("shape", [(1, 2), (3, 5), (40, 5), (5, 64), (300, 8)], ids=lambda s: f"B{s[0]}C{s[1]}")
def test_lam_one_everywhere_is_the_one_target_criterion(shape):
    B, C = shape
    for eps, use_w, ign in ((0.1, True, 1), (0.0, False, -100), (1.0, True, None), (0.0, True, None)):
        logits, ya, yb, _, w, *_ = case(B, C, eps, use_w, ign)
        crit = P().HybridCrossEntropyLoss(weight=w, ignore_index=ign, label_smoothing=eps).cuda()
        l1, g1 = _run(crit, logits.cuda(), _target(ya, yb, torch.ones(B)))
        l0, g0 = _run(lambda lg, t: ops().cross_entropy_opts(lg, t, crit.weight, ign, eps), logits.cuda(), ya.cuda())
        assert torch.equal(l1, l0) and torch.equal(g1, g0), (eps, use_w, ign)          # bit for bit: loss and gradient
        # lam == 0 everywhere is the criterion on the second target
        l2, g2 = _run(crit, logits.cuda(), _target(ya, yb, torch.zeros(B)))
        l3, g3 = _run(lambda lg, t: ops().cross_entropy_opts(lg, t, crit.weight, ign, eps), logits.cuda(), yb.cuda())
        assert torch.equal(l2, l3) and torch.equal(g2, g3), (eps, use_w, ign)
    # no options: within the gates of the plain criterion (its kernels keep their own summation)
    logits, ya, yb, *_ = case(B, C, 0.0, False, None)
    l1, g1 = _run(P().HybridCrossEntropyLoss(), logits.cuda(), _target(ya, yb, torch.ones(B)))
    l0, g0 = _run(P().HybridCrossEntropyLoss(), logits.cuda(), ya.cuda())
    _, _, _, _, _, l64, g64, _, arb = _plain_case(B, C)
    assert abs(float(l1) - l64) <= 1e-5 * max(1.0, abs(l64)) and abs(float(l0) - l64) <= 1e-5 * max(1.0, abs(l64))
    for g in (g1, g0):
        assert float((g.double().cpu() - g64).abs().max()) <= 4.0 * arb + 1e-6 * float(g64.abs().max())


@functools.lru_cache(maxsize=None)
def _plain_case(B, C):
    """case(B, C, 0, False, None) with lam == 1: the float64 reference and the arbiter of the plain criterion on y_a."""
    logits, ya, yb, _, w, *_ = case(B, C, 0.0, False, None)
    one = torch.ones(B)

    def run(dtype):
        lg = logits.clone().to(dtype).requires_grad_(True)
        loss = mix_ce_ref(lg, ya, yb, one, None, None, 0.0)
        (loss * DLOSS).backward()
        return loss.detach(), lg.grad
    l64, g64 = run(torch.float64)
    l32, g32 = run(torch.float32)
    return logits, ya, yb, one, w, float(l64), g64, abs(float(l32) - float(l64)), float((g32.double() - g64).abs().max())


@pytest.mark.parametrize("bad", [1.5, -0.1, float("nan")])
def test_lam_outside_the_unit_interval_gives_a_nan_loss(bad):
    for B in (1, 5, 300):
        torch.manual_seed(B)
        logits = 3 * torch.randn(B, 6, device="cuda")
        y = torch.randint(0, 6, (B,), device="cuda")
        lam = torch.full((B,), 0.5, device="cuda")
        lam[B // 2] = bad
        for kw in (dict(), dict(label_smoothing=0.1, ignore_index=2)):
            assert math.isnan(float(P().HybridCrossEntropyLoss(**kw).cuda()(logits, P().MixTarget(y, y.flip(0), lam))))


@pytest.mark.parametrize("B", [1, 5, 300])
def test_nothing_kept_on_either_side_gives_nan_loss_and_zero_gradient(B):
    torch.manual_seed(B)
    logits = 3 * torch.randn(B, 6, device="cuda")
    lam = torch.rand(B, device="cuda")
    for ign in (2, -100):
        y = torch.full((B,), ign, device="cuda")
        for eps in (0.0, 0.1):
            loss, g = _run(P().HybridCrossEntropyLoss(ignore_index=ign, label_smoothing=eps).cuda(), logits, P().MixTarget(y, y.clone(), lam))
            assert math.isnan(float(loss)) and torch.equal(g, torch.zeros_like(g))
    # zero total weight on both sides
    w = torch.tensor([1.0, 0.0, 0.5, 0.0, 2.0, 1.0])
    ya, yb = torch.tensor([1, 3] * B, device="cuda")[:B], torch.tensor([3, 1] * B, device="cuda")[:B]
    loss, g = _run(P().HybridCrossEntropyLoss(weight=w, label_smoothing=0.1).cuda(), logits, P().MixTarget(ya, yb, lam))
    assert math.isnan(float(loss)) and torch.equal(g, torch.zeros_like(g))


def test_a_side_with_no_weight_is_not_looked_at():
    logits = torch.randn(4, 5, device="cuda")
    ya, yb = torch.tensor([0, 4, 2, 1], device="cuda"), torch.tensor([3, 0, 1, 2], device="cuda")
    lam = torch.tensor([1.0, 0.3, 0.0, 0.7], device="cuda")
    w = torch.tensor([1.0, 2.0, 0.5, 1.0, 0.25])
    for kw in (dict(), dict(weight=w, label_smoothing=0.2, ignore_index=-100)):
        crit = P().HybridCrossEntropyLoss(**kw).cuda()
        l0, g0 = _run(crit, logits, P().MixTarget(ya, yb, lam))
        assert math.isfinite(float(l0))
        for bad in (5, -1, 2 ** 40):
            yb2, ya2 = yb.clone(), ya.clone()
            yb2[0], ya2[2] = bad, bad                               # c_0 under l_0 == 1, a_2 under l_2 == 0: neither may change anything
            l1, g1 = _run(crit, logits, P().MixTarget(ya2, yb2, lam))
            assert torch.equal(l0, l1) and torch.equal(g0, g1), (kw, bad)
            yb3 = yb.clone()
            yb3[1] = bad                                            # a kept side that is looked at: poisons the loss
            assert math.isnan(float(crit(logits, P().MixTarget(ya, yb3, lam))))
    with pytest.raises(ValueError, match="lam"):
        P().HybridCrossEntropyLoss()(logits, P().MixTarget(ya, yb, lam[:3]))
    with pytest.raises(TypeError, match="float32"):
        P().HybridCrossEntropyLoss()(logits, P().MixTarget(ya, yb, lam.double()))


def _mix_labels(B, classes, ignore=None):
    g = torch.Generator().manual_seed(17 + B)
    ya = torch.randint(0, classes, (B,), generator=g)
    ya[0] = 0
    if ignore is not None:
        ya[B - 1] = ignore
    yb = ya[torch.randperm(B, generator=g)]
    lam = torch.rand(B, generator=g)
    lam[0] = 1.0 if B > 1 else 0.4
    if B > 2:
        lam[1] = 0.0
    return P().MixTarget(ya.cuda(), yb.cuda(), lam.cuda())


@pytest.mark.parametrize("opts", [True, False], ids=["options", "plain"])
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(3, 5), (8, 16), (2, 1), (40, 4)], ids=["B3S5", "B8S16", "B2S1", "B40S4"])
def test_mix_loss_inside_the_temporal_launches_equals_the_separate_criterion_bitwise(mode, shape, opts):
    """hybrid::temporal_ce_mix against `criterion(model(x), MixTarget)` with the criterion's own two launches: loss, logits and every
    gradient bit for bit.  B = 40 takes the fallback inside hyb_temporal_ce_mix_*."""
    B, S = shape
    torch.manual_seed(9)
    kw = dict(cnn_channels=(32, 64), d_model=64, num_heads=4, num_layers=2, hidden_dim=128, dropout=0.1, num_classes=5, compute_dtype=mode)
    a, b = P().TransformerCNNHybrid(**kw).cuda().train(), P().TransformerCNNHybrid(**kw).cuda().train()
    b.load_state_dict(a.state_dict())
    x = torch.rand(B, S, 3, 16, 16, device="cuda")
    y = _mix_labels(B, 5, ignore=1 if opts else None)
    mask = (torch.rand(B, S, S, device="cuda") > 0.3).float()
    mask[:, :, 0] = 1
    crit = _option_criterion(5) if opts else P().HybridCrossEntropyLoss()
    o = ops()
    torch.manual_seed(11); o._SEED_COUNTER[0] = 100
    la = crit(a(x, mask), y)
    (la * DLOSS).backward()
    torch.manual_seed(11); o._SEED_COUNTER[0] = 100
    h, Bh = b.forward_backbone(x)
    lb, logits_b = b.forward_temporal_loss(h, Bh, y, mask, crit)
    (lb * DLOSS).backward()
    assert math.isfinite(float(la.detach())) and torch.equal(la.detach(), lb.detach())
    with torch.no_grad():
        torch.manual_seed(11); o._SEED_COUNTER[0] = 100
        assert torch.equal(a(x, mask), logits_b)
    for (n, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(pa.grad, pb.grad), n
    assert any(bool((p.grad != 0).any()) for p in b.parameters())
    want = mix_ce_ref(logits_b.detach().cpu().double(), y.y_a.cpu(), y.y_b.cpu(), y.lam.cpu(), crit.weight.cpu() if opts else None,
                      1 if opts else None, 0.1 if opts else 0.0)
    assert abs(float(lb.detach()) - float(want)) <= 1e-5 * max(1.0, abs(float(want)))
    # the unfused path (one operator per stage, the criterion as its own launch) takes the MixTarget too: held to the definition on its own logits
    b.fuse_model_ops = False
    torch.manual_seed(11); o._SEED_COUNTER[0] = 100
    h, Bh = b.forward_backbone(x)
    lc, logits_c = b.forward_temporal_loss(h, Bh, y, mask, crit)
    want_c = mix_ce_ref(logits_c.detach().cpu().double(), y.y_a.cpu(), y.y_b.cpu(), y.lam.cpu(), crit.weight.cpu() if opts else None,
                        1 if opts else None, 0.1 if opts else 0.0)
    assert math.isfinite(float(lc.detach())) and abs(float(lc.detach()) - float(want_c)) <= 1e-5 * max(1.0, abs(float(want_c)))
    # the ticket word behind the per-clip terms is back at zero in every scratch buffer in use
    torch.cuda.synchronize()
    for key, buf in o._CE_SCRATCH.items():
        assert int(buf[-1:].view(torch.int32).item()) == 0, key


@pytest.mark.parametrize("mode", ["bf16", "mixed"])
def test_graphed_steps_with_a_mix_target_equal_eager_steps_bitwise(mode):
    """The set-up of the existing graph tests with a MixTarget: the loss stays inside the captured temporal launches, K replays are K eager
    steps, a load() with new lam and new partners reaches the next replay without a recapture, a changed label_smoothing is refused, and a
    plain tensor cannot be loaded into a step built with a MixTarget (nor the reverse)."""
    K, WARM = 4, 2
    m1, x, _ = _setup(mode)
    m2, _, _ = _setup(mode)
    crit = _option_criterion(8)
    y = P().MixTarget(torch.tensor([0, 6, 1]).cuda(), torch.tensor([6, 1, 0]).cuda(), torch.tensor([0.7, 1.0, 0.25]).cuda())
    cur = [y]
    o1, o2 = P().HybridAdamW(m1.parameters(), lr=1e-3), P().HybridAdamW(m2.parameters(), lr=1e-3)

    def eager_step():
        o1.zero_grad(set_to_none=True)
        loss = crit(m1(x), cur[0])
        loss.backward()
        o1.step()
        return loss.item()
    eager_losses = [eager_step() for _ in range(WARM + K)]
    tr = P().GraphedTrainStep(m2, crit, o2, x, y, warmup=WARM)
    try:
        assert tr._fused_loss and isinstance(tr.y, P().MixTarget) and all(s.data_ptr() != t.data_ptr() for s, t in zip(tr.y, y))
        graph_losses = [tr.step().item() for _ in range(K)]
        assert all(math.isfinite(v) for v in graph_losses)
        assert graph_losses == eager_losses[WARM:], (graph_losses, eager_losses)
        assert tr.steps_done() == WARM + K
        for (n, a), (_, b) in zip(m1.named_parameters(), m2.named_parameters()):
            assert torch.equal(a, b), n
        for (n, a), (_, b) in zip(m1.named_buffers(), m2.named_buffers()):
            assert torch.equal(a, b), n
        for pa, pb in zip(m1.parameters(), m2.parameters()):
            assert torch.equal(o1.state[pa]["exp_avg"], o2.state[pb]["exp_avg"])
            assert torch.equal(o1.state[pa]["exp_avg_sq"], o2.state[pb]["exp_avg_sq"])
        # new lam and new partners: read from device memory by the next replay
        cur[0] = P().MixTarget(torch.tensor([0, 6, 2]).cuda(), torch.tensor([2, 0, 6]).cuda(), torch.tensor([0.1, 0.6, 0.0]).cuda())
        tr.load(x, cur[0])
        want = eager_step()
        got = tr.step().item()
        assert got == want and got == crit(tr.logits, cur[0]).item() and got != crit(tr.logits, y).item()
        for (n, a), (_, b) in zip(m1.named_parameters(), m2.named_parameters()):
            assert torch.equal(a, b), n
        with pytest.raises(TypeError, match="MixTarget"):
            tr.load(x, cur[0].y_a)
        crit.label_smoothing = 0.2
        with pytest.raises(RuntimeError, match="criterion's label_smoothing changed"):
            tr.step()
        crit.label_smoothing = 0.1
        tr.step()
    finally:
        tr.close()
    assert ops().step_counter() is None
    # the reverse: a step built with class indices refuses a MixTarget
    m3, x3, y3 = _setup(mode)
    tr = P().GraphedTrainStep(m3, P().HybridCrossEntropyLoss(), P().HybridAdamW(m3.parameters(), lr=1e-3), x3, y3, warmup=1)
    try:
        with pytest.raises(TypeError, match="MixTarget"):
            tr.load(x3, y)
    finally:
        tr.close()


def _opcheck(op, args, **kw):
    torch.library.opcheck(op, args, test_utils=OPCHECK_TESTS, **kw)


@pytest.mark.parametrize("dt", [0, 1], ids=["fp32", "bf16"])
def test_opcheck_mix_loss_operators(dt):
    o = ops()
    tdt = o.torch_dtype(dt)
    torch.manual_seed(6)
    w5 = torch.tensor([1.0, 0.0, 0.5, 2.0, 1.5], device="cuda")
    logits = torch.randn(4, 5, device="cuda", requires_grad=True)
    tgt, tgt_b = torch.tensor([0, 4, 2, 1], device="cuda"), torch.tensor([2, 0, 1, 4], device="cuda")
    lam = torch.tensor([1.0, 0.3, 0.0, 0.6], device="cuda")
    if dt == 0:                                                    # (the stand-alone criterion has no dtype: once)
        for weight, ign, has, eps in ((w5, 2, True, 0.1), (None, 0, False, 0.3), (None, 0, False, 0.0)):
            _opcheck(torch.ops.hybrid.cross_entropy_mix.default, (logits, tgt, tgt_b, lam, weight, ign, has, eps))
            _opcheck(torch.ops.hybrid.cross_entropy_mix_bwd.default, (torch.ones((), device="cuda"), logits.detach(), tgt, tgt_b, lam, weight, ign, has,
                                                                      eps))
    B, S, D, Hid, L, H = 4, 8, 32, 64, 2, 2
    enc = P().TransformerEncoder(D, Hid, L, H, 0.1).cuda()
    params = [p.detach().clone().requires_grad_(True) for p in enc._flat_params()]
    h = torch.rand(B * S, 2, 3, 64, device="cuda").to(tdt).requires_grad_(True)
    tw = (torch.randn(D, 64, device="cuda") * 0.1).requires_grad_(True)
    tb = torch.randn(D, device="cuda").requires_grad_(True)
    hw = (torch.randn(5, D, device="cuda") * 0.1).requires_grad_(True)
    hb = torch.randn(5, device="cuda").requires_grad_(True)
    args_ce = (h, tw, tb, params, hw, hb, None, tgt, tgt_b, lam, w5, 2, True, 0.1, B, dt, Hid, L, H, 0.1, 0.1, 77)
    _opcheck(torch.ops.hybrid.temporal_ce_mix.default, args_ce)
    loss, logits2, feat, saved_blob, enc_out = torch.ops.hybrid.temporal_ce_mix(*args_ce)
    assert math.isfinite(float(loss))
    _opcheck(torch.ops.hybrid.temporal_ce_mix_bwd.default,
             (torch.ones_like(loss).detach(), logits2.detach(), tgt, tgt_b, lam, w5, 2, True, 0.1, tw.detach(), [p.detach() for p in params],
              hw.detach(), None, feat.detach(), saved_blob, enc_out.detach(), 2, 3, dt, Hid, L, H, 0.1, 0.1, 77))
    # lam and the class weights get no gradient
    wg, lg_ = w5.clone().requires_grad_(True), lam.clone().requires_grad_(True)
    l = torch.ops.hybrid.cross_entropy_mix(logits, tgt, tgt_b, lg_, wg, 2, True, 0.1)
    gl, gw, glam = torch.autograd.grad(l, [logits, wg, lg_], allow_unused=True)
    assert gw is None and glam is None and gl is not None
