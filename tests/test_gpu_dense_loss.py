"""The loss on dense targets (one fp32 row of C numbers per clip) on the GPU: soft-target cross-entropy through HybridCrossEntropyLoss
(kind 0) and binary cross-entropy with logits through HybridBCEWithLogitsLoss (kind 1).  The criteria alone against tests/dense_ref.py in
float64, one-hot rows against the plain criterion bit for bit, reproducibility, the loss inside the temporal part's launches against the
separate criterion bit for bit, the graphed training step with a dense target, and opcheck of the four new operators.

Grid and gates are those of tests/test_gpu_loss_options.py: (B, C) in its SHAPES, plus (4, 1) for kind 1; kind 0: eps {0, 0.1, 1} x
weighted / unweighted, kind 1: weight on / off x pos_weight on / off; none skipped; loss error <= 1e-5 * max(1, |ref|); gradient error
<= 4 * (the fp32 CPU arbiter's error against the same float64 reference) + 1e-6 * max|g_ref|.  tests/dense_ref.py builds the inputs: kind 0
rows of probabilities with an exact one-hot row and (B > 2) an all-zero row, kind 1 targets in [0, 1] with an exact 0 and an exact 1 and
logits of +100 and -100.  Every case prints its figures before it asserts (pytest -s); profiles/dense_loss_errors.txt
(scripts/dense_loss_errors.py, from measure() below) lists the measured worst figures per combination."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from dense_ref import BCE_SHAPES, EPS, SHAPES, dense_case, dense_ref
from test_gpu_loss_options import DLOSS, OPCHECK_TESTS, _setup

pytestmark = pytest.mark.gpu


def P():
    import transformer_cnn_hybrid_network_for_video_processing_amd as pkg
    return pkg


def ops():
    from transformer_cnn_hybrid_network_for_video_processing_amd import ops as o
    return o


@functools.lru_cache(maxsize=None)
def case(kind, B, C, eps, use_w, use_pw):
    """One grid case, on the CPU, computed once: (logits, target, weight or None, pos_weight or None, float64 loss, float64 gradient for
    dloss = 1.5, the fp32 CPU arbiter's loss and gradient errors)."""
    logits, t, w, pw = dense_case(kind, B, C, use_w, use_pw)

    def run(dtype):
        lg = logits.clone().to(dtype).requires_grad_(True)
        loss = dense_ref(kind, lg, t, w, pw, eps)
        (loss * DLOSS).backward()
        return loss.detach(), lg.grad
    l64, g64 = run(torch.float64)
    l32, g32 = run(torch.float32)
    assert math.isfinite(float(l64)) and bool(torch.isfinite(g64).all())            # no case is skipped: the reference is finite on this grid
    return logits, t, w, pw, float(l64), g64, abs(float(l32) - float(l64)), float((g32.double() - g64).abs().max())


def _criterion(kind, w, pw, eps):
    if kind == 1:
        return P().HybridBCEWithLogitsLoss(weight=w, pos_weight=pw).cuda()
    return P().HybridCrossEntropyLoss(weight=w, label_smoothing=eps).cuda()


def measure(kind, B, C, eps, use_w, use_pw):
    """-> (loss error, loss bound, gradient error, gradient bound, arbiter's gradient error) of the criterion on the GPU for one case."""
    logits, t, w, pw, l64, g64, _, arb = case(kind, B, C, eps, use_w, use_pw)
    crit = _criterion(kind, w, pw, eps)
    lg = logits.cuda().requires_grad_(True)
    loss = crit(lg, t.cuda())
    (loss * DLOSS).backward()
    assert math.isfinite(float(loss.detach())) and bool(torch.isfinite(lg.grad).all())
    gerr = float((lg.grad.double().cpu() - g64).abs().max())
    return abs(float(loss.detach()) - l64), 1e-5 * max(1.0, abs(l64)), gerr, 4.0 * arb + 1e-6 * float(g64.abs().max()), arb


def _gate(kind, shapes, eps, use_w, use_pw):
    bad = []
    for B, C in shapes:
        lerr, lbound, gerr, gbound, arb = measure(kind, B, C, eps, use_w, use_pw)
        print(f"kind={kind} B={B} C={C} eps={eps} weighted={use_w} pos_weight={use_pw}: loss err {lerr:.3e} (<= {lbound:.1e})  grad err {gerr:.3e} "
              f"(<= {gbound:.3e}, arbiter {arb:.3e})")
        if not (lerr <= lbound and gerr <= gbound):
            bad.append((B, C, lerr, lbound, gerr, gbound))
    assert not bad, bad


@pytest.mark.parametrize("use_w", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("eps", EPS, ids=["eps0", "eps0.1", "eps1"])
def test_soft_target_criterion_against_the_float64_definition(eps, use_w):
    """Six shapes per combination, 36 cases.  Measured on the MI355X (profiles/dense_loss_errors.txt, both kinds): worst loss error 0.012
    of its bound, worst gradient error 0.14 of its gate; the gates are those of tests/test_gpu_loss_options.py, unchanged."""
    _gate(0, SHAPES, eps, use_w, False)


@pytest.mark.parametrize("use_pw", [False, True], ids=["nopw", "pw"])
@pytest.mark.parametrize("use_w", [False, True], ids=["unweighted", "weighted"])
def test_bce_criterion_against_the_float64_definition(use_w, use_pw):
    """Seven shapes per combination, 28 cases, each with a logit of +100 (target 0) and one of -100 (target 1): loss and gradient finite
    (measure() asserts it) and within the same gates."""
    _gate(1, BCE_SHAPES, 0.0, use_w, use_pw)


def test_an_all_zero_row_has_no_term_and_no_gradient():
    logits, t, *_ = case(0, 8, 8, 0.0, False, False)
    assert bool((t[2] == 0).all())
    lg = logits.cuda().requires_grad_(True)
    P().HybridCrossEntropyLoss()(lg, t.cuda()).backward()
    assert torch.equal(lg.grad[2], torch.zeros(8, device="cuda")) and bool((lg.grad[1] != 0).any())


def _run(crit, logits, y):
    lg = logits.clone().requires_grad_(True)
    loss = crit(lg, y)
    (loss * DLOSS).backward()
    return loss.detach(), lg.grad


@pytest.mark.parametrize("shape", [(1, 2), (3, 5), (40, 5), (5, 64), (300, 8)], ids=lambda s: f"B{s[0]}C{s[1]}")
def test_one_hot_rows_are_the_plain_criterion_bitwise(shape):
    """Kind 0 without weight and smoothing on t = one_hot(y): the term is summed in class order from 0.f, so it adds exact zeros and multiplies
    by exact ones, and the divisor and the tree are the plain criterion's: the same bits, loss and gradient."""
    B, C = shape
    g = torch.Generator().manual_seed(31 * B + C)
    logits = (3.0 * torch.randn(B, C, generator=g)).cuda()
    y = torch.randint(0, C, (B,), generator=g).cuda()
    crit = P().HybridCrossEntropyLoss()
    l1, g1 = _run(crit, logits, F.one_hot(y, C).float())
    l0, g0 = _run(crit, logits, y)
    assert math.isfinite(float(l0)) and torch.equal(l1, l0) and torch.equal(g1, g0)
    assert torch.equal(P().dense_target(y, C), F.one_hot(y, C).float())


@pytest.mark.parametrize("kind", [0, 1], ids=["soft", "bce"])
def test_the_same_call_twice_gives_the_same_bits(kind):
    logits, t, w, pw, *_ = case(kind, 300, 8, 0.1 if kind == 0 else 0.0, True, kind == 1)
    crit = _criterion(kind, w, pw, 0.1 if kind == 0 else 0.0)
    l1, g1 = _run(crit, logits.cuda(), t.cuda())
    l2, g2 = _run(crit, logits.cuda(), t.cuda())
    assert math.isfinite(float(l1)) and torch.equal(l1, l2) and torch.equal(g1, g2)


def _dense_labels(kind, B, classes):
    g = torch.Generator().manual_seed(17 + B + kind)
    t = torch.rand(B, classes, generator=g)
    if kind == 0:
        t = t / t.sum(1, keepdim=True)
        t[0] = F.one_hot(torch.tensor(2), classes).float()
    else:
        t[0, 0], t[B - 1, classes - 1] = 0.0, 1.0
    return t.contiguous().cuda()


def _weighted_criterion(kind, classes):
    w = torch.linspace(0.5, 1.5, classes)
    w[3] = 0.0
    if kind == 1:
        return P().HybridBCEWithLogitsLoss(weight=w, pos_weight=torch.linspace(2.0, 0.5, classes)).cuda()
    return P().HybridCrossEntropyLoss(weight=w, label_smoothing=0.1).cuda()


def _want(kind, crit, logits, t):
    return dense_ref(kind, logits.detach().cpu().double(), t.cpu(), crit.weight.cpu(), crit.pos_weight.cpu() if kind == 1 else None,
                     0.1 if kind == 0 else 0.0)


@pytest.mark.parametrize("kind", [0, 1], ids=["soft", "bce"])
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(3, 5), (8, 16), (2, 1), (40, 4)], ids=["B3S5", "B8S16", "B2S1", "B40S4"])
def test_dense_loss_inside_the_temporal_launches_equals_the_separate_criterion_bitwise(mode, shape, kind):
    """hybrid::temporal_ce_dense against `criterion(model(x), t)` with the criterion's own two launches: loss, logits and every gradient bit
    for bit, with class weights (one of them zero) and smoothing / pos_weight.  B = 40 takes the fallback inside hyb_temporal_ce_dense_*."""
    B, S = shape
    torch.manual_seed(9)
    kw = dict(cnn_channels=(32, 64), d_model=64, num_heads=4, num_layers=2, hidden_dim=128, dropout=0.1, num_classes=5, compute_dtype=mode)
    a, b = P().TransformerCNNHybrid(**kw).cuda().train(), P().TransformerCNNHybrid(**kw).cuda().train()
    b.load_state_dict(a.state_dict())
    x = torch.rand(B, S, 3, 16, 16, device="cuda")
    t = _dense_labels(kind, B, 5)
    mask = (torch.rand(B, S, S, device="cuda") > 0.3).float()
    mask[:, :, 0] = 1
    crit = _weighted_criterion(kind, 5)
    o = ops()
    torch.manual_seed(11); o._SEED_COUNTER[0] = 100
    la = crit(a(x, mask), t)
    (la * DLOSS).backward()
    torch.manual_seed(11); o._SEED_COUNTER[0] = 100
    h, Bh = b.forward_backbone(x)
    lb, logits_b = b.forward_temporal_loss(h, Bh, t, mask, crit)
    (lb * DLOSS).backward()
    assert math.isfinite(float(la.detach())) and torch.equal(la.detach(), lb.detach())
    with torch.no_grad():
        torch.manual_seed(11); o._SEED_COUNTER[0] = 100
        assert torch.equal(a(x, mask), logits_b)
    for (n, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(pa.grad, pb.grad), n
    assert any(bool((p.grad != 0).any()) for p in b.parameters())
    want = _want(kind, crit, logits_b, t)
    assert abs(float(lb.detach()) - float(want)) <= 1e-5 * max(1.0, abs(float(want)))
    # the unfused path (one operator per stage, the criterion as its own launch) takes the dense target too: held to the definition on its own logits
    b.fuse_model_ops = False
    torch.manual_seed(11); o._SEED_COUNTER[0] = 100
    h, Bh = b.forward_backbone(x)
    lc, logits_c = b.forward_temporal_loss(h, Bh, t, mask, crit)
    want_c = _want(kind, crit, logits_c, t)
    assert math.isfinite(float(lc.detach())) and abs(float(lc.detach()) - float(want_c)) <= 1e-5 * max(1.0, abs(float(want_c)))
    # the ticket word behind the per-clip terms is back at zero in every scratch buffer in use
    torch.cuda.synchronize()
    for key, buf in o._CE_SCRATCH.items():
        assert int(buf[-1:].view(torch.int32).item()) == 0, key


@pytest.mark.parametrize("kind", [0, 1], ids=["soft", "bce"])
@pytest.mark.parametrize("mode", ["bf16", "mixed"])
def test_graphed_steps_with_a_dense_target_equal_eager_steps_bitwise(mode, kind):
    """The set-up of the existing graph tests with a dense target: the loss stays inside the captured temporal launches, K replays are K eager
    steps, a load() with a new target reaches the next replay without a recapture, so does an in-place update of weight (kind 0) / pos_weight
    (kind 1), a changed label_smoothing is refused, and targets of another form cannot be loaded (nor a dense one into a step built with
    class indices)."""
    K, WARM = 4, 2
    m1, x, y_idx = _setup(mode)
    m2, _, _ = _setup(mode)
    crit = _weighted_criterion(kind, 8)
    y = _dense_labels(kind, 3, 8)
    cur = [y]
    o1, o2 = P().HybridAdamW(m1.parameters(), lr=1e-3), P().HybridAdamW(m2.parameters(), lr=1e-3)
    mix = P().MixTarget(torch.tensor([0, 6, 1]).cuda(), torch.tensor([6, 1, 0]).cuda(), torch.tensor([0.7, 1.0, 0.25]).cuda())

    def eager_step():
        o1.zero_grad(set_to_none=True)
        loss = crit(m1(x), cur[0])
        loss.backward()
        o1.step()
        return loss.item()

    def same_parameters():
        for (n, a), (_, b) in zip(m1.named_parameters(), m2.named_parameters()):
            assert torch.equal(a, b), n
    eager_losses = [eager_step() for _ in range(WARM + K)]
    tr = P().GraphedTrainStep(m2, crit, o2, x, y, warmup=WARM)
    try:
        assert tr._fused_loss and tr.y.data_ptr() != y.data_ptr() and torch.equal(tr.y, y)
        graph_losses = [tr.step().item() for _ in range(K)]
        assert all(math.isfinite(v) for v in graph_losses)
        assert graph_losses == eager_losses[WARM:], (graph_losses, eager_losses)
        assert tr.steps_done() == WARM + K
        same_parameters()
        for (n, a), (_, b) in zip(m1.named_buffers(), m2.named_buffers()):
            assert torch.equal(a, b), n
        for pa, pb in zip(m1.parameters(), m2.parameters()):
            assert torch.equal(o1.state[pa]["exp_avg"], o2.state[pb]["exp_avg"])
            assert torch.equal(o1.state[pa]["exp_avg_sq"], o2.state[pb]["exp_avg_sq"])
        # a new dense target: read from device memory by the next replay
        cur[0] = _dense_labels(kind, 3, 8).flip(0).contiguous()
        tr.load(x, cur[0])
        want = eager_step()
        got = tr.step().item()
        assert got == want and got == crit(tr.logits, cur[0]).item() and got != crit(tr.logits, y).item()
        same_parameters()
        # an in-place update of the criterion's buffer reaches the next replay
        before = crit(tr.logits, cur[0]).item()
        with torch.no_grad():
            (crit.pos_weight if kind == 1 else crit.weight).mul_(1.5)
        want = eager_step()
        got = tr.step().item()
        assert got == want and got == crit(tr.logits, cur[0]).item() and crit(tr.logits, cur[0]).item() != before
        same_parameters()
        with pytest.raises(TypeError, match="dense target"):
            tr.load(x, y_idx)
        with pytest.raises(TypeError, match="dense target"):
            tr.load(x, mix)
        if kind == 0:
            crit.label_smoothing = 0.2
            with pytest.raises(RuntimeError, match="criterion's label_smoothing changed"):
                tr.step()
            crit.label_smoothing = 0.1
        tr.step()
    finally:
        tr.close()
    assert ops().step_counter() is None
    # the reverse: a step built with class indices refuses a dense target
    m3, x3, y3 = _setup(mode)
    tr = P().GraphedTrainStep(m3, P().HybridCrossEntropyLoss(), P().HybridAdamW(m3.parameters(), lr=1e-3), x3, y3, warmup=1)
    try:
        with pytest.raises(TypeError, match="dense target"):
            tr.load(x3, y)
    finally:
        tr.close()


def _opcheck(op, args, **kw):
    torch.library.opcheck(op, args, test_utils=OPCHECK_TESTS, **kw)


@pytest.mark.parametrize("dt", [0, 1], ids=["fp32", "bf16"])
def test_opcheck_dense_loss_operators(dt):
    o = ops()
    tdt = o.torch_dtype(dt)
    torch.manual_seed(6)
    w5 = torch.tensor([1.0, 0.0, 0.5, 2.0, 1.5], device="cuda")
    pw5 = torch.tensor([2.0, 1.0, 0.25, 1.0, 3.0], device="cuda")
    logits = torch.randn(4, 5, device="cuda", requires_grad=True)
    t = torch.rand(4, 5, device="cuda")
    combos = ((w5, None, 0, 0.1), (None, None, 0, 0.0), (w5, pw5, 1, 0.0), (None, None, 1, 0.0))
    if dt == 0:                                                    # (the stand-alone criterion has no dtype: once)
        for weight, pw, kind, eps in combos:
            _opcheck(torch.ops.hybrid.cross_entropy_dense.default, (logits, t, weight, pw, kind, eps))
            _opcheck(torch.ops.hybrid.cross_entropy_dense_bwd.default, (torch.ones((), device="cuda"), logits.detach(), t, weight, pw, kind, eps))
    B, S, D, Hid, L, H = 4, 8, 32, 64, 2, 2
    enc = P().TransformerEncoder(D, Hid, L, H, 0.1).cuda()
    params = [p.detach().clone().requires_grad_(True) for p in enc._flat_params()]
    h = torch.rand(B * S, 2, 3, 64, device="cuda").to(tdt).requires_grad_(True)
    tw = (torch.randn(D, 64, device="cuda") * 0.1).requires_grad_(True)
    tb = torch.randn(D, device="cuda").requires_grad_(True)
    hw = (torch.randn(5, D, device="cuda") * 0.1).requires_grad_(True)
    hb = torch.randn(5, device="cuda").requires_grad_(True)
    for weight, pw, kind, eps in combos[::2]:
        args_ce = (h, tw, tb, params, hw, hb, None, t, weight, pw, kind, eps, B, dt, Hid, L, H, 0.1, 0.1, 77)
        _opcheck(torch.ops.hybrid.temporal_ce_dense.default, args_ce)
        loss, logits2, feat, saved_blob, enc_out = torch.ops.hybrid.temporal_ce_dense(*args_ce)
        assert math.isfinite(float(loss.detach()))
        _opcheck(torch.ops.hybrid.temporal_ce_dense_bwd.default,
                 (torch.ones_like(loss).detach(), logits2.detach(), t, weight, pw, kind, eps, tw.detach(), [p.detach() for p in params],
                  hw.detach(), None, feat.detach(), saved_blob, enc_out.detach(), 2, 3, dt, Hid, L, H, 0.1, 0.1, 77))
    # the target and the weights get no gradient
    wg, pg, tg = w5.clone().requires_grad_(True), pw5.clone().requires_grad_(True), t.clone().requires_grad_(True)
    l = torch.ops.hybrid.cross_entropy_dense(logits, tg, wg, pg, 1, 0.0)
    gl, gw, gp, gt = torch.autograd.grad(l, [logits, wg, pg, tg], allow_unused=True)
    assert gw is None and gp is None and gt is None and gl is not None
    # the operators' own refusals
    with pytest.raises(ValueError, match="contiguous"):
        o.cross_entropy_dense(logits, torch.rand(5, 4, device="cuda").t())
    with pytest.raises(TypeError, match="float32"):
        o.cross_entropy_dense(logits, t.double())
    with pytest.raises(ValueError, match="pos_weight"):
        o.cross_entropy_dense(logits, t, None, pw5, 0, 0.0)
    with pytest.raises(ValueError, match="label_smoothing"):
        o.cross_entropy_dense(logits, t, None, None, 1, 0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        o.cross_entropy_dense(logits, t.cpu())
