"""On-device evaluation on the GPU: hyb_eval_metrics through hybrid::eval_metrics_, ClassificationMeter, TransformerCNNHybrid.evaluate and
GraphedEval, held to tests/eval_metrics_ref.py (float64; tests/test_eval_metrics_cpu.py pins that reference to torch and to the tie rule).

Integer results (counts, confusion matrix, predictions) are compared exactly.  The one-view loss has the gate of test_gpu_loss_options.py
for this arithmetic, |loss - l64| <= 1e-5 max(1, |l64|).  With several views the scores must be within 4 * 2^-23 of the float64 mean
softmax (one rounding each for exp, divide, add and scale, on values <= 1) and the loss within 4 |l32 - l64| + 1e-6 max(1, |l64|), l32 being
the same formula in fp32 torch on the CPU (the arbiter pattern of test_gpu_loss_options.py).  Every figure is printed before it is asserted
(pytest -s); scripts/eval_metrics_errors.py writes the worst per option combination to profiles/eval_metrics_errors.txt from measure_*()."""
import math

import pytest
import torch

from eval_metrics_ref import (MULTIVIEW, OPTION_IDS, OPTIONS, SHAPES, case, eval_metrics_ref, loss_of, multiview_left_out, topks)

pytestmark = pytest.mark.gpu

OPCHECK_TESTS = ("test_schema", "test_autograd_registration", "test_faketensor", "test_aot_dispatch_static")
KW = dict(cnn_channels=(32, 64), d_model=64, num_heads=4, num_layers=2, hidden_dim=128)      # tests/test_gpu_graph.py
SCORE_TOL = 4 * 2.0 ** -23


def P():
    import transformer_cnn_hybrid_network_for_video_processing_amd as pkg
    return pkg


def _criterion(w, ign, eps):
    if w is None and ign is None and eps == 0.0:
        return None
    return P().HybridCrossEntropyLoss(weight=w, ignore_index=ign, label_smoothing=eps).cuda()


def _meter(C, topk, w=None, ign=None, eps=0.0, confusion=True):
    return P().ClassificationMeter(C, topk=topk, confusion=confusion, criterion=_criterion(w, ign, eps))


def _state(m):
    torch.cuda.synchronize()
    return m.sums.cpu(), m.counts.cpu(), None if m.confusion is None else m.confusion.cpu()


def _loss(sums):
    return float(sums[0] / sums[1])


# ---- one view: counts exactly, loss against float64 -----------------------------------------------------------------------------------
def measure_one_view(opt, check=None):
    """Every (B, C) of SHAPES and every topk under one option combination -> [(B, C, loss error, its bound)]; `check` gets each case's
    integer results next to the reference's."""
    weighted, ign, eps = opt
    rows = []
    for B, C in SHAPES:
        logits, y, w = case(B, C, weighted, ign)
        for k in topks(C):
            ref = eval_metrics_ref(logits, y, w, ign, eps, topk=k)
            m = _meter(C, k, w, ign, eps)
            pred = m.update(logits.cuda(), y.cuda())
            sums, counts, conf = _state(m)
            l64 = loss_of(ref)
            err, bound = abs(_loss(sums) - l64), 1e-5 * max(1.0, abs(l64))
            print(f"B={B} C={C} topk={k} weighted={weighted} ignore={ign} eps={eps}: counts {counts.tolist()} loss {_loss(sums):.7f} "
                  f"err {err:.3e} (<= {bound:.1e})")
            if check is not None:
                check(B, C, k, ref, counts, conf, pred.cpu())
            rows.append((B, C, err, bound))
    return rows


@pytest.mark.parametrize("opt", OPTIONS, ids=OPTION_IDS)
def test_one_view_counts_exactly_and_loss_against_float64(opt):
    """Measured on the MI355X: profiles/eval_metrics_errors.txt."""
    def check(B, C, k, ref, counts, conf, pred):
        assert counts.tolist() == ref["counts"], (B, C, k)
        assert torch.equal(conf, ref["confusion"]), (B, C, k)
        assert torch.equal(pred, ref["pred"]), (B, C, k)
    rows = measure_one_view(opt, check)
    assert all(math.isfinite(err) for _, _, err, _ in rows)
    bad = [r for r in rows if not r[2] <= r[3]]
    assert not bad, bad


@pytest.mark.parametrize("kw", [dict(), dict(ign=3), dict(eps=0.1), dict(ign=3, eps=0.1)], ids=["plain", "ignore3", "eps0.1", "ignore3+eps0.1"])
def test_single_video_updates_carry_the_criterions_bits(kw):
    """weight=None and one video per update: den is 1, the term is the criterion's own function and each launch makes one double add, so
    sums[0] is exactly the running double sum of hybrid::cross_entropy_opts on that row, and sums[1] the running count."""
    from transformer_cnn_hybrid_network_for_video_processing_amd import ops
    ign, eps = kw.get("ign"), kw.get("eps", 0.0)
    g = torch.Generator().manual_seed(21)
    logits = (3.0 * torch.randn(12, 8, generator=g)).cuda()
    y = torch.randint(0, 8, (12,), generator=g)
    y[0], y[5] = 0, 3
    m = _meter(8, 2, None, ign, eps)
    if m.criterion is None:                                     # the plain case through explicit defaults as well
        m = P().ClassificationMeter(8, topk=2, criterion=P().HybridCrossEntropyLoss().cuda())
    num, den = 0.0, 0.0
    for b in range(12):
        m.update(logits[b:b + 1], y[b:b + 1].cuda())
        if ign is None or int(y[b]) != ign:
            num += float(ops.cross_entropy_opts(logits[b:b + 1], y[b:b + 1].cuda(), None, ign, eps))
            den += 1.0
        sums, counts, _ = _state(m)
        assert sums.tolist() == [num, den], (b, sums.tolist(), num, den)
        assert counts[0] == b + 1 and counts[1] == den


def test_updates_accumulate_and_are_reproducible_bit_for_bit():
    C = 8
    g = torch.Generator().manual_seed(33)
    w = torch.rand(C, generator=g) + 0.25
    w[1] = 0.0
    chunks = [(3.0 * torch.randn(n, C, generator=g), torch.randint(0, C, (n,), generator=g)) for n in (7, 1, 257)]
    chunks[0][1][0] = 0
    runs = []
    for _ in range(2):
        m = _meter(C, 3, w, 2, 0.1)
        preds = [m.update(lg.cuda(), y.cuda()) for lg, y in chunks]
        runs.append(_state(m) + (torch.cat(preds).cpu(),))
    ref = eval_metrics_ref(torch.cat([c[0] for c in chunks]), torch.cat([c[1] for c in chunks]), w, 2, 0.1, topk=3)
    sums, counts, conf, pred = runs[0]
    assert counts.tolist() == ref["counts"] and torch.equal(conf, ref["confusion"]) and torch.equal(pred, ref["pred"])
    l64 = loss_of(ref)
    print(f"three updates (7, 1, 257): loss {_loss(sums):.7f}, float64 {l64:.7f}, err {abs(_loss(sums) - l64):.3e}")
    assert abs(_loss(sums) - l64) <= 1e-5 * max(1.0, abs(l64))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])
    # reset() zeroes in place, and the meter starts again
    m.reset()
    assert all(int((t != 0).sum()) == 0 for t in _state(m))
    m.update(chunks[0][0].cuda(), chunks[0][1].cuda())
    assert _state(m)[1].tolist() == eval_metrics_ref(*chunks[0], w, 2, 0.1, topk=3)["counts"]


# ---- edges ----------------------------------------------------------------------------------------------------------------------------
def _against_ref(logits, y, topk, w=None, ign=None, eps=0.0, views=1):
    ref = eval_metrics_ref(logits, y, w, ign, eps, topk=topk, views=views)
    m = _meter(logits.shape[1], topk, w, ign, eps)
    out = m.update(logits.cuda(), y.cuda(), views)
    sums, counts, conf = _state(m)
    pred = (out[0] if views > 1 else out).cpu()
    assert counts.tolist() == ref["counts"] and torch.equal(conf, ref["confusion"]) and torch.equal(pred, ref["pred"]), (counts, ref["counts"], pred)
    return ref, sums, m


def test_exact_ties_follow_the_rank_rule():
    logits = torch.tensor([[2.0, 5.0, 5.0, 1.0], [2.0, 5.0, 5.0, 1.0], [3.0, 3.0, 3.0, 3.0], [3.0, 3.0, 3.0, 3.0], [0.0, 4.0, 0.0, 4.0],
                           [7.0, 1.0, 1.0, 1.0]])
    y = torch.tensor([1, 2, 0, 3, 2, 2])
    for k in (1, 2, 3, 4):
        ref, _, _ = _against_ref(logits, y, k)
    assert ref["pred"].tolist() == [1, 1, 0, 0, 1, 0]
    ref, _, _ = _against_ref(logits, y, 2)
    assert ref["counts"] == [6, 6, 2, 3, 0]
    _against_ref(logits.repeat_interleave(2, 0), y, 2, views=2)                  # identical views: the averaged scores tie exactly too


def test_every_target_ignored():
    logits = 3.0 * torch.randn(5, 4, generator=torch.Generator().manual_seed(2))
    ref, sums, m = _against_ref(logits, torch.full((5,), -100), 2, ign=-100, eps=0.1)
    assert ref["counts"] == [5, 0, 0, 0, 0] and sums.tolist() == [0.0, 0.0]
    out = m.compute()
    assert out["videos"] == 5 and out["kept"] == 0 and all(math.isnan(out[k]) for k in ("loss", "top1", "topk", "mean_class_accuracy"))


@pytest.mark.parametrize("bad", [-1, 4], ids=["minus1", "C"])
def test_out_of_range_kept_target_poisons_the_sums_and_touches_nothing(bad):
    C = 4
    logits = (3.0 * torch.randn(3, C, generator=torch.Generator().manual_seed(4))).cuda()
    y = torch.tensor([0, bad, 1]).cuda()
    wbig = torch.full((C + 2,), 7.5, device="cuda")
    wbig[1:-1] = torch.tensor([1.0, 2.0, 0.5, 1.0], device="cuda")
    cbig = torch.full((C * C + 2,), 77, dtype=torch.int64, device="cuda")
    conf = cbig[1:-1].view(C, C).zero_()
    sums = torch.zeros(2, dtype=torch.float64, device="cuda")
    counts = torch.zeros(5, dtype=torch.int64, device="cuda")
    pred, _ = torch.ops.hybrid.eval_metrics_(logits, y, wbig[1:-1], 0, False, 0.1, 2, 1, sums, counts, conf)
    torch.cuda.synchronize()
    ref = eval_metrics_ref(logits.cpu(), y.cpu(), wbig[1:-1].cpu(), None, 0.1, topk=2)
    assert math.isnan(float(sums[0])) and math.isnan(float(sums[1]))
    assert counts.tolist() == ref["counts"] and counts[1] == 3 and counts[2] <= 2 and counts[3] <= 2        # kept, and wrong
    assert torch.equal(conf.cpu(), ref["confusion"]) and int(conf.sum()) == 2
    assert cbig[0] == 77 and cbig[-1] == 77 and wbig[0] == 7.5 and wbig[-1] == 7.5
    assert torch.equal(wbig[1:-1].cpu(), torch.tensor([1.0, 2.0, 0.5, 1.0]))
    assert torch.equal(pred.cpu(), ref["pred"])


def test_nan_row_and_minus_infinity_row():
    inf = float("inf")
    logits = torch.tensor([[1.0, 2.0, 3.0, 0.0], [float("nan"), 0.0, 1.0, 2.0], [-inf, -inf, 2.0, -inf], [0.5, 1.0, 0.0, -1.0],
                           [1.0, float("nan"), 0.0, 0.0]])
    ref, sums, m = _against_ref(logits, torch.tensor([2, 3, 2, 1, 3]), 2, ign=3)
    assert ref["counts"] == [5, 3, 3, 3, 0] and ref["pred"].tolist() == [2, -1, 2, 1, -1]                 # the NaN rows are ignored videos here
    assert float(sums[1]) == 3.0 and abs(float(sums[0]) - float(ref["num"])) <= 1e-5
    ref, sums, m = _against_ref(logits, torch.tensor([2, 1, 2, 1, 0]), 2)
    assert ref["counts"] == [5, 5, 3, 3, 2] and math.isnan(float(sums[0])) and float(sums[1]) == 5.0
    out = m.compute()
    assert out["nan_rows"] == 2 and out["top1"] == 0.6 and math.isnan(out["loss"])
    # all -inf except one class: right when that class is the target (term 0), wrong otherwise (term +inf)
    ref, sums, _ = _against_ref(logits[2:4], torch.tensor([2, 1]), 1)
    assert ref["counts"] == [2, 2, 2, 2, 0] and abs(float(sums[0]) - float(ref["num"])) <= 1e-5
    ref, sums, _ = _against_ref(logits[2:3], torch.tensor([0]), 2)
    assert ref["counts"] == [1, 1, 0, 1, 0] and float(sums[0]) == inf and float(ref["num"]) == inf      # rank 1: only the finite class scores higher


# ---- several views ----------------------------------------------------------------------------------------------------------------------
def measure_multiview(shape, opt):
    """-> (score error, loss error, loss gate, arbiter's error, videos left out) of one (B, V, C) case under one option combination."""
    B, V, C = shape
    weighted, ign, eps = opt
    logits, y, w = case(B, C, weighted, ign, V)
    ref = eval_metrics_ref(logits, y, w, ign, eps, topk=min(2, C), views=V)
    l64 = loss_of(ref)
    arb = abs(loss_of(eval_metrics_ref(logits, y, w, ign, eps, topk=min(2, C), views=V, dtype=torch.float32)) - l64)
    m = _meter(C, min(2, C), w, ign, eps)
    pred, scores = m.update(logits.cuda(), y.cuda(), V)
    sums, counts, conf = _state(m)
    serr = float((scores.cpu().double() - ref["scores"]).abs().max())
    lerr, gate = abs(_loss(sums) - l64), 4.0 * arb + 1e-6 * max(1.0, abs(l64))
    left = multiview_left_out(B, V, C)
    print(f"B={B} V={V} C={C} weighted={weighted} ignore={ign} eps={eps}: score err {serr:.3e} (<= {SCORE_TOL:.3e})  loss {_loss(sums):.7f} "
          f"err {lerr:.3e} (<= {gate:.3e}, arbiter {arb:.3e})  left out {int(left.sum())}")
    assert tuple(scores.shape) == (B, C) and math.isfinite(l64)
    # integer results: the videos the CPU margin test leaves out are taken out of the batch, and the rest compared exactly
    keepv = ~left
    if bool(left.any()):
        sub = logits.reshape(B, V, C)[keepv].reshape(-1, C)
        ref_i = eval_metrics_ref(sub, y[keepv], w, ign, eps, topk=min(2, C), views=V)
        mi = _meter(C, min(2, C), w, ign, eps)
        pred_i = mi.update(sub.cuda(), y[keepv].cuda(), V)[0]
        _, counts, conf = _state(mi)
    else:
        ref_i, pred_i = ref, pred
    assert counts.tolist() == ref_i["counts"] and torch.equal(conf, ref_i["confusion"]) and torch.equal(pred_i.cpu(), ref_i["pred"])
    return serr, lerr, gate, arb, int(left.sum())


@pytest.mark.parametrize("opt", [OPTIONS[0], OPTIONS[-1]], ids=[OPTION_IDS[0], OPTION_IDS[-1]])
@pytest.mark.parametrize("shape", MULTIVIEW, ids=[f"B{b}V{v}C{c}" for b, v, c in MULTIVIEW])
def test_several_views_scores_loss_and_counts(shape, opt):
    """Measured on the MI355X: profiles/eval_metrics_errors.txt."""
    serr, lerr, gate, _, _ = measure_multiview(shape, opt)
    assert serr <= SCORE_TOL
    assert lerr <= gate


# ---- model and graph --------------------------------------------------------------------------------------------------------------------
def _model(mode="bf16", seed=0):
    torch.manual_seed(seed)
    return P().TransformerCNNHybrid(dropout=0.0, compute_dtype=mode, **KW).cuda().eval()


def _batches(n, B=4, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(B, 4, 3, 32, 32, generator=g).cuda(), torch.randint(0, 8, (B,), generator=g).cuda()) for _ in range(n)]


def _option_criterion():
    w = torch.linspace(0.5, 1.5, 8)
    w[3] = 0.0
    return P().HybridCrossEntropyLoss(weight=w, ignore_index=1, label_smoothing=0.1).cuda()


def _same(a, b):
    sa, sb = _state(a), _state(b)
    return all(torch.equal(x, y) for x, y in zip(sa, sb))


def test_evaluate_returns_predicts_logits_and_updates_the_meter():
    m = _model()
    (x, y), = _batches(1)
    meter = P().ClassificationMeter(8, topk=5)
    logits = m.evaluate(x, y, meter)
    assert torch.equal(logits, m.predict(x))
    ref = eval_metrics_ref(logits.cpu(), y.cpu(), topk=5)
    sums, counts, conf = _state(meter)
    assert counts.tolist() == ref["counts"] and torch.equal(conf, ref["confusion"])
    assert abs(_loss(sums) - loss_of(ref)) <= 1e-5 * max(1.0, abs(loss_of(ref)))
    # two views per video: the same four clips as two videos
    meter2 = P().ClassificationMeter(8, topk=5)
    assert torch.equal(m.evaluate(x, y[:2], meter2, views=2), logits)
    assert _state(meter2)[1][0] == 2
    with pytest.raises(ValueError):
        m.evaluate(x, y[:3], meter2, views=2)


@pytest.mark.parametrize("mode", ["bf16", "mixed"])
def test_graphed_eval_replays_equal_eager_evaluate(mode):
    K = 3
    m = _model(mode)
    batches = _batches(K + 2)
    crit = _option_criterion()
    mg, me = P().ClassificationMeter(8, topk=3, criterion=crit), P().ClassificationMeter(8, topk=3, criterion=crit)
    mg.update(torch.randn(4, 8, device="cuda"), batches[0][1])                   # whatever the meter held goes with the warm-up
    ge = P().GraphedEval(m, *batches[0], mg, warmup=2)
    gp = P().GraphedPredict(m, batches[0][0])
    try:
        assert all(int((t != 0).sum()) == 0 for t in _state(mg))                   # a freshly built GraphedEval leaves the meter zeroed
        for x, y in batches[:K]:
            got = ge(x, y).clone()
            assert torch.equal(got, gp(x)) and torch.equal(got, m.evaluate(x, y, me))
        assert _same(mg, me) and int(_state(mg)[1][0]) == 4 * K
        # the class weights are read when the replay runs
        stale = P().ClassificationMeter(8, topk=3, criterion=P().HybridCrossEntropyLoss(weight=crit.weight.clone(), ignore_index=1,
                                                                                       label_smoothing=0.1).cuda())
        stale.merge(mg)
        with torch.no_grad():
            crit.weight[0] *= 4.0
            crit.weight[6] *= 0.25
        x, y = batches[K]
        ge(x, y)
        m.evaluate(x, y, me)
        m.evaluate(x, y, stale)
        assert _same(mg, me) and not torch.equal(_state(mg)[0], _state(stale)[0])
        # by-value options cannot change under a captured launch
        crit.label_smoothing = 0.2
        with pytest.raises(RuntimeError, match="criterion's label_smoothing changed"):
            ge(x, y)
        crit.label_smoothing = 0.1
        crit.ignore_index = 2
        with pytest.raises(RuntimeError, match="criterion's ignore_index changed"):
            ge(x, y)
        crit.ignore_index = 1
        ge(*batches[K + 1])
        m.evaluate(*batches[K + 1], me)
        assert _same(mg, me)
        out = mg.compute()
        assert out["videos"] == 4 * (K + 2) and math.isfinite(out["loss"])
        with pytest.raises(ValueError):
            ge(torch.rand(4, 5, 3, 32, 32).cuda(), y)
    finally:
        ge.close()
        gp.close()
    with pytest.raises(RuntimeError, match="closed"):
        ge(*batches[0])


def test_meter_state_cannot_be_born_or_reset_under_capture():
    meter = P().ClassificationMeter(8, topk=2)
    cap = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    errors, buf = [], torch.zeros(1, device="cuda")
    with torch.cuda.graph(g, stream=cap):
        buf.add_(1)
        for fn in (lambda: P().ClassificationMeter(8, topk=2), meter.reset):
            try:
                fn()
            except RuntimeError as e:
                errors.append(str(e))
    assert len(errors) == 2 and "under stream capture" in errors[0] and "under stream capture" in errors[1]


def test_ema_twin_evaluates():
    torch.manual_seed(0)
    m = P().TransformerCNNHybrid(dropout=0.0, **KW).cuda().train()
    for a in m.encoder.attention_layers:
        a.dropoutLayer.p = 0.0
    batches = _batches(3, B=2)
    crit = P().HybridCrossEntropyLoss()
    opt = P().HybridAdamW(m.parameters(), lr=1e-2, ema_decay=0.5)
    for x, y in batches[:2]:
        opt.zero_grad(set_to_none=True)
        crit(m(x), y).backward()
        opt.step()
    twin = opt.ema_model(m)
    me, mg = P().ClassificationMeter(8), P().ClassificationMeter(8)
    x, y = batches[2]
    logits = twin.evaluate(x, y, me)
    assert torch.equal(logits, twin.predict(x)) and not torch.equal(logits, m.predict(x))
    ge = P().GraphedEval(twin, x, y, mg, warmup=1)
    try:
        assert torch.equal(ge(x, y), logits)
    finally:
        ge.close()
    assert _same(me, mg) and me.compute()["videos"] == 2


# ---- operator ---------------------------------------------------------------------------------------------------------------------------
def test_opcheck_eval_metrics():
    torch.manual_seed(6)
    w5 = torch.tensor([1.0, 0.0, 0.5, 2.0, 1.5], device="cuda")
    logits = torch.randn(8, 5, device="cuda")
    tgt = torch.tensor([0, 4, 2, 1, 3, 3, 2, 0], device="cuda")

    def state(conf=True):
        return (torch.zeros(2, dtype=torch.float64, device="cuda"), torch.zeros(5, dtype=torch.int64, device="cuda"),
                torch.zeros(5, 5, dtype=torch.int64, device="cuda") if conf else None)
    op = torch.ops.hybrid.eval_metrics_.default
    torch.library.opcheck(op, (logits, tgt, w5, 2, True, 0.1, 2, 1, *state()), test_utils=OPCHECK_TESTS)
    torch.library.opcheck(op, (logits, tgt[:4], None, 0, False, 0.0, 1, 2, *state(False)), test_utils=OPCHECK_TESTS)
    with pytest.raises(ValueError, match="topk"):
        op(logits, tgt, None, 0, False, 0.0, 6, 1, *state())
    with pytest.raises(ValueError, match="class indices"):
        op(logits, tgt[:3], None, 0, False, 0.0, 1, 2, *state())
    with pytest.raises(ValueError, match="float32"):
        op(logits.double(), tgt, None, 0, False, 0.0, 1, 1, *state())
    with pytest.raises(ValueError, match="sums"):
        op(logits, tgt, None, 0, False, 0.0, 1, 1, torch.zeros(2, device="cuda"), *state()[1:])
    lg = logits.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="no autograd formula"):
        op(lg, tgt, None, 0, False, 0.0, 1, 1, *state())
