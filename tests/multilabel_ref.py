"""Reference for hyb_eval_multilabel (include/hybrid_hip.h) and for MultiLabelMeter's average precision: a float64 torch / numpy restatement
of what one update adds to a multi-label meter -- scores, the loss terms for one and for several views, labels, predictions, the cells, the
NaN rule -- and the shared cases of tests/test_multilabel_cpu.py and tests/test_gpu_multilabel.py.  Not a test module.

Per video b with target row t [C], V views z_v [C], weights w, pw (ones when absent) and thresholds thr (fp32 values widened to float64):
    s_c    = (1 / V) sum_v sigmoid(z_vc)
    V == 1: term = sum_c w_c [ (1 - t_c) z_c + (1 + (pw_c - 1) t_c) (log1p(exp(-|z_c|)) + max(-z_c, 0)) ]          (BCE with logits)
    V > 1:  term = sum_c w_c [ pw_c t_c (-max(log s_c, -100)) + (1 - t_c) (-max(log1p(-s_c), -100)) ]              (BCE on the mean score)
    y_c    = t_c >= 0.5 (a NaN target: negative);   pred_c = s_c >= thr_c;   cells[c] = (tp, fp, fn)
    a NaN among the scores: counted, every pred 0 (positive labels become fn), never an exact match, bank score -inf
    loss   = sum_b term_b / (B C)
Average precision (scikit-learn's definition): for class c the distinct scores in descending order are the thresholds tau,
    P(tau) = TP(>= tau) / N(>= tau),  R(tau) = TP(>= tau) / P_c,  AP_c = sum_tau (R(tau) - R(previous tau)) P(tau);  NaN without a positive."""
import numpy as np
import torch

SCORE_TOL = 4 * 2.0 ** -23                                    # the project's gate for one fp32 sigmoid (exp, add, divide on values <= 1)


def multiview_score_tol(V):
    return (V + 3) * 2.0 ** -23


def multilabel_ref(logits, target, weight=None, pos_weight=None, threshold=0.5, views=1):
    """-> dict(num, counts [videos, nan videos, exact matches], cells [C, 3] int64, pred [B, C] uint8, labels [B, C] uint8, scores [B, C]
    float64, bank [B, C] float64 (the scores, -inf for a NaN video), terms [B] float64) for ONE update on zeroed state."""
    V = views
    B, C = target.shape
    assert logits.shape == (B * V, C)
    z = logits.double().reshape(B, V, C)
    t = target.double()
    w = torch.ones(C, dtype=torch.float64) if weight is None else weight.double()
    pw = torch.ones(C, dtype=torch.float64) if pos_weight is None else pos_weight.double()
    thr = torch.as_tensor(threshold, dtype=torch.float32).double().expand(C)
    s = torch.sigmoid(z).sum(1) / V
    if V == 1:
        z1 = z[:, 0]
        sp = torch.log1p(torch.exp(-z1.abs())) + torch.clamp(-z1, min=0.0)
        cell = w * ((1.0 - t) * z1 + (1.0 + (pw - 1.0) * t) * sp)
    else:
        cell = w * (pw * t * -torch.clamp(torch.log(s), min=-100.0) + (1.0 - t) * -torch.clamp(torch.log1p(-s), min=-100.0))
    terms = cell.sum(1)
    has_nan = torch.isnan(s).any(1)
    y = t >= 0.5
    pred = (s >= thr) & ~has_nan[:, None]
    cells = torch.stack([(pred & y).sum(0), (pred & ~y).sum(0), (~pred & y).sum(0)], 1).to(torch.int64)
    exact = ((pred == y).all(1) & ~has_nan)
    bank = torch.where(has_nan[:, None], torch.full_like(s, float("-inf")), s)
    return dict(num=terms.sum(), counts=[B, int(has_nan.sum()), int(exact.sum())], cells=cells, pred=pred.to(torch.uint8),
                labels=y.to(torch.uint8), scores=s, bank=bank, terms=terms, cell_terms=cell)


def loss_of(ref):
    B, C = ref["scores"].shape
    return float(ref["num"]) / (B * C)


def threshold_distance(ref, threshold):
    """The smallest |s - thr| over the (video, class) cells of a reference: the integer comparisons hang on its sign."""
    C = ref["scores"].shape[1]
    thr = torch.as_tensor(threshold, dtype=torch.float32).double().expand(C)
    return float((ref["scores"] - thr).abs().min())


def average_precision_ref(scores, labels):
    """float64 [C]: the definition above, class by class, with numpy on the host."""
    s, y = np.asarray(scores, dtype=np.float64), np.asarray(labels).astype(np.float64)
    out = np.full(s.shape[1], np.nan)
    for c in range(s.shape[1]):
        pos = y[:, c].sum()
        if pos == 0:
            continue
        ap, prev = 0.0, 0.0
        for tau in np.unique(s[:, c])[::-1]:
            at = s[:, c] >= tau
            tp = y[at, c].sum()
            ap += (tp / pos - prev) * (tp / at.sum())
            prev = tp / pos
        out[c] = ap
    return out


def average_precision_brute(scores, labels):
    """The same number from the O(N^2) form: every positive row i adds (1 / P_c) P(s_i) -- a tie group with k positives adds k / P_c times
    its precision, which is its recall step times its precision."""
    s, y = np.asarray(scores, dtype=np.float64), np.asarray(labels).astype(bool)
    N, C = s.shape
    out = np.full(C, np.nan)
    for c in range(C):
        pos = int(y[:, c].sum())
        if pos == 0:
            continue
        acc = 0.0
        for i in range(N):
            if y[i, c]:
                n = sum(1 for j in range(N) if s[j, c] >= s[i, c])
                tp = sum(1 for j in range(N) if s[j, c] >= s[i, c] and y[j, c])
                acc += tp / n
        out[c] = acc / pos
    return out


# ---- shared cases ---------------------------------------------------------------------------------------------------------------------
# one view: the grid of tests/eval_metrics_ref.py -- one video, a single class, a partial tree, exactly one pass of the thread loop, its
# second pass, a wide row
SHAPES = [(1, 1), (1, 2), (3, 5), (255, 8), (256, 8), (257, 8), (300, 8), (5, 64)]
OPTIONS = [(False, False), (True, False), (False, True), (True, True)]          # (weight, pos_weight)
OPTION_IDS = ["plain", "weight", "pos_weight", "both"]
THRESHOLDS = [0.5, float(np.float32(0.3))]                    # a scalar 0.5, and 0.3 as fp32 holds it
MULTIVIEW = [(2, 3, 5), (1, 2, 2), (130, 3, 8)]               # (B, V, C)


def _weights(C, g, weighted, pos_weighted):
    w = torch.rand(C, generator=g) + 0.25
    if C > 2:
        w[1] = 0.0                                            # one class weighs nothing
    pw = 2.0 * torch.rand(C, generator=g) + 0.5
    return (w if weighted else None), (pw if pos_weighted else None)


def case(B, C, weighted=False, pos_weighted=False):
    """(logits [B, C] fp32, target [B, C] fp32 multi-hot, weight or None, pos_weight or None) of one one-view case, on the CPU."""
    g = torch.Generator().manual_seed(7000 + 100 * B + C)
    logits = 3.0 * torch.randn(B, C, generator=g)
    target = (torch.rand(B, C, generator=g) < 0.35).float()
    return (logits, target) + _weights(C, g, weighted, pos_weighted)


def multiview_case(B, V, C, weighted=False, pos_weighted=False):
    """(logits [B * V, C], target [B, C], weight, pos_weight): the views of one video adjacent."""
    g = torch.Generator().manual_seed(9000 + 1000 * V + 100 * B + C)
    logits = (1.5 * torch.randn(B * V, C, generator=g)).clamp(-5.0, 5.0)
    target = (torch.rand(B, C, generator=g) < 0.35).float()
    return (logits, target) + _weights(C, g, weighted, pos_weighted)


# average precision: logits on the grid k / 4, k in [-24, 24], so that many scores tie EXACTLY; with several views every video's view v is
# its grid row plus a fixed offset, so equal grid rows give bit-equal fp32 scores and distinct ones stay far apart
AP_B, AP_C = 40, 5
AP_SPLITS = (13, 13, 14)
AP_VIEW_OFFSETS = (0.0, 1.0 / 8, -1.0 / 16)


def ap_case(V):
    """(logits [AP_B * V, AP_C] fp32, target [AP_B, AP_C] fp32): every class has positives and negatives."""
    g = torch.Generator().manual_seed(11000 + V)
    base = torch.randint(-24, 25, (AP_B, AP_C), generator=g).float() / 4.0
    target = (torch.rand(AP_B, AP_C, generator=g) < 0.4).float()
    target[0], target[1] = 1.0, 0.0
    off = torch.tensor(AP_VIEW_OFFSETS[:V]).reshape(1, V, 1)
    return (base[:, None, :] + off).reshape(AP_B * V, AP_C).contiguous(), target


def min_distinct_gap(scores):
    """The smallest gap between two DISTINCT values of a class's scores, over the classes."""
    s = np.asarray(scores, dtype=np.float64)
    gaps = [np.diff(np.unique(s[:, c])) for c in range(s.shape[1])]
    return min(float(d.min()) for d in gaps if d.size)
