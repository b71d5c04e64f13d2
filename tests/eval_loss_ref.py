"""References for the validation loss under the focal, soft-target and asymmetric criteria (hyb_eval_metrics_focal, hyb_eval_metrics_soft,
hyb_eval_multilabel_asym; include/hybrid_hip.h states the six rules): a torch restatement in ``dtype`` -- float64 as the reference, float32
on the CPU as the arbiter of the several-view gate, as tests/eval_metrics_ref.py does.  Built on tests/focal_ref.py, tests/dense_ref.py,
tests/eval_metrics_ref.py and tests/multilabel_ref.py, whose cases the tests share.  Not a test module.

Per video b with V views z_v [C], pbar = (1 / V) sum_v softmax(z_v), s_c = (1 / V) sum_v sigmoid(z_vc), qbar_c = (1 / V) sum_v sigmoid(-z_vc):
    focal, V == 1:  term = keep w[y] u^gamma (lse - z_y),  u = sum_{c != y} softmax(z)_c;          den share keep w[y]
    focal, V > 1:   term = keep w[y] ubar^gamma (-log pbar_y),  ubar = sum_{c != y} pbar_c;        the same den share
    soft,  V == 1:  term = sum_c w_c q_c (lse - z_c),  q_c = (1 - e) t_c + e / C;                  den share 1
    soft,  V > 1:   term = sum_c w_c q_c (-log pbar_c);                                            den share 1
    soft label:     the lowest index among the maxima of t; -1 for a row that holds a NaN
    asym,  V == 1:  term = sum_c cell_c, focal_ref.asym_ref's cell on (z, t)
    asym,  V > 1:   the same cell with p -> s_c, q -> qbar_c, logp = max(log s_c, -100),
                    logn = max(log qbar_c, -100) if clip == 0 else log(min(qbar_c + clip, 1))
    loss = num / den  (asymmetric: den = videos * C, what MultiLabelMeter.compute() divides by)"""
import torch

from focal_ref import _pow


def _views(logits, B, V, dtype):
    C = logits.shape[1]
    assert logits.shape[0] == B * V
    return logits.to(dtype).reshape(B, V, C)


def _vector(v, C, dtype):
    return torch.ones(C, dtype=dtype) if v is None else v.to(dtype)


def _sigmoids(z):
    """(sigmoid(z), sigmoid(-z)) in the overflow-safe form of the kernels: each its own quotient, neither formed as 1 - the other."""
    ez = torch.exp(-z.abs())
    one = torch.ones_like(z)
    return torch.where(z >= 0, one, ez) / (1 + ez), torch.where(z >= 0, ez, one) / (1 + ez)


def _result(terms, shares):
    return dict(num=terms.double().sum(), den=shares.double().sum(), terms=terms)


def loss_of(ref):
    return float(ref["num"] / ref["den"])


def focal_eval_ref(logits, target, gamma, weight=None, ignore_index=None, views=1, dtype=torch.float64):
    """-> dict(num, den, terms [B]) of one update.  Targets are in range (the out-of-range rule is eval_metrics_ref's)."""
    B, C = target.shape[0], logits.shape[1]
    z = _views(logits, B, views, dtype)
    w = _vector(weight, C, dtype)
    keep = torch.ones(B, dtype=torch.bool) if ignore_index is None else target != ignore_index
    y = torch.where(keep, target, torch.zeros_like(target))
    rows = torch.arange(B)
    hot = torch.nn.functional.one_hot(y, C).bool()
    if views == 1:
        p = torch.softmax(z[:, 0], 1)
        nl = torch.logsumexp(z[:, 0], 1) - z[:, 0][rows, y]
    else:
        p = torch.softmax(z, -1).sum(1) / views
        nl = -torch.log(p[rows, y])
    u = p.masked_fill(hot, 0.0).sum(1)
    zero = torch.zeros(B, dtype=dtype)
    terms = torch.where(keep, _pow(u, gamma) * (w[y] * nl), zero)
    return _result(terms, torch.where(keep, w[y], zero))


def soft_label(target):
    """int64 [B]: the lowest index among the maxima of every row; -1 for a row that holds a NaN."""
    B, C = target.shape
    idx = torch.arange(C)[None, :]
    mx = target.max(1, keepdim=True).values
    label = torch.where(target == mx, idx, torch.full_like(idx, C)).min(1).values
    return torch.where(torch.isnan(target).any(1), torch.full_like(label, -1), label)


def soft_eval_ref(logits, target, label_smoothing=0.0, weight=None, views=1, dtype=torch.float64):
    """-> dict(num, den, terms [B], labels [B]) of one update: every video kept, den = B."""
    B, C = target.shape
    z = _views(logits, B, views, dtype)
    w = _vector(weight, C, dtype)
    q = (1 - label_smoothing) * target.to(dtype) + label_smoothing / C
    if views == 1:
        nl = torch.logsumexp(z[:, 0], 1, keepdim=True) - z[:, 0]
    else:
        nl = -torch.log(torch.softmax(z, -1).sum(1) / views)
    out = _result((w * q * nl).sum(1), torch.ones(B, dtype=dtype))
    out["labels"] = soft_label(target)
    return out


def asym_eval_ref(logits, target, gamma_pos, gamma_neg, clip, weight=None, pos_weight=None, views=1, dtype=torch.float64):
    """-> dict(num, den = B C, terms [B], scores [B, C]) of one update."""
    B, C = target.shape
    z = _views(logits, B, views, dtype)
    w, pw = _vector(weight, C, dtype), _vector(pos_weight, C, dtype)
    t = target.to(dtype)
    p, q = _sigmoids(z)
    if views == 1:
        z1 = z[:, 0]
        p, q = p[:, 0], q[:, 0]
        l1 = torch.log1p(torch.exp(-z1.abs()))
        logp = -(l1 + torch.clamp(-z1, min=0))
        logn = -(l1 + torch.clamp(z1, min=0)) if clip == 0 else torch.log(torch.clamp(q + clip, max=1))
    else:
        p, q = p.sum(1) / views, q.sum(1) / views
        logp = torch.clamp(torch.log(p), min=-100.0)
        logn = torch.clamp(torch.log(q), min=-100.0) if clip == 0 else torch.log(torch.clamp(q + clip, max=1))
    r = torch.clamp(p - clip, min=0)
    base = t * q + (1 - t) * r
    gt = gamma_pos * t + gamma_neg * (1 - t)
    L = 1 + (pw - 1) * t
    cell = -w * L * _pow(base, gt) * (t * logp + (1 - t) * logn)
    out = _result(cell.sum(1), torch.full((B,), float(C), dtype=dtype))
    out["scores"] = p
    return out


def tree_sum(values):
    """The double sum of up to 256 per-video numbers in the order of the kernels' fixed 256-leaf tree (leaf t holds video t)."""
    leaves = [float(v) for v in values] + [0.0] * (256 - len(values))
    h = 128
    while h:
        for i in range(h):
            leaves[i] += leaves[i + h]
        h //= 2
    return leaves[0]
