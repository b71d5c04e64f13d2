"""Reference for hyb_eval_metrics (include/hybrid_hip.h): a torch restatement, float64 by default, of what one update adds to a
classification meter -- the loss terms for one and for several views, the prediction, the rank rule, the NaN rule and the counts -- and
the shared cases of tests/test_eval_metrics_cpu.py and tests/test_gpu_eval_metrics.py.  Not a test module.

Per video b with target y, V views z_v [C] and scores s:
    V == 1: s = z;            nl_c = logsumexp(z) - z_c
    V > 1:  s = pbar = (1 / V) sum_v softmax(z_v);   nl_c = -log pbar_c
    term = keep [ (1 - e) w[y] nl_y + (e / C) sum_c w[c] nl_c ]      (the smoothing sum only when e > 0),   den share = keep w[y]
    pred = lowest index among the maxima of s;  rank = #{c : s_c > s_y} + #{c < y : s_c == s_y};  top-k correct iff rank < k
    a NaN in s: pred = -1, wrong, no confusion entry, counted (when kept) in counts[4]
    ignored (y == ignore_index): counted in counts[0] only;  kept y outside [0, C): NaN term and den share, kept, wrong, no confusion entry
Comparisons run on the scores in `dtype`; float64 holds every fp32 logit exactly, so for V == 1 they are the kernel's comparisons."""
import torch


def eval_metrics_ref(logits, target, weight=None, ignore_index=None, label_smoothing=0.0, topk=1, views=1, dtype=torch.float64):
    """-> dict(num, den, counts [5] list, confusion [C, C] int64, pred [B] int64, rank [B] int64 (-1 where there is none), scores [B, C],
    terms [B]) for ONE update on zeroed state; sum the integer entries (and num / den) over updates."""
    V = views
    C = logits.shape[1]
    B = target.shape[0]
    assert logits.shape[0] == B * V
    z = logits.to(dtype).reshape(B, V, C)
    if V == 1:
        s = z[:, 0]
        nl = torch.logsumexp(s, 1, keepdim=True) - s
    else:
        s = torch.softmax(z, -1).sum(1) / V
        nl = -torch.log(s)
    w = torch.ones(C, dtype=dtype) if weight is None else weight.to(dtype)
    keep = torch.ones(B, dtype=torch.bool) if ignore_index is None else target != ignore_index
    inrange = (target >= 0) & (target < C)
    tc = target.clamp(0, C - 1)
    rows = torch.arange(B)
    term = (1.0 - label_smoothing) * (w[tc] * nl[rows, tc])
    if label_smoothing > 0.0:
        term = term + (label_smoothing / C) * (w[None, :] * nl).sum(1)
    nan = torch.full((B,), float("nan"), dtype=dtype)
    zero = torch.zeros(B, dtype=dtype)
    term = torch.where(keep, torch.where(inrange, term, nan), zero)
    share = torch.where(keep, torch.where(inrange, w[tc], nan), zero)
    has_nan = torch.isnan(s).any(1)
    idx = torch.arange(C)[None, :]
    mx = s.max(1, keepdim=True).values
    pred = torch.where(s == mx, idx, torch.full_like(idx, C)).min(1).values
    pred = torch.where(has_nan, torch.full_like(pred, -1), pred)
    sy = s[rows, tc][:, None]
    rank = (s > sy).sum(1) + ((s == sy) & (idx < target[:, None])).sum(1)
    valid = keep & inrange & ~has_nan
    rank = torch.where(valid, rank, torch.full_like(rank, -1))
    conf = torch.zeros(C, C, dtype=torch.int64)
    for b in torch.nonzero(valid).flatten().tolist():
        conf[int(target[b]), int(pred[b])] += 1
    counts = [B, int(keep.sum()), int((valid & (rank == 0)).sum()), int((valid & (rank >= 0) & (rank < topk)).sum()), int((keep & has_nan).sum())]
    return dict(num=term.double().sum(), den=share.double().sum(), counts=counts, confusion=conf, pred=pred, rank=rank, scores=s, terms=term)


def loss_of(ref):
    return float(ref["num"] / ref["den"])


# ---- shared cases ---------------------------------------------------------------------------------------------------------------------
# one view: one video, a single class, a partial tree, exactly one pass of the thread loop, its second pass, C at the temporal tail's limit
SHAPES = [(1, 1), (1, 2), (3, 5), (255, 8), (256, 8), (257, 8), (300, 8), (5, 64)]
# (weighted, ignore_index, label_smoothing)
OPTIONS = [(False, None, 0.0), (True, None, 0.0), (False, 1, 0.0), (False, None, 0.1), (True, 1, 0.1)]
OPTION_IDS = ["plain", "weighted", "ignore1", "eps0.1", "all"]
MULTIVIEW = [(2, 3, 5), (1, 2, 2), (130, 3, 8)]            # (B, V, C)
GAP = 1e-4


def topks(C):
    return sorted({1, min(2, C), C})


def class_weight(C, generator):
    w = torch.rand(C, generator=generator) + 0.25
    if C > 2:
        w[1] = 0.0                                          # one class weighs nothing
    return w


def case(B, C, weighted, ign, views=1):
    """(logits [B * views, C] fp32, target [B], weight or None) of one grid case, on the CPU.  Video 0 is kept and its class carries weight;
    with an ignore_index and B > 1 the last video is ignored (and others may be, where the draw hits that class)."""
    g = torch.Generator().manual_seed(1000 * views + 100 * B + C)
    logits = 3.0 * torch.randn(B * views, C, generator=g)
    y = torch.randint(0, C, (B,), generator=g)
    w = class_weight(C, g) if weighted else None
    y[0] = 0
    if ign is not None and B > 1:
        y[B - 1] = ign
    return logits, y, w


def multiview_margins(B, V, C):
    """Per video of the (B, V, C) case, in float64: the smallest relative gap that an integer result hangs on -- between pbar_y and any other
    pbar_c (the rank), and between the two largest scores (the prediction).  fp32 averaging may order a pair closer than GAP the other way."""
    logits, y, _ = case(B, C, False, None, V)
    p = torch.softmax(logits.double().reshape(B, V, C), -1).sum(1) / V
    if C == 1:
        return torch.full((B,), float("inf"), dtype=torch.float64)
    py = p[torch.arange(B), y][:, None]
    rel = (p - py).abs() / torch.maximum(p, py)
    rel[torch.arange(B), y] = float("inf")
    top = p.topk(2, dim=1).values
    return torch.minimum(rel.min(1).values, (top[:, 0] - top[:, 1]) / top[:, 0])


def multiview_left_out(B, V, C):
    """Boolean [B]: the videos left out of the integer comparison on the GPU."""
    return multiview_margins(B, V, C) < GAP
