"""References for the loss on dense targets (hyb_cross_entropy_dense_*), shared by tests/test_dense_loss_cpu.py and
tests/test_gpu_dense_loss.py: the two definitions of include/hybrid_hip.h restated in torch, in the dtype of the logits -- float64 as the
reference, float32 as the arbiter of the gradient gate.  ``dense_case`` builds the inputs of one grid case, the same for both files."""
import torch
import torch.nn.functional as F

SHAPES = [(1, 2), (3, 5), (8, 8), (40, 5), (5, 64), (300, 8)]      # the grid of tests/test_gpu_loss_options.py
BCE_SHAPES = SHAPES + [(4, 1)]                                     # kind 1 also takes the binary case
EPS = [0.0, 0.1, 1.0]


def soft_ce_ref(logits, target, weight=None, label_smoothing=0.0):
    """kind 0: q = (1 - e) t + e / C;  loss = (1 / B) sum_b sum_c w_c q_bc (lse_b - z_bc)."""
    B, C = logits.shape
    dt = logits.dtype
    w = torch.ones(C, dtype=dt) if weight is None else weight.to(dt)
    q = (1 - label_smoothing) * target.to(dt) + label_smoothing / C
    nll = torch.logsumexp(logits, 1)[:, None] - logits
    return (w * q * nll).sum() / B


def bce_ref(logits, target, weight=None, pos_weight=None):
    """kind 1: L = 1 + (pw - 1) t;  loss = (1 / (B C)) sum_bc w_c [(1 - t) z + L (log1p(exp(-|z|)) + max(-z, 0))]."""
    B, C = logits.shape
    dt = logits.dtype
    w = torch.ones(C, dtype=dt) if weight is None else weight.to(dt)
    pw = torch.ones(C, dtype=dt) if pos_weight is None else pos_weight.to(dt)
    t = target.to(dt)
    L = 1 + (pw - 1) * t
    sp = torch.log1p(torch.exp(-logits.abs())) + torch.clamp(-logits, min=0)
    return (w * ((1 - t) * logits + L * sp)).sum() / (B * C)


def dense_ref(kind, logits, target, weight=None, pos_weight=None, label_smoothing=0.0):
    return bce_ref(logits, target, weight, pos_weight) if kind == 1 else soft_ce_ref(logits, target, weight, label_smoothing)


def torch_ref(kind, logits, target, weight=None, pos_weight=None, label_smoothing=0.0):
    """torch's own functions on the same inputs."""
    if kind == 1:
        return F.binary_cross_entropy_with_logits(logits, target.to(logits.dtype), weight=weight, pos_weight=pos_weight)
    return F.cross_entropy(logits, target.to(logits.dtype), weight=weight, label_smoothing=label_smoothing)


def dense_case(kind, B, C, use_w, use_pw=False):
    """-> (logits fp32 [B,C], target fp32 [B,C], weight fp32 [C] or None, pos_weight fp32 [C] or None).  Logits are 3 randn.
    kind 0: rows of random probabilities that sum to 1, row 0 an exact one-hot row, and (B > 2) row 2 all zero; the weighted case has one zero
    weight when C > 2.  kind 1: targets uniform in [0, 1] with an exact 0 at the first entry and an exact 1 at the last, the first logit
    +100 and the last -100."""
    g = torch.Generator().manual_seed(100 * B + C + 7 * kind)
    logits = 3.0 * torch.randn(B, C, generator=g)
    w = pw = None
    if use_w:
        w = torch.rand(C, generator=g) + 0.25
        if C > 2:
            w[1] = 0.0
    if kind == 0:
        t = torch.rand(B, C, generator=g) + 0.05
        t = t / t.sum(1, keepdim=True)
        t[0] = 0.0
        t[0, C - 1] = 1.0
        if B > 2:
            t[2] = 0.0
    else:
        if use_pw:
            pw = 2.0 * torch.rand(C, generator=g) + 0.25
        t = torch.rand(B, C, generator=g)
        t.view(-1)[0], t.view(-1)[-1] = 0.0, 1.0
        logits.view(-1)[0], logits.view(-1)[-1] = 100.0, -100.0
    return logits, t.contiguous(), w, pw
