"""References for the focal and asymmetric losses (hyb_cross_entropy_focal_*, hyb_cross_entropy_asym_*), shared by
tests/test_focal_loss_cpu.py and tests/test_gpu_focal_loss.py: the two definitions of include/hybrid_hip.h restated in torch, in the dtype of
the logits -- float64 as the reference, float32 on the CPU as the arbiter of the gradient gate; gradients come from autograd.  Inputs come
from tests/dense_ref.py's SHAPES / BCE_SHAPES and dense_case: the focal cases add random class indices, the asymmetric cases replace the
uniform targets by multi-hot ones (rand < 0.3) with an exact 0 on the +100 logit and an exact 1 on the -100 logit."""
import torch
import torch.nn.functional as F

from dense_ref import BCE_SHAPES, SHAPES, dense_case

FOCAL_GAMMAS = [0.0, 1.0, 2.0, 5.0]
ASYM_CONFIGS = [(0.0, 0.0, 0.0), (2.0, 2.0, 0.0), (0.0, 4.0, 0.05), (1.0, 4.0, 0.05), (0.0, 1.0, 0.05)]        # (gamma_pos, gamma_neg, clip)
KINK = 1e-5            # no cell of the grid may have |p - clip| below this: the gamma_neg = 0 case has a kink in z there


def _pow(x, g):
    """x ** g with the family's rule for an exponent of 0: exactly 1, derivative 0 (g a float or a tensor)."""
    if not isinstance(g, torch.Tensor):
        return torch.ones_like(x) if g == 0 else x.pow(g)
    zero = g == 0
    return torch.where(zero, torch.ones_like(x), torch.where(zero, torch.ones_like(x), x).pow(g))


def focal_ref(logits, y, gamma, weight=None, ignore_index=None):
    """term_b = keep_b w[y] u_b^gamma (lse_b - z_by),  u_b = sum_{c != y} softmax(z_b)_c,  loss = sum term / sum keep_b w[y]."""
    B, C = logits.shape
    dt = logits.dtype
    w = torch.ones(C, dtype=dt) if weight is None else weight.to(dt)
    keep = torch.ones(B, dtype=torch.bool) if ignore_index is None else y != ignore_index
    yy = torch.where(keep, y, torch.zeros_like(y))
    hot = F.one_hot(yy, C).bool()
    p = torch.softmax(logits, 1)
    u = p.masked_fill(hot, 0.0).sum(1)
    ce = torch.logsumexp(logits, 1) - logits.gather(1, yy[:, None])[:, 0]
    kw = keep.to(dt) * w[yy]
    return (kw * _pow(u, gamma) * ce).sum() / kw.sum()


def asym_ref(logits, target, gamma_pos, gamma_neg, clip, weight=None, pos_weight=None):
    """cell = -w L base^g_t (t logp + (1 - t) logn),  loss = mean over all B C cells (include/hybrid_hip.h)."""
    B, C = logits.shape
    dt = logits.dtype
    w = torch.ones(C, dtype=dt) if weight is None else weight.to(dt)
    pw = torch.ones(C, dtype=dt) if pos_weight is None else pos_weight.to(dt)
    z, t = logits, target.to(dt)
    ez = torch.exp(-z.abs())
    l1 = torch.log1p(ez)
    one = torch.ones_like(z)
    p = torch.where(z >= 0, one, ez) / (1 + ez)
    q = torch.where(z >= 0, ez, one) / (1 + ez)
    logp = -(l1 + torch.clamp(-z, min=0))
    r = torch.clamp(p - clip, min=0)
    logn = -(l1 + torch.clamp(z, min=0)) if clip == 0 else torch.log(torch.clamp(q + clip, max=1))
    base = t * q + (1 - t) * r
    gt = gamma_pos * t + gamma_neg * (1 - t)
    L = 1 + (pw - 1) * t
    cell = -w * L * _pow(base, gt) * (t * logp + (1 - t) * logn)
    return cell.sum() / (B * C)


def focal_case(B, C, use_w):
    """-> (logits fp32 [B,C] = 3 randn, class indices int64 [B], weight fp32 [C] or None; one zero weight when C > 2)."""
    logits, _, w, _ = dense_case(0, B, C, use_w)
    y = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(1000 * B + C + 1))
    return logits, y, w


def asym_case(B, C, use_w, use_pw, soft=False):
    """-> (logits, target, weight, pos_weight) of dense_case(1, ...): the first logit +100, the last -100; the targets multi-hot (rand < 0.3)
    with an exact 0 on the first cell and an exact 1 on the last, or (soft) dense_case's uniform ones."""
    logits, t, w, pw = dense_case(1, B, C, use_w, use_pw)
    if not soft:
        t = (torch.rand(B, C, generator=torch.Generator().manual_seed(500 * B + C + 3)) < 0.3).float()
        t.view(-1)[0], t.view(-1)[-1] = 0.0, 1.0
    return logits, t.contiguous(), w, pw


def clear_of_the_kink(logits, clip):
    """Whether every cell's probability is at least KINK away from clip (float64)."""
    return clip == 0 or bool(((torch.sigmoid(logits.double()) - clip).abs() >= KINK).all())


__all__ = ["FOCAL_GAMMAS", "ASYM_CONFIGS", "SHAPES", "BCE_SHAPES", "focal_ref", "asym_ref", "focal_case", "asym_case", "clear_of_the_kink"]
