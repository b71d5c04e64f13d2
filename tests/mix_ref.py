"""References for Mixup / CutMix (hyb_clips_u8_transform_mix) and the two-target loss (hyb_cross_entropy_mix_*), shared by
tests/test_mix_cpu.py, tests/test_gpu_mix_transform.py and tests/test_gpu_mix_loss.py.

``clip_mix_ref`` is float64 on top of tests/clip_transform_ref.py: every clip's own value from its own parameter row, then the blend or
the box.  ``mix_ce_ref`` is the loss's definition in torch, in the dtype of the logits: float64 as the reference, float32 as the arbiter
of the gradient gate."""
import numpy as np
import torch

from clip_transform_ref import clip_transform_ref


def lam_bits(lam):
    """The int32 a mix row carries for the fp32 value ``lam``."""
    return int(np.asarray(lam, dtype=np.float32).view(np.int32))


def clamp_mix_rows(mix, B, Ho, Wo):
    """The kernel's clamps of {partner, kind, by0, bx0, bh, bw}: partner into [0, B-1], a kind outside 0..2 is 0, by0 into [0, Ho] and bh into
    [0, Ho-by0], the same for bx0 / bw.  lam_bits stays as it is (the kernel clamps the VALUE: ``mix_lam``)."""
    mix = np.array(mix, dtype=np.int64).reshape(-1, 8)
    out = mix.copy()
    out[:, 0] = np.clip(mix[:, 0], 0, B - 1)
    out[:, 1] = np.where((mix[:, 1] >= 0) & (mix[:, 1] <= 2), mix[:, 1], 0)
    out[:, 2] = np.clip(mix[:, 2], 0, Ho)
    out[:, 3] = np.clip(mix[:, 3], 0, Wo)
    out[:, 4] = np.clip(mix[:, 4], 0, Ho - out[:, 2])
    out[:, 5] = np.clip(mix[:, 5], 0, Wo - out[:, 3])
    return out


def mix_lam(bits):
    """The fp32 whose bits are ``bits``, clamped into [0, 1]; a NaN counts as 1."""
    v = float(np.asarray(int(bits), dtype=np.int64).astype(np.int32).view(np.float32))
    return 1.0 if not v <= 1.0 else max(v, 0.0)


def clip_mix_ref(src, rows, mix, mean_invstd, Tout, Ho, Wo):
    """src uint8 [B,Tin,Hin,Win,C], rows / mix int [B,8] -> float64 [B,Tout,C,Ho,Wo]."""
    B = np.asarray(src).shape[0]
    own = clip_transform_ref(src, rows, mean_invstd, Tout, Ho, Wo)
    m = clamp_mix_rows(mix, B, Ho, Wo)
    out = own.copy()
    for b in range(B):
        p, kind, by0, bx0, bh, bw = (int(v) for v in m[b, :6])
        if kind == 1:
            lam = mix_lam(m[b, 6])
            out[b] = lam * own[b] + (1.0 - lam) * own[p]
        elif kind == 2:
            out[b, :, :, by0:by0 + bh, bx0:bx0 + bw] = own[p, :, :, by0:by0 + bh, bx0:bx0 + bw]
    return out


def mix_ce_ref(logits, ya, yb, lam, weight=None, ignore_index=None, label_smoothing=0.0):
    """loss = sum_b [l_b term(b, a_b) + (1 - l_b) term(b, c_b)] / sum_b [l_b d(b, a_b) + (1 - l_b) d(b, c_b)] with
    term(b, y) = keep [(1 - e) w[y] (lse_b - z_b[y]) + (e / C) sum_c w[c] (lse_b - z_b[c])] and d(b, y) = keep w[y], in logits.dtype."""
    B, C = logits.shape
    dt = logits.dtype
    w = torch.ones(C, dtype=dt) if weight is None else weight.to(dt)
    nll = torch.logsumexp(logits, 1)[:, None] - logits                      # [B,C]
    smooth = (nll * w).sum(1) * (label_smoothing / C)

    def side(y):
        keep = torch.ones(B, dtype=torch.bool) if ignore_index is None else (y != ignore_index)
        ys = torch.where(keep, y, torch.zeros_like(y))
        wy = w[ys]
        term = (1 - label_smoothing) * wy * nll.gather(1, ys[:, None])[:, 0] + smooth
        return torch.where(keep, term, torch.zeros_like(term)), torch.where(keep, wy, torch.zeros_like(wy))
    ta, da = side(ya)
    tb, db = side(yb)
    lam = lam.to(dt)
    return (lam * ta + (1 - lam) * tb).sum() / (lam * da + (1 - lam) * db).sum()
