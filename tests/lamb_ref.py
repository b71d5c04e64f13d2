"""LAMB as HybridLAMB defines it (You et al. 2020; timm's Lamb, apex's FusedLAMB without nvlamb), in torch on the CPU in a given dtype:
float64 is the reference, float32 the error yardstick (the same rule restated in the kernels' precision, every sum torch's own).

Per tensor at applied step t, G the effective gradient (the mean of the micro-batches' gradients, clipped like clip_grad_norm_):
    m' = m + (1 - b1)(G - m)      v' = b2 v + (1 - b2) G^2
    q  = (m' / (1 - b1^t)) / (sqrt(v') / sqrt(1 - b2^t) + eps)        u = q + wd p
    r  = |p| / |u|  if (wd != 0 or always_adapt) and |p| > 0 and |u| > 0, else 1
    p <- p - lr r u"""
import math

import torch


class LambRef:
    """groups: dicts with params (tensors, copied and cast to dtype), lr, betas, eps, weight_decay.  step(grads) takes one gradient per
    parameter in the order of the groups (any dtype; cast to dtype) and returns (total norm before clipping, clip coefficient)."""

    def __init__(self, groups, dtype, always_adapt=False, max_grad_norm=None):
        self.dtype, self.always_adapt, self.max_grad_norm = dtype, always_adapt, max_grad_norm
        self.groups = [dict(g, params=[p.detach().cpu().to(dtype).clone() for p in g["params"]]) for g in groups]
        self.params = [p for g in self.groups for p in g["params"]]
        self.exp_avg = [torch.zeros_like(p) for p in self.params]
        self.exp_avg_sq = [torch.zeros_like(p) for p in self.params]
        self.trust = [None] * len(self.params)           # per parameter (|p|, |u|, r) of the last step, Python floats
        self.t = 0

    def step(self, grads):
        grads = [g.detach().cpu().to(self.dtype).clone() for g in grads]
        assert len(grads) == len(self.params)
        # torch.nn.utils.clip_grad_norm_: the norm of the per-tensor norms, clamp(max_norm / (total + 1e-6), max = 1)
        total = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g) for g in grads]))
        coef = 1.0
        if self.max_grad_norm is not None:
            coef = torch.clamp(self.max_grad_norm / (total + 1e-6), max=1.0)
            grads = [g * coef for g in grads]
        self.t += 1
        i = 0
        for group in self.groups:
            lr, (b1, b2), eps, wd = group["lr"], group["betas"], group["eps"], group["weight_decay"]
            bc1, bc2 = 1.0 - b1 ** self.t, 1.0 - b2 ** self.t
            for p in group["params"]:
                g, m, v = grads[i], self.exp_avg[i], self.exp_avg_sq[i]
                m.add_((g - m) * (1.0 - b1))
                v.mul_(b2).add_(g * g * (1.0 - b2))
                q = (m / bc1) / (v.sqrt() / math.sqrt(bc2) + eps)
                u = q + wd * p
                w_norm, u_norm = torch.linalg.vector_norm(p).item(), torch.linalg.vector_norm(u).item()
                r = w_norm / u_norm if (wd != 0 or self.always_adapt) and w_norm > 0 and u_norm > 0 else 1.0
                self.trust[i] = (w_norm, u_norm, r)
                p.sub_(u * (lr * r))
                i += 1
        return float(total), float(coef)
