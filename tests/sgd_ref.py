"""SGD with momentum and LARS as HybridSGD / HybridLARS define them (torch.optim.SGD's rule; timm's Lars with trust_clip=False), in torch on
the CPU in a given dtype: float64 is the reference, float32 the error yardstick (the same rule restated in the kernels' precision, every
sum torch's own).

Per tensor at applied step t, G the effective gradient (the mean of the micro-batches' gradients, clipped like clip_grad_norm_):
    d    = G + wd p                                  coupled L2 decay
    r    = trust_coeff |p| / (|G| + wd |p| + eps)    LARS; 1 where |p| == 0 or |G| == 0, and where wd == 0 unless always_adapt
    d    = r d
    buf' = d  if t == 1  else  mu buf + (1 - dampening) d
    p'   = p - lr (d + mu buf'  if nesterov  else  buf')      and p' = p - lr d where mu == 0 (torch keeps no buffer then: no dampening)
    e'   = c e + (1 - c) p'                          the average; c = min(decay, (1 + n) / (10 + n)) after n earlier steps with warm-up
A step whose total gradient norm is not finite is skipped under the guard: nothing changes, t does not advance.

`gate` and `check_trust` are the two comparisons tests/test_gpu_sgd.py makes (those of tests/test_gpu_lamb.py); tests/test_sgd_cpu.py shows
that they catch wrong rules (`mutate`)."""
import torch

MUTATIONS = ("first-step dampening applied", "Nesterov using the old buffer", "decay after the trust scaling", "gn taken before clipping")


class SgdRef:
    """groups: dicts with params (tensors, copied and cast to dtype), lr, momentum, dampening, weight_decay, and optionally eps (LARS),
    ema_decay, ema_warmup.  trust_coeff None: plain SGD.  step(grads) takes one gradient per parameter in the order of the groups, or a
    list of k such lists (the micro-batches of an accumulated step: their mean), and returns (total norm before clipping, clip
    coefficient).  mutate: one of MUTATIONS, a deliberately wrong rule."""

    def __init__(self, groups, dtype, nesterov=False, trust_coeff=None, always_adapt=False, max_grad_norm=None, skip_nonfinite=False, mutate=None):
        assert mutate is None or mutate in MUTATIONS
        self.dtype, self.nesterov, self.trust_coeff, self.always_adapt = dtype, nesterov, trust_coeff, always_adapt
        self.max_grad_norm, self.skip_nonfinite, self.mutate = max_grad_norm, skip_nonfinite, mutate
        self.groups = [dict(g, params=[p.detach().cpu().to(dtype).clone() for p in g["params"]]) for g in groups]
        self.params = [p for g in self.groups for p in g["params"]]
        self.buf = [torch.zeros_like(p) for p in self.params]
        self.ema = [p.clone() for p in self.params]      # (moved only in groups with an ema_decay)
        self.trust = [None] * len(self.params)           # per parameter (|p|, |G|, r) of the last applied step, Python floats
        self.t = 0                                       # applied steps
        self.skipped = 0

    def step(self, grads):
        micro = grads if isinstance(grads[0], (list, tuple)) else [grads]
        micro = [[g.detach().cpu().to(self.dtype) for g in gs] for gs in micro]
        assert all(len(gs) == len(self.params) for gs in micro)
        k = len(micro)
        grads = [sum(gs[i] for gs in micro[1:]) + micro[0][i] for i in range(len(self.params))] if k > 1 else [g.clone() for g in micro[0]]
        if k > 1:
            grads = [g * (1.0 / k) for g in grads]
        # torch.nn.utils.clip_grad_norm_: the norm of the per-tensor norms, clamp(max_norm / (total + 1e-6), max = 1)
        total = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g) for g in grads]))
        if self.skip_nonfinite and not bool(torch.isfinite(total)):
            self.skipped += 1
            return float(total), float("nan")
        coef = 1.0
        unclipped = grads
        if self.max_grad_norm is not None:
            coef = torch.clamp(self.max_grad_norm / (total + 1e-6), max=1.0)
            grads = [g * coef for g in grads]
        self.t += 1
        i = 0
        for group in self.groups:
            lr, mu, damp, wd = group["lr"], group["momentum"], group["dampening"], group["weight_decay"]
            for p in group["params"]:
                g, buf = grads[i], self.buf[i]
                r = 1.0
                if self.trust_coeff is not None:
                    w_norm = torch.linalg.vector_norm(p).item()
                    g_norm = torch.linalg.vector_norm(unclipped[i] if self.mutate == "gn taken before clipping" else g).item()
                    if (wd != 0 or self.always_adapt) and w_norm > 0 and g_norm > 0:
                        r = self.trust_coeff * w_norm / (g_norm + w_norm * wd + group.get("eps", 0.0))
                    self.trust[i] = (w_norm, g_norm, r)
                if self.mutate == "decay after the trust scaling":
                    d = g * r + wd * p
                else:
                    d = (g + wd * p) * r
                old = buf.clone()
                if self.t == 1 and self.mutate != "first-step dampening applied":
                    buf.copy_(d)
                elif self.t == 1:
                    buf.copy_(d * (1.0 - damp))
                else:
                    buf.mul_(mu).add_(d * (1.0 - damp))
                s = d + mu * (old if self.mutate == "Nesterov using the old buffer" else buf) if self.nesterov else d if mu == 0 else buf
                p.sub_(s * lr)
                if group.get("ema_decay") is not None:
                    c = group["ema_decay"]
                    if group.get("ema_warmup"):
                        n = self.t - 1
                        c = min(c, (1.0 + n) / (10.0 + n))
                    self.ema[i].mul_(c).add_(p * (1.0 - c))
                i += 1
        return float(total), float(coef)


def gate(name, i, steps, got, ref32, ref64, verbose=True):
    """max|x - x64| <= 4 max|x32 - x64| + steps 2^-23 max|x64| -> (error, bound); prints each figure"""
    ref64 = ref64.double().flatten()
    err = (got.double().cpu().flatten() - ref64).abs().max().item()
    yard, big = (ref32.double().flatten() - ref64).abs().max().item(), ref64.abs().max().item()
    bound = 4 * yard + steps * 2.0 ** -23 * big
    if verbose:
        print(f"{name} tensor {i} ({ref64.numel()} elements) after {steps} steps: error {err:.3e}, fp32 restatement {yard:.3e}, gate {bound:.3e}, "
              f"ratio {err / bound if bound else float('inf'):.3f}")
    return err, bound


def check_trust(got, ref, tag, verbose=True):
    """got: [n, 3] (|p|, |G|, r) under test; ref: the fp64 reference's tuples -> the worst relative error (absolute where the reference is
    zero: a zero norm must come out as zero); the bound is 1e-5.  Prints every ratio."""
    want = torch.tensor(ref, dtype=torch.float64)
    got = torch.as_tensor(got).double().cpu()
    rel = (got - want).abs() / want.abs().clamp_min(1e-300)
    rel[want == 0] = (got - want).abs()[want == 0]
    if verbose:
        print(f"{tag}: ratios {[float(f'{x:.6g}') for x in got[:, 2].tolist()]}; worst relative error of (|p|, |G|, r) {rel.max(dim=0).values.tolist()}")
    return rel.max().item()
