"""Integer-valued data, an fp64 reference and the case table for the backward of a conv stage (hyb_convstage_bwd: Conv3x3 -> BatchNorm ->
ReLU -> MaxPool2d).  Imports without a GPU; tests/test_convstage_bwd_ref_cpu.py checks the recipe on the reference alone,
tests/test_gpu_convstage_bwd_exact.py and tests/convstage_bwd_worker.py compare the kernels with it.

The recipe.  x in 0..2, weights in -2..2, y_raw = conv(x, w) an integer of magnitude <= 256, dpooled in -2..2; per channel invstd in
{1/2, 1}, gamma in +-{1/2, 1, 2} or 0, integer mean and beta.  Then scale = gamma * invstd and shift = beta - mean * scale are multiples of
1/4, every pre-activation scale * y + shift is exact in fp32, a tenth and more of the pooling windows tie and many pre-activations are exactly
zero (first maximum in scan order and relu'(0) = 0 decide the routing; both are taken from torch's own max_pool2d and relu autograd in fp64),
and every product and sum down to dweight and dx is exactly representable: in eval mode the kernels must EQUAL the reference.  In training
mode the batch means m1, m2 enter; with a power-of-two count they are exact too (any fp32 evaluation order gives the same bits), with other
counts an element of the dense gradient may round to either neighbouring bf16 value and the comparison allows exactly that (`unsafe`).

Every tensor here is fp64 on the CPU, NCHW, with the layer's true channel counts (no padding)."""
import functools

import torch
import torch.nn.functional as F

# (Ci, Co, N, H, W): fused bf16 weight-gradient code, bf16 dgrad conv code (hyb_conv3x3_fwd_variant with the channels exchanged), the layout
# of the dense gradient between the two kernels, and whether N * H * W is a power of two.  tests/test_convstage_bwd_ref_cpu.py asserts the
# codes from the library's own queries.
CASES = [
    (32, 32, 2, 16, 32, 132, 100, "nhwc", True),
    (16, 24, 2, 9, 7, 132, 100, "nhwc", False),           # padded channels, odd H and W
    (64, 96, 2, 16, 16, 164, 101, "nhwc", True),
    (64, 32, 2, 16, 32, 164, 200, "nhwc", True),
    (32, 64, 2, 16, 32, 232, 100, "planar", True),
    (96, 64, 1, 16, 32, 232, 100, "planar", True),        # three input-channel blocks
    (64, 64, 2, 16, 32, 264, 101, "planar", True),
    (64, 64, 2, 29, 57, 264, 101, "planar", False),       # odd H and W: pixels outside every window
    (256, 64, 1, 8, 16, 264, 105, "planar", True),
    (64, 128, 2, 28, 28, 364, 101, "planar", False),
    (128, 64, 1, 12, 56, 364, 103, "planar", False),      # a whole and a half tile, two tile columns
    (128, 256, 1, 8, 28, 364, 103, "planar", False),      # eight channel-block pairs
    (128, 256, 5, 40, 56, 364, 103, "planar", False),     # 50 tiles on 32 slabs: runs of two, a shorter last run, runs across images
    (64, 64, 130, 4, 56, 264, 102, "planar", False),      # the 4 x 56 tile orientations of the dgrad conv
    (128, 64, 130, 4, 56, 264, 104, "planar", False),
    (256, 64, 130, 4, 56, 264, 106, "planar", False),
    (64, 32, 130, 4, 56, 164, 201, "nhwc", False),
]
SHAPES = [c[:5] for c in CASES]
IDS = ["%dto%d_%dx%dx%d" % s for s in SHAPES]
COMBO_SHAPES = [(32, 32, 2, 16, 32), (64, 64, 2, 16, 32), (64, 128, 2, 28, 28), (16, 24, 2, 9, 7)]      # pooled / packed_bwd given or NULL
# first stage (first = 1, eval mode): the first-stage shapes of tests/test_gpu_parity.py
FIRST_SHAPES = [(3, 32, 2, 16, 32), (3, 64, 2, 8, 16), (1, 32, 2, 16, 32), (4, 32, 1, 8, 16), (3, 32, 2, 16, 20), (2, 64, 1, 24, 48)]

WGRAD_BF16 = {132, 164, 232, 264, 364}
WGRAD_F32 = {132, 164}
DGRAD_BF16 = set(range(100, 107)) | {200, 201}
DGRAD_F32 = {0, 1, 2, 3}


def pad32(c):
    return (c + 31) // 32 * 32


def fl32(t):
    """round to fp32 (one rounding), kept in fp64"""
    return t.float().double()


def bf16_rne(t):
    """fp64 -> nearest bf16 (8 significant bits), ties to even, in ONE rounding, kept in fp64 (no subnormals / overflow at these magnitudes)"""
    bits = t.contiguous().view(torch.int64)
    bits = bits + ((1 << 44) - 1) + ((bits >> 45) & 1)
    return (bits & ~((1 << 45) - 1)).view(torch.float64)


def ulp_bf16(t):
    """spacing of bf16 at |t| (at zero: 0)"""
    _, e = torch.frexp(t)
    return torch.where(t == 0, torch.zeros_like(t), torch.ldexp(torch.ones_like(t), e - 8))


def sparse_int(shape, gen, lo, hi, p):
    v = torch.randint(lo, hi + 1, shape, generator=gen).double()
    return v * (torch.rand(shape, generator=gen) < p).double()


def channel_constants(Co, gen):
    """-> gamma, beta, mean, invstd [Co].  Octet 0: no zero gamma, one negative gamma, |beta / gamma| <= 4 with equality in channel 0 (the
    from-pooled sums take it); octet 1: gamma[8] == 0 (raw-output sums); octet 2: |beta / gamma| <= 4 again; the rest as drawn."""
    mag = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (Co,), generator=gen)]
    u = torch.rand(Co, generator=gen)
    gamma = torch.where(u < 0.06, torch.zeros_like(mag), torch.where(u < 0.36, -mag, mag))
    beta = torch.randint(-6, 7, (Co,), generator=gen).double()
    mean = torch.randint(-2, 3, (Co,), generator=gen).double()
    invstd = torch.tensor([0.5, 1.0], dtype=torch.float64)[torch.randint(0, 2, (Co,), generator=gen)]
    for o in (0, 2):
        sl = slice(8 * o, 8 * o + 8)
        gamma[sl] = torch.where(gamma[sl] == 0, mag[sl], gamma[sl])
        lim = 4 * gamma[sl].abs()
        beta[sl] = torch.maximum(torch.minimum(beta[sl], lim), -lim)
    gamma[0], beta[0] = 1.0, -4.0
    gamma[1] = -gamma[1].abs()
    if Co > 8:                                     # (the first stage's 8-channel row of tests/stage1_run_shapes.py has one octet only)
        gamma[8] = 0.0
    return gamma, beta, mean, invstd


def make_case(ci, co, n, h, w, first=False):
    """One seeded CPU generator per case -> dict of fp64 tensors."""
    g = torch.Generator().manual_seed(ci * 100003 + co * 1009 + n * 101 + h * 7 + w)
    x = sparse_int((n, ci, h, w), g, 0, 2, 0.5)
    wt = sparse_int((co, ci, 3, 3), g, -2, 2, 0.6 if first else 0.15)
    y = F.conv2d(x, wt, padding=1)
    assert y.abs().max() <= 256
    dp = sparse_int((n, co, h // 2, w // 2), g, -2, 2, 0.5)
    gamma, beta, mean, invstd = channel_constants(co, g)
    scale = gamma * invstd
    shift = beta - mean * scale
    z = scale.view(1, -1, 1, 1) * y + shift.view(1, -1, 1, 1)
    pooled = F.max_pool2d(F.relu(z), 2)
    return dict(shape=(ci, co, n, h, w), x=x, w=wt, y=y, dp=dp, gamma=gamma, beta=beta, mean=mean, invstd=invstd, scale=scale, shift=shift,
                z=z, pooled=pooled)


@functools.lru_cache(maxsize=2)
def case(ci, co, n, h, w):
    return make_case(ci, co, n, h, w)


def route_autograd(z, dp):
    """dz = d/dz sum(dp * max_pool2d(relu(z))): torch's first maximum in scan order and relu'(0) = 0"""
    zr = z.detach().clone().requires_grad_(True)
    F.max_pool2d(F.relu(zr), 2).backward(dp)
    return zr.grad


def route_manual(z, dp, last=False, gate_ge=False):
    """The same routing written out, with the two mutations a kernel could hold: the LAST maximum of a window, a >= 0 ReLU gate."""
    N, C, H, W = z.shape
    Ho, Wo = H // 2, W // 2
    win = z[:, :, :2 * Ho, :2 * Wo].reshape(N, C, Ho, 2, Wo, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, Ho, Wo, 4)      # (0,0) (0,1) (1,0) (1,1)
    vmax = win.amax(-1, keepdim=True)
    eq = win == vmax
    pick = eq & ((eq.flip(-1).cumsum(-1).flip(-1) if last else eq.cumsum(-1)) == 1)
    gate = (vmax >= 0) if gate_ge else (vmax > 0)
    dwin = pick.double() * gate.double() * dp.unsqueeze(-1)
    dz = torch.zeros_like(z)
    dz[:, :, :2 * Ho, :2 * Wo] = dwin.reshape(N, C, Ho, Wo, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, 2 * Ho, 2 * Wo)
    return dz


def conv_grads(x, wt, dy, want_dx=True):
    """-> (dW, dx) of conv2d(x, w, padding = 1) for the output gradient dy, fp64"""
    xr = x.detach().clone().requires_grad_(want_dx)
    wr = wt.detach().clone().requires_grad_(True)
    F.conv2d(xr, wr, padding=1).backward(dy)
    return wr.grad, (xr.grad if want_dx else None)


def last_tile_column(W):
    """first column of the last tile column of the weight-gradient kernels (28 wide; 16 for the first generation's narrow images)"""
    tw = 28 if W > 28 else 16 if W > 16 else 4
    return (W - 1) // tw * tw


MUTATIONS = ("last_max", "gate_ge", "drop_outside", "swap_m", "abs_gamma", "rotate_block", "zero_last_column")


def reference(c, training, storage="bf16", mutate=None, dz=None, with_bounds=True, round_means=True):
    """c: make_case(...).  storage "bf16" / "fp32": how the dense gradient is stored between the kernels ("fp64": not rounded; with
    round_means = False this is the plain fp64 backward, which tests/test_convstage_bwd_ref_cpu.py holds against torch autograd).  mutate: None or one of
    MUTATIONS (what a subtly wrong kernel would compute).  -> dict: dz, s1, s2, m1, m2, pre, dyraw, dW, dx, dgamma, dbeta and -- the terms of
    the training-mode bounds -- absW = sum |x| |dyraw|, absX = dgrad(|dyraw|, |w|), unsafe (mask), flipW, flipX."""
    ci, co, n, h, w = c["shape"]
    count = n * h * w
    v = lambda t: t.view(1, -1, 1, 1)
    if dz is None:
        if mutate in ("last_max", "gate_ge"):
            dz = route_manual(c["z"], c["dp"], last=mutate == "last_max", gate_ge=mutate == "gate_ge")
        else:
            dz = route_autograd(c["z"], c["dp"])
    xhat = (c["y"] - v(c["mean"])) * v(c["invstd"])
    s1 = dz.sum(dim=(0, 2, 3))
    s2 = (dz * xhat).sum(dim=(0, 2, 3))
    if mutate == "abs_gamma":                      # xhat at the arg-max formed as (pooled - beta) / |gamma|
        s2 = s2 * torch.where(c["gamma"] < 0, -1.0, 1.0)
    if training:
        if round_means:                            # one fp32 product each, as every kernel forms them: sums * (1.0f / (float)count)
            inv = fl32(torch.tensor(1.0 / count, dtype=torch.float64))
            m1, m2 = fl32(s1 * inv), fl32(s2 * inv)
        else:
            m1, m2 = s1 / count, s2 / count
        if mutate == "swap_m":
            m1, m2 = m2, m1
    else:
        m1, m2 = torch.zeros_like(s1), torch.zeros_like(s2)
    k = c["gamma"] * c["invstd"]
    pre = v(k) * (dz - v(m1) - xhat * v(m2))
    if mutate == "drop_outside":                   # pixels outside every pooling window (odd H / W) left without their dense gradient
        pre = pre.clone()
        pre[:, :, 2 * (h // 2):, :] = 0
        pre[:, :, :, 2 * (w // 2):] = 0
    dyraw = bf16_rne(pre) if storage == "bf16" else fl32(pre) if storage == "fp32" else pre
    if mutate == "rotate_block" and co >= 64:      # the 32-channel blocks of the dense gradient, each written one plane further
        dyraw = torch.roll(dyraw, 32, dims=1)
    if mutate == "zero_last_column":
        dyraw = dyraw.clone()
        dyraw[:, :, :, last_tile_column(w):] = 0
    dW, dx = conv_grads(c["x"], c["w"], dyraw)
    out = dict(dz=dz, xhat=xhat, s1=s1, s2=s2, m1=m1, m2=m2, k=k, pre=pre, dyraw=dyraw, dW=dW, dx=dx, dgamma=s2, dbeta=s1, count=count)
    if with_bounds:
        absW, absX = conv_grads(c["x"].abs(), c["w"].abs(), dyraw.abs())
        out.update(absW=absW, absX=absX)
        if training and storage == "bf16" and count & (count - 1):        # (a power-of-two count is exact: nothing can flip)
            # 8 fp32 roundings, doubled, on the magnitudes the terms of pre pass through (either algebraic form)
            T = v(k.abs()) * (dz.abs() + v(m1.abs()) + (xhat * v(m2)).abs()) + v((k * m2 * c["invstd"] * c["mean"]).abs())
            E = 16 * 2.0 ** -24 * T
            lo, hi = bf16_rne(pre - E), bf16_rne(pre + E)
            unsafe = lo != hi
            flip = torch.where(unsafe, torch.maximum(ulp_bf16(dyraw), (hi - lo).abs()), torch.zeros_like(pre))
            flipW, flipX = conv_grads(c["x"].abs(), c["w"].abs(), flip)
            out.update(unsafe=unsafe, flipW=flipW, flipX=flipX)
        else:
            out.update(unsafe=torch.zeros_like(pre, dtype=torch.bool), flipW=torch.zeros_like(dW), flipX=torch.zeros_like(dx))
    return out


@functools.lru_cache(maxsize=3)
def reference_for(shape, training, storage="bf16"):
    """the reference of a row of the table, computed once and shared (callers leave it unchanged)"""
    return reference(case(*shape), training, storage)


def exact_in_fp32(t):
    return bool(torch.equal(fl32(t), t))


def pow2_forms(c, r):
    """Training mode, power-of-two count: every intermediate of both algebraic forms of pre -- the header's k (dz - m1 - xhat m2) and the fused
    kernels' a1 y + a0 + k dz -- as a dict of fp64 tensors; when each is unchanged by a round trip through fp32, any fp32 order is exact."""
    v = lambda t: t.view(1, -1, 1, 1)
    k, m1, m2, inv, mean = r["k"], r["m1"], r["m2"], c["invstd"], c["mean"]
    a1 = -k * m2 * inv
    a0 = -k * m1 + k * m2 * inv * mean
    form2 = v(a1) * c["y"] + v(a0) + v(k) * r["dz"]
    return dict(m1=m1, m2=m2, xhat_m2=r["xhat"] * v(m2), km2=k * m2, a1=a1, a1_y=v(a1) * c["y"], km1=k * m1, km2im=k * m2 * inv * mean, a0=a0,
                a1y_a0=v(a1) * c["y"] + v(a0), inner=r["dz"] - v(m1), inner2=r["dz"] - v(m1) - r["xhat"] * v(m2), form1=r["pre"], form2=form2)


def compare(r, got, training, storage="bf16", cop=None):
    """The comparison the GPU tests make.  got: dict of CPU tensors dW [Co,Ci,3,3], dx [N,Ci,H,W], dgamma, dbeta [Co] (fp64 copies of what the
    kernels wrote).  -> (list of failure strings, dict of largest error / bound ratios)."""
    fails, ratios = [], {}
    for name, ref in (("dgamma", r["dgamma"]), ("dbeta", r["dbeta"])):
        if not torch.equal(got[name], ref):
            bad = (got[name] != ref).nonzero().flatten().tolist()
            fails.append(f"{name}: channels {bad[:8]} differ ({len(bad)} in all)")
    dx_ref = bf16_rne(r["dx"]) if storage == "bf16" else r["dx"]
    if not training:
        for name, ref in (("dW", r["dW"]), ("dx", dx_ref)):
            if not torch.equal(got[name], ref):
                bad = (got[name] != ref).nonzero()
                fails.append(f"{name}: {bad.shape[0]} of {ref.numel()} elements differ, first at {bad[:4].tolist()}")
        return fails, ratios
    cp = cop if cop is not None else pad32(r["dyraw"].shape[1])
    bW = (r["count"] + 8) * 2.0 ** -24 * r["absW"] + r["flipW"]
    bX = 2.0 ** -8 * r["dx"].abs() + (9 * cp + 8) * 2.0 ** -23 * r["absX"] + r["flipX"]
    for name, ref, b in (("dW", r["dW"], bW), ("dx", r["dx"], bX)):
        err = (got[name] - ref).abs()
        over = err > b
        ratios[name] = float((err / b.clamp_min(1e-300)).where(err > 0, torch.zeros_like(err)).max())
        if over.any():
            fails.append(f"{name}: {int(over.sum())} of {ref.numel()} elements above the bound, first at {over.nonzero()[:4].tolist()}, "
                         f"largest error / bound {ratios[name]:.3g}")
    return fails, ratios


def mutated_outputs(c, training, mutate, storage="bf16"):
    """What a kernel holding the mutation would hand back: the mutated reference's results in the kernels' output formats."""
    m = reference(c, training, storage, mutate=mutate, with_bounds=False)
    return dict(dW=fl32(m["dW"]), dx=bf16_rne(m["dx"]) if storage == "bf16" else fl32(m["dx"]), dgamma=fl32(m["dgamma"]), dbeta=fl32(m["dbeta"]))
