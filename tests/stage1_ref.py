"""fp64 reference and comparison functions for the FIRST conv stage where a wave walks a run of blocks (tests/stage1_run_shapes.py).
Imports without a GPU: tests/test_stage1_run_cpu.py checks the recipe, the bounds' premises and -- by mutation -- that the comparisons reject what
a kernel with a wrong carry from block to block would hand back; tests/test_gpu_stage1_runs.py and tests/stage1_run_worker.py compare the kernels.

Data: convstage_bwd_ref.make_case(first = True) as it stands -- x in 0..2, weights in -2..2, dpooled in -2..2, so the raw conv output y is an
integer of magnitude <= 108 and every sum below is an exact integer in fp64.

Eval mode (hand-made statistics: scale and shift multiples of 1/4): everything is exactly representable; pooled, the routing codes and the
gradients must EQUAL the reference.

Training mode: the batch statistics come from exact integer sums, sum y and sum y^2 per channel.
  gram path   (s1_gram_stats_kernel: sums and algebra in double, ONE fp32 rounding each for mean, invstd and the unbiased variance)
      mean      equal where N H W is a power of two, within one fp32 ulp otherwise
      invstd    within 2^-23 relative
  stats path  (bn_stats_finalize_kernel, all fp32, after the statistics pass: fp32 storage, ragged frames, the block-level kernels); u = 2^-24
      inv_n = fl(1 / n) (exact for powers of two), mean = fl(s1 inv_n):            e_mean = 2 u |mean| + e_s1 / n   (power of two: u -> 0)
      var = fl(fl(s2 inv_n) - fl(mean mean)) (either contraction):                 e_var  = 2 u E2 + e_s2 / n + 2 |mean| e_mean + u mean^2 + u var
      invstd = rsqrtf(var + eps), 2 ulp (the OpenCL bound of rsqrt):               e_inv  = invstd (e_var + u (var + eps)) / (2 (var + eps)) + 4 u invstd
      e_s = 0 where the sum of magnitudes stays below 2^24 (every partial sum is then an exact fp32 integer); otherwise the partial rows are
      still exact and a value passes through at most rows / 64 + 33 fp32 additions of rows_reduce_1024 (two chains per thread over 32 row
      groups, their sum, 32 in sequence): e_s = (rows / 64 + 33) u sum|.|
  both        scale = fl(g invstd):                                                e_scale = |g| e_inv + u |scale|
              shift = fl(b - fl(mean scale)) (or one fma):                         e_shift = |scale| e_mean + |mean| e_scale + u |mean scale| + u |shift|
              running = fl(fl(fl(1 - mom) r0) + fl(mom v)) (or contracted):        e_run   = 2 u |(1 - mom) r0| + mom e_v + u |mom v| + u |running|
  each bound times (1 + 2^-10) for the second-order terms.  All of it from the reference's magnitudes; nothing is fitted to a kernel.
The later checks take the kernel's own fp32 scale_shift / mean_invstd as given (they were compared just before):
  pooled     |out - ref| <= st |ref| + 4 u max_window(|sc y| + |sh|), st = 2^-8 (bf16 storage) or u (fp32): the form of tests/test_gpu_infer.py
  codes      equal on every safe window; a window is unsafe when its maximum sc y + sh lies within the slack 4 u max_window(|sc y| + |sh|) of 0 or
             of the runner-up (equal y, or sc == 0, give equal fp32 values: ties are safe; a maximum with sc y == 0 exactly is sh itself in any
             evaluation order: its sign is safe); there the code must name a pixel within the slack
  backward   S1 and G are exact integers (fp32 partial rows below 2^24, summed in double), s1_bwd_finalize_kernel runs in double and rounds once:
             |dW - ref| <= u |ref| + 64 2^-52 sum|terms| + flips, the terms of gamma inv (S1 - m1 sp - m2 inv (w G - mean sp)) taken at their
             magnitudes from the reference; flips = what the unsafe windows with a non-zero dpooled can move (none in eval mode)."""
import functools

import torch
import torch.nn.functional as F

import convstage_bwd_ref as R

U = 2.0 ** -24
SECOND = 1 + 2.0 ** -10
SENTINEL = 7.0
MOMENTUM = float(torch.tensor(0.1, dtype=torch.float32))
EPS = float(torch.tensor(1e-5, dtype=torch.float32))


def draw(ci, co, n, h, w):
    """make_case(first = True)'s draws in its order, without forming y: x, w, dp, gamma, beta, mean, invstd"""
    g = torch.Generator().manual_seed(ci * 100003 + co * 1009 + n * 101 + h * 7 + w)
    x = R.sparse_int((n, ci, h, w), g, 0, 2, 0.5)
    wt = R.sparse_int((co, ci, 3, 3), g, -2, 2, 0.6)
    dp = R.sparse_int((n, co, h // 2, w // 2), g, -2, 2, 0.5)
    gamma, beta, mean, invstd = R.channel_constants(co, g)
    return x, wt, dp, gamma, beta, mean, invstd


@functools.lru_cache(maxsize=2)
def case(shape):
    return R.make_case(*shape, first=True)


def windows(t):
    """[N, C, H, W] -> [N, C, Ho, Wo, 4] in scan order (0,0) (0,1) (1,0) (1,1)"""
    N, C, H, W = t.shape
    Ho, Wo = H // 2, W // 2
    return t[:, :, :2 * Ho, :2 * Wo].reshape(N, C, Ho, 2, Wo, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, Ho, Wo, 4)


def unwindows(dwin, H, W):
    N, C, Ho, Wo, _ = dwin.shape
    out = torch.zeros(N, C, H, W, dtype=dwin.dtype)
    out[:, :, :2 * Ho, :2 * Wo] = dwin.reshape(N, C, Ho, Wo, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, 2 * Ho, 2 * Wo)
    return out


def pick_gate(z, last=False):
    """the routing decisions of route_manual: pick [N, C, Ho, Wo, 4] (one-hot: the first -- mutation: last -- maximum), gate [N, C, Ho, Wo]"""
    win = windows(z)
    vmax = win.amax(-1, keepdim=True)
    eq = win == vmax
    pick = eq & ((eq.flip(-1).cumsum(-1).flip(-1) if last else eq.cumsum(-1)) == 1)
    return pick, (vmax > 0).squeeze(-1)


def codes_from(pick, gate):
    """4 bits per pooled element as stage1w_kernel<.., ROUTE> writes them: bit 2 = the ReLU passed, bits 0-1 = the first maximum; 0 otherwise.
    -> int8 [N, C, Ho, Wo]"""
    idx = pick.to(torch.int8).argmax(-1).to(torch.int8)
    return torch.where(gate, idx + 4, torch.zeros_like(idx))


def code_words(codes, cop):
    """int8 [N, C, Ho, Wo] -> int32 [N * Ho * Wo * cop / 8]: one word per pooled pixel and 8 channels, at the NHWC pooled tensor's byte offset / 4
    (16-bit storage), nibble e = channel 8 o + e; padded channels 0"""
    N, C, Ho, Wo = codes.shape
    full = torch.zeros(N, Ho, Wo, cop, dtype=torch.int64)
    full[..., :C] = codes.permute(0, 2, 3, 1).to(torch.int64)
    sh = 4 * torch.arange(8, dtype=torch.int64)
    words = (full.view(N, Ho, Wo, cop // 8, 8) << sh).sum(-1)
    words = torch.where(words >= 2 ** 31, words - 2 ** 32, words)
    return words.to(torch.int32).flatten()


def words_to_codes(words, N, C, Ho, Wo, cop):
    w = words.to(torch.int64).view(N, Ho, Wo, cop // 8, 1) & 0xFFFFFFFF
    nib = (w >> (4 * torch.arange(8, dtype=torch.int64))) & 15
    return nib.view(N, Ho, Wo, cop)[..., :C].permute(0, 3, 1, 2).to(torch.int8).contiguous()


# ---- eval mode ------------------------------------------------------------------------------------------------------------------------------------
def eval_forward(shape, slice_images=16):
    """pooled (fp64 [N, Co, Ho, Wo]) and codes (int8) of the hand-made statistics, formed in slices of images (the 181-image row)"""
    ci, co, n, h, w = shape
    x, wt, dp, gamma, beta, mean, invstd = draw(*shape)
    scale = gamma * invstd
    shift = beta - mean * scale
    pooled, codes = [], []
    for i in range(0, n, slice_images):
        y = F.conv2d(x[i:i + slice_images], wt, padding=1)
        z = scale.view(1, -1, 1, 1) * y + shift.view(1, -1, 1, 1)
        pick, gate = pick_gate(z)
        pooled.append(F.max_pool2d(F.relu(z), 2))
        codes.append(codes_from(pick, gate))
    return dict(shape=shape, x=x, w=wt, gamma=gamma, beta=beta, mean=mean, invstd=invstd, scale=scale, shift=shift, pooled=torch.cat(pooled), codes=torch.cat(codes))


@functools.lru_cache(maxsize=1)
def eval_reference(shape, sliced=False):
    """the eval-mode forward reference of a row, computed once and shared (callers leave it unchanged): from make_case's own z and pooled, or
    -- the 181-image row -- in slices of images (tests/test_stage1_run_cpu.py holds the two forms against each other)"""
    if sliced:
        return eval_forward(shape)
    c = case(shape)
    pick, gate = pick_gate(c["z"])
    return dict(c, codes=codes_from(pick, gate))


def compare_exact(name, got, ref):
    if torch.equal(got, ref):
        return []
    bad = (got != ref).nonzero()
    return [f"{name}: {bad.shape[0]} of {ref.numel()} elements differ, first at {bad[:4].tolist()}: got {got[tuple(bad[0])].item()} want {ref[tuple(bad[0])].item()}"]


def compare_eval_forward(ref, got):
    """got: pooled (fp64 NCHW, true channels), pad_zero, codes (int8 NCHW) or None"""
    fails = compare_exact("pooled", got["pooled"], ref["pooled"])
    if not got["pad_zero"]:
        fails.append("padded channels of pooled are not exact zeros")
    if got.get("codes") is not None:
        fails += compare_exact("codes", got["codes"], ref["codes"])
    return fails


# ---- training mode: statistics -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def sliced_case(shape, slice_images=16):
    """the 181-image row in training mode: make_case's draws without y; the exact sums are formed in slices of images.  -> a dict train_stats takes"""
    ci, co, n, h, w = shape
    x, wt, dp, gamma, beta, mean, invstd = draw(*shape)
    sums = torch.zeros(3, co, dtype=torch.float64)
    for i in range(0, n, slice_images):
        y = F.conv2d(x[i:i + slice_images], wt, padding=1)
        sums += torch.stack([y.sum(dim=(0, 2, 3)), (y * y).sum(dim=(0, 2, 3)), y.abs().sum(dim=(0, 2, 3))])
    return dict(shape=shape, x=x, w=wt, dp=dp, gamma=gamma, beta=beta, mean=mean, invstd=invstd, sums=sums)


def train_stats(c, r0=None, rv0=None):
    """c: make_case(first = True) or sliced_case.  The exact integer sums and what BatchNorm makes of them, fp64."""
    ci, co, n, h, w = c["shape"]
    count = n * h * w
    if "sums" in c:
        s1, s2, a1 = c["sums"]
    else:
        y = c["y"]
        s1, s2 = y.sum(dim=(0, 2, 3)), (y * y).sum(dim=(0, 2, 3))
        a1 = y.abs().sum(dim=(0, 2, 3))
    assert float(s2.max()) < 2.0 ** 53
    mean = s1 / count
    e2 = s2 / count
    var = (e2 - mean * mean).clamp_min(0)
    invstd = 1.0 / torch.sqrt(var + EPS)
    unbiased = var * (count / (count - 1.0))
    r0 = c["mean"] if r0 is None else r0
    rv0 = 1.0 / (c["invstd"] * c["invstd"]) if rv0 is None else rv0
    omm = float(torch.tensor(1.0, dtype=torch.float32) - torch.tensor(MOMENTUM, dtype=torch.float32))
    scale = c["gamma"] * invstd
    shift = c["beta"] - mean * scale
    return dict(count=count, pow2=count & (count - 1) == 0, s1=s1, s2=s2, a1=a1, mean=mean, e2=e2, var=var, invstd=invstd, unbiased=unbiased, r0=r0, rv0=rv0,
                omm=omm, run_mean=omm * r0 + MOMENTUM * mean, run_var=omm * rv0 + MOMENTUM * unbiased, scale=scale, shift=shift)


def ulp32(t):
    """spacing of fp32 at |t| (at zero: the smallest normal spacing is irrelevant here: 0)"""
    _, e = torch.frexp(t)
    return torch.where(t == 0, torch.zeros_like(t), torch.ldexp(torch.ones_like(t), e - 24))


def stat_bounds(s, c, path, rows=1024):
    """-> dict of per-channel absolute bounds (module docstring).  path: "gram" or "stats"."""
    n = s["count"]
    mean, var, inv = s["mean"].abs(), s["var"], s["invstd"]
    if path == "gram":
        e_mean = torch.zeros_like(mean) if s["pow2"] else ulp32(s["mean"])
        e_inv = 2.0 ** -23 * inv
        e_unb = U * s["unbiased"] * SECOND
    else:
        es = lambda mag: torch.where(mag < 2.0 ** 24, torch.zeros_like(mag), (rows / 64 + 33) * U * mag)
        e_s1, e_s2 = es(s["a1"]), es(s["s2"])
        un = 0.0 if s["pow2"] else U
        e_mean = (2 * un * mean + e_s1 / n) * SECOND
        e_var = (2 * un * s["e2"] + e_s2 / n + 2 * mean * e_mean + U * mean * mean + U * var) * SECOND
        e_inv = (inv * (e_var + U * (var + EPS)) / (2 * (var + EPS)) + 4 * U * inv) * SECOND
        e_unb = (e_var * (n / (n - 1.0)) + 3 * U * s["unbiased"]) * SECOND
    g = c["gamma"].abs()
    e_scale = (g * e_inv + U * s["scale"].abs()) * SECOND
    e_shift = (s["scale"].abs() * e_mean + mean * e_scale + U * (mean * s["scale"].abs()) + U * s["shift"].abs()) * SECOND
    run = lambda r0, v, e_v, res: (2 * U * (s["omm"] * r0).abs() + MOMENTUM * e_v + U * (MOMENTUM * v).abs() + U * res.abs()) * SECOND
    return dict(mean=e_mean, invstd=e_inv, scale=e_scale, shift=e_shift, run_mean=run(s["r0"], s["mean"], e_mean, s["run_mean"]),
                run_var=run(s["rv0"], s["unbiased"], e_unb, s["run_var"]))


def compare_stats(s, c, got, path, rows=1024):
    """got: fp64 [Co] mean, invstd, scale, shift, run_mean, run_var and nbt (int), pad_zero.  -> (fails, ratios)"""
    b = stat_bounds(s, c, path, rows)
    fails, ratios = [], {}
    for k in ("mean", "invstd", "scale", "shift", "run_mean", "run_var"):
        err = (got[k] - s[k]).abs()
        over = err > b[k]
        ratios[k] = float(torch.where(err > 0, err / b[k].clamp_min(1e-300), torch.zeros_like(err)).max())
        if over.any():
            ch = over.nonzero().flatten().tolist()
            fails.append(f"{k}: channels {ch[:6]} above the bound ({len(ch)} in all); channel {ch[0]}: got {got[k][ch[0]].item()!r} want {s[k][ch[0]].item()!r} bound {b[k][ch[0]].item():.3g}")
    if got["nbt"] != 1:
        fails.append(f"num_batches_tracked is {got['nbt']}")
    if not got["pad_zero"]:
        fails.append("padded channels of scale_shift / mean_invstd are not zero")
    return fails, ratios


# ---- training mode: pooled and codes, given the kernel's fp32 scale and shift --------------------------------------------------------------------
def train_forward(c, sc, sh):
    """sc, sh: fp64 copies of the fp32 rows the kernel returned.  -> pooled reference, slack, pick / gate, safe mask, the window values"""
    v = lambda t: t.view(1, -1, 1, 1)
    y = c["y"]
    t = v(sc) * y + v(sh)
    win = windows(t)
    slack = 4 * U * windows((v(sc) * y).abs() + v(sh).abs()).amax(-1)
    pick, gate = pick_gate(t)
    tmax = win.amax(-1)
    ywin = windows(y)
    ymax = (ywin * pick).sum(-1, keepdim=True)                       # y at the first maximum
    same = (ywin == ymax) | (v(sc) == 0).unsqueeze(-1)
    runner = torch.where(same, torch.full_like(win, -float("inf")), win).amax(-1)
    # (a maximum whose product sc y is exactly zero -- y == 0 or sc == 0 -- evaluates to sh itself in any fp32 order: its sign is not in doubt)
    exact = (ymax.squeeze(-1) == 0) | (v(sc) == 0).expand_as(tmax)
    safe = ((tmax.abs() > slack) | exact) & ((tmax - runner) > slack)
    return dict(pooled=F.relu(tmax), slack=slack, pick=pick, gate=gate, safe=safe, win=win, tmax=tmax, codes=codes_from(pick, gate))


def compare_train_pooled(f, got_pooled, storage):
    st = 2.0 ** -8 if storage == "bf16" else U
    b = st * f["pooled"].abs() + f["slack"]
    err = (got_pooled - f["pooled"]).abs()
    ratio = float(torch.where(err > 0, err / b.clamp_min(1e-300), torch.zeros_like(err)).max())
    over = err > b
    fails = []
    if over.any():
        i = tuple(over.nonzero()[0].tolist())
        fails.append(f"pooled: {int(over.sum())} of {err.numel()} elements above the bound, first (n, co, oy, ox) {list(i)}: got {got_pooled[i].item()!r} want {f['pooled'][i].item()!r}, "
                     f"largest error / bound {ratio:.3g}")
    return fails, ratio


def compare_train_codes(f, codes):
    """codes: int8 [N, C, Ho, Wo] decoded from the kernel's words.  Equal on safe windows; within the slack elsewhere."""
    fails = []
    bad = (codes != f["codes"]) & f["safe"]
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        fails.append(f"codes: {int(bad.sum())} safe windows differ, first (n, co, oy, ox) {list(i)}: got {int(codes[i])} want {int(f['codes'][i])}")
    un = ~f["safe"]
    if un.any():
        cu = codes[un].to(torch.int64)
        win, tmax, slack = f["win"][un], f["tmax"][un], f["slack"][un]
        valid = (cu == 0) | ((cu >= 4) & (cu <= 7))
        named = win.gather(-1, (cu & 3).unsqueeze(-1)).squeeze(-1)
        ok = torch.where(cu == 0, tmax <= slack, (named >= tmax - slack) & (named > -slack)) & valid
        if not ok.all():
            fails.append(f"codes: {int((~ok).sum())} unsafe windows name a pixel outside the slack")
    return fails


# ---- training mode: backward, given the kernel's fp32 scale / shift (routing) and mean / invstd ----------------------------------------------------
def train_backward(c, f, mean, invstd, training=True):
    """The first stage's backward computed directly: dz from the routing of f (train_forward), dyraw = gamma invstd (dz - mean(dz) - xhat mean(dz xhat)),
    then dW, dgamma, dbeta -- no Gram algebra.  -> dict with the bounds of the module docstring."""
    ci, co, n, h, w = c["shape"]
    count = n * h * w
    v = lambda t: t.view(1, -1, 1, 1)
    y, x, wt, dp, gamma = c["y"], c["x"], c["w"], c["dp"], c["gamma"]
    dz = unwindows(f["pick"].double() * f["gate"].double().unsqueeze(-1) * dp.unsqueeze(-1), h, w)
    xhat = (y - v(mean)) * v(invstd)
    sdz, sdzx = dz.sum(dim=(0, 2, 3)), (dz * xhat).sum(dim=(0, 2, 3))
    m1, m2 = (sdz / count, sdzx / count) if training else (torch.zeros_like(sdz), torch.zeros_like(sdzx))
    k = gamma * invstd
    dyraw = v(k) * (dz - v(m1) - xhat * v(m2))
    dW, _ = R.conv_grads(x, wt, dyraw, want_dx=False)
    # magnitudes of the kernel's terms: |S1[k]| <= sum |dz| P, |m1 sp| = |m1| sum P, |m2 inv (w G - mean sp)| <= M2 inv sum (conv(|x|, |w|) + |mean|) P,
    # with M2 = the magnitude of m2's own terms (rowdot(w, S1) - mean sum dz) inv / n
    yabs = F.conv2d(x.abs(), wt.abs(), padding=1)
    sdzy_abs = (dz.abs() * yabs).sum(dim=(0, 2, 3))
    m2_abs = (sdzy_abs + mean.abs() * sdz.abs()) * invstd / count if training else torch.zeros_like(sdz)
    terms = v(k.abs()) * (dz.abs() + v(m1.abs()) + v(m2_abs * invstd) * (yabs + v(mean.abs())))
    absW, _ = R.conv_grads(x.abs(), wt.abs(), terms, want_dx=False)
    # unsafe windows: the gradient may sit at another pixel of the window or be gated the other way -- at most |dp| moves at two pixels (|x| <= 2,
    # 2 |k| |dp| each) and the two means move by |dp| / n and 2 |dp| max|xhat| / n (times sum |x| <= 2 n and sum |xhat x| <= 2 n max|xhat|)
    un = (~f["safe"]).double() * dp.abs()
    xm = xhat.abs().amax(dim=(0, 2, 3))
    flip = k.abs() * un.sum(dim=(0, 2, 3)) * (4 + (2 + 4 * xm * xm if training else 0))
    flip_g = un.sum(dim=(0, 2, 3)) * 2 * xm
    flip_b = un.sum(dim=(0, 2, 3))
    cancel = 64 * 2.0 ** -52
    bW = U * dW.abs() + cancel * absW + flip.view(-1, 1, 1, 1)
    bG = U * sdzx.abs() + cancel * (sdzy_abs + mean.abs() * sdz.abs()) * invstd + flip_g
    bB = flip_b
    return dict(dW=dW, dgamma=sdzx, dbeta=sdz, bW=bW, bG=bG, bB=bB, dz=dz)


def compare_backward(r, got):
    """got: fp64 dW [Co, Ci, 3, 3], dgamma, dbeta [Co].  -> (fails, ratios)"""
    fails, ratios = [], {}
    for name, ref, b in (("dW", r["dW"], r["bW"]), ("dgamma", r["dgamma"], r["bG"]), ("dbeta", r["dbeta"], r["bB"])):
        err = (got[name] - ref).abs()
        over = err > b
        ratios[name] = float(torch.where(err > 0, err / b.clamp_min(1e-300), torch.zeros_like(err)).max())
        if over.any():
            i = tuple(over.nonzero()[0].tolist())
            fails.append(f"{name}: {int(over.sum())} of {ref.numel()} elements above the bound, first at {list(i)}: got {got[name][i].item()!r} want {ref[i].item()!r} bound {b[i].item():.3g}")
    return fails, ratios


def eval_backward(c):
    """eval mode: the hand-made statistics; everything exact -> dW, dgamma, dbeta (compared with torch.equal after one fp32 rounding)"""
    r = R.reference(c, False, with_bounds=False)
    return dict(dW=R.fl32(r["dW"]), dgamma=R.fl32(r["dgamma"]), dbeta=R.fl32(r["dbeta"]))


# ---- what a kernel with a wrong carry from block to block would hand back --------------------------------------------------------------------------
def block_slices(shape, b, pooled=True):
    """block b (row-major inside an image) -> (image, row slice, column slice) of the pooled map (or of the frame)"""
    _, _, n, h, w = shape
    bx, by = -(-w // 16), -(-h // 8)
    img, r = divmod(b, bx * by)
    ry, rx = divmod(r, bx)
    s = 2 if pooled else 1
    return img, slice(ry * 8 // s, min(ry * 8 + 8, h) // s), slice(rx * 16 // s, min(rx * 16 + 16, w) // s)


def mutate_stale_halo(shape, pooled, b):
    """(a) block b computed from block b - 1's halo image (the double buffer not flipped, or the single image rewritten too late): its pooled
    values are block b - 1's"""
    out = pooled.clone()
    n0, r0, c0 = block_slices(shape, b - 1)
    n1, r1, c1 = block_slices(shape, b)
    src = pooled[n0, :, r0, c0]
    hh, ww = out[n1, :, r1, c1].shape[-2:]
    out[n1, :, r1, c1] = src[..., :hh, :ww]
    return out


def mutate_sentinel_block(shape, pooled, b):
    """(b) block b -- a run's last -- never written"""
    out = pooled.clone()
    n1, r1, c1 = block_slices(shape, b)
    out[n1, :, r1, c1] = SENTINEL
    return out


def mutate_stale_row(c, blocks):
    """(c) one stale partial row added into the Gram sums: the patches of `blocks` counted twice -> the make_case dict whose sums a kernel would
    then finalise (only y of those blocks doubled in the sums: returned as the extra sum y, sum y^2)"""
    y = c["y"]
    e1, e2 = torch.zeros(y.shape[1], dtype=torch.float64), torch.zeros(y.shape[1], dtype=torch.float64)
    for b in blocks:
        n1, r1, c1 = block_slices(c["shape"], b, pooled=False)
        yy = y[n1, :, r1, c1]
        e1 += yy.sum(dim=(1, 2))
        e2 += (yy * yy).sum(dim=(1, 2))
    return e1, e2


def stats_outputs(s, c, extra=(0.0, 0.0)):
    """what s1_gram_stats_kernel hands back for the sums of s (+ extra): double algebra, one fp32 rounding per output, fp32 products after it"""
    n = s["count"]
    f = lambda t: t.float()
    m = (s["s1"] + extra[0]) * (1.0 / n)
    var = ((s["s2"] + extra[1]) * (1.0 / n) - m * m).clamp_min(0)
    mean, invstd, unb = f(m), f(1.0 / torch.sqrt(var + EPS)), f(var * (n / (n - 1.0)))
    mom, g, b = torch.tensor(MOMENTUM, dtype=torch.float32), f(c["gamma"]), f(c["beta"])
    scale = g * invstd
    out = dict(mean=mean, invstd=invstd, scale=scale, shift=b - mean * scale, run_mean=(1 - mom) * f(s["r0"]) + mom * mean, run_var=(1 - mom) * f(s["rv0"]) + mom * unb)
    out = {k: t.double() for k, t in out.items()}
    out.update(nbt=1, pad_zero=True)
    return out
