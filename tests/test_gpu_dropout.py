"""Train-mode dropout, checked exactly (run with -m gpu on an MI355X).

Dropout in the HIP library is a stateless counter hash of (seed, element index), so oracle/dropout_masks.py reproduces every mask bit on the
host.  Two kinds of test follow from that:

A. mask read-out, bit-exact, no tolerance: inputs chosen so that each kernel's output IS its mask (attention with zero scores and one-hot
   values, the encoder's zeros, dropout of a tensor of ones) -- compared element for element with the replica;
B. train mode against the masked oracle: the fp64 reference (oracle/hybrid_ref_masked.py) and the bf16-rounded one (oracle/hybrid_ref_bf16.py)
   applying the SAME masks as the kernels, at the gates of tests/test_gpu_parity.py -- forward values and every gradient.

Seeds are fixed by passing them to the operators, or, through the modules, by replacing ops.next_seed; the device step counter (seed_inc,
graph replays) is set explicitly, including values that make seed + counter wrap around 2^64.
"""
import contextlib
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import padding_masks  # noqa: E402
from oracle import dropout_masks as DM  # noqa: E402
from oracle import hybrid_ref as R  # noqa: E402
from oracle import hybrid_ref_bf16 as RB  # noqa: E402
from oracle import hybrid_ref_masked as RM  # noqa: E402
from test_gpu_parity import BF16_FWD, BF16_GRAD, TOL, check  # noqa: E402

MASK63 = (1 << 63) - 1


def P():
    import transformer_cnn_hybrid_network_for_video_processing_amd as pkg
    return pkg


def _lib():
    from transformer_cnn_hybrid_network_for_video_processing_amd import _lib
    return _lib


def _st():
    return torch.cuda.current_stream().cuda_stream


def _counter(value):
    """The device step counter (int64 [1]); `value` as the kernels read it, i.e. mod 2^64."""
    v = value & ((1 << 64) - 1)
    return torch.tensor([v - (1 << 64) if v > MASK63 else v], dtype=torch.int64, device="cuda")


def _chk(got, want, tol, what, mode, floor=0.0, bwd=False):
    # bf16x3 gradients: relative L2 (a pre-activation within 1e-5 of zero may flip its ReLU; tests/test_gpu_parity.py, TOL)
    check(got, want, tol, what, mode, floor=floor, kind="dropout bwd" if (bwd and mode == "bf16x3") else None)


@pytest.fixture
def fixed_seed(monkeypatch):
    """ops.next_seed() -> the given seed; records every call (the modules draw one seed per operator call)."""
    from transformer_cnn_hybrid_network_for_video_processing_amd import ops
    calls = []

    def use(seed):
        def nxt():
            calls.append(seed)
            return seed
        monkeypatch.setattr(ops, "next_seed", nxt)
        return calls
    return use


@pytest.fixture
def step_counter():
    """ops.set_step_counter(<value>) for one test; cleared afterwards."""
    from transformer_cnn_hybrid_network_for_video_processing_amd import ops

    def use(value):
        c = None if value is None else _counter(value)
        ops.set_step_counter(c)
        return c
    yield use
    ops.set_step_counter(None)


# =============================================================================================================================
# A. mask read-out
# =============================================================================================================================
def _attention_readout(long, dt, B, S, H, p, seed, inc=None):
    """q = k = 0: every probability is exactly 1/S.  V is one-hot over a window of keys (head feature j of window w0 = key w0 + j), so
    out[b, q, h*dh + j] = mult(key w0 + j) / S.  Returns (got [B*H, S, S] fp32 from the kernels, want [B*H, S, S] multipliers / S)."""
    lib = _lib().lib
    dh = 64 if long else max(8, -(-S // 8) * 8)
    D = H * dh
    tdt = torch.float32 if dt == _lib().HYB_F32 else torch.bfloat16
    qk = torch.zeros(B, S, D, dtype=tdt, device="cuda")
    got = torch.empty(B * H, S, S, dtype=torch.float32, device="cuda")
    stats = torch.empty(B * H * S * 2, dtype=torch.float32, device="cuda")
    ws = None
    if long:
        ws = torch.empty(lib.query("hyb_attention_long_workspace", dt, B, S, D, H), dtype=torch.uint8, device="cuda")
    for w0 in range(0, S, dh):
        n = min(dh, S - w0)
        v = torch.zeros(B, S, H, dh, dtype=tdt, device="cuda")
        j = torch.arange(n, device="cuda")
        v[:, w0 + j, :, j] = 1
        out = torch.full((B, S, D), float("nan"), dtype=tdt, device="cuda")
        if long:
            lib.call("hyb_attention_long_fwd", dt, qk.data_ptr(), qk.data_ptr(), v.data_ptr(), D, None, out.data_ptr(), stats.data_ptr(), B, S, D, H,
                     float(p), seed, inc.data_ptr() if inc is not None else None, ws.data_ptr(), ws.numel(), _st())
        else:
            lib.call("hyb_attention_fwd", dt, qk.data_ptr(), qk.data_ptr(), v.data_ptr(), None, out.data_ptr(), stats.data_ptr(), B, S, D, H, float(p),
                     seed, _st())
        o = out.float().reshape(B, S, H, dh).permute(0, 2, 1, 3).reshape(B * H, S, dh)
        assert torch.isfinite(o).all()
        assert (o[:, :, n:] == 0).all()                   # features past the window: no key behind them
        got[:, :, w0:w0 + n] = o[:, :, :n]
    m = DM.mult(DM.with_step(seed, p, None if inc is None else int(inc.item())), DM.attn_index(B, H, S), p)
    want = torch.from_numpy(m.astype(np.float64) / S)
    return got.cpu().double(), want


def _assert_mask(got, want, dt, what):
    zg, zw = got == 0, want == 0
    bad = (zg != zw).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.shape[0]} of {zw.numel()} mask elements differ (first at {bad[0].tolist()})"
    assert 0 < zw.double().mean().item() < 1
    if dt == _lib().HYB_F32:
        err = ((got - want).abs() / want.abs().clamp_min(1e-30))[~zw].max().item()
        assert err <= 1e-6, f"{what}: kept values off by {err:.2e} relative"


@pytest.mark.parametrize("dtn", ["fp32", "bf16"])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("B,S,H", [(4, 1, 2), (3, 5, 4), (2, 16, 8), (3, 17, 2), (2, 40, 3), (2, 64, 2),
                                   (683, 7, 3)])      # 2049 problems: four per workgroup, a ragged last workgroup of one
def test_short_attention_dropout_mask_is_the_replica(dtn, p, B, S, H):
    L = _lib()
    dt = L.HYB_F32 if dtn == "fp32" else L.HYB_BF16
    seed = 0x0123456789ABCDEF ^ (S * 7919 + B)
    got, want = _attention_readout(False, dt, B, S, H, p, seed)
    _assert_mask(got, want, dt, f"short attention {dtn} B={B} S={S} H={H} p={p}")


@pytest.mark.parametrize("dtn", ["fp32", "bf16"])
@pytest.mark.parametrize("S,p,inc", [(65, 0.1, None), (96, 0.5, None), (130, 0.1, None), (200, 0.5, None),
                                     (96, 0.1, 1000), (130, 0.5, -(1 << 40))])      # a step counter: seed + counter wraps past 2^64
def test_long_attention_dropout_mask_is_the_replica(dtn, S, p, inc):
    L = _lib()
    dt = L.HYB_F32 if dtn == "fp32" else L.HYB_BF16
    B, H = 2, 3
    seed = (1 << 64) - 17 if inc is not None else 0xDEADBEEF + S        # (wraps: (2^64 - 17) + 1000, (2^64 - 17) - 2^40 as uint64)
    got, want = _attention_readout(True, dt, B, S, H, p, seed, _counter(inc) if inc is not None else None)
    _assert_mask(got, want, dt, f"long attention {dtn} S={S} p={p} inc={inc}")


def _encoder_params(D, Hid, L, H, seed=3):
    torch.manual_seed(seed)
    ref = R.TransformerEncoder(D, Hid, L, H, 0.0)
    with torch.no_grad():
        for ln in ref.layer_norm:
            ln.weight.copy_(torch.randn(D) * 0.3 + 1.0)
            ln.bias.copy_(torch.randn(D) * 0.1)
    return ref


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("B,S,D,Hid,L,H", [(2, 16, 64, 128, 2, 4), (3, 9, 768, 1024, 2, 8), (2, 96, 64, 128, 1, 4)])
@pytest.mark.parametrize("p,inc", [(0.1, None), (0.5, None), (0.5, (1 << 63) + 5)])
def test_layer_dropout_zeros_are_the_replica(mode, B, S, D, Hid, L, H, p, inc):
    """attn_p = 0, layer_p = p: the encoder's output is zero exactly where the last layer's per-layer dropout drops (quirk Q6)."""
    from transformer_cnn_hybrid_network_for_video_processing_amd import ops
    ref = _encoder_params(D, Hid, L, H)
    hip = P().TransformerEncoder(D, Hid, L, H, p, compute_dtype=mode)
    hip.load_state_dict(ref.state_dict())
    hip = hip.cuda()
    params = [t.detach() for t in hip._flat_params()]
    x = ops.to_compute(torch.randn(B, S, D, device="cuda"), hip._dt)
    seed = 0x5DEECE66D
    c = _counter(inc) if inc is not None else None
    y0, _ = torch.ops.hybrid.encoder(x, None, params, hip._dt, Hid, L, H, 0.0, 0.0, seed, c)
    assert (y0 != 0).all() and torch.isfinite(y0.float()).all()
    y, _ = torch.ops.hybrid.encoder(x, None, params, hip._dt, Hid, L, H, 0.0, p, seed, c)
    want = DM.layer_mask(seed, L - 1, B, S, D, p, inc) == 0
    got = (y == 0).cpu().numpy()
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} elements differ"
    assert 0 < want.mean() < 1


@pytest.mark.parametrize("p,inc", [(0.1, None), (0.5, None), (0.5, 77)])
def test_dropout2d_planes_are_the_replica(p, inc):
    from transformer_cnn_hybrid_network_for_video_processing_amd import ops
    N, Hh, Ww, C = 5, 7, 9, 12                          # NHWC, H*W = 63 (ragged), C >= 8
    seed = 987654321
    x = torch.ones(N, Hh, Ww, C, device="cuda")
    y = ops.dropout2d_op(x, p, seed, _counter(inc) if inc is not None else None).cpu()
    s = (seed + inc) if inc is not None else seed           # (dropout2d adds the counter unconditionally)
    m = torch.from_numpy(DM.mult(s, DM.plane_index(N, C), p))
    assert torch.equal(y, m[:, None, None, :].expand(N, Hh, Ww, C))
    assert 0 < (m == 0).double().mean().item() < 1


@pytest.mark.parametrize("p,inc", [(0.1, None), (0.5, -3)])
def test_fct_dropout_elements_are_the_replica(p, inc):
    from transformer_cnn_hybrid_network_for_video_processing_amd import ops
    shape = (3, 5, 7, 11)
    seed = 42
    x = torch.ones(shape, device="cuda")
    y = ops.fct_dropout_op(x, p, seed, _counter(inc) if inc is not None else None).cpu()
    s = (seed + inc) & ((1 << 64) - 1) if inc is not None else seed
    m = torch.from_numpy(DM.mult(s, np.arange(x.numel(), dtype=np.uint64), p)).reshape(shape)
    assert torch.equal(y, m)


# =============================================================================================================================
# B. train mode against the masked oracle
# =============================================================================================================================
def _oracle(ref):
    """fp64 copy of an oracle module: the fp64 reference, or (bf16 mode) the accumulation of the bf16-rounded one."""
    import copy
    return copy.deepcopy(ref).double()


@pytest.mark.parametrize("mode", ["fp32", "bf16", "bf16x3"])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("B,S,D,H,use_mask", [(683, 7, 24, 3, False), (300, 16, 64, 8, True),     # packed: four problems per workgroup
                                              (3, 40, 96, 2, True), (2, 17, 32, 4, False),          # 3 and 2 token tiles, ragged
                                              (2, 96, 64, 4, False), (2, 70, 32, 4, True),          # > 64 tokens: online-softmax kernels
                                              # a padding mask (tests/padding_masks.py): dropout on the uniform weights of fully masked rows,
                                              # and the backward's regenerated mask on them
                                              (2, 16, 64, 4, "pad"), (2, 70, 32, 4, "pad")])
def test_multihead_attention_train_mode_matches_masked_oracle(mode, p, B, S, D, H, use_mask, fixed_seed):
    ftol, gtol = TOL[mode]
    if mode == "bf16" and S > 64:
        ftol, gtol = 2 * ftol, 2 * gtol                 # as in tests/test_gpu_parity.py: fp32 long-sequence core on bf16 operands
    seed = 0x1F2E3D4C5B6A7988 + S
    calls = fixed_seed(seed)
    torch.manual_seed(2)
    ref = R.MultiheadAttention(D, H)
    hip = P().MultiheadAttention(D, H, compute_dtype=mode)
    hip.load_state_dict(ref.state_dict())
    hip = hip.cuda().train()
    hip.dropoutLayer.p = p
    q, k, v = (torch.randn(B, S, D) for _ in range(3))
    mask = None
    if use_mask == "pad":
        mask = padding_masks.pad(B, S)
        assert min(padding_masks.row_census(mask, B, S, H)) > 0         # fully masked rows and rows with a visible key
    elif use_mask:
        mask = (torch.rand(B, S, S) > 0.3).float()
        mask[:, :, 0] = 1
    r = torch.randn(B, S, D)
    drop = DM.mult(seed, DM.attn_index(B, H, S), p)
    orc = _oracle(ref)
    qr, kr, vr = (t.clone().double().requires_grad_(True) for t in (q, k, v))
    md = mask.double() if mask is not None else None
    if mode == "bf16":
        yr = RB.mha(orc, qr, kr, vr, md, drop)
        (yr * r.bfloat16().double()).sum().backward()
    else:
        yr = RM.mha(orc, qr, kr, vr, md, drop)
        (yr * r.double()).sum().backward()
    qh, kh, vh = (t.cuda().requires_grad_(True) for t in (q, k, v))
    yh = hip(qh, kh, vh, mask.cuda() if mask is not None else None)
    (yh * r.cuda()).sum().backward()
    assert calls == [seed]
    _chk(yh, yr, ftol, "out", mode)
    G = max(t.grad.abs().max().item() for t in (qr, kr, vr))
    for name, a, b in (("dq_in", qh, qr), ("dk_in", kh, kr), ("dv_in", vh, vr)):
        _chk(a.grad, b.grad, gtol, name, mode, floor=1e-4 * G, bwd=True)
    hp = dict(hip.named_parameters())
    Gp = max(t.grad.abs().max().item() for t in orc.parameters())
    for n_, pr in orc.named_parameters():
        _chk(hp[n_].grad, pr.grad, gtol, "grad:" + n_, mode, floor=1e-4 * Gp, bwd=True)


@contextlib.contextmanager
def _relu_margin(enc):
    """Smallest |pre-activation| of the ReLUs in front of q, k, v and the FFN (src L70, L107) while the fp64 oracle runs.  The fp32 mode's
    max-norm gradient gate presumes that fp32 arithmetic takes every ReLU decision the fp64 oracle takes: a pre-activation within fp32
    rounding of zero (~1e-6 for these widths) may land on the other side, which moves one row of a weight gradient by O(1) -- a valid gradient
    of a function 1e-7 away (one measured case: a layer-1 query unit at 2.6e-7 gave 6e-2 on that row; every other element agreed to 3e-4).
    The inputs and masks are fixed, so this is a property of the chosen data, and the counter value of the layer_p = 0.5 runs is one where no
    shape has such a tie."""
    m = [math.inf]

    def hook(mod, inp, out):
        m[0] = min(m[0], out.detach().abs().min().item())
    hs = [getattr(a, n).register_forward_hook(hook) for a in enc.attention_layers for n in ("query_layer", "key_layer", "value_layer")]
    hs += [ff[0].register_forward_hook(hook) for ff in enc.feedforward_layers]
    try:
        yield m
    finally:
        for h in hs:
            h.remove()


# (B, S, D, Hid, L, H) and the path each takes -- hyb_gemm_nt_ln (csrc/linear.hip) fuses the LayerNorm into the next GEMM only in bf16, for grids of
# at most 256 32x32 tiles (x 3 for Q | K | V) and 256 <= D with the 32 x (D + 16) bf16 row image in 64 KB (D <= 1008); <1> up to D = 512, <2> above
ENC_SHAPES = [
    (8, 16, 512, 2048, 2, 8),      # bf16: gemm_nt_ln<1> for the second layer's Q|K|V (16 x 4 x 3 tiles) and both FFN-in GEMMs (64 x 4)
    (2, 16, 768, 1024, 2, 8),      # bf16: gemm_nt_ln<2> (Q|K|V 24 x 1 x 3, FFN 32 x 1)
    (3, 9, 768, 1024, 2, 8),       # bf16: gemm_nt_ln<2>, M = 27: a ragged row tile
    (2, 20, 1008, 1024, 2, 9),     # bf16: gemm_nt_ln<2> at its real upper bound, 32 x 1024 x 2 B = 64 KB of LDS
    (2, 20, 1024, 1024, 2, 8),     # just past it: the LayerNorm as its own launch (ln_residual_fwd), plain GEMMs
    (2, 8, 520, 512, 2, 5),        # bf16: gemm_nt_ln<2> with D not a multiple of 32: a ragged column tile (65 row chunks of 8)
    (2, 96, 512, 512, 2, 8),       # Q|K|V grid 16 x 6 x 3 = 288 > 256 tiles (unfused), FFN-in 16 x 6 fused (<1>); S > 64: long attention
    (2, 16, 64, 128, 1, 4),        # one layer: only the last layer's stand-alone LayerNorm draws the layer mask (D < 256: never fused)
    (2, 16, 64, 128, 3, 4),        # three layers: the backward's layer loop past two
    (1, 8, 32, 64, 4, 2),          # four layers: per-layer weight conversion (L > 3)
]


@pytest.mark.parametrize("mode", ["fp32", "bf16", "bf16x3"])
@pytest.mark.parametrize("layer_p", [0.1, 0.5])
@pytest.mark.parametrize("B,S,D,Hid,L,H", ENC_SHAPES)
def test_transformer_encoder_train_mode_matches_masked_oracle(mode, layer_p, B, S, D, Hid, L, H, fixed_seed, step_counter):
    attn_p = 0.1
    inc = None if layer_p == 0.1 else (1 << 64) - 8000024    # a step counter whose addition wraps every layer's seeds (value: see _relu_margin)
    ftol, gtol = TOL[mode]
    seed = 0x243F6A8885A308D3 + D
    calls = fixed_seed(seed)
    step_counter(inc)
    ref = _encoder_params(D, Hid, L, H)
    hip = P().TransformerEncoder(D, Hid, L, H, layer_p, compute_dtype=mode)
    hip.load_state_dict(ref.state_dict())
    hip = hip.cuda().train()
    for a in hip.attention_layers:
        a.dropoutLayer.p = attn_p
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, S, D, generator=g)
    mask = None
    if L == 4:
        mask = (torch.rand(B, S, S, generator=g) > 0.3).float()
        mask[:, :, 0] = 1
    r = torch.randn(B, S, D, generator=g)
    am, lm = DM.encoder_masks(seed, L, B, S, D, H, attn_p, layer_p, inc)
    orc = _oracle(ref)
    xr = x.clone().double().requires_grad_(True)
    md = mask.double() if mask is not None else None
    if mode == "bf16":
        yr = RB.encoder(orc, xr, md, am, lm)
        (yr * r.bfloat16().double()).sum().backward()
        ftol, gtol = 3 * L * BF16_FWD, 2 * L * BF16_GRAD     # the encoder's compounding rounding points (tests/test_gpu_parity.py)
        if S > 64:
            ftol, gtol = 2 * ftol, 2 * gtol
    else:
        with _relu_margin(orc) as margin:
            yr = RM.encoder(orc, xr, md, am, lm)
        (yr * r.double()).sum().backward()
        if mode == "fp32":
            assert margin[0] > 5e-7, f"test data: a ReLU pre-activation {margin[0]:.1e} from zero (see _relu_margin)"
    xh = x.cuda().requires_grad_(True)
    yh = hip(xh, mask.cuda() if mask is not None else None)
    (yh * r.cuda()).sum().backward()
    assert calls == [seed]
    assert torch.equal((yh == 0).cpu(), torch.from_numpy(lm[-1] == 0))      # the last layer's mask, exactly
    _chk(yh, yr, ftol, "out", mode)
    _chk(xh.grad, xr.grad, gtol, "dx", mode, bwd=True)
    hp = dict(hip.named_parameters())
    Gp = max(t.grad.abs().max().item() for t in orc.parameters())
    for n_, pr in orc.named_parameters():
        _chk(hp[n_].grad, pr.grad, gtol, "grad:" + n_, mode, floor=1e-4 * Gp, bwd=True)


# the fused temporal part: token projection, encoder, and the last layer's LayerNorm + dropout inside the head / loss launch
# (layernorm.hip temporal_tail_fwd_kernel) -- the only caller of that dropout site
@pytest.mark.parametrize("mode", ["fp32", "bf16x3"])
@pytest.mark.parametrize("L", [1, 2, 3])
def test_fused_temporal_loss_train_mode_matches_masked_oracle(mode, L, fixed_seed, step_counter):
    B, T, D, H, Hid, C, Hh, Ww = 3, 8, 64, 4, 128, 32, 2, 3
    attn_p = layer_p = 0.1
    inc = 0x7FFFFFFF00000000 + 12345
    seed = 0x6A09E667F3BCC908
    ftol, gtol = TOL[mode]
    calls = fixed_seed(seed)
    step_counter(inc)
    torch.manual_seed(7)
    kw = dict(cnn_channels=(16, C), d_model=D, num_heads=H, num_layers=L, hidden_dim=Hid, dropout=layer_p)
    ref = R.TransformerCNNHybridRef(**kw)
    with torch.no_grad():
        for ln in ref.encoder.layer_norm:
            ln.weight.copy_(torch.randn(D) * 0.3 + 1.0)
            ln.bias.copy_(torch.randn(D) * 0.1)
    hip = P().TransformerCNNHybrid(compute_dtype=mode, **kw)
    hip.load_state_dict(ref.state_dict())
    hip = hip.cuda().train()
    for a in hip.encoder.attention_layers:
        a.dropoutLayer.p = attn_p
    assert hip._fused()
    g = torch.Generator().manual_seed(11)
    h = torch.rand(B * T, Hh, Ww, C, generator=g)                # the last pooled map, NHWC (C = 32: no padded channels)
    y = torch.randint(0, 8, (B,), generator=g)
    am, lm = DM.encoder_masks(seed, L, B, T, D, H, attn_p, layer_p, inc)
    orc = _oracle(ref)
    hr = h.clone().double().requires_grad_(True)
    lr_ = RM.temporal(orc, hr.mean(dim=(1, 2)), B, None, am, lm)
    loss_r = R.loss_fn(lr_, y)
    loss_r.backward()
    hh = h.cuda().requires_grad_(True)
    loss_h, lh = hip.forward_temporal_loss(hh, B, y.cuda())
    loss_h.backward()
    assert calls == [seed]
    _chk(lh, lr_, ftol, "logits", mode)
    _chk(loss_h.reshape(1), loss_r.reshape(1), ftol, "loss", mode)
    _chk(hh.grad, hr.grad, gtol, "dh", mode, bwd=True)
    hp = dict(hip.named_parameters())
    tparams = [(n_, p_) for n_, p_ in orc.named_parameters() if not n_.startswith("encoder") or n_.startswith("encoder.")]
    Gp = max(p_.grad.abs().max().item() for _, p_ in tparams)
    for n_, pr in tparams:
        _chk(hp[n_].grad, pr.grad, gtol, "grad:" + n_, mode, floor=1e-4 * Gp, bwd=True)


# the whole model, one training step in fp32, eagerly and as the replayed graph
MODEL_KW = dict(cnn_channels=(32, 64), d_model=64, num_heads=4, num_layers=2, hidden_dim=128, dropout=0.1)


def _model_check(hip_sd, x, y, seed, inc, logits, loss, grads):
    """The masked fp64 oracle on the state dict `hip_sd` with the masks drawn at (seed, inc): logits and loss at 1e-3, and every gradient
    outside the conv stack (the full-size fp32 gates, tests/test_gpu_fullsize.py)."""
    torch.manual_seed(0)
    ref = R.TransformerCNNHybridRef(**MODEL_KW)
    ref.load_state_dict(hip_sd, strict=False)
    ref = ref.double().train()
    B, T = x.shape[:2]
    am, lm = DM.encoder_masks(seed, 2, B, T, 64, 4, 0.1, 0.1, inc)
    lr_ = RM.forward(ref, x.double(), None, am, lm)
    loss_r = R.loss_fn(lr_, y)
    loss_r.backward()
    check(logits, lr_, 1e-3, "logits")
    check(loss.reshape(1), loss_r.reshape(1), 1e-3, "loss")
    rp = [(n_, p_) for n_, p_ in ref.named_parameters() if not n_.startswith("encoder") or n_.startswith("encoder.")]
    Gp = max(p_.grad.abs().max().item() for _, p_ in rp)
    for n_, pr in rp:
        check(grads[n_], pr.grad, 1e-3, "grad:" + n_, floor=1e-4 * Gp)


def _model_setup():
    torch.manual_seed(0)
    hip = P().TransformerCNNHybrid(compute_dtype="fp32", **MODEL_KW).cuda().train()
    g = torch.Generator().manual_seed(3)
    x = torch.rand(2, 8, 3, 32, 32, generator=g)
    y = torch.randint(0, 8, (2,), generator=g)
    return hip, x, y


def _state(hip):
    return {k: v.detach().cpu().clone() for k, v in hip.state_dict().items() if "num_batches_tracked" not in k}


def test_whole_model_training_step_with_dropout_matches_masked_oracle_eager(fixed_seed):
    seed = 0x3C6EF372FE94F82B
    calls = fixed_seed(seed)
    hip, x, y = _model_setup()
    sd = _state(hip)
    logits = hip(x.cuda())
    loss = P().HybridCrossEntropyLoss()(logits, y.cuda())
    loss.backward()
    assert calls == [seed]
    _model_check(sd, x, y, seed, None, logits, loss, {n_: p_.grad for n_, p_ in hip.named_parameters()})


def test_whole_model_graph_replay_draws_seed_plus_counter(fixed_seed):
    """GraphedTrainStep: the captured launches keep their by-value seed and add the device counter -- one replay's logits, loss and gradients
    are the masked oracle's at masks drawn with seed + counter (the counter value before the replay)."""
    seed = 0x510E527FADE682D1
    calls = fixed_seed(seed)
    hip, x, y = _model_setup()
    opt = P().HybridAdamW(hip.parameters(), lr=1e-3)
    tr = P().GraphedTrainStep(hip, P().HybridCrossEntropyLoss(), opt, x.cuda(), y.cuda(), warmup=2)
    try:
        assert calls and set(calls) == {seed}
        tr.step()                                           # one replay past the warm-up: the counter is not where a fresh step would start
        torch.cuda.synchronize()
        c = int(tr.counter.item())
        assert c >= 3
        sd = _state(hip)
        loss = tr.step()
        torch.cuda.synchronize()
        names = [n_ for n_, _ in hip.named_parameters()]
        grads = {n_: p_.grad.detach().clone() for n_, p_ in hip.named_parameters()}
        assert len(grads) == len(names) and all(g is not None for g in grads.values())
        _model_check(sd, x, y, seed, c, tr.logits.clone(), loss.detach().clone(), grads)
        assert int(tr.counter.item()) == c + 1
    finally:
        tr.close()
