"""Attention under masks with FULLY MASKED query rows (run with -m gpu on an MI355X).

Every other masked test of the suite keeps key 0 visible in every row, so no fully masked row ever reached a kernel -- yet that row is what
the most common real mask produces: ``valid (x) valid`` for clips of different lengths zeroes the whole row of every padded frame, and so
does a ``[B,S,1]`` query mask.  The reference (oracle/hybrid_ref.py, ``masked_fill(mask == 0, -1e9)`` then softmax) fixes the semantics:

  forward    the row is uniform, 1/S per key: the output is the plain mean of the problem's value rows;
  backward   masked_fill passes NO gradient to a masked score: the row adds nothing to dq or dk, and dv gets 1/S of its dO.

A backward kernel that only replaces the recomputed score by -1e9 gets the second line right by accident for partially masked rows
(exp(-1e9 - max) underflows) and wrong for fully masked ones (max = -1e9, P = 1/S, dS != 0); the online-softmax kernels also have to
recover 1/S from a saved log-sum-exp that fp32 rounds to -1e9.

No tolerance is new: module-level parity runs at the gates and error norms of tests/test_gpu_parity.py (TOL, check, check_param_grads, the
doubling for bf16 with S > 64, the encoder's 3 L / 2 L factors), the whole model at those of test_full_model_logits_loss_and_grads_match_oracle,
predict at those of tests/test_gpu_infer.py.  tests/test_oracle.py measures the fp32 CPU oracle against fp64 on every module-level case
(at least 10 x inside the fp32 gates) and pins the oracle's own fully-masked-row semantics.  Mask builders and the case table:
tests/padding_masks.py.  Measured figures (run with -s): profiles/padding_mask_errors.txt.
"""
import copy
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import padding_masks as PM  # noqa: E402
from oracle import hybrid_ref as R  # noqa: E402
from oracle import hybrid_ref_bf16 as RB  # noqa: E402
from test_gpu_parity import TOL, as_oracle, check, check_param_grads, rel  # noqa: E402

MODES = ["fp32", "bf16", "bf16x3"]


def P():
    import transformer_cnn_hybrid_network_for_video_processing_amd as pkg
    return pkg


def _norms(mode):
    """The norms `check` applies: (forward is relative L2, gradients are relative L2)."""
    return mode == "bf16", mode != "fp32"


def _report(what, mode, fwd, grad, ftol, gtol):
    print(f"\n[{what} {mode}] forward {fwd:.2e} (gate {ftol:.1e}); worst gradient {grad:.2e} (gate {gtol:.1e})")


def _assert_rows(mname, mask, B, S, H):
    """The case has what it is here for -- a condition on the test data, not a measurement."""
    n_full, n_open = PM.row_census(mask, B, S, H)
    assert n_open > 0, f"{mname}: no row with a visible key"
    if mname == "keys":
        assert n_full == 0, "keys is the control: no fully masked row"
    else:
        assert n_full > 0, f"{mname}: no fully masked (problem, query) row at B={B} S={S} H={H}"


# --------------------------------------------------------------------------------------------
# module-level parity
# --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mha_reference(B, S, D, H, mname, rounded):
    """Seeded module, inputs, mask and the oracle's result, computed once per (case, oracle) and left unchanged."""
    torch.manual_seed(2)
    ref = R.MultiheadAttention(D, H).eval()
    q, k, v = (torch.randn(B, S, D) for _ in range(3))
    r = torch.randn(B, S, D)
    mask = PM.build(mname, B, S)
    orc = as_oracle(ref, "bf16" if rounded else "fp32")
    dt = next(orc.parameters()).dtype
    qr, kr, vr = (t.clone().to(dt).requires_grad_(True) for t in (q, k, v))
    if rounded:
        yr = RB.mha(orc, qr, kr, vr, mask)
        (yr * r.bfloat16().double()).sum().backward()
    else:
        yr = ref(qr, kr, vr, mask)
        (yr * r).sum().backward()
    return ref, orc, (q, k, v, r, mask), yr.detach(), (qr.grad, kr.grad, vr.grad)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,S,D,H,mname", PM.MHA_CASES)
def test_multihead_attention_with_fully_masked_rows_matches_oracle(mode, B, S, D, H, mname):
    ftol, gtol = TOL[mode]
    if mode == "bf16" and S > 64:
        ftol, gtol = 2 * ftol, 2 * gtol                 # as tests/test_gpu_parity.py: fp32 long-sequence core on bf16 operands
    ref, orc, (q, k, v, r, mask), yr, (dqr, dkr, dvr) = _mha_reference(B, S, D, H, mname, mode == "bf16")
    _assert_rows(mname.partition(":")[0], mask, B, S, H)
    hip = P().MultiheadAttention(D, H, compute_dtype=mode)
    hip.load_state_dict(ref.state_dict())
    hip = hip.cuda().eval()
    qh, kh, vh = (t.cuda().requires_grad_(True) for t in (q, k, v))
    yh = hip(qh, kh, vh, mask.cuda())
    (yh * r.cuda()).sum().backward()
    l2f, l2g = _norms(mode)
    G = max(t.abs().max().item() for t in (dqr, dkr, dvr))
    Gp = max(p.grad.abs().max().item() for p in orc.parameters())
    hp = dict(hip.named_parameters())
    figs = {"dq_in": rel(qh.grad, dqr, 1e-4 * G, l2=l2g), "dk_in": rel(kh.grad, dkr, 1e-4 * G, l2=l2g), "dv_in": rel(vh.grad, dvr, 1e-4 * G, l2=l2g)}
    figs.update({n: rel(hp[n].grad, p.grad, 1e-4 * Gp, l2=l2g) for n, p in orc.named_parameters()})
    worst = max(figs, key=figs.get)
    _report(f"mha B{B} S{S} D{D} H{H} {mname}", mode, rel(yh, yr, l2=l2f), figs[worst], ftol, gtol)
    print(f"    worst gradient: {worst}; dq_in {figs['dq_in']:.2e} dk_in {figs['dk_in']:.2e} dv_in {figs['dv_in']:.2e}")
    check(yh, yr, ftol, "out", mode, kind="mha fwd")
    check(qh.grad, dqr, gtol, "dq_in", mode, floor=1e-4 * G, kind="mha bwd")
    check(kh.grad, dkr, gtol, "dk_in", mode, floor=1e-4 * G, kind="mha bwd")
    check(vh.grad, dvr, gtol, "dv_in", mode, floor=1e-4 * G, kind="mha bwd")
    check_param_grads(hip, orc, gtol, mode, kind="mha bwd")


@functools.lru_cache(maxsize=None)
def _encoder_reference(B, S, D, Hid, L, H, rounded):
    torch.manual_seed(3)
    ref = R.TransformerEncoder(D, Hid, L, H, 0.0).eval()
    with torch.no_grad():
        for ln in ref.layer_norm:
            ln.weight.copy_(torch.randn(D) * 0.3 + 1.0)
            ln.bias.copy_(torch.randn(D) * 0.1)
    x = torch.randn(B, S, D)
    r = torch.randn(B, S, D)
    mask = PM.pad(B, S)
    orc = as_oracle(ref, "bf16" if rounded else "fp32")
    xr = x.clone().to(next(orc.parameters()).dtype).requires_grad_(True)
    if rounded:
        yr = RB.encoder(orc, xr, mask)
        (yr * r.bfloat16().double()).sum().backward()
    else:
        yr = ref(xr, mask)
        (yr * r).sum().backward()
    return ref, orc, (x, r, mask), yr.detach(), xr.grad


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,S,D,Hid,L,H", PM.ENCODER_CASES)
def test_transformer_encoder_with_padding_mask_matches_oracle(mode, B, S, D, Hid, L, H):
    ftol, gtol = TOL[mode]
    if mode == "bf16":
        ftol, gtol = 3 * L * ftol, 2 * L * gtol         # as tests/test_gpu_parity.py: the encoder's compounding rounding points
        if S > 64:
            ftol, gtol = 2 * ftol, 2 * gtol
    ref, orc, (x, r, mask), yr, dxr = _encoder_reference(B, S, D, Hid, L, H, mode == "bf16")
    _assert_rows("pad", mask, B, S, H)
    hip = P().TransformerEncoder(D, Hid, L, H, 0.0, compute_dtype=mode)
    hip.load_state_dict(ref.state_dict())
    hip = hip.cuda().eval()
    xh = x.cuda().requires_grad_(True)
    yh = hip(xh, mask.cuda())
    (yh * r.cuda()).sum().backward()
    l2f, l2g = _norms(mode)
    Gp = max(p.grad.abs().max().item() for p in orc.parameters())
    hp = dict(hip.named_parameters())
    figs = {"dx": rel(xh.grad, dxr, l2=l2g)}
    figs.update({n: rel(hp[n].grad, p.grad, 1e-4 * Gp, l2=l2g) for n, p in orc.named_parameters()})
    worst = max(figs, key=figs.get)
    _report(f"encoder B{B} S{S} D{D} L{L} H{H} pad", mode, rel(yh, yr, l2=l2f), figs[worst], ftol, gtol)
    print(f"    worst gradient: {worst}; dx {figs['dx']:.2e}")
    check(yh, yr, ftol, "out", mode, kind=f"encoder L={L} fwd")
    check(xh.grad, dxr, gtol, "dx", mode, kind=f"encoder L={L} bwd")
    check_param_grads(hip, orc, gtol, mode, kind=f"encoder L={L} bwd")


# --------------------------------------------------------------------------------------------
# exact checks through the C ABI
# --------------------------------------------------------------------------------------------
def _split(t, B, S, H):
    """[B,S,D] -> [B*H,S,dh]: problem b * H + h is head h of clip b."""
    return t.reshape(B, S, H, -1).permute(0, 2, 1, 3).reshape(B * H, S, -1)


def _core64(q, k, v, mask, dout, H, rounded):
    """The attention core restated in fp64: masked_fill, softmax, matmul (rounded: with the bf16 kernels' rounding points, as
    oracle/hybrid_ref_bf16._mha).  Returns out, dq, dk, dv as [B*H,S,dh]."""
    B, S, D = q.shape
    qd, kd, vd = (_split(t.double(), B, S, H).clone().requires_grad_(True) for t in (q, k, v))
    dot = torch.matmul(qd, kd.transpose(-2, -1))
    dot = (RB.rg(dot) if rounded else dot) / math.sqrt(D)
    dot = dot.masked_fill(mask[torch.arange(B * H) % B] == 0, -1e9)      # problem b * H + h reads mask[(b * H + h) % B]
    w = torch.softmax(dot, dim=-1)
    a = torch.matmul(RB.rv(w), vd) if rounded else torch.matmul(w, vd)
    a = RB.rb(a) if rounded else a
    (a * _split(dout.double(), B, S, H)).sum().backward()
    return a.detach(), qd.grad, kd.grad, vd.grad


def _core_hip(dtn, q, k, v, mask, dout, H):
    """hyb_attention_fwd / _bwd (S <= 64) or hyb_attention_long_fwd / _bwd, p_drop = 0 -> out, dq, dk, dv [B,S,D] on the host, fp64."""
    from transformer_cnn_hybrid_network_for_video_processing_amd import _lib as L
    lib = L.lib
    dt = L.HYB_F32 if dtn == "fp32" else L.HYB_BF16
    B, S, D = q.shape
    st = torch.cuda.current_stream().cuda_stream
    qc, kc, vc, gc = (t.cuda().contiguous() for t in (q, k, v, dout))
    mc = mask.cuda().float().contiguous()
    out, dq, dk, dv = (torch.full_like(qc, float("nan")) for _ in range(4))
    if S <= 64:
        stats = torch.empty(B * H * S * 2, device="cuda")
        lib.call("hyb_attention_fwd", dt, qc.data_ptr(), kc.data_ptr(), vc.data_ptr(), mc.data_ptr(), out.data_ptr(), stats.data_ptr(), B, S, D, H, 0.0, 1, st)
        lib.call("hyb_attention_bwd", dt, qc.data_ptr(), kc.data_ptr(), vc.data_ptr(), mc.data_ptr(), stats.data_ptr(), gc.data_ptr(), dq.data_ptr(),
                 dk.data_ptr(), dv.data_ptr(), B, S, D, H, 0.0, 1, st)
    else:
        ws = torch.empty(lib.query("hyb_attention_long_workspace", dt, B, S, D, H), dtype=torch.uint8, device="cuda")
        lse = torch.empty(B * H, S, device="cuda")
        lib.call("hyb_attention_long_fwd", dt, qc.data_ptr(), kc.data_ptr(), vc.data_ptr(), D, mc.data_ptr(), out.data_ptr(), lse.data_ptr(), B, S, D, H, 0.0, 1,
                 None, ws.data_ptr(), ws.numel(), st)
        lib.call("hyb_attention_long_bwd", dt, qc.data_ptr(), kc.data_ptr(), vc.data_ptr(), D, mc.data_ptr(), out.data_ptr(), lse.data_ptr(), gc.data_ptr(),
                 dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), D, B, S, D, H, 0.0, 1, None, ws.data_ptr(), ws.numel(), st)
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in (out, dq, dk, dv))


@pytest.mark.parametrize("dtn", ["fp32", "bf16"])
@pytest.mark.parametrize("B,S,D,H", [(2, 16, 64, 4), (2, 40, 64, 4), (2, 96, 64, 4)])       # one tile, several tiles, online softmax
def test_attention_core_fully_masked_rows_are_exact(dtn, B, S, D, H):
    tdt = torch.float32 if dtn == "fp32" else torch.bfloat16
    ftol, gtol = TOL[dtn]
    if dtn == "bf16" and S > 64:
        ftol, gtol = 2 * ftol, 2 * gtol
    l2 = dtn == "bf16"
    g = torch.Generator().manual_seed(11)
    q, k, v, dout1 = (torch.randn(B, S, D, generator=g).to(tdt) for _ in range(4))     # (rounded once: exact inputs for both sides)
    mask = PM.pad(B, S)
    _assert_rows("pad", mask, B, S, H)
    full = PM.problem_rows_fully_masked(mask, B, S, H)                                 # [B*H, S]
    sel = full.reshape(B, H, S).permute(0, 2, 1)[..., None].expand(B, S, H, D // H).reshape(B, S, D)
    # the second run's dO differs in the fully masked (problem, query) rows only
    dout2 = torch.where(sel, (dout1.float() + 4.0 * torch.randn(B, S, D, generator=g)).to(tdt), dout1)
    assert torch.equal(dout1[~sel], dout2[~sel]) and not torch.equal(dout1[sel], dout2[sel])
    out1, dq1, dk1, dv1 = _core_hip(dtn, q, k, v, mask, dout1, H)
    out2, dq2, dk2, dv2 = _core_hip(dtn, q, k, v, mask, dout2, H)
    o_out, o_dq, o_dk, o_dv = _core64(q, k, v, mask, dout1, H, rounded=l2)
    sp = lambda t: _split(t.double(), B, S, H)                                         # noqa: E731
    outp, dqp = sp(out1), sp(dq1)
    # 1. forward: a fully masked row is the plain mean of its problem's value rows
    vmean = sp(v).mean(dim=1, keepdim=True).expand(-1, S, -1)
    if l2 and S <= 64:
        # the bf16 gate is defined against the rounded oracle: the short bf16 kernels feed P.V the weight bf16(1/S) and store a bf16 output
        vmean = (sp(v).sum(dim=1, keepdim=True) * float(torch.tensor(1.0 / S).bfloat16())).bfloat16().double().expand(-1, S, -1)
    r_mean = rel(outp[full], vmean[full], l2=l2)
    # 2. dq of those rows is exactly zero
    dq_nonzero = int((dqp[full] != 0).sum()) + int((sp(dq2)[full] != 0).sum())
    # 3. dk does not see dO of those rows at all; dv sees 1/S of it
    ib = torch.int32 if dtn == "fp32" else torch.int16
    dk_same = torch.equal(dk1.view(ib), dk2.view(ib))
    want_dv = (sp(dout2) - sp(dout1)).mul(full[..., None]).sum(dim=1, keepdim=True).expand(-1, S, -1) / S
    got_dv = sp(dv2) - sp(dv1)
    # each stored dv carries one rounding of its storage format (2^-9 bf16, 2^-24 fp32), so their difference is off by that much of both
    # on top of the gradient gate on the expected difference
    ulp = 2.0 ** -9 if l2 else 2.0 ** -24
    if l2:
        err_dv, bound_dv = (got_dv - want_dv).norm().item(), gtol * want_dv.norm().item() + ulp * (sp(dv1).norm().item() + sp(dv2).norm().item())
    else:
        err_dv = (got_dv - want_dv).abs().max().item()
        bound_dv = gtol * want_dv.abs().max().item() + ulp * (sp(dv1).abs().max().item() + sp(dv2).abs().max().item())
    # 4. everything else against the fp64 restatement
    r_out = rel(outp[~full], o_out[~full], l2=l2)
    r_dq, r_dk, r_dv = rel(dqp[~full], o_dq[~full], l2=l2), rel(sp(dk1), o_dk, l2=l2), rel(sp(dv1), o_dv, l2=l2)
    print(f"\n[core {dtn} B{B} S{S} D{D} H{H} pad] {int(full.sum())} fully masked rows: out vs mean(v) {r_mean:.2e}, other rows {r_out:.2e} (gate {ftol:.1e}); "
          f"non-zero dq elements in masked rows {dq_nonzero}; dk bit-identical {dk_same}; dv difference error {err_dv:.2e} (bound {bound_dv:.2e}); "
          f"dq {r_dq:.2e} dk {r_dk:.2e} dv {r_dv:.2e} (gate {gtol:.1e})")
    assert all(torch.isfinite(t.float()).all() for t in (out1, dq1, dk1, dv1, out2, dq2, dk2, dv2))
    assert torch.equal(out1, out2) and torch.equal(dq1[~sel], dq2[~sel])
    check(outp[full], vmean[full], ftol, "fully masked rows: out vs mean of v", dtn)
    assert dq_nonzero == 0, f"dq of fully masked rows: {dq_nonzero} non-zero elements"
    assert dk_same, "dk changed with dO of fully masked rows"
    assert err_dv <= bound_dv, f"dv difference: {err_dv:.3e} > {bound_dv:.3e}"
    check(outp[~full], o_out[~full], ftol, "out", dtn)
    check(dqp[~full], o_dq[~full], gtol, "dq", dtn)
    check(sp(dk1), o_dk, gtol, "dk", dtn)
    check(sp(dv1), o_dv, gtol, "dv", dtn)


# --------------------------------------------------------------------------------------------
# whole path
# --------------------------------------------------------------------------------------------
MODEL_KW = dict(cnn_channels=(32, 64), d_model=64, num_heads=4, num_layers=2, hidden_dim=128)
MB, MT, MHW = 3, 5, 32


@functools.lru_cache(maxsize=None)
def _model_reference(rounded, training):
    torch.manual_seed(0)
    ref = R.TransformerCNNHybridRef(**MODEL_KW)
    sd = copy.deepcopy(ref.state_dict())
    x, y = R.synthetic_batch(MB, MT, MHW, MHW, seed=0)
    mask = PM.pad(MB, MT)
    orc = as_oracle(ref, "bf16" if rounded else "fp32")
    orc.train(training)
    for a in orc.encoder.attention_layers:
        a.dropoutLayer.p = 0.0
    lr = RB.forward(orc, x.double(), mask) if rounded else orc(x, mask)
    loss = R.loss_fn(lr, y)
    loss.backward()
    return sd, orc, (x, y, mask), lr.detach(), loss.detach()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
def test_whole_model_with_padding_mask_matches_oracle(mode, training):
    """model(x, mask) at the gates of test_full_model_logits_loss_and_grads_match_oracle: eval-mode and train-mode BatchNorm, no dropout."""
    ftol, gtol = TOL[mode]
    ftol = 2e-2 if mode == "bf16" else 1e-3
    if mode == "bf16":
        gtol = 1.5e-1
    sd, orc, (x, y, mask), lr, loss_r = _model_reference(mode == "bf16", training)
    _assert_rows("pad", mask, MB, MT, MODEL_KW["num_heads"])
    hip = P().TransformerCNNHybrid(compute_dtype=mode, **MODEL_KW)
    hip.load_state_dict(sd)
    hip = hip.cuda().train(training)
    for a in hip.encoder.attention_layers:
        a.dropoutLayer.p = 0.0
    lh = hip(x.cuda(), mask.cuda())
    loss_h = P().HybridCrossEntropyLoss()(lh, y.cuda())
    loss_h.backward()
    l2f, l2g = _norms(mode)
    Gp = max(p.grad.abs().max().item() for p in orc.parameters())
    hp = dict(hip.named_parameters())
    figs = {n: rel(hp[n].grad, p.grad, 1e-4 * Gp, l2=l2g) for n, p in orc.named_parameters()}
    worst = max(figs, key=figs.get)
    _report(f"model B{MB} T{MT} {MHW}px pad training={training}", mode, rel(lh, lr, l2=l2f), figs[worst], ftol, gtol)
    print(f"    worst gradient: {worst}")
    check(lh, lr, ftol, f"logits (training={training})", mode, kind="whole model fwd")
    assert abs(loss_h.item() - loss_r.item()) <= ftol * max(1.0, abs(loss_r.item())), (loss_h.item(), loss_r.item())
    check_param_grads(hip, orc, gtol, mode, kind="whole model bwd")


@pytest.mark.parametrize("mode", ["fp32", "bf16x3", "bf16", "mixed"])
def test_predict_and_graphed_predict_with_padding_mask(mode):
    """predict(x, mask) against model.eval()(x, mask): the same bits where predict is the eval forward (fp32, bf16x3), tests/test_gpu_infer.py's
    masked gate where it has its own kernels (1.2e-2 of the largest logit); GraphedPredict replays predict's bits."""
    torch.manual_seed(7)
    m = P().TransformerCNNHybrid(compute_dtype=mode, **MODEL_KW).cuda().eval()
    x = torch.rand(MB, MT, 3, MHW, MHW, device="cuda")
    mask = PM.pad(MB, MT).cuda()
    _assert_rows("pad", mask.cpu(), MB, MT, MODEL_KW["num_heads"])
    with torch.no_grad():
        want = m(x, mask)
        none = m(x)
    got = m.predict(x, mask)
    err = (got.float() - want.float()).abs().max().item() / want.float().abs().max().item()
    print(f"\n[predict {mode} pad] against the eval forward: {err:.2e}")
    assert torch.isfinite(got.float()).all() and not torch.equal(want, none)
    if mode in ("fp32", "bf16x3"):
        assert torch.equal(got, want)
    else:
        assert err <= 1.2e-2
    gp = P().GraphedPredict(m, x, mask)
    assert torch.equal(gp(x, mask).clone(), got)
    ones = torch.ones_like(mask)
    assert torch.equal(gp(x, ones).clone(), m.predict(x, ones))
    gp.close()


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("training", [True, False])
def test_model_level_operators_equal_the_stage_operators_bitwise_under_padding_mask(mode, training):
    """tests/test_gpu_ops.py's test_model_level_operators_equal_the_stage_operators_bitwise with a padding mask: bit-equality exactly where
    that test asserts it (the four sums the one-workgroup-per-clip tail regroups are equal to rounding)."""
    from transformer_cnn_hybrid_network_for_video_processing_amd import ops as o
    torch.manual_seed(5)
    kw = dict(dropout=0.1, compute_dtype=mode, **MODEL_KW)
    a, b = P().TransformerCNNHybrid(**kw).cuda(), P().TransformerCNNHybrid(**kw).cuda()
    b.load_state_dict(a.state_dict())
    b.fuse_model_ops = False
    a.train(training); b.train(training)
    x = torch.rand(MB, MT, 3, MHW, MHW, device="cuda")
    y = torch.tensor([1, 0, 7], device="cuda")
    mask = PM.pad(MB, MT).cuda()
    res = []
    for m in (a, b):
        torch.manual_seed(11)
        o._SEED_COUNTER[0] = 100                                    # same dropout seeds on both paths
        logits = m(x, mask)
        loss = P().HybridCrossEntropyLoss()(logits, y)
        loss.backward()
        res.append((logits.detach(), loss.detach()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    regrouped = {"head.weight", "head.bias", f"encoder.layer_norm.{kw['num_layers'] - 1}.weight", f"encoder.layer_norm.{kw['num_layers'] - 1}.bias"}
    for (n, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.isfinite(pa.grad).all(), n
        if n in regrouped:
            torch.testing.assert_close(pa.grad, pb.grad, rtol=2e-5, atol=2e-6 * float(pb.grad.abs().max()), msg=n)
        else:
            assert torch.equal(pa.grad, pb.grad), n
    for (n, ba), (_, bb) in zip(a.named_buffers(), b.named_buffers()):
        assert torch.equal(ba, bb), n
