"""The fused temporal half (global average pool -> token projection -> Transformer encoder -> mean over frames -> head -> cross-entropy;
hybrid::temporal / hybrid::temporal_ce, i.e. hyb_temporal_ce_fwd / hyb_temporal_ce_bwd) ALONE against a float64 oracle, at the shapes where
its host code takes a different branch.

``forward_temporal`` / ``forward_temporal_loss`` take the last pooled map h [B*S, Hh, Ww, Cp] directly, so there is no conv stack in front:
no BatchNorm, no arg-max, and the only non-smooth points left are the ReLUs of the q/k/v projections and of the feed-forward.  The gates are
the project's per-stage ones (tests/test_gpu_parity.py: TOL, check, check_param_grads with its 1e-4 * G floor), ten to a hundred times
tighter than the whole-model gates:

  fp32, ("bf16", "fp32")   1e-4 forward, 1e-3 gradients, maximum-relative, against the fp64 oracle
  bf16x3, mixed            1e-4 forward (max-rel), 2e-2 gradients (relative L2: a ReLU in front), against the fp64 oracle
  bf16                     3 L x 2e-3 forward, 2 L x 2e-2 gradients (relative L2; both doubled for S > 64, as the encoder test does), against
                           the fp64 oracle with the bf16 path's rounding points (oracle/hybrid_ref_bf16.temporal)
  dh with a bf16 map in front of an fp32-storage temporal part (mixed, the pair): stored in bf16 -- relative L2 <= the mode's gradient gate + 2^-8

What the fp32 CPU oracle itself measures against fp64 on these shapes: logits 1e-7 .. 4e-7, dh 3e-7 .. 7e-7, worst parameter gradient
1e-6 .. 1e-5 -- 10 x to 100 x inside the fp32 gates.  bf16 rounding noise (rounded oracle against plain fp64): logits 2e-3 .. 8e-3, dh 3e-2 ..
6e-2, i.e. the bf16 gates sit at the scale of the rounding itself.  (The padding cases L1P / LONGP / CFG2P: logits 2e-7 .. 4e-7, worst
gradient 1e-6 .. 8e-6, asserted at 10 x inside the gates by tests/test_oracle.py.)

Each case lands on a known side of the dispatch rules, re-read from the code:

  fused tail taken (hyb_temporal_tail_ok, layernorm.hip)   B <= ln_rows = min(32, ceil(B S / 4)), D % 8 == 0, D <= 1536, classes <= 64
  tail forward keeps the clip's rows in LDS                (D + 320) 4 + S D es <= 60 KB (es = 4 fp32 storage, 2 bf16); 512 threads for S >= 8
  tail backward row blocks per clip                        nsb = min(ceil(S / 4), ln_rows / B), rows per block rounded up to 4, last block ragged
  workspace set of the last layer (hyb_encoder_bwd_tail)   parity (L - 1) & 1
  padded channels (temporal_bwd_impl)                      Cp = 32 ceil(C / 32) > C: a memset, padded lanes of dh zero
  attention family                                         S <= 16 one tile, S <= 64 several, S > 64 online softmax

The "tail" field below ("in" / "out") is that side as data (the decision functions are internal C++ symbols);
profiles/temporal_tail_dispatch.txt is a kernel trace showing, per case, whether temporal_tail_fwd_kernel / temporal_tail_bwd_kernel ran.
temporal_bwd_impl's `!ride` branch (C % 8 != 0) cannot be reached: the module refuses cnn_channels[-1] % 8 != 0 and hyb_linear_fwd checks
K % 8 == 0 on the token projection before any backward exists, so there is no case for it.
"""
import collections
import copy
import functools
import types

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import padding_masks  # noqa: E402
from oracle import hybrid_ref as R  # noqa: E402
from oracle import hybrid_ref_bf16 as RB  # noqa: E402
from test_gpu_parity import TOL, check, check_param_grads, rel  # noqa: E402

Case = collections.namedtuple("Case", "B S D Hid L heads classes C Hh Ww mask tail")
CASES = {
    # workspace parity 0; Cp = 32 > C = 24; S < 8 (256-thread tail forward); one ragged tail-backward block (8 rows for 5)
    "L1": Case(3, 5, 64, 128, 1, 4, 5, 24, 3, 3, True, "in"),
    # parity 0 with layers behind it; HW = 1
    "L3": Case(2, 16, 64, 128, 3, 4, 8, 64, 1, 1, False, "in"),
    # parity 1, deep; B = 1; odd HW = 49
    "L4": Case(1, 8, 32, 64, 4, 2, 8, 32, 7, 7, True, "in"),
    # tail-backward blocks of 8, 8, 2 rows; head width 128; D = 256 the lower edge of the bf16 LayerNorm prologue; Cp = C
    "RAG": Case(2, 18, 256, 512, 2, 2, 8, 96, 5, 3, False, "in"),
    # B = 32 = ln_rows / B = 33 > ln_rows = 32
    "B32": Case(32, 4, 64, 128, 2, 4, 8, 32, 2, 2, False, "in"),
    "B33": Case(33, 4, 64, 128, 2, 4, 8, 32, 2, 2, False, "out"),
    # ceil(24 / 4) = 6 partial rows < 8 clips, though B <= 32
    "S3": Case(8, 3, 64, 128, 2, 4, 8, 32, 2, 2, False, "out"),
    # one token: ln_rows = 1
    "ONE": Case(1, 1, 32, 64, 1, 2, 8, 32, 2, 2, False, "in"),
    # the largest D the tail takes (its backward holds 64 + 9 D floats in LDS) / the first D above it that the attention limits accept
    "D1536": Case(2, 8, 1536, 1536, 2, 12, 8, 32, 2, 2, False, "in"),
    "DBIG": Case(2, 8, 1600, 1536, 2, 25, 8, 32, 2, 2, False, "out"),
    # classes = 64: the head's per-clip gradient rows (sized for 64) exactly full
    "C64": Case(2, 18, 256, 512, 2, 2, 64, 96, 5, 3, False, "in"),
    # rows-in-LDS boundary of the tail forward at D = 512: 28 | 29 rows of fp32, 56 | 57 rows of bf16; several token tiles
    "LDS28": Case(2, 28, 512, 1024, 2, 8, 8, 256, 2, 2, False, "in"),
    "LDS29": Case(2, 29, 512, 1024, 2, 8, 8, 256, 2, 2, False, "in"),
    "LDS56": Case(2, 56, 512, 1024, 2, 8, 8, 256, 2, 2, False, "in"),
    "LDS57": Case(2, 57, 512, 1024, 2, 8, 8, 256, 2, 2, False, "in"),
    # online-softmax attention in front of the fused tail
    "LONG": Case(2, 70, 64, 128, 2, 4, 8, 32, 2, 2, True, "in"),
    # the benchmarked step's own temporal shape (224 px -> 7 x 7 map) / the 448 px map (HW = 196 in the global average pool)
    "CFG2": Case(8, 16, 512, 2048, 2, 8, 8, 256, 7, 7, False, "in"),
    "CFG5": Case(4, 16, 512, 2048, 2, 8, 8, 256, 14, 14, False, "in"),
    # B > 32; 1280 output tiles: the many-tile side of every "at most 256 tiles" GEMM rule
    "WIDE": Case(40, 16, 512, 2048, 2, 8, 8, 256, 2, 2, False, "out"),
    # mask = "pad": a valid (x) valid padding mask (tests/padding_masks.py) -- every padded frame is a fully masked query row, which the random
    # masks above never contain (they keep key 0).  L1's and LONG's geometry, and the benchmarked temporal shape
    "L1P": Case(3, 5, 64, 128, 1, 4, 5, 24, 3, 3, "pad", "in"),
    "LONGP": Case(2, 70, 64, 128, 2, 4, 8, 32, 2, 2, "pad", "in"),
    "CFG2P": Case(8, 16, 512, 2048, 2, 8, 8, 256, 7, 7, "pad", "in"),
}
C65 = Case(2, 18, 256, 512, 2, 2, 65, 96, 5, 3, False, "out")       # C64's geometry with one class too many for hyb_head_bwd
MODES = ["fp32", "bf16x3", "bf16", "mixed", "bf16-fp32"]
_COMPUTE = {"fp32": "fp32", "bf16x3": "bf16x3", "bf16": "bf16", "mixed": "mixed", "bf16-fp32": ("bf16", "fp32")}
_GATE_AS = {"fp32": "fp32", "bf16-fp32": "fp32", "bf16x3": "bf16x3", "mixed": "bf16x3", "bf16": "bf16"}     # whose TOL entry and error norm
_H_BF16 = ("bf16", "mixed", "bf16-fp32")                               # modes whose pooled map is stored in bf16
_TEMPORAL = ("token_proj", "encoder", "head")
# A ReLU pre-activation within fp32 round-off of zero makes the gradient two-valued: the unit's whole contribution appears or vanishes with the
# last bit of the dot product, and the fp64 oracle holds one of the two answers.  WIDE on the bf16-rounded map has such a unit (layer 0, value
# projection, token 420, feature 135: 2.98e-8 in fp64 where the mean |pre-activation| is 0.30), and the fp32 CPU ORACLE itself lands on the other
# side of it: against fp64 it measures 2.005e-3 on that projection's weight gradient and 1.914e-3 on its bias gradient (maximum-relative, same
# floor; tests/test_oracle.py pins both figures on the CPU), everything else 2.1e-4 and below.  No fp32 arithmetic can be asked to beat the fp32
# reference, so for these two tensors of this one case the 1e-3 gate becomes 2 x the reference's own error.  (WIDE on the fp32 map has two such
# feed-forward units, 5e-8 and 7e-8: the reference measures 2.0e-4 there, inside the gate.)  {(case, map is bf16-rounded): {tensor: fp32 CPU oracle}}
FP32_ORACLE_ERROR = {("WIDE", True): {"encoder.attention_layers.0.value_layer.weight": 2.005e-3,
                                      "encoder.attention_layers.0.value_layer.bias": 1.914e-3}}
_MEASURED = {}                                                          # (mode, quantity) -> (worst figure, case): printed at the end


def P():
    import transformer_cnn_hybrid_network_for_video_processing_amd as pkg
    return pkg


def ops():
    from transformer_cnn_hybrid_network_for_video_processing_amd import ops as o
    return o


def tail_taken(c):
    """hyb_temporal_tail_ok as read from layernorm.hip (the profile listing checks this restatement against the kernels that ran)."""
    ln_rows = min(32, -(-c.B * c.S // 4))
    return c.B <= ln_rows and c.D % 8 == 0 and c.D <= 1536 and c.classes <= 64


def gates(mode, c):
    ftol, gtol = TOL[_GATE_AS[mode]]
    if mode == "bf16":
        ftol, gtol = 3 * c.L * ftol, 2 * c.L * gtol
        if c.S > 64:
            ftol, gtol = 2 * ftol, 2 * gtol
    return ftol, gtol


def _pad(c):
    return (c.C + 31) // 32 * 32


@functools.lru_cache(maxsize=None)
def _inputs(c):
    """Seeded oracle module (LayerNorm affines randomised), pooled map h [N, Hh, Ww, Cp] fp32 with zero padded lanes, labels, mask."""
    torch.manual_seed(3)
    ref = R.TransformerCNNHybridRef(cnn_channels=(8, c.C), d_model=c.D, num_heads=c.heads, num_layers=c.L, hidden_dim=c.Hid,
                                    num_classes=c.classes, dropout=0.0).train()
    with torch.no_grad():
        for ln in ref.encoder.layer_norm:
            ln.weight.copy_(torch.randn(c.D) * 0.3 + 1.0)
            ln.bias.copy_(torch.randn(c.D) * 0.1)
    for a in ref.encoder.attention_layers:
        a.dropoutLayer.p = 0.0
    g = torch.Generator().manual_seed(7)
    h = torch.zeros(c.B * c.S, c.Hh, c.Ww, _pad(c))
    h[..., :c.C] = torch.rand(c.B * c.S, c.Hh, c.Ww, c.C, generator=g) * 2.0          # a pooled map is what a ReLU and a max left: >= 0
    y = torch.randint(0, c.classes, (c.B,), generator=g)
    mask = None
    if c.mask == "pad":
        mask = padding_masks.pad(c.B, c.S)
        assert min(padding_masks.row_census(mask, c.B, c.S, c.heads)) > 0       # fully masked rows and rows with a visible key
    elif c.mask:
        mask = (torch.rand(c.B, c.S, c.S, generator=g) > 0.3).float()
        mask[:, :, 0] = 1
    return ref, h, y, mask


def _pooled(c, mode):
    """The map both sides get: for a bf16 map, drawn in fp32 and rounded once, so the input is exact for the kernels and for the oracle."""
    h = _inputs(c)[1]
    return h.bfloat16().float() if mode in _H_BF16 else h


@functools.lru_cache(maxsize=None)
def _oracle(c, rounded, h16):
    """fp64 oracle on the temporal half: logits, loss (unscaled), and the gradients of 1.5 * loss w.r.t. h [N, Hh, Ww, C] and every temporal
    parameter.  rounded: with the bf16 path's rounding points (oracle/hybrid_ref_bf16.py).  h16: on the bf16-rounded map."""
    ref, h, y, mask = _inputs(c)
    orc = copy.deepcopy(ref).double()
    hd = (h.bfloat16() if h16 else h).double()[..., :c.C].clone().requires_grad_(True)
    if rounded:
        logits = RB.temporal(orc, hd.permute(0, 3, 1, 2), c.B, mask)
    else:
        tok = orc.token_proj(hd.mean(dim=(1, 2))).reshape(c.B, c.S, -1)
        logits = orc.head(orc.encoder(tok, mask).mean(dim=1))
    loss = F.cross_entropy(logits, y)
    named = [(n, p) for n, p in orc.named_parameters() if n.split(".")[0] in _TEMPORAL]
    grads = torch.autograd.grad(1.5 * loss, [hd] + [p for _, p in named])
    return logits.detach(), loss.detach(), grads[0], {n: g for (n, _), g in zip(named, grads[1:])}


def _model(c, mode, fused=True):
    ref = _inputs(c)[0]
    m = P().TransformerCNNHybrid(cnn_channels=(8, c.C), d_model=c.D, num_heads=c.heads, num_layers=c.L, hidden_dim=c.Hid, num_classes=c.classes,
                                 dropout=0.0, compute_dtype=_COMPUTE[mode])
    m.load_state_dict({k: v for k, v in ref.state_dict().items() if "num_batches_tracked" not in k}, strict=False)
    for a in m.encoder.attention_layers:
        a.dropoutLayer.p = 0.0
    m.fuse_model_ops = fused
    return m.cuda().train()


def _run(m, c, mode, fused_loss, h=None):
    """One forward + backward of the temporal half with an upstream gradient of 1.5 -> (logits, loss, dh, {name: gradient})."""
    y, mask = _inputs(c)[2:]
    h = _pooled(c, mode) if h is None else h
    hh = (h.bfloat16() if mode in _H_BF16 else h).cuda().requires_grad_(True)
    maskc = mask.cuda() if mask is not None else None
    if fused_loss:
        loss, logits = m.forward_temporal_loss(hh, c.B, y.cuda(), maskc)
    else:
        logits = m.forward_temporal(hh, c.B, maskc)
        loss = P().HybridCrossEntropyLoss()(logits, y.cuda())
    named = [(n, p) for n, p in m.named_parameters() if n.split(".")[0] in _TEMPORAL]
    grads = torch.autograd.grad(loss * 1.5, [hh] + [p for _, p in named])
    torch.cuda.synchronize()
    return logits.detach(), loss.detach(), grads[0], {n: g for (n, _), g in zip(named, grads[1:])}


class _Grads:
    """{name: gradient} with the named_parameters() / parameters() face check_param_grads reads."""

    def __init__(self, grads):
        self._named = [(n, types.SimpleNamespace(grad=g)) for n, g in grads.items()]

    def named_parameters(self):
        return list(self._named)

    def parameters(self):
        return [p for _, p in self._named]


def _note(mode, what, case, r):
    if r > _MEASURED.get((mode, what), (-1.0, None))[0]:
        _MEASURED[(mode, what)] = (r, case)
    return r


def _against_oracle(name, c, mode, res, path):
    logits, loss, dh, grads = res
    gate_as = _GATE_AS[mode]
    ftol, gtol = gates(mode, c)
    o_logits, o_loss, o_dh, o_grads = _oracle(c, mode == "bf16", mode in _H_BF16)
    l2f, l2g = gate_as == "bf16", gate_as != "fp32"              # the norms `check` applies: relative L2 for bf16, and for bf16x3 gradients
    kind = "temporal bwd" if gate_as == "bf16x3" else None
    G = max(g.abs().max().item() for g in o_grads.values())
    worst = max(rel(grads[n], o_grads[n], 1e-4 * G, l2=l2g) for n in o_grads)
    dh_l2 = l2g or mode in ("mixed", "bf16-fp32")
    figs = (_note(mode, "logits", name, rel(logits, o_logits, l2=l2f)), _note(mode, "loss", name, rel(loss, o_loss, l2=l2f)),
            _note(mode, "dh", name, rel(dh[..., :c.C], o_dh, l2=dh_l2)), _note(mode, "param grads", name, worst))
    print(f"\n[{name} {mode} {path}] logits {figs[0]:.2e} loss {figs[1]:.2e} (gate {ftol:.1e}); dh {figs[2]:.2e} worst parameter gradient {worst:.2e} "
          f"(gate {gtol:.1e})")
    check(logits, o_logits, ftol, f"{path} logits", gate_as)
    check(loss, o_loss, ftol, f"{path} loss", gate_as)
    if mode in ("mixed", "bf16-fp32"):
        # dh leaves through a bf16 store behind fp32 arithmetic: the mode's gradient gate plus one bf16 rounding, as a relative L2 distance
        r = rel(dh[..., :c.C], o_dh, l2=True)
        assert r <= gtol + 2.0 ** -8, f"{path} dh: L2 rel err {r:.3e} > {gtol + 2.0 ** -8:.2e}"
    else:
        check(dh[..., :c.C], o_dh, gtol, f"{path} dh", gate_as, kind=kind)
    kinked = FP32_ORACLE_ERROR.get((name, mode in _H_BF16), {}) if gate_as == "fp32" else {}
    if not kinked:
        check_param_grads(_Grads(grads), _Grads(o_grads), gtol, gate_as, kind=kind)
    else:                                                          # check_param_grads, with the listed tensors at 2 x the fp32 reference's own error
        for n in o_grads:
            check(grads[n], o_grads[n], max(gtol, 2 * kinked.get(n, 0.0)), "grad:" + n, gate_as, floor=1e-4 * G, kind=kind)


def _assert_same_bits(a, b, what, but=None):
    """Two runs (logits, loss, dh, grads): bit-equal, except the gradients named in ``but`` (rtol 2e-5, as tests/test_gpu_ops.py)."""
    assert torch.equal(a[0], b[0]), f"{what}: logits differ"
    assert torch.equal(a[1], b[1]), f"{what}: loss differs ({float(a[1])!r} vs {float(b[1])!r})"
    assert a[2].dtype == b[2].dtype and torch.equal(a[2], b[2]), f"{what}: dh differs"
    assert a[3].keys() == b[3].keys()
    for n in a[3]:
        if but and n in but:
            torch.testing.assert_close(a[3][n], b[3][n], rtol=2e-5, atol=2e-6 * float(b[3][n].abs().max()), msg=f"{what}: {n}")
        else:
            assert torch.equal(a[3][n], b[3][n]), f"{what}: gradient of {n} differs"


def _ticket(c):
    o = ops()
    t = o._CE_SCRATCH[(torch.cuda.current_device(), o._stream(), c.B)]
    return int(t[-1].view(torch.int32).item())


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if _MEASURED:
        print("\nworst measured against the fp64 oracle (mode, quantity: figure at case):")
        for (mode, what), (r, case) in sorted(_MEASURED.items()):
            print(f"  {mode:10s} {what:12s} {r:.2e}  at {case}")


def test_case_table_sides_match_the_dispatch_rule():
    """The "tail" column is data; it has to agree with the rule as restated in tail_taken(), and both sides of every clause stay covered."""
    for name, c in list(CASES.items()) + [("C65", C65)]:
        assert tail_taken(c) == (c.tail == "in"), name
        assert c.D % c.heads == 0 and (c.D // c.heads) % 8 == 0 and c.D // c.heads <= 128 and c.C % 8 == 0, name
    out = {n for n, c in CASES.items() if c.tail == "out"}
    assert out == {"B33", "S3", "DBIG", "WIDE"}
    assert {(CASES[n].L - 1) & 1 for n in CASES if CASES[n].tail == "in"} == {0, 1}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(CASES))
def test_temporal_half_matches_fp64_oracle_and_its_own_unfused_forms(name, mode):
    c = CASES[name]
    fused, staged = _model(c, mode), _model(c, mode, fused=False)
    assert fused._fused() and not staged._fused()
    a = _run(fused, c, mode, fused_loss=True)                 # hybrid::temporal_ce
    assert _ticket(c) == 0                                    # the ticket word behind the per-clip loss terms is left at zero
    b = _run(fused, c, mode, fused_loss=False)                # hybrid::temporal + hybrid::cross_entropy
    s = _run(staged, c, mode, fused_loss=False)               # one operator per stage
    # 1. against the oracle, both fused forms
    _against_oracle(name, c, mode, a, "temporal_ce")
    _against_oracle(name, c, mode, b, "temporal+ce")
    # 3. the loss inside the temporal launches == the criterion as its own launches, bit for bit
    _assert_same_bits(a, b, "temporal_ce vs temporal + cross_entropy")
    # 2. fused == per-stage operators: bit-equal, except (when the one-workgroup-per-clip tail runs) the four sums it groups per clip
    regrouped = {"head.weight", "head.bias", f"encoder.layer_norm.{c.L - 1}.weight", f"encoder.layer_norm.{c.L - 1}.bias"} if c.tail == "in" else None
    if mode in ("mixed", "bf16-fp32"):
        assert s[2].dtype == torch.bfloat16                   # (the per-stage path casts h first; its dh returns through that cast)
    _assert_same_bits(b, s, "fused vs per-stage operators", but=regrouped)
    # 5. a second call gives the same bits: every sum of the path has a fixed order
    _assert_same_bits(a, _run(fused, c, mode, fused_loss=True), "repeat of temporal_ce")
    assert _ticket(c) == 0
    # padded lanes of dh: what the conv stages' backward reads as d(pooled) ("padded channels hold zeros", include/hybrid_hip.h)
    assert a[2].shape[-1] == _pad(c) and not a[2][..., c.C:].any()


@pytest.mark.parametrize("mode", MODES)
def test_padded_feature_lanes_are_ignored_and_get_zero_gradient(mode):
    """L1: Cp = 32 > C = 24.  Finite non-zero values in lanes C..Cp-1 of h change no output bit, and dh is exactly zero there (the internal
    layout's contract: padded channels hold zeros -- hyb_backbone_bwd takes dh as the last stage's d(pooled) without masking it)."""
    c = CASES["L1"]
    assert _pad(c) == 32 and c.C == 24
    m = _model(c, mode)
    clean = _pooled(c, mode)
    dirty = clean.clone()
    dirty[..., c.C:] = torch.randn(dirty[..., c.C:].shape, generator=torch.Generator().manual_seed(2)) * 3.0 + 5.0
    if mode in _H_BF16:
        dirty = dirty.bfloat16().float()
    assert torch.isfinite(dirty).all() and (dirty[..., c.C:] != 0).all()
    for fused_loss in (True, False):
        a, b = _run(m, c, mode, fused_loss, clean), _run(m, c, mode, fused_loss, dirty)
        _assert_same_bits(a, b, f"padded lanes filled (fused_loss={fused_loss})")
        assert not b[2][..., c.C:].any() and b[2][..., :c.C].any()


@pytest.mark.parametrize("mode", MODES)
def test_more_than_64_classes_is_refused_not_wrong(mode):
    """65 classes: hyb_head_bwd checks classes <= 64 and the fused tail does not take them, so the backward must raise on the fused and on the
    per-stage path.  The forward may raise too; where it returns, its logits and loss meet the forward gate.  Nothing is silently wrong."""
    c = C65
    ftol, _ = gates(mode, c)
    gate_as = _GATE_AS[mode]
    y, mask = _inputs(c)[2:]
    assert mask is None
    o_logits, o_loss = _oracle(c, mode == "bf16", mode in _H_BF16)[:2]
    for fused, fused_loss in ((True, True), (True, False), (False, False)):
        m = _model(c, mode, fused=fused)
        h = _pooled(c, mode)
        hh = (h.bfloat16() if mode in _H_BF16 else h).cuda().requires_grad_(True)
        try:
            if fused_loss:
                loss, logits = m.forward_temporal_loss(hh, c.B, y.cuda())
            else:
                logits = m.forward_temporal(hh, c.B)
                loss = P().HybridCrossEntropyLoss()(logits, y.cuda())
            torch.cuda.synchronize()
        except RuntimeError:
            continue
        r_logits, r_loss = rel(logits, o_logits, l2=gate_as == "bf16"), rel(loss, o_loss)
        print(f"\n[C65 {mode} fused={fused} fused_loss={fused_loss}] forward returned: logits {r_logits:.2e} loss {r_loss:.2e} (gate {ftol:.1e})")
        check(logits, o_logits, ftol, "logits", gate_as)
        check(loss, o_loss, ftol, "loss", gate_as)
        with pytest.raises(RuntimeError):
            (loss * 1.5).backward()
        torch.cuda.synchronize()
    assert _ticket(c) == 0
