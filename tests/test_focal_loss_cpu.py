"""The focal and asymmetric losses as far as they go without a GPU: tests/focal_ref.py against torch's cross_entropy and
binary_cross_entropy_with_logits at their common points, against the sigmoid focal loss and the official asymmetric-loss expression restated
inline, the finiteness of the references on the whole grid of tests/test_gpu_focal_loss.py (and why an exponent between 0 and 1 is
refused), the eight new entry points of both libraries and the arguments they refuse, and the host-side checks of the two criteria."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

import transformer_cnn_hybrid_network_for_video_processing_amd as P
from transformer_cnn_hybrid_network_for_video_processing_amd import _lib

from focal_ref import ASYM_CONFIGS, BCE_SHAPES, FOCAL_GAMMAS, SHAPES, asym_case, asym_ref, clear_of_the_kink, focal_case, focal_ref

NEW = ("hyb_cross_entropy_focal_fwd", "hyb_cross_entropy_focal_bwd", "hyb_cross_entropy_asym_fwd", "hyb_cross_entropy_asym_bwd",
       "hyb_temporal_ce_focal_fwd", "hyb_temporal_ce_focal_bwd", "hyb_temporal_ce_asym_fwd", "hyb_temporal_ce_asym_bwd")
HYB_E_ARG = -1


@pytest.fixture(scope="module")
def built():
    from transformer_cnn_hybrid_network_for_video_processing_amd import build
    build.build()
    return _lib.lib


def _lg(fn, logits, dtype=torch.float64):
    lg = logits.to(dtype).requires_grad_(True)
    loss = fn(lg)
    loss.backward()
    return float(loss.detach()), lg.grad


@pytest.mark.parametrize("ign", [None, 1, -100], ids=["keepall", "ignore1", "ignore-100"])
@pytest.mark.parametrize("use_w", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"B{s[0]}C{s[1]}")
def test_focal_reference_at_gamma_0_is_cross_entropy(shape, use_w, ign):
    logits, y, w = focal_case(*shape, use_w)
    y = y.clone()
    if ign is not None and shape[0] > 1:
        y[-1] = ign
    y[0] = 0                                                          # clip 0 is kept and its class carries weight (the zero weight is w[1])
    l, g = _lg(lambda lg: focal_ref(lg, y, 0.0, w, ign), logits)
    lt, gt = _lg(lambda lg: F.cross_entropy(lg, y, weight=None if w is None else w.double(), ignore_index=-100 if ign is None else ign), logits)
    assert math.isfinite(l) and abs(l - lt) <= 1e-12 * max(1.0, abs(lt))
    assert float((g - gt).abs().max()) <= 1e-12 * max(1.0, float(gt.abs().max()))


def test_focal_reference_is_the_usual_focal_loss():
    """(1 - p_y) ** gamma * (-log p_y), mean over the batch, restated inline."""
    g = torch.Generator().manual_seed(5)
    z = torch.randn(6, 7, generator=g, dtype=torch.float64)
    y = torch.randint(0, 7, (6,), generator=g)
    logp = torch.log_softmax(z, 1).gather(1, y[:, None])[:, 0]
    for gamma in (1.0, 2.0, 5.0):
        want = ((1 - logp.exp()) ** gamma * -logp).mean()
        assert abs(float(focal_ref(z, y, gamma)) - float(want)) <= 1e-12


@pytest.mark.parametrize("use_pw", [False, True], ids=["nopw", "pw"])
@pytest.mark.parametrize("use_w", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("shape", BCE_SHAPES, ids=lambda s: f"B{s[0]}C{s[1]}")
def test_asymmetric_reference_at_zero_exponents_is_bce(shape, use_w, use_pw):
    """Multi-hot targets: with a soft target and a pos_weight the two definitions differ (L multiplies both logarithms here)."""
    logits, t, w, pw = asym_case(*shape, use_w, use_pw)
    d = lambda v: None if v is None else v.double()
    l, g = _lg(lambda lg: asym_ref(lg, t, 0.0, 0.0, 0.0, w, pw), logits)
    lt, gt = _lg(lambda lg: F.binary_cross_entropy_with_logits(lg, t.double(), weight=d(w), pos_weight=d(pw)), logits)
    assert math.isfinite(l) and abs(l - lt) <= 1e-12 * max(1.0, abs(lt))
    assert float((g - gt).abs().max()) <= 1e-12 * max(1.0, float(gt.abs().max()))
    # without a pos_weight a soft target agrees as well
    logits, t, w, _ = asym_case(*shape, use_w, False, soft=True)
    l = float(asym_ref(logits.double(), t, 0.0, 0.0, 0.0, w))
    lt = float(F.binary_cross_entropy_with_logits(logits.double(), t.double(), weight=d(w)))
    assert abs(l - lt) <= 1e-12 * max(1.0, abs(lt))


@pytest.mark.parametrize("soft", [False, True], ids=["multihot", "soft"])
def test_sigmoid_focal_is_the_usual_formula(soft):
    """alpha_t (1 - p_t) ** gamma bce, mean (the formula of torchvision.ops.sigmoid_focal_loss, restated), against the asymmetric reference
    with what HybridAsymmetricLoss.sigmoid_focal sets."""
    g = torch.Generator().manual_seed(8)
    z = 3.0 * torch.randn(9, 6, generator=g, dtype=torch.float64)
    t = torch.rand(9, 6, generator=g, dtype=torch.float64)
    if not soft:
        t = (t < 0.3).double()
    for gamma, alpha in ((2.0, 0.25), (1.0, 0.6), (0.0, 0.5)):
        p = torch.sigmoid(z)
        ce = F.binary_cross_entropy_with_logits(z, t, reduction="none")
        p_t = p * t + (1 - p) * (1 - t)
        want = ((alpha * t + (1 - alpha) * (1 - t)) * ce * (1 - p_t) ** gamma).mean()
        crit = P.HybridAsymmetricLoss.sigmoid_focal(gamma, alpha)
        assert (crit.gamma_pos, crit.gamma_neg, crit.clip) == (gamma, gamma, 0.0)
        crit._check_weight(6, torch.device("cpu"))
        assert crit.weight.shape == (6,) and crit.pos_weight.shape == (6,) and crit.weight.dtype == torch.float32
        assert abs(float(crit.weight[0]) - (1 - alpha)) <= 1e-7 and abs(float(crit.pos_weight[5]) - alpha / (1 - alpha)) <= 1e-6
        got = asym_ref(z, t, gamma, gamma, 0.0, torch.full((6,), 1 - alpha, dtype=torch.float64), torch.full((6,), alpha / (1 - alpha), dtype=torch.float64))
        assert abs(float(got) - float(want)) <= 1e-12 * max(1.0, abs(float(want)))


@pytest.mark.parametrize("cfg", ASYM_CONFIGS, ids=lambda c: f"gp{c[0]:g}gn{c[1]:g}m{c[2]:g}")
def test_asymmetric_reference_is_the_official_expression_where_no_clamp_binds(cfg):
    """The published AsymmetricLossOptimized forward (logs clamped at 1e-8, the focusing factor in the graph), restated; logits of 3 randn
    keep every probability far above 1e-8."""
    gp, gn, clip = cfg
    g = torch.Generator().manual_seed(12)
    x = (3.0 * torch.randn(16, 10, generator=g, dtype=torch.float64)).requires_grad_(True)
    y = (torch.rand(16, 10, generator=g) < 0.3).double()
    xs_pos = torch.sigmoid(x)
    xs_neg = 1.0 - xs_pos
    if clip > 0:
        xs_neg = (xs_neg + clip).clamp(max=1)
    assert float(xs_pos.detach().min()) > 1e-7 and float(xs_neg.detach().min()) > 1e-7
    loss = y * torch.log(xs_pos.clamp(min=1e-8)) + (1 - y) * torch.log(xs_neg.clamp(min=1e-8))
    if gp > 0 or gn > 0:
        loss = loss * torch.pow(1 - xs_pos * y - xs_neg * (1 - y), gp * y + gn * (1 - y))
    want = -loss.sum()
    want.backward()
    want = want.detach()
    got, grad = _lg(lambda lg: asym_ref(lg, y, gp, gn, clip) * x.numel(), x.detach())
    assert abs(got - float(want)) <= 1e-10 * max(1.0, abs(float(want)))
    assert float((grad - x.grad).abs().max()) <= 1e-10 * max(1.0, float(x.grad.abs().max()))


def test_references_are_finite_on_the_whole_gpu_grid_and_base_zero_is_exercised():
    """No case of tests/test_gpu_focal_loss.py is skipped: float64 and float32 losses and gradients are finite everywhere, no cell sits on
    the kink of the clipped probability, and many cells have base == 0 exactly (a clipped negative), where the rule for exponents applies."""
    zero_base = 0
    for dtype in (torch.float64, torch.float32):
        for shape in SHAPES:
            for use_w in (False, True):
                logits, y, w = focal_case(*shape, use_w)
                for gamma in FOCAL_GAMMAS:
                    l, g = _lg(lambda lg: focal_ref(lg, y, gamma, w), logits, dtype)
                    assert math.isfinite(l) and bool(torch.isfinite(g).all()), (shape, use_w, gamma)
        for shape in BCE_SHAPES:
            for use_w in (False, True):
                for use_pw in (False, True):
                    logits, t, w, pw = asym_case(*shape, use_w, use_pw)
                    for gp, gn, clip in ASYM_CONFIGS:
                        assert clear_of_the_kink(logits, clip), (shape, clip)
                        l, g = _lg(lambda lg: asym_ref(lg, t, gp, gn, clip, w, pw), logits, dtype)
                        assert math.isfinite(l) and bool(torch.isfinite(g).all()), (shape, use_w, use_pw, gp, gn, clip)
                        if dtype == torch.float32 and clip > 0:
                            zero_base += int(((t == 0) & (torch.sigmoid(logits) <= clip)).sum())
    assert zero_base > 500


def test_an_exponent_between_0_and_1_breaks_on_clipped_negatives():
    """Why such an exponent is refused: with multi-hot targets a clipped negative has base == 0 exactly, where the derivative of base ** 0.5
    is infinite and the gradient NaN; the uniform soft targets of dense_case never reach base == 0 and stay finite."""
    bad = soft_ok = 0
    for shape in BCE_SHAPES:
        logits, t, w, pw = asym_case(*shape, True, True)
        _, g = _lg(lambda lg: asym_ref(lg, t, 0.0, 0.5, 0.05, w, pw), logits)
        bad += int(not bool(torch.isfinite(g).all()))
        logits, t, w, pw = asym_case(*shape, True, True, soft=True)
        l, g = _lg(lambda lg: asym_ref(lg, t, 0.0, 0.5, 0.05, w, pw), logits)
        soft_ok += int(math.isfinite(l) and bool(torch.isfinite(g).all()))
    assert bad >= 3 and soft_ok == len(BCE_SHAPES)


def test_both_libraries_export_the_new_symbols_under_abi_9(built):
    for path in (_lib.LIB_PATH, _lib.LIB_X3_PATH):
        dll = ctypes.CDLL(path)
        for name in NEW:
            assert name in built.protos, name
            assert hasattr(dll, name), f"{name} is not exported by {path}"
    assert built.query("hyb_abi_version") == 9 and built.x3.query("hyb_abi_version") == 9
    header = open(_lib.HEADER).read()
    for name in NEW:
        assert header.count(name + "(") == 1, name
    pr = built.protos
    assert pr["hyb_cross_entropy_focal_fwd"] == ("int", ["ptr", "ptr", "ptr", "long long", "int", "float", "ptr", "int", "int", "ptr"])
    assert pr["hyb_cross_entropy_focal_bwd"] == ("int", ["ptr", "ptr", "ptr", "long long", "int", "float", "ptr", "ptr", "int", "int", "ptr"])
    assert pr["hyb_cross_entropy_asym_fwd"] == ("int", ["ptr", "ptr", "ptr", "ptr", "float", "float", "float", "ptr", "int", "int", "ptr"])
    assert pr["hyb_cross_entropy_asym_bwd"] == ("int", ["ptr", "ptr", "ptr", "ptr", "float", "float", "float", "ptr", "ptr", "int", "int", "ptr"])
    # the *_opts_* lists with gamma in label_smoothing's place; the *_dense_* lists with (gamma_pos, gamma_neg, clip) for (kind, label_smoothing)
    for way, at in (("fwd", 8), ("bwd", 3)):
        assert pr[f"hyb_temporal_ce_focal_{way}"] == pr[f"hyb_temporal_ce_opts_{way}"]
        dense, asym = pr[f"hyb_temporal_ce_dense_{way}"][1], pr[f"hyb_temporal_ce_asym_{way}"][1]
        assert asym[:at + 3] == dense[:at + 3] and asym[at + 3:at + 6] == ["float"] * 3 and asym[at + 6:] == dense[at + 5:]
    assert "hyb_temporal_ce_asym_fwd" in _lib.DTYPE_FIRST and "hyb_cross_entropy_focal_fwd" not in _lib.DTYPE_FIRST
    # the structs and kernel signatures of the earlier families are where they were
    internal = open(_lib.HEADER.replace("include/hybrid_hip.h", "transformer_cnn_hybrid_network_for_video_processing_amd/csrc/hyb_internal.h")).read()
    assert "struct HybCeOpts { const float* weight; long long ignore_index; int has_ignore; float label_smoothing; };" in internal
    assert "struct HybCeDense { const float* target; const float* pos_weight; int kind; };" in internal
    assert "struct HybCeMix { const long long* target_b; const float* lam; };" in internal


@pytest.mark.parametrize("which", ["main", "x3"])
def test_new_entry_points_refuse_bad_arguments_without_a_device(built, which):
    lib = built if which == "main" else built.x3
    for name in NEW:
        args = [None if a == "ptr" else 0 for a in lib.protos[name][1]]
        assert lib.raw(name)(*args) == HYB_E_ARG, name
    one = ctypes.c_float(0.0)
    p = ctypes.addressof(one)
    f = ctypes.c_float
    bad_gammas = (0.5, -1.0, 0.999, float("nan"), float("inf"))
    fwd, bwd = lib.raw("hyb_cross_entropy_focal_fwd"), lib.raw("hyb_cross_entropy_focal_bwd")
    # (logits, target, weight, ignore_index, has_ignore, gamma, loss, B, C, stream)
    assert fwd(None, p, None, 0, 0, f(2.0), p, 1, 2, None) == HYB_E_ARG
    assert fwd(p, None, None, 0, 0, f(2.0), p, 1, 2, None) == HYB_E_ARG
    assert fwd(p, p, None, 0, 0, f(2.0), None, 1, 2, None) == HYB_E_ARG
    assert bwd(p, p, None, 0, 0, f(2.0), None, p, 1, 2, None) == HYB_E_ARG
    assert bwd(p, p, None, 0, 0, f(2.0), p, None, 1, 2, None) == HYB_E_ARG
    for g in bad_gammas:
        assert fwd(p, p, None, 0, 0, f(g), p, 1, 2, None) == HYB_E_ARG, g
        assert bwd(p, p, None, 0, 0, f(g), p, p, 1, 2, None) == HYB_E_ARG, g
    fwd, bwd = lib.raw("hyb_cross_entropy_asym_fwd"), lib.raw("hyb_cross_entropy_asym_bwd")
    # (logits, target, weight, pos_weight, gamma_pos, gamma_neg, clip, loss, B, C, stream)
    assert fwd(None, p, None, None, f(0.0), f(4.0), f(0.05), p, 1, 2, None) == HYB_E_ARG
    assert fwd(p, None, None, None, f(0.0), f(4.0), f(0.05), p, 1, 2, None) == HYB_E_ARG
    assert fwd(p, p, None, None, f(0.0), f(4.0), f(0.05), None, 1, 2, None) == HYB_E_ARG
    assert bwd(p, p, None, None, f(0.0), f(4.0), f(0.05), None, p, 1, 2, None) == HYB_E_ARG
    assert bwd(p, p, None, None, f(0.0), f(4.0), f(0.05), p, None, 1, 2, None) == HYB_E_ARG
    for g in bad_gammas:
        assert fwd(p, p, None, None, f(g), f(4.0), f(0.05), p, 1, 2, None) == HYB_E_ARG, g
        assert fwd(p, p, None, None, f(0.0), f(g), f(0.05), p, 1, 2, None) == HYB_E_ARG, g
        assert bwd(p, p, None, None, f(0.0), f(g), f(0.05), p, p, 1, 2, None) == HYB_E_ARG, g
    for clip in (-0.1, 1.0, 1.5, float("nan")):
        assert fwd(p, p, None, None, f(0.0), f(4.0), f(clip), p, 1, 2, None) == HYB_E_ARG, clip
        assert bwd(p, p, None, None, f(0.0), f(4.0), f(clip), p, p, 1, 2, None) == HYB_E_ARG, clip
    # the temporal pairs: every other argument in order, the scalars bad
    for stem, at_scalar in (("focal", 4), ("asym", 3)):
        for way, at in (("fwd", 8), ("bwd", 3)):
            name = f"hyb_temporal_ce_{stem}_{way}"
            base = [p if a == "ptr" else 1 for a in lib.protos[name][1]]
            base[0], base[-1] = 0, None                                             # dtype fp32, stream
            good = [0, 0, f(2.0)] if stem == "focal" else [None, f(0.0), f(4.0), f(0.05)]       # from the argument behind weight on
            first = at + 2
            base[at + 1] = None                                                      # weight
            for patch in ([(at_scalar - 2 if stem == "focal" else 1, f(0.5))], [(len(good) - 1, f(float("nan")))], [(-1, None)]):
                args = list(base)
                args[first:first + len(good)] = good
                for i, v in patch:
                    if i < 0:
                        args[at] = v                                                 # the target itself
                    else:
                        args[first + i] = v
                assert lib.raw(name)(*args) == HYB_E_ARG, (name, patch)


def test_constructor_checks_of_the_two_criteria():
    good = torch.tensor([1.0, 0.0, 2.0])
    fl = P.HybridFocalLoss()
    assert fl.gamma == 2.0 and fl.weight is None and fl.ignore_index is None
    fl = P.HybridFocalLoss(gamma=0, weight=good, ignore_index=-100)
    assert fl.gamma == 0.0 and torch.equal(fl.weight, good) and fl.weight.data_ptr() != good.data_ptr() and "weight" in fl.state_dict()
    asl = P.HybridAsymmetricLoss()
    assert (asl.gamma_neg, asl.gamma_pos, asl.clip) == (4.0, 0.0, 0.05) and asl.weight is None and asl.pos_weight is None
    asl = P.HybridAsymmetricLoss(1, 1.5, 0, weight=good, pos_weight=good)
    assert (asl.gamma_neg, asl.gamma_pos, asl.clip) == (1.0, 1.5, 0.0) and {"weight", "pos_weight"} <= set(dict(asl.named_buffers()))
    for g in (0.5, -1.0, 0.99, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="0 or >= 1"):
            P.HybridFocalLoss(gamma=g)
        with pytest.raises(ValueError, match="gamma_neg must be 0 or >= 1"):
            P.HybridAsymmetricLoss(gamma_neg=g)
        with pytest.raises(ValueError, match="gamma_pos must be 0 or >= 1"):
            P.HybridAsymmetricLoss(gamma_pos=g)
        with pytest.raises(ValueError, match="0 or >= 1"):
            P.HybridAsymmetricLoss.sigmoid_focal(gamma=g)
    for g in ("2", None, True):
        with pytest.raises(TypeError, match="must be a number"):
            P.HybridFocalLoss(gamma=g)
    for clip in (-0.01, 1.0, 2.0, float("nan")):
        with pytest.raises(ValueError, match=r"clip must be in \[0, 1\)"):
            P.HybridAsymmetricLoss(clip=clip)
    for alpha in (0.0, 1.0, -0.2, 1.5):
        with pytest.raises(ValueError, match="alpha"):
            P.HybridAsymmetricLoss.sigmoid_focal(alpha=alpha)
    with pytest.raises(TypeError, match="ignore_index"):
        P.HybridFocalLoss(ignore_index=1.5)
    for cls in (P.HybridFocalLoss, P.HybridAsymmetricLoss):
        with pytest.raises(ValueError, match="1-D float32"):
            cls(weight=good.double())
        with pytest.raises(ValueError, match="negative"):
            cls(weight=torch.tensor([1.0, -0.5]))
    with pytest.raises(ValueError, match="negative"):
        P.HybridAsymmetricLoss(pos_weight=torch.tensor([1.0, float("nan")]))
    assert "HybridFocalLoss" in P.__all__ and "HybridAsymmetricLoss" in P.__all__


def test_host_side_checks_of_targets_and_operators():
    from transformer_cnn_hybrid_network_for_video_processing_amd import ops
    logits, t, y = torch.randn(4, 3), torch.rand(4, 3), torch.tensor([0, 1, 2, 0])
    mix = P.MixTarget(y, torch.tensor([1, 1, 0, 2]), torch.rand(4))
    fl, asl = P.HybridFocalLoss(), P.HybridAsymmetricLoss()
    for bad in (t, mix):
        with pytest.raises(TypeError, match="class indices"):
            fl(logits, bad)
    for bad in (y, mix):
        with pytest.raises(TypeError, match="floating target"):
            asl(logits, bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fl(logits, y)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        asl(logits, t)
    with pytest.raises(ValueError, match="shape of the logits"):
        asl(logits, t[:3])
    with pytest.raises(TypeError, match="float32"):
        asl(logits, t.double())
    with pytest.raises(ValueError, match="weight has 4 entries"):
        P.HybridFocalLoss(weight=torch.ones(4))(logits, y)
    with pytest.raises(ValueError, match="pos_weight has 2 entries"):
        P.HybridAsymmetricLoss(pos_weight=torch.ones(2))(logits, t)
    # an exponent or clip changed on the module to a refused value is caught at the call, before anything is launched
    fl.gamma = 0.5
    with pytest.raises(ValueError, match="0 or >= 1"):
        fl(logits, y)
    asl.clip = 1.0
    with pytest.raises(ValueError, match="clip"):
        asl(logits, t)
    for call in (lambda: ops.cross_entropy_focal(logits, y, None, None, 0.5), lambda: ops.cross_entropy_asym(logits, t, None, None, 0.5, 4.0, 0.05),
                 lambda: ops.cross_entropy_asym(logits, t, None, None, 0.0, float("nan"), 0.05)):
        with pytest.raises(ValueError, match="0 or >= 1"):
            call()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cross_entropy_asym(logits, t, None, None, 0.0, 4.0, 0.05)
    # the meters keep refusing criteria they do not know
    with pytest.raises((TypeError, ValueError)):
        P.ClassificationMeter(3, criterion=fl)
