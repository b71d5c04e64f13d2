"""CPU-only tests of multi-label evaluation: hyb_eval_multilabel is declared, exported by both builds and refuses bad arguments without
touching a device; the float64 reference of tests/multilabel_ref.py agrees with torch's BCE functions, with a brute-force evaluation of the
average-precision definition and with scikit-learn; the shared cases keep every score away from its threshold, so that the GPU test's exact
integer comparisons leave out no cell; and MultiLabelMeter's host side (validation, reset, compute, merge, all_reduce over gloo) works on CPU
tensors, while update() has no CPU fallback."""
import ctypes
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import transformer_cnn_hybrid_network_for_video_processing_amd as P
from transformer_cnn_hybrid_network_for_video_processing_amd import _lib
from transformer_cnn_hybrid_network_for_video_processing_amd.meter import average_precision

from multilabel_ref import (AP_B, AP_C, MULTIVIEW, OPTION_IDS, OPTIONS, SCORE_TOL, SHAPES, THRESHOLDS, ap_case, average_precision_brute,
                            average_precision_ref, case, loss_of, min_distinct_gap, multilabel_ref, multiview_case, multiview_score_tol,
                            threshold_distance)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    from transformer_cnn_hybrid_network_for_video_processing_amd import build
    build.build()
    return _lib.lib


# ---- header and exports -----------------------------------------------------------------------------------------------------------------
def test_prototype_is_parsed():
    protos = _lib.parse_header()
    assert protos["hyb_eval_multilabel"] == ("int", ["ptr"] * 5 + ["int"] + ["ptr"] * 5 + ["long long"] + ["ptr"] * 2 + ["int", "int", "ptr"])


def test_both_builds_export_the_symbol_and_the_abi_version_stays(built):
    built.raw("hyb_eval_multilabel")
    built.x3.raw("hyb_eval_multilabel")
    assert built.query("hyb_abi_version") == 9 and built.x3.query("hyb_abi_version") == 9


def test_argument_checks_fail_without_a_device(built):
    fake = ctypes.c_void_p(16)                     # never dereferenced: every check below fails before any HIP call
    for dll in (built, built.x3):
        fn = dll.raw("hyb_eval_multilabel")

        def m(logits=fake, target=fake, weight=None, pw=None, thr=fake, views=1, sums=fake, counts=fake, cells=fake, bs=None, bl=None, cap=0,
              pred=None, scores=fake, B=4, C=5):
            return fn(logits, target, weight, pw, thr, views, sums, counts, cells, bs, bl, cap, pred, scores, B, C, None)
        for name in ("logits", "target", "thr", "sums", "counts", "cells", "scores"):
            assert m(**{name: None}) == -1, name
        assert m(B=0) == -1 and m(B=-3) == -1 and m(C=0) == -1 and m(C=-1) == -1
        assert m(views=0) == -1 and m(views=-2) == -1
        assert m(cap=-1) == -1 and m(cap=-1, bs=fake, bl=fake) == -1
        assert m(bs=fake, cap=8) == -1 and m(bl=fake, cap=8) == -1                       # exactly one of the two bank pointers
        assert m(bs=fake, bl=fake, cap=0) == -1                                          # a bank of no rows
    with pytest.raises(RuntimeError, match="argument check"):
        built.call("hyb_eval_multilabel", fake, fake, None, None, fake, 0, fake, fake, fake, None, None, 0, None, fake, 4, 5, None)


# ---- the reference itself ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", OPTIONS, ids=OPTION_IDS)
def test_reference_loss_is_torchs_bce(opt):
    for B, C in SHAPES:
        logits, target, w, pw = case(B, C, *opt)
        ref = multilabel_ref(logits, target, w, pw)
        want = F.binary_cross_entropy_with_logits(logits.double(), target.double(), weight=None if w is None else w.double(),
                                                  pos_weight=None if pw is None else pw.double(), reduction="sum")
        assert abs(float(ref["num"]) - float(want)) <= 1e-12 * max(1.0, abs(float(want))), (B, C)
        assert torch.equal(ref["scores"], torch.sigmoid(logits.double()))
    for B, V, C in MULTIVIEW:
        logits, target, w, pw = multiview_case(B, V, C, *opt)
        ref = multilabel_ref(logits, target, w, pw, views=V)
        s = torch.sigmoid(logits.double()).reshape(B, V, C).mean(1)
        assert float((ref["scores"] - s).abs().max()) <= 1e-15
        # F.binary_cross_entropy has no pos_weight: weigh the positive cells by hand
        cw = (torch.ones(C, dtype=torch.float64) if w is None else w.double()).expand(B, C)
        if pw is not None:
            cw = cw * torch.where(target.double() >= 0.5, pw.double().expand(B, C), torch.ones(B, C, dtype=torch.float64))
        want = F.binary_cross_entropy(ref["scores"], target.double(), weight=cw, reduction="sum")
        assert abs(float(ref["num"]) - float(want)) <= 1e-12 * max(1.0, abs(float(want))), (B, V, C)


def test_reference_cells_nan_and_threshold_rules():
    z = torch.tensor([[0.0, 2.0, -2.0], [float("nan"), 3.0, 3.0], [1.0, -1.0, 0.0]])
    t = torch.tensor([[1.0, 0.0, 1.0], [1.0, 1.0, 0.0], [0.0, float("nan"), 0.49]])
    ref = multilabel_ref(z, t)
    assert ref["pred"].tolist() == [[1, 1, 0], [0, 0, 0], [1, 0, 1]]                    # sigmoid(0) = 0.5 reaches 0.5; the NaN video predicts nothing
    assert ref["labels"].tolist() == [[1, 0, 1], [1, 1, 0], [0, 0, 0]]                  # a NaN target is a negative label
    assert ref["cells"].tolist() == [[1, 1, 1], [0, 1, 1], [0, 1, 1]]
    assert ref["counts"] == [3, 1, 0] and math.isnan(float(ref["num"]))
    assert ref["bank"][1].tolist() == [float("-inf")] * 3
    ref = multilabel_ref(z[[0, 2]], t[[0, 2]].nan_to_num(0.0), threshold=[0.6, 0.2, 0.1])
    assert ref["pred"].tolist() == [[0, 1, 1], [1, 1, 1]]


def _ap_inputs():
    out = []
    for V in (1, 3):
        logits, target = ap_case(V)
        out.append((V, multilabel_ref(logits, target, views=V)["scores"].numpy(), target.numpy()))
    return out


def test_reference_ap_is_the_brute_force_definition_and_scikit_learns():
    for V, s, y in _ap_inputs():
        ap = average_precision_ref(s, y)
        assert np.isfinite(ap).all()
        brute = average_precision_brute(s, y)
        assert np.abs(ap - brute).max() <= 1e-12, (V, ap, brute)
        assert any(len(np.unique(s[:, c])) < AP_B for c in range(AP_C))                  # there ARE ties
    try:
        from sklearn.metrics import average_precision_score
    except ImportError:
        return                                                                           # the brute-force check above stands
    for V, s, y in _ap_inputs():
        want = np.array([average_precision_score(y[:, c], s[:, c]) for c in range(AP_C)])
        assert np.abs(average_precision_ref(s, y) - want).max() <= 1e-12, V


def test_ap_ignores_the_order_of_the_rows_and_the_meters_torch_form_agrees():
    g = torch.Generator().manual_seed(5)
    for V, s, y in _ap_inputs():
        ap = average_precision_ref(s, y)
        perm = torch.randperm(AP_B, generator=g).numpy()
        assert np.array_equal(average_precision_ref(s[perm], y[perm]), ap)              # per-threshold counts: nothing depends on the order
        got = average_precision(torch.from_numpy(s).float(), torch.from_numpy(y).to(torch.uint8))
        # fp32 rounding is monotonic and keeps these well-separated values distinct: the same ranks, the same AP
        assert float((got - torch.from_numpy(ap)).abs().max()) <= 1e-12
        got_p = average_precision(torch.from_numpy(s[perm]).float(), torch.from_numpy(y[perm]).to(torch.uint8))
        assert torch.equal(got, got_p)                                                   # bit-identical whatever the row order
        # rows marked invalid weigh nothing wherever they sort
        pad_s = torch.cat([torch.from_numpy(s).float(), torch.full((7, AP_C), 0.5)])
        pad_y = torch.cat([torch.from_numpy(y).to(torch.uint8), torch.ones(7, AP_C, dtype=torch.uint8)])
        valid = torch.arange(AP_B + 7) < AP_B
        assert torch.equal(average_precision(pad_s, pad_y, valid), got)
    none = average_precision(torch.rand(6, 2), torch.tensor([[1, 0]] * 6, dtype=torch.uint8))
    assert float(none[0]) == 1.0 and math.isnan(float(none[1]))                          # no positive label: NaN


# ---- conditions that keep the GPU comparisons honest ------------------------------------------------------------------------------------
def test_no_score_of_a_shared_case_sits_on_its_threshold():
    """The GPU test compares pred, cells and counts EXACTLY and leaves out nothing: an fp32 score is within SCORE_TOL (one view) or
    (V + 3) 2^-23 (several) of the float64 one, so no cell may be that close to its threshold."""
    closest = float("inf")
    for B, C in SHAPES:
        for thr in THRESHOLDS:
            logits, target, _, _ = case(B, C)
            d = threshold_distance(multilabel_ref(logits, target, threshold=thr), thr)
            closest = min(closest, d)
            assert d > SCORE_TOL, (B, C, thr, d)
    print(f"one view: the closest cell is {closest:.3e} from its threshold (must exceed {SCORE_TOL:.3e})")
    closest = float("inf")
    for B, V, C in MULTIVIEW:
        for thr in THRESHOLDS:
            logits, target, _, _ = multiview_case(B, V, C)
            d = threshold_distance(multilabel_ref(logits, target, threshold=thr, views=V), thr)
            closest = min(closest, d)
            assert d > multiview_score_tol(V), (B, V, C, thr, d)
    print(f"several views: the closest cell is {closest:.3e} from its threshold")


def test_multiview_scores_stay_away_from_zero_and_one():
    """The multi-view loss bound divides by min(s, 1 - s): it must stay >= 0.05 in every shared case."""
    lo = 1.0
    for B, V, C in MULTIVIEW:
        logits, target, _, _ = multiview_case(B, V, C)
        s = multilabel_ref(logits, target, views=V)["scores"]
        lo = min(lo, float(torch.minimum(s, 1.0 - s).min()))
    print(f"several views: min(s, 1 - s) = {lo:.4f}")
    assert lo >= 0.05


def test_ap_cases_keep_distinct_scores_apart():
    for V, s, y in _ap_inputs():
        gap = min_distinct_gap(s)
        print(f"AP case V={V}: distinct scores at least {gap:.3e} apart")
        assert gap >= 1e-4
        assert y.sum(0).min() >= 1 and (1 - y).sum(0).min() >= 1


# ---- the meter on the CPU ---------------------------------------------------------------------------------------------------------------
def _filled(seed, capacity=6, stored=3, C=4):
    g = torch.Generator().manual_seed(seed)
    m = P.MultiLabelMeter(C, capacity=capacity, device="cpu")
    m.sums.copy_(torch.rand(1, generator=g, dtype=torch.float64) * 50)
    m.counts.copy_(torch.tensor([stored + 2, 1, 2, stored if capacity else 0, 2 if capacity else 0]))
    m.cells.copy_(torch.randint(0, 9, (C, 3), generator=g))
    if capacity:
        m.bank_scores[:stored] = torch.rand(stored, C, generator=g)
        m.bank_labels[:stored] = (torch.rand(stored, C, generator=g) < 0.5).to(torch.uint8)
    return m


def test_constructor_validation():
    for bad in (0, -2, 3.0, True):
        with pytest.raises(ValueError, match="num_classes"):
            P.MultiLabelMeter(bad, device="cpu")
    for bad in (-1, 2.5, True):
        with pytest.raises(ValueError, match="capacity"):
            P.MultiLabelMeter(3, capacity=bad, device="cpu")
    for bad in (0.0, 1.0, -0.2, [0.5, 0.5], [0.5, 0.2, 1.5], float("nan")):
        with pytest.raises(ValueError, match="threshold"):
            P.MultiLabelMeter(3, threshold=bad, device="cpu")
    for bad in ("half", None, True):
        with pytest.raises(TypeError, match="threshold"):
            P.MultiLabelMeter(3, threshold=bad, device="cpu")
    for bad in (torch.nn.BCEWithLogitsLoss(), P.HybridCrossEntropyLoss(), "bce", 1.0):
        with pytest.raises(TypeError, match="criterion"):
            P.MultiLabelMeter(3, criterion=bad, device="cpu")
    with pytest.raises(ValueError, match="weight has 4 entries"):
        P.MultiLabelMeter(3, criterion=P.HybridBCEWithLogitsLoss(weight=torch.ones(4)), device="cpu")
    with pytest.raises(ValueError, match="pos_weight has 2 entries"):
        P.MultiLabelMeter(3, criterion=P.HybridBCEWithLogitsLoss(pos_weight=torch.ones(2)), device="cpu")
    crit = P.HybridBCEWithLogitsLoss(weight=torch.ones(3), pos_weight=2 * torch.ones(3))
    m = P.MultiLabelMeter(3, threshold=[0.2, 0.5, 0.7], criterion=crit, capacity=4, device="cpu")
    assert m.loss_options()[0] is crit.weight and m.loss_options()[1] is crit.pos_weight
    assert m.threshold.dtype == torch.float32 and m.threshold.tolist() == [float(np.float32(v)) for v in (0.2, 0.5, 0.7)]
    assert P.MultiLabelMeter(3, threshold=torch.tensor([0.25, 0.5, 0.75], dtype=torch.float64), device="cpu").threshold.tolist() == [0.25, 0.5, 0.75]
    assert P.MultiLabelMeter(2, device="cpu").threshold.tolist() == [0.5, 0.5] and P.MultiLabelMeter(2, device="cpu").loss_options() == (None, None)
    assert "MultiLabelMeter" in P.__all__


def test_state_is_created_zeroed_and_reset_zeroes_in_place():
    m = P.MultiLabelMeter(4, capacity=6, device="cpu")
    assert m.sums.dtype == torch.float64 and m.sums.tolist() == [0.0]
    assert m.counts.dtype == torch.int64 and m.counts.tolist() == [0] * 5
    assert m.cells.dtype == torch.int64 and tuple(m.cells.shape) == (4, 3) and int(m.cells.abs().sum()) == 0
    assert m.bank_scores.dtype == torch.float32 and tuple(m.bank_scores.shape) == (6, 4)
    assert m.bank_labels.dtype == torch.uint8 and tuple(m.bank_labels.shape) == (6, 4)
    none = P.MultiLabelMeter(4, device="cpu")
    assert none.bank_scores is None and none.bank_labels is None and "mAP" not in none.compute()
    f = _filled(1)
    ptrs = [t.data_ptr() for t in f._state()]
    f.reset()
    assert [t.data_ptr() for t in f._state()] == ptrs
    assert f.sums.tolist() == [0.0] and f.counts.tolist() == [0] * 5 and int(f.cells.abs().sum()) == 0      # the cursor too
    assert f.compute()["stored"] == 0 and math.isnan(f.compute()["mAP"])


def test_compute_reports_every_derived_number():
    m = P.MultiLabelMeter(3, capacity=5, device="cpu")
    out = m.compute()
    assert (out["videos"], out["nan_rows"], out["stored"], out["dropped"]) == (0, 0, 0, 0) and out["support"] == [0, 0, 0]
    for k in ("loss", "exact_match", "hamming_accuracy", "micro_precision", "micro_recall", "micro_f1", "macro_f1", "mAP"):
        assert math.isnan(out[k]), k
    for k in ("per_class_precision", "per_class_recall", "per_class_f1", "per_class_ap"):
        assert all(math.isnan(v) for v in out[k]), k
    #                      tp fp fn
    m.cells.copy_(torch.tensor([[3, 1, 1], [0, 0, 0], [0, 2, 2]]))
    m.sums.copy_(torch.tensor([18.0], dtype=torch.float64))
    m.counts.copy_(torch.tensor([8, 1, 2, 4, 0]))
    m.bank_scores[:4] = torch.tensor([[0.9, 0.1, 0.5], [0.8, 0.2, 0.5], [0.3, 0.3, 0.4], [0.3, 0.4, 0.1]])
    m.bank_labels[:4] = torch.tensor([[1, 0, 0], [0, 0, 1], [1, 0, 0], [0, 0, 1]], dtype=torch.uint8)
    m.bank_scores[4] = 7.0                                                               # beyond the cursor: never read
    m.bank_labels[4] = 1
    out = m.compute()
    assert out["loss"] == 18.0 / 24 and (out["videos"], out["nan_rows"], out["stored"], out["dropped"]) == (8, 1, 4, 0)
    assert out["exact_match"] == 0.25 and out["hamming_accuracy"] == 1.0 - 6 / 24 and out["support"] == [4, 0, 2]
    assert out["per_class_precision"][0] == 0.75 and math.isnan(out["per_class_precision"][1]) and out["per_class_precision"][2] == 0.0
    assert out["per_class_recall"][0] == 0.75 and math.isnan(out["per_class_recall"][1]) and out["per_class_recall"][2] == 0.0
    assert out["per_class_f1"][0] == 0.75 and math.isnan(out["per_class_f1"][1]) and out["per_class_f1"][2] == 0.0
    assert out["micro_precision"] == 0.5 and out["micro_recall"] == 0.5 and out["micro_f1"] == 0.5 and out["macro_f1"] == 0.375
    # class 0: thresholds 0.9 (P 1, R 1/2), 0.8 (no step), 0.3 (tie of a positive and a negative: P 2/4, R 1) -> 1/2 + 1/4
    # class 1: no positive -> NaN; class 2: 0.5 (tie: P 1/2, R 1/2), 0.4 (no step), 0.1 (P 2/4, R 1) -> 1/4 + 1/4
    assert out["per_class_ap"][0] == 0.75 and math.isnan(out["per_class_ap"][1]) and out["per_class_ap"][2] == 0.5
    assert out["mAP"] == 0.625
    want = average_precision_ref(m.bank_scores[:4].numpy(), m.bank_labels[:4].numpy())
    assert out["per_class_ap"][0] == want[0] and out["per_class_ap"][2] == want[2]
    m.counts[4] = 1                                                                      # a partial bank gives no silent answer
    out = m.compute()
    assert out["dropped"] == 1 and math.isnan(out["mAP"]) and all(math.isnan(v) for v in out["per_class_ap"])
    assert out["micro_f1"] == 0.5                                                        # the cells cover every video all the same


def test_merge_adds_exactly_appends_the_bank_and_counts_the_overflow():
    a, b = _filled(1), _filled(2)
    want = [x.clone() + y for x, y in zip(a._state(), b._state())]
    rows = torch.cat([a.bank_scores[:3], b.bank_scores[:3]]), torch.cat([a.bank_labels[:3], b.bank_labels[:3]])
    theirs = [t.clone() for t in b._state() + [b.bank_scores, b.bank_labels]]
    assert a.merge(b) is a
    assert torch.equal(a.sums, want[0]) and torch.equal(a.cells, want[2])
    assert a.counts.tolist() == [10, 2, 4, 6, 4]                                         # six rows fill the bank exactly
    assert torch.equal(a.bank_scores, rows[0]) and torch.equal(a.bank_labels, rows[1])
    for got, w in zip(b._state() + [b.bank_scores, b.bank_labels], theirs):
        assert torch.equal(got, w)                                                       # the other meter is left as it is
    a.merge(_filled(3, stored=2))                                                        # no room left: both rows dropped
    assert a.counts.tolist() == [14, 3, 6, 6, 4 + 2 + 2] and torch.equal(a.bank_scores, rows[0])
    c = _filled(4, stored=5)
    c.merge(b)                                                                           # one of three fits
    assert c.counts[3] == 6 and c.counts[4] == 2 + 2 + 2 and torch.equal(c.bank_scores[5], b.bank_scores[0])
    with pytest.raises(ValueError):
        a.merge(P.MultiLabelMeter(5, capacity=6, device="cpu"))
    with pytest.raises(ValueError):
        a.merge(P.MultiLabelMeter(4, device="cpu"))
    with pytest.raises(TypeError):
        a.merge(P.ClassificationMeter(4, topk=1, device="cpu"))
    n1, n2 = _filled(5, capacity=0), _filled(6, capacity=0)                              # no bank on either side
    w = [x.clone() + y for x, y in zip(n1._state(), n2._state())]
    n1.merge(n2)
    assert all(torch.equal(x, y) for x, y in zip(n1._state(), w))


def test_update_has_no_cpu_fallback():
    m = P.MultiLabelMeter(5, capacity=4, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.update(torch.randn(4, 5), torch.zeros(4, 5))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.update(torch.randn(8, 5), torch.zeros(4, 5), views=2)
    assert m.counts.tolist() == [0] * 5
    with pytest.raises(ValueError, match="views"):
        m.update(torch.randn(4, 5), torch.zeros(4, 5), views=0)


_WORKER = """
import sys, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import transformer_cnn_hybrid_network_for_video_processing_amd as P
from test_multilabel_cpu import _filled
rank = int(sys.argv[2])
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:" + sys.argv[3], rank=rank, world_size=2)
a, b = _filled(10, capacity=7, stored=4), _filled(11, capacity=7, stored=5)
m = _filled(10 + rank, capacity=7, stored=4 + rank)
assert m.all_reduce() is m
assert torch.equal(m.sums, a.sums + b.sums) and torch.equal(m.cells, a.cells + b.cells)
assert m.counts.tolist() == [6 + 7, 2, 4, 7, 2 + 2 + 2], m.counts.tolist()
assert torch.equal(m.bank_scores, torch.cat([a.bank_scores[:4], b.bank_scores[:3]]))
assert torch.equal(m.bank_labels, torch.cat([a.bank_labels[:4], b.bank_labels[:3]]))
n = _filled(20 + rank, capacity=0)
want = [x + y for x, y in zip(_filled(20, capacity=0)._state(), _filled(21, capacity=0)._state())]
n.all_reduce()
assert all(torch.equal(x, y) for x, y in zip(n._state(), want))
bad = P.MultiLabelMeter(4, capacity=3 + rank, device="cpu")
try:
    bad.all_reduce()
    raise SystemExit("unequal capacities were accepted")
except ValueError:
    pass
dist.destroy_process_group()
print("rank", rank, "ok")
"""


def test_all_reduce_over_two_gloo_ranks():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = str(s.getsockname()[1])
    procs = [subprocess.Popen([sys.executable, "-c", _WORKER, ROOT, str(r), port], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(2)]
    for r, p in enumerate(procs):
        out = p.communicate(timeout=120)[0].decode()
        assert p.returncode == 0 and f"rank {r} ok" in out, out
