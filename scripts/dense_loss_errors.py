"""Worst loss / gradient errors of the two criteria on dense targets per option combination, from measure() of tests/test_gpu_dense_loss.py
(its grid, its reference, its gates).  Needs the GPU.

    python scripts/dense_loss_errors.py > profiles/dense_loss_errors.txt
"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import test_gpu_dense_loss as T

print("# HybridCrossEntropyLoss(weight, label_smoothing)(logits, t) [kind 0] and HybridBCEWithLogitsLoss(weight, pos_weight)(logits, t) [kind 1], t an")
print("# fp32 [B,C] target, on the MI355X against tests/dense_ref.py in float64 (CPU), dloss = 1.5; grid of tests/test_gpu_dense_loss.py: (B,C) in")
print("#", T.SHAPES, "plus (4, 1) for kind 1; kind 0 rows hold an exact one-hot row and an all-zero row, kind 1 logits hold +100 and -100")
print("# per combination, worst over the shapes: loss error / its bound 1e-5 max(1,|ref|); gradient error, the arbiter's (the same definition")
print("# in fp32 on the CPU against the same reference), and gradient error / gate (gate = 4 * arbiter + 1e-6 * max|g_ref|)")
print(f"{'kind':>4} {'eps':>4} {'weighted':>8} {'pos_w':>6} | {'loss err':>10} {'loss/bound':>10} | {'grad err':>10} {'arbiter':>10} {'kernel/gate':>11} {'worst (B,C)':>12}")
combos = [(0, eps, use_w, False) for eps in T.EPS for use_w in (False, True)] + [(1, 0.0, use_w, use_pw) for use_w in (False, True) for use_pw in (False, True)]
worst_all = (0, None)
worst_loss = 0.0
n = 0
for kind, eps, use_w, use_pw in combos:
    wl = wlr = 0.0; wg = (-1, 0, 0, None)
    for B, C in (T.BCE_SHAPES if kind == 1 else T.SHAPES):
        lerr, lb, gerr, gb, arb = T.measure(kind, B, C, eps, use_w, use_pw)
        n += 1
        wl = max(wl, lerr); wlr = max(wlr, lerr / lb)
        if gerr / gb > wg[0]:
            wg = (gerr / gb, gerr, arb, (B, C))
    worst_loss = max(worst_loss, wlr)
    print(f"{kind:>4} {eps:>4} {str(use_w):>8} {str(use_pw):>6} | {wl:10.3e} {wlr:10.3f} | {wg[1]:10.3e} {wg[2]:10.3e} {wg[0]:11.3f} {str(wg[3]):>12}")
    if wg[0] > worst_all[0]:
        worst_all = (wg[0], (kind, eps, use_w, use_pw) + wg[3])
print(f"# {n} cases; worst loss/bound {worst_loss:.3f}; worst kernel/gate {worst_all[0]:.3f} at (kind, eps, weighted, pos_weight, B, C) = {worst_all[1]}")
