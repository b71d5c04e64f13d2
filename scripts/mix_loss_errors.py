"""Worst loss / gradient errors of the criterion with a MixTarget per option combination, from measure() of tests/test_gpu_mix_loss.py (its
grid, its reference, its gates).  Needs the GPU.

    python scripts/mix_loss_errors.py > profiles/mix_loss_errors.txt
"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import test_gpu_mix_loss as T

print("# HybridCrossEntropyLoss(weight, ignore_index, label_smoothing)(logits, MixTarget(y_a, y_b, lam)) on the MI355X against tests/mix_ref.py")
print("# in float64 (CPU), dloss = 1.5; grid of tests/test_gpu_mix_loss.py: (B,C) in", T.SHAPES, "per-clip lam with an exact 1 and an exact 0")
print("# per option combination, worst over the six shapes: loss error / its bound 1e-5 max(1,|ref|); gradient error, the arbiter's")
print("# (the same definition in fp32 on the CPU against the same reference), and gradient error / gate (gate = 4 * arbiter + 1e-6 * max|g_ref|)")
print(f"{'eps':>4} {'weighted':>8} {'ignore':>7} | {'loss err':>10} {'loss/bound':>10} | {'grad err':>10} {'arbiter':>10} {'kernel/gate':>11} {'worst (B,C)':>12}")
worst_all = (0, None)
worst_loss = 0.0
n = 0
for eps in T.EPS:
    for use_w in (False, True):
        for ign in T.IGNORE:
            wl = wlr = 0.0; wg = (-1, 0, 0, None)
            for B, C in T.SHAPES:
                lerr, lb, gerr, gb, arb = T.measure(B, C, eps, use_w, ign)
                n += 1
                wl = max(wl, lerr); wlr = max(wlr, lerr / lb)
                if gerr / gb > wg[0]:
                    wg = (gerr / gb, gerr, arb, (B, C))
            worst_loss = max(worst_loss, wlr)
            print(f"{eps:>4} {str(use_w):>8} {str(ign):>7} | {wl:10.3e} {wlr:10.3f} | {wg[1]:10.3e} {wg[2]:10.3e} {wg[0]:11.3f} {str(wg[3]):>12}")
            if wg[0] > worst_all[0]:
                worst_all = (wg[0], (eps, use_w, ign) + wg[3])
print(f"# {n} cases; worst loss/bound {worst_loss:.3f}; worst kernel/gate {worst_all[0]:.3f} at (eps, weighted, ignore, B, C) = {worst_all[1]}")
