"""Worst loss / gradient errors of HybridFocalLoss and HybridAsymmetricLoss per option combination, from measure_focal() / measure_asym() of
tests/test_gpu_focal_loss.py (its grid, its reference, its gates).  Needs the GPU.

    python scripts/focal_loss_errors.py > profiles/focal_loss_errors.txt
"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import test_gpu_focal_loss as T

print("# HybridFocalLoss(gamma, weight)(logits, y) and HybridAsymmetricLoss(gamma_neg, gamma_pos, clip, weight, pos_weight)(logits, t) on the")
print("# MI355X against tests/focal_ref.py in float64 (CPU), dloss = 1.5; grid of tests/test_gpu_focal_loss.py: (B,C) in")
print("#", T.SHAPES, "plus (4, 1) for the asymmetric loss, whose logits hold +100 (target 0) and -100 (target 1)")
print("# per combination, worst over the shapes: loss error / its bound 1e-5 max(1,|ref|); gradient error, the arbiter's (the same definition")
print("# in fp32 on the CPU against the same reference), and gradient error / gate (gate = 4 * arbiter + 1e-6 * max|g_ref|)")
print(f"{'loss':>5} {'gamma / (gp, gn, clip)':>22} {'weighted':>8} {'pos_w':>6} | {'loss err':>10} {'loss/bound':>10} | {'grad err':>10} {'arbiter':>10} {'kernel/gate':>11} {'worst (B,C)':>12}")
combos = [("focal", g, use_w, False) for g in T.FOCAL_GAMMAS for use_w in (False, True)]
combos += [("asym", cfg, use_w, use_pw) for cfg in T.ASYM_CONFIGS for use_w in (False, True) for use_pw in (False, True)]
worst_all = (0, None)
worst_loss = (0.0, None)
n = 0
for which, cfg, use_w, use_pw in combos:
    wl = wlr = 0.0; wg = (-1, 0, 0, None)
    for B, C in (T.BCE_SHAPES if which == "asym" else T.SHAPES):
        lerr, lb, gerr, gb, arb = T.measure_asym(B, C, cfg, use_w, use_pw) if which == "asym" else T.measure_focal(B, C, cfg, use_w)
        n += 1
        wl = max(wl, lerr); wlr = max(wlr, lerr / lb)
        if gerr / gb > wg[0]:
            wg = (gerr / gb, gerr, arb, (B, C))
    if wlr > worst_loss[0]:
        worst_loss = (wlr, (which, cfg, use_w, use_pw))
    print(f"{which:>5} {str(cfg):>22} {str(use_w):>8} {str(use_pw):>6} | {wl:10.3e} {wlr:10.3f} | {wg[1]:10.3e} {wg[2]:10.3e} {wg[0]:11.3f} {str(wg[3]):>12}")
    if wg[0] > worst_all[0]:
        worst_all = (wg[0], (which, cfg, use_w, use_pw) + wg[3])
print(f"# {n} cases; worst loss/bound {worst_loss[0]:.3f} at {worst_loss[1]}; worst kernel/gate {worst_all[0]:.3f} at (loss, exponents, weighted, pos_weight, B, C) = {worst_all[1]}")
