"""Worst errors of the multi-label meter per option combination, from measure_one_view() / measure_multiview() of
tests/test_gpu_multilabel.py (its cases, its references, its gates).  Needs the GPU.

    python scripts/multilabel_errors.py > profiles/multilabel_errors.txt
"""
import contextlib, io, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_multilabel as T
from multilabel_ref import MULTIVIEW, OPTION_IDS, OPTIONS, SCORE_TOL, SHAPES, THRESHOLDS

print("# MultiLabelMeter.update (hyb_eval_multilabel) on the MI355X against tests/multilabel_ref.py in float64 (CPU).")
print("# One view: (B,C) in", SHAPES, "x thresholds", [round(t, 3) for t in THRESHOLDS], "; scores against the float64 sigmoid (tolerance 4 * 2^-23 =")
print("# %.3e), loss = sums[0] / (B C) with the bound 1e-5 max(1,|ref|); counts, cells and pred equal the reference's exactly in every case." % SCORE_TOL)
print(f"{'options':>10} | {'cases':>5} {'score err':>10} {'score/tol':>9} | {'loss err':>10} {'loss/bound':>10} {'worst (B,C)':>12}")
for name, opt in zip(OPTION_IDS, OPTIONS):
    with contextlib.redirect_stdout(io.StringIO()):
        rows = T.measure_one_view(opt, T._check_integers)
    B, C, _, _, err, bound = max(rows, key=lambda r: r[4] / r[5])
    serr = max(r[3] for r in rows)
    print(f"{name:>10} | {len(rows):5d} {serr:10.3e} {serr / SCORE_TOL:9.3f} | {max(r[4] for r in rows):10.3e} {err / bound:10.4f} {str((B, C)):>12}")
print("# Several views: scores against the float64 mean sigmoid (tolerance (V + 3) 2^-23); loss bound = that score error through the logarithm's")
print("# slope, sum_bc w_c max(pw_c t, 1 - t) (V + 3) 2^-23 / min(s, 1 - s) / (B C) + 1e-6 max(1,|l64|); integer results exact; the worse threshold shown.")
print(f"{'options':>10} {'(B,V,C)':>12} | {'score err':>10} {'score/tol':>9} | {'loss err':>10} {'bound':>10} {'loss/bound':>10}")
for name, opt in zip(OPTION_IDS, OPTIONS):
    for shape in MULTIVIEW:
        with contextlib.redirect_stdout(io.StringIO()):
            serr, tol, lerr, bound = T.measure_multiview(shape, opt, T._check_integers)
        print(f"{name:>10} {str(shape):>12} | {serr:10.3e} {serr / tol:9.3f} | {lerr:10.3e} {bound:10.3e} {lerr / bound:10.4f}")
