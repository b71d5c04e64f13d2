"""Worst errors of the classification meter per option combination, from measure_one_view() / measure_multiview() of
tests/test_gpu_eval_metrics.py (its cases, its references, its gates).  Needs the GPU.

    python scripts/eval_metrics_errors.py > profiles/eval_metrics_errors.txt
"""
import contextlib, io, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_eval_metrics as T
from eval_metrics_ref import MULTIVIEW, OPTION_IDS, OPTIONS, SHAPES

print("# ClassificationMeter.update (hyb_eval_metrics) on the MI355X against tests/eval_metrics_ref.py in float64 (CPU).")
print("# One view: (B,C) in", SHAPES, "x topk in {1, 2, C}; loss = sums[0] / sums[1], bound 1e-5 max(1,|ref|); counts, confusion and pred equal exactly.")
print(f"{'options':>9} | {'cases':>5} {'loss err':>10} {'loss/bound':>10} {'worst (B,C)':>12}")
for name, opt in zip(OPTION_IDS, OPTIONS):
    with contextlib.redirect_stdout(io.StringIO()):
        rows = T.measure_one_view(opt)
    B, C, err, bound = max(rows, key=lambda r: r[2] / r[3])
    print(f"{name:>9} | {len(rows):5d} {max(r[2] for r in rows):10.3e} {err / bound:10.4f} {str((B, C)):>12}")
print("# Several views: scores against the float64 mean softmax (tolerance 4 * 2^-23 = %.3e); loss gate 4 |l32 - l64| + 1e-6 max(1,|l64|)," % T.SCORE_TOL)
print("# l32 = the same formula in fp32 torch on the CPU (the arbiter); left out = videos whose integer results hang on a relative gap < 1e-4.")
print(f"{'options':>9} {'(B,V,C)':>12} | {'score err':>10} {'score/tol':>9} | {'loss err':>10} {'arbiter':>10} {'loss/gate':>9} | {'left out':>8}")
for name, opt in ((OPTION_IDS[0], OPTIONS[0]), (OPTION_IDS[-1], OPTIONS[-1])):
    for shape in MULTIVIEW:
        with contextlib.redirect_stdout(io.StringIO()):
            serr, lerr, gate, arb, left = T.measure_multiview(shape, opt)
        print(f"{name:>9} {str(shape):>12} | {serr:10.3e} {serr / T.SCORE_TOL:9.3f} | {lerr:10.3e} {arb:10.3e} {lerr / gate:9.4f} | {left:8d}")
