"""Loss errors of the two meters under the focal, soft-target and asymmetric criteria, from the measure_*() functions of
tests/test_gpu_eval_loss.py (its cases, its references, its gates): every case's error and bound, and the arbiter's error with several
views.  Needs the GPU.

    python scripts/eval_loss_errors.py [--out profiles/eval_loss_errors.txt]
"""
import contextlib, io, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_eval_loss as T
import eval_metrics_ref as EM
import multilabel_ref as ML
from dense_ref import EPS
from focal_ref import ASYM_CONFIGS, FOCAL_GAMMAS

out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "eval_loss_errors.txt")
lines, worst = [], {}


def quiet(fn, *args):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*args)


def note(family, ratio):
    worst[family] = max(worst.get(family, 0.0), ratio)


def one_view(family, label, rows):
    for B, C, err, bound in rows:
        lines.append(f"{family:>10} {label:<34} {str((B, C)):>10} | {err:10.3e} {bound:10.3e} {err / bound:9.4f}")
        note(family + ", one view", err / bound)


def views(family, label, shape, res):
    err, gate, arb = res
    lines.append(f"{family:>10} {label:<34} {str(shape):>12} | {err:10.3e} {gate:10.3e} {err / gate:9.4f} {arb:10.3e}")
    note(family + ", several views", err / gate)


lines.append("# ClassificationMeter / MultiLabelMeter under HybridFocalLoss, soft targets and HybridAsymmetricLoss on the MI355X against")
lines.append("# tests/eval_loss_ref.py in float64 (CPU).  Counts, confusion / cells, pred, scores and the bank equal a meter without the criterion bit for bit.")
lines.append("# One view: the criterion's own device function; bound 1e-5 max(1, |l64|).")
lines.append(f"{'family':>10} {'options':<34} {'(B,C)':>10} | {'loss err':>10} {'bound':>10} {'err/bound':>9}")
for gamma in FOCAL_GAMMAS:
    for weighted in (False, True):
        one_view("focal", f"gamma={gamma} weighted={weighted}", quiet(T.measure_focal_one_view, gamma, weighted))
one_view("focal", "gamma=2.0 weighted=True ignore=1", quiet(T.measure_focal_one_view, 2.0, True, 1))
for cfg in ASYM_CONFIGS:
    for name, opt in zip(ML.OPTION_IDS, ML.OPTIONS):
        one_view("asymmetric", f"{cfg} {name}", quiet(T.measure_asym_one_view, cfg, opt))
for eps in EPS:
    for weighted in (False, True):
        one_view("soft", f"eps={eps} weighted={weighted}", quiet(T.measure_soft_one_view, eps, weighted))
lines.append("# Several views: gate 4 |l32 - l64| + 1e-6 max(1, |l64|), l32 = the same formula in fp32 torch on the CPU (the arbiter).")
lines.append(f"{'family':>10} {'options':<34} {'(B,V,C)':>12} | {'loss err':>10} {'gate':>10} {'err/gate':>9} {'arbiter':>10}")
for shape in EM.MULTIVIEW:
    for gamma in FOCAL_GAMMAS:
        for opt in ((False, None), (True, 1)):
            views("focal", f"gamma={gamma} weighted={opt[0]} ignore={opt[1]}", shape, quiet(T.measure_focal_views, shape, gamma, opt))
    for eps in EPS:
        for weighted in (False, True):
            views("soft", f"eps={eps} weighted={weighted}", shape, quiet(T.measure_soft_views, shape, eps, weighted))
for shape in ML.MULTIVIEW:
    for cfg in ASYM_CONFIGS:
        for name, opt in ((ML.OPTION_IDS[0], ML.OPTIONS[0]), (ML.OPTION_IDS[-1], ML.OPTIONS[-1])):
            views("asymmetric", f"{cfg} {name}", shape, quiet(T.measure_asym_views, shape, cfg, opt))
lines.append("# Worst error over its bound, per family:")
for family in sorted(worst):
    lines.append(f"#   {family:<28} {worst[family]:.4f}")
text = "\n".join(lines) + "\n"
print(text, end="")
with open(out, "w") as f:
    f.write(text)
