"""HybridSGD / HybridLARS against the fp64 rule (tests/sgd_ref.py) on the tensors, groups, cases and steps of
tests/test_gpu_sgd.py::test_against_fp64: per case and family (p, momentum_buffer, ema) the worst error / gate over tensors and steps,
gate = 4 max|x32 - x64| + steps 2^-23 max|x64| with x32 the rule restated in torch float32 on the CPU; and for the LARS cases the worst
relative error of the norms and ratios (gate 1e-5).  One line per case and family, with the tensor and step of the worst case.

    python scripts/sgd_errors.py [--out profiles/sgd_errors.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sgd_errors.txt"))
    args = ap.parse_args()
    import torch
    import test_gpu_sgd as T
    from sgd_ref import check_trust, gate
    from test_gpu_param_groups import _bind, _params
    lines = ["HybridSGD and HybridLARS against the fp64 rule (scripts/sgd_errors.py): the eight tensors and three groups of tests/test_gpu_sgd.py, five",
             "steps at max_grad_norm = 1 with the weight average.  error / gate, gate = 4 max|x32 - x64| + steps 2^-23 max|x64| (x32: the rule in torch",
             "float32 on the CPU); the worst case over tensors and steps.  Norms and ratios (LARS): worst relative error against fp64, gate 1e-5."]
    for case, (lars, kw, momenta, damp) in T.CASES.items():
        init, grads, ref = T._references(case)
        ps = _params(init)
        opt = T._make(lars, ps, momenta=momenta, dampening=damp, max_grad_norm=1.0, ema_decay=0.9, **kw)
        worst = {name: (0.0, None) for name in ("p", "momentum_buffer", "ema")}
        trust_worst = 0.0
        for s in range(T.STEPS):
            _bind(ps, [g.cuda() for g in grads[s]])
            opt.step()
            snap, trust64 = ref[s]
            for i, p in enumerate(ps):
                st = opt.state[p]
                for j, (name, x) in enumerate((("p", p.detach()), ("momentum_buffer", st["momentum_buffer"]), ("ema", st["ema"]))):
                    err, bound = gate(name, i, s + 1, x, snap[torch.float32][j][i], snap[torch.float64][j][i], verbose=False)
                    if err / bound > worst[name][0]:
                        worst[name] = (err / bound, f"tensor {i} ({x.numel()} elements), step {s + 1}: error {err:.3e}, gate {bound:.3e}")
            if lars:
                trust_worst = max(trust_worst, check_trust(T._trust(opt, ps), trust64, case, verbose=False))
        for name, (ratio, where) in worst.items():
            lines.append(f"  {case:<18} {name:<16} error / gate {ratio:.3f}   {where}" + ("   ABOVE ONE HALF" if ratio > 0.5 else ""))
        if lars:
            lines.append(f"  {case:<18} |p|, |G|, r      worst relative error {trust_worst:.2e}   (gate 1e-5)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
