"""HybridLAMB against the fp64 rule (tests/lamb_ref.py) on the tensors, groups and steps of tests/test_gpu_lamb.py::test_against_fp64: per
family (p, exp_avg, exp_avg_sq) the worst error / gate over tensors and steps, gate = 4 max|x32 - x64| + steps 2^-23 max|x64| with x32 the
rule restated in torch float32 on the CPU; and the worst relative error of the norms and ratios (gate 1e-5).  One line per family and
always_adapt, with the tensor and step of the worst case.

    python scripts/lamb_errors.py [--out profiles/lamb_errors.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lamb_errors.txt"))
    args = ap.parse_args()
    import torch
    import test_gpu_lamb as T
    from test_gpu_param_groups import _bind, _params
    lines = ["HybridLAMB against the fp64 rule (scripts/lamb_errors.py): the eight tensors and three groups of tests/test_gpu_lamb.py, five steps at",
             "max_grad_norm = 1.  error / gate, gate = 4 max|x32 - x64| + steps 2^-23 max|x64| (x32: the rule in torch float32 on the CPU); the worst",
             "case over tensors and steps, with the fp32 restatement's own error there in units of 2^-23 max|x64|.  Norms and ratios: worst relative",
             "error against fp64, gate 1e-5."]
    for always_adapt in (False, True):
        init, grads, ref = T._references(always_adapt)
        ps = _params(init)
        opt = T._lamb(ps, always_adapt=always_adapt, max_grad_norm=1.0)
        worst = {name: (0.0, None) for name in ("p", "exp_avg", "exp_avg_sq")}
        trust_worst = [0.0, 0.0, 0.0]
        for s in range(T.STEPS):
            _bind(ps, [g.cuda() for g in grads[s]])
            opt.step()
            snap, trust64 = ref[s]
            for i, p in enumerate(ps):
                st = opt.state[p]
                for j, (name, x) in enumerate((("p", p.detach()), ("exp_avg", st["exp_avg"]), ("exp_avg_sq", st["exp_avg_sq"]))):
                    r32, r64 = snap[torch.float32][j][i].double().flatten(), snap[torch.float64][j][i].flatten()
                    err, yard, big = (x.double().cpu().flatten() - r64).abs().max().item(), (r32 - r64).abs().max().item(), r64.abs().max().item()
                    ratio = err / (4 * yard + (s + 1) * 2.0 ** -23 * big)
                    if ratio > worst[name][0]:
                        worst[name] = (ratio, f"tensor {i} ({r64.numel()} elements), step {s + 1}: error {err:.3e}, fp32 restatement {yard / (2.0 ** -23 * big):.2f} x 2^-23 max|x64|")
            want = torch.tensor(trust64, dtype=torch.float64)
            rel = ((T._trust(opt, ps).double() - want).abs() / want.abs()).max(dim=0).values.tolist()
            trust_worst = [max(a, b) for a, b in zip(trust_worst, rel)]
        for name, (ratio, where) in worst.items():
            lines.append(f"  always_adapt={always_adapt!s:<5} {name:<10} error / gate {ratio:.3f}   {where}" + ("   ABOVE ONE HALF" if ratio > 0.5 else ""))
        lines.append(f"  always_adapt={always_adapt!s:<5} |p|, |u|, r  worst relative error {trust_worst[0]:.2e}, {trust_worst[1]:.2e}, {trust_worst[2]:.2e}   (gate 1e-5)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
