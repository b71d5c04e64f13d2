"""What HybridLAMB costs per replayed training step: BASELINE config 2, bf16, one GPU, graph.GraphedTrainStep, one parameter group, clipping
at max_grad_norm = 1 in every leg.

Legs, each measured in a fresh child process (its own import of the package, its own capture) under a time limit of its own, alternated
ROUNDS times; a child warms up, then puts device events around REPLAYS replays.  The first abnormal exit of a child ends the script (what
was measured until then is written out).
  parent   HybridAdamW(max_grad_norm=1) from the tree given by --parent (a built checkout of the parent commit)
  adamw    the same from this tree
  lamb     HybridLAMB: the norm call, hyb_lamb_trust (two launches), hyb_lamb_step_dev
  foreach  the same rule written with torch._foreach_* ops (ForeachLAMB below: norms per tensor, no host read), captured behind the same step

--stats adds one rocprofv3 --kernel-trace --stats run of the leg lamb (50 replays, a run of its own): the optimizer's kernels.

    python scripts/lamb_ab.py [--parent DIR] [--replays 300] [--rounds 3] [--stats] [--out profiles/lamb_ab.txt]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR = 1e-12          # (a vanishing rate: the step's cost does not depend on it)
WARM = 52           # replays before the timed window
CFG2 = dict(batch=8, frames=16, size=224, d_model=512, num_heads=8, hidden_dim=2048)        # bench.py CONFIGS[2]


def foreach_lamb(P, torch):
    class ForeachLAMB(P.HybridAdamW):
        """The rule of HybridLAMB (always_adapt=False) in torch._foreach_* ops on the device: what a user writes today to stay inside the
        captured step.  The step number comes from the device counter, so one capture serves every replay."""

        @torch.no_grad()
        def step(self, closure=None):
            group = self.param_groups[0]
            ps = [p for p in group["params"] if p.grad is not None]
            for p in ps:
                st = self.state[p]
                if "exp_avg" not in st:
                    st["step"], st["exp_avg"], st["exp_avg_sq"] = 0, torch.zeros_like(p), torch.zeros_like(p)
            gs = [p.grad for p in ps]
            ms, vs = [self.state[p]["exp_avg"] for p in ps], [self.state[p]["exp_avg_sq"] for p in ps]
            lr, (b1, b2), eps, wd = group["lr"], group["betas"], group["eps"], group["weight_decay"]
            t = (self._step_counter.reshape(()) + 1).double()
            bc1, inv_sqrt_bc2 = (1.0 - torch.pow(b1, t)).float(), torch.rsqrt(1.0 - torch.pow(b2, t)).float()
            total = torch.linalg.vector_norm(torch.stack(torch._foreach_norm(gs)))
            coef = torch.clamp(group["max_grad_norm"] / (total + 1e-6), max=1.0)
            gs = torch._foreach_mul(gs, coef)
            torch._foreach_lerp_(ms, gs, 1.0 - b1)
            torch._foreach_mul_(vs, b2)
            torch._foreach_addcmul_(vs, gs, gs, value=1.0 - b2)
            den = torch._foreach_sqrt(vs)
            torch._foreach_mul_(den, inv_sqrt_bc2)
            torch._foreach_add_(den, eps)
            u = torch._foreach_div(ms, den)
            torch._foreach_div_(u, bc1)
            torch._foreach_add_(u, ps, alpha=wd)
            w_norm, u_norm = torch.stack(torch._foreach_norm(ps)), torch.stack(torch._foreach_norm(u))
            ok = (w_norm > 0) & (u_norm > 0) if wd != 0 else torch.zeros_like(w_norm, dtype=torch.bool)
            rate = torch.where(ok, w_norm / u_norm, torch.ones_like(w_norm)) * lr
            torch._foreach_mul_(u, list(rate.unbind(0)))
            torch._foreach_sub_(ps, u)
            if self._advance:
                self._step_counter.add_(1)
    return ForeachLAMB


def worker(leg, root, replays):
    """One window of one leg in this process -> a JSON line {leg, us_per_step, last_loss, steps}."""
    sys.path.insert(0, root)
    import torch
    import transformer_cnn_hybrid_network_for_video_processing_amd as P
    assert os.path.realpath(os.path.dirname(os.path.dirname(P.__file__))) == os.path.realpath(root)
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = P.TransformerCNNHybrid(cnn_channels=(32, 64, 128, 256), d_model=CFG2["d_model"], num_heads=CFG2["num_heads"], num_layers=2,
                                   hidden_dim=CFG2["hidden_dim"], num_classes=8, dropout=0.0, compute_dtype="bf16").to(dev).train()
    g = torch.Generator(device="cpu").manual_seed(1000)
    x = torch.rand(CFG2["batch"], CFG2["frames"], 3, CFG2["size"], CFG2["size"], generator=g).to(dev)
    y = torch.randint(0, 8, (CFG2["batch"],), generator=g).to(dev)
    kw = dict(lr=LR, eps=1e-6, weight_decay=1e-2, max_grad_norm=1.0)
    if leg == "lamb":
        opt = P.HybridLAMB(list(model.parameters()), **kw)
    elif leg == "foreach":
        opt = foreach_lamb(P, torch)(list(model.parameters()), **kw)
    else:
        opt = P.HybridAdamW(list(model.parameters()), **kw)
    tr = P.GraphedTrainStep(model, P.HybridCrossEntropyLoss(), opt, x, y)
    assert tr._fused_loss and tr.gs is not None and tr._advancing
    for _ in range(WARM):
        tr.step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        tr.step()
    e1.record()
    torch.cuda.synchronize()
    steps = tr._warm_steps + WARM + replays
    assert int(tr.counter.item()) == steps
    res = {"leg": leg, "us_per_step": e0.elapsed_time(e1) * 1e3 / replays, "last_loss": float(tr.loss.item()), "steps": steps,
           "tensors": sum(1 for _ in model.parameters()), "parameters": sum(p.numel() for p in model.parameters())}
    tr.close()
    print(json.dumps(res))


def child(prefix, leg, root, replays, limit):
    """Run one leg as a fresh process under `timeout` -> its JSON line, or None after an abnormal exit (a fault, an abort, the time limit)."""
    cmd = ["timeout", "-k", "10", str(limit)] + prefix + [sys.executable, os.path.abspath(__file__), "--worker", leg, "--root", root,
                                                          "--replays", str(replays)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, cwd=root)
    if r.returncode != 0:
        print(f"leg {leg} ({root}) ended with exit status {r.returncode}: stopping here, nothing more is started on the GPU", file=sys.stderr)
        return None
    return json.loads([l for l in r.stdout.decode().strip().splitlines() if l.startswith("{")][-1])


def kernel_rows(leg, replays, limit):
    """rocprofv3 kernel statistics of one leg (a run of its own) -> (steps taken, [(name, calls, average us)] of all kernels), or None."""
    d = tempfile.mkdtemp(prefix="lamb_ab_")
    try:
        out = child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"], leg, ROOT, replays, limit)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if out is None or not files:
            return None
        rows = list(csv.DictReader(open(files[0])))
    finally:
        shutil.rmtree(d, ignore_errors=True)
    return out["steps"], [(r["Name"], int(r["Calls"]), float(r["AverageNs"]) / 1e3) for r in rows]


def report(args, times, info, stats, ended):
    lines = ["HybridLAMB in the replayed training step: BASELINE config 2, bf16, one MI355X, graph.GraphedTrainStep, one parameter group, clipping at",
             "max_grad_norm = 1 in every leg, us per step (forward + backward + optimizer of 8 clips); every figure is a fresh process (capture,",
             f"{WARM} warm-up replays, device events around {args.replays} replays), legs alternated over {args.rounds} rounds (scripts/lamb_ab.py).",
             "parent / adamw: HybridAdamW of the parent commit / of this one; lamb: HybridLAMB (norm call + hyb_lamb_trust + hyb_lamb_step_dev);",
             "foreach: the same rule in torch._foreach_* ops with per-tensor norms, captured behind the same step."]
    done = {n: v for n, v in times.items() if v}
    for name, v in done.items():
        lines.append(f"  {name:<8} " + " / ".join(f"{t:.2f}" for t in v) + f"   mean {sum(v) / len(v):.1f}, min-to-max {max(v) - min(v):.2f}   "
                     f"({info[name]['tensors']} tensors, {info[name]['parameters']} parameters, last loss {info[name]['last_loss']:.6f})")
    m = {n: sum(v) / len(v) for n, v in done.items()}
    spread = {n: max(v) - min(v) for n, v in done.items()}
    widest = max(spread.values()) if spread else 0.0

    def against(a, b, what, outside_any=False):
        if a not in m or b not in m:
            return None
        diff = m[a] - m[b]
        ref = widest if outside_any else max(spread[a], spread[b])
        return (f"  {a} - {b} = {diff:+.2f} us   {what} ({'the widest min-to-max of any leg' if outside_any else 'the two legs own min-to-max'}: {ref:.2f}: "
                + ("inside it" if abs(diff) <= ref else "OUTSIDE it") + ")")
    for line in (against("adamw", "parent", "the AdamW step, this commit against its parent"),
                 against("lamb", "adamw", "what the trust ratios cost"),
                 against("foreach", "lamb", "what the fused form saves", outside_any=True)):
        if line:
            lines.append(line)
    if stats:
        steps, rows = stats
        total = sum(calls for _, calls, _ in rows)
        lines.append(f"  kernels, leg lamb (rocprofv3 --kernel-trace --stats, a run of its own, {steps} steps): {total} launches in all = {total / steps:.1f} per step")
        for name, calls, avg in rows:
            short = name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
            if any(s in short for s in ("adamw", "lamb", "grad_norm")):
                lines.append(f"      {short[:88]:<88} calls {calls:5d} = {calls / steps:5.2f} per step  avg {avg:6.2f} us")
    if ended:
        lines.append(f"  INCOMPLETE: {ended}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return text


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", default=None, help="(internal) measure this one leg in this process: adamw | lamb | foreach")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (leg parent)")
    ap.add_argument("--replays", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=150, help="time limit of one child process, seconds")
    ap.add_argument("--stats", action="store_true", help="also one rocprofv3 kernel-statistics run of the leg lamb")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lamb_ab.txt"))
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, os.path.abspath(args.root), args.replays)
    legs = ([("parent", "adamw", os.path.abspath(args.parent))] if args.parent else []) + [(n, n, ROOT) for n in ("adamw", "lamb", "foreach")]
    times, info = {n: [] for n, _, _ in legs}, {}
    for rnd in range(args.rounds):
        for name, leg, root in legs:
            out = child([], leg, root, args.replays, args.limit)
            if out is None:
                print(report(args, times, info, None, f"leg {name} ended abnormally in round {rnd + 1}; nothing was run after it"), end="")
                sys.exit(1)
            times[name].append(out["us_per_step"])
            info[name] = out
            print(f"{name}: {out['us_per_step']:.2f} us per step", file=sys.stderr, flush=True)
        report(args, times, info, None, f"{rnd + 1} of {args.rounds} rounds" if rnd + 1 < args.rounds else None)
    stats = None
    if args.stats:
        stats = kernel_rows("lamb", 50, args.limit + 150)
        if stats is None:
            print(report(args, times, info, None, "the kernel-statistics run ended abnormally or left no file"), end="")
            sys.exit(1)
    print(report(args, times, info, stats, None), end="")


if __name__ == "__main__":
    main()
