"""What HybridSGD and HybridLARS cost per replayed training step: BASELINE config 2, bf16, one GPU, graph.GraphedTrainStep, one parameter
group, clipping at max_grad_norm = 1 in every leg.

Legs, each measured in a fresh child process (its own import of the package, its own capture) under a time limit of its own, alternated
ROUNDS times; a child warms up, then puts device events around REPLAYS replays.  The first abnormal exit of a child ends the script (what
was measured until then is written out).
  parent   HybridAdamW(max_grad_norm=1) from the tree given by --parent (a built checkout of the parent commit)
  adamw    the same from this tree
  sgd      HybridSGD(momentum=0.9, nesterov=True): the norm call and hyb_sgd_step_dev
  lars     HybridLARS(momentum=0.9): the norm call, hyb_lars_trust (two launches), hyb_sgd_step_dev
  foreach  torch.nn.utils.clip_grad_norm_(foreach=True) and torch.optim.SGD(momentum=0.9, nesterov=True, foreach=True), captured behind
           the same forward and backward

--stats adds one rocprofv3 --kernel-trace --stats run each of the legs adamw, sgd and lars (50 replays, runs of their own): the optimizer's
kernels.

    python scripts/sgd_ab.py [--parent DIR] [--replays 300] [--rounds 3] [--stats] [--out profiles/sgd_ab.txt]
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
SGD = dict(momentum=0.9, weight_decay=1e-4)


def torch_sgd(P, torch):
    class TorchSGD(P.HybridAdamW):
        """clip_grad_norm_ and torch.optim.SGD(foreach=True) behind GraphedTrainStep's interface: what a user writes today to train with SGD
        inside the captured step (no host read in either; the momentum buffers are created by the eager warm-up steps)."""

        def __init__(self, params, lr):
            params = list(params)
            super().__init__(params, lr=lr)
            self._sgd = torch.optim.SGD(params, lr=lr, nesterov=True, foreach=True, **SGD)

        @torch.no_grad()
        def step(self, closure=None):
            ps = [p for p in self.param_groups[0]["params"] if p.grad is not None]
            torch.nn.utils.clip_grad_norm_(ps, 1.0, foreach=True)
            self._sgd.step()
            if self._advance:
                self._step_counter.add_(1)
    return TorchSGD


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
    if leg == "sgd":
        opt = P.HybridSGD(list(model.parameters()), lr=LR, nesterov=True, max_grad_norm=1.0, **SGD)
    elif leg == "lars":
        opt = P.HybridLARS(list(model.parameters()), lr=LR, max_grad_norm=1.0, **SGD)
    elif leg == "foreach":
        opt = torch_sgd(P, torch)(model.parameters(), lr=LR)
    else:
        opt = P.HybridAdamW(list(model.parameters()), lr=LR, eps=1e-6, weight_decay=1e-2, max_grad_norm=1.0)
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
    d = tempfile.mkdtemp(prefix="sgd_ab_")
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
    lines = ["HybridSGD and HybridLARS in the replayed training step: BASELINE config 2, bf16, one MI355X, graph.GraphedTrainStep, one parameter group,",
             "clipping at max_grad_norm = 1 in every leg, us per step (forward + backward + optimizer of 8 clips); every figure is a fresh process",
             f"(capture, {WARM} warm-up replays, device events around {args.replays} replays), legs alternated over {args.rounds} rounds (scripts/sgd_ab.py).",
             "parent / adamw: HybridAdamW of the parent commit / of this one; sgd: HybridSGD, Nesterov 0.9 (norm call + hyb_sgd_step_dev); lars:",
             "HybridLARS (norm call + hyb_lars_trust + hyb_sgd_step_dev); foreach: clip_grad_norm_ + torch.optim.SGD(foreach=True), captured behind",
             "the same forward and backward."]
    done = {n: v for n, v in times.items() if v}
    for name, v in done.items():
        lines.append(f"  {name:<8} " + " / ".join(f"{t:.2f}" for t in v) + f"   mean {sum(v) / len(v):.1f}, min-to-max {max(v) - min(v):.2f}   "
                     f"({info[name]['tensors']} tensors, {info[name]['parameters']} parameters, last loss {info[name]['last_loss']:.6f})")
    m = {n: sum(v) / len(v) for n, v in done.items()}
    spread = {n: max(v) - min(v) for n, v in done.items()}

    def against(a, b, what):
        if a not in m or b not in m:
            return None
        diff, ref = m[a] - m[b], max(spread[a], spread[b])
        return f"  {a} - {b} = {diff:+.2f} us   {what} (the two legs' own min-to-max: {ref:.2f}: " + ("inside it" if abs(diff) <= ref else "OUTSIDE it") + ")"
    for line in (against("adamw", "parent", "the AdamW step, this commit against its parent"),
                 against("sgd", "adamw", "the SGD step against the AdamW step"),
                 against("lars", "sgd", "what the trust ratios cost"),
                 against("foreach", "sgd", "what the fused form saves")):
        if line:
            lines.append(line)
    for leg, (steps, rows) in (stats or {}).items():
        total = sum(calls for _, calls, _ in rows)
        lines.append(f"  kernels, leg {leg} (rocprofv3 --kernel-trace --stats, a run of its own, {steps} steps): {total} launches in all = {total / steps:.1f} per step")
        for name, calls, avg in rows:
            short = name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
            if any(s in short for s in ("adamw", "sgd_dev", "lars", "grad_norm")):
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
    ap.add_argument("--worker", default=None, help="(internal) measure this one leg in this process: adamw | sgd | lars | foreach")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (leg parent)")
    ap.add_argument("--replays", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=150, help="time limit of one child process, seconds")
    ap.add_argument("--stats", action="store_true", help="also one rocprofv3 kernel-statistics run each of the legs adamw, sgd and lars")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sgd_ab.txt"))
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, os.path.abspath(args.root), args.replays)
    legs = ([("parent", "adamw", os.path.abspath(args.parent))] if args.parent else []) + [(n, n, ROOT) for n in ("adamw", "sgd", "lars", "foreach")]
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
    stats = {}
    if args.stats:
        for leg in ("adamw", "sgd", "lars"):
            rows = kernel_rows(leg, 50, args.limit + 150)
            if rows is None:
                print(report(args, times, info, stats, f"the kernel-statistics run of leg {leg} ended abnormally or left no file; nothing was run after it"), end="")
                sys.exit(1)
            stats[leg] = rows
    print(report(args, times, info, stats, None), end="")


if __name__ == "__main__":
    main()
