"""What the weight average kept inside the AdamW launch costs per replayed step, against a separate pass over the weights, and whether the
default step moved: BASELINE config 2, bf16, one GPU, graph.GraphedTrainStep.

Legs, each measured in a fresh child process (its own import of the package, its own capture) under a time limit of its own, alternated
ROUNDS times; a child warms up, then puts device events around REPLAYS replays.  The first abnormal exit of a child ends the script.
  parent  HybridAdamW(lr) from the tree given by --parent (a built checkout of the parent commit)
  off     the same from this tree: no average, the plain launch (hyb_adamw_step)
  fused   this tree, HybridAdamW(lr, ema_decay=0.999): hyb_adamw_step_dev_ema, the average inside the AdamW launch
  lerp    this tree, no ema_decay; the optimizer's step() is followed by torch._foreach_lerp_(averages, parameters, 1 - 0.999), captured
          into the step graph with it (what a user could do before)
  dyn     (kernel statistics only) this tree, dynamic_hyper=True, no average: adamw_dev_kernel<false>, the launch `fused` extends

    python scripts/ema_ab.py [--parent DIR] [--replays 700] [--rounds 3] [--stats] [--out profiles/ema_ab.txt]
--stats adds one rocprofv3 --kernel-trace --stats run each of the legs dyn and fused (50 replays) and the adamw_dev_kernel rows of both.
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
DECAY = 0.999
CFG2 = dict(batch=8, frames=16, size=224, d_model=512, num_heads=8, hidden_dim=2048)        # bench.py CONFIGS[2]
PARAM_BYTES_PER_ELEMENT = (7 * 4, 9 * 4)                                                     # p, m, v in and out + g in; + e in and out


def worker(leg, root, replays):
    """One window of one leg in this process -> a JSON line {leg, us_per_step, last_loss}."""
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
    params = list(model.parameters())
    if leg == "fused":
        opt = P.HybridAdamW(params, lr=LR, ema_decay=DECAY)
    elif leg == "lerp":
        class WithLerp(P.HybridAdamW):
            """The average as a second pass: one multi-tensor lerp behind the AdamW launch, in the same captured step."""
            averages = [p.detach().clone() for p in params]

            def step(self, closure=None):
                loss = super().step(closure)
                torch._foreach_lerp_(self.averages, [p.detach() for p in params], 1.0 - DECAY)
                return loss
        opt = WithLerp(params, lr=LR)
    else:
        opt = P.HybridAdamW(params, lr=LR)
    tr = P.GraphedTrainStep(model, P.HybridCrossEntropyLoss(), opt, x, y, **({"dynamic_hyper": True} if leg == "dyn" else {}))
    assert tr._fused_loss and tr.gs is not None
    for _ in range(50):
        tr.step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        tr.step()
    e1.record()
    torch.cuda.synchronize()
    res = {"leg": leg, "us_per_step": e0.elapsed_time(e1) * 1e3 / replays, "last_loss": float(tr.loss.item()),
           "param_elements": sum(p.numel() for p in params)}
    tr.close()
    print(json.dumps(res))


def child(prefix, leg, root, replays, limit):
    """Run one leg as a fresh process under `timeout`; an abnormal exit (a fault, an abort, the time limit) ends the whole script."""
    cmd = ["timeout", "-k", "10", str(limit)] + prefix + [sys.executable, os.path.abspath(__file__), "--worker", leg, "--root", root,
                                                          "--replays", str(replays)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, cwd=root)
    if r.returncode != 0:
        sys.exit(f"leg {leg} ({root}) ended with exit status {r.returncode}: stopping here, nothing more is started on the GPU")
    return json.loads([l for l in r.stdout.decode().strip().splitlines() if l.startswith("{")][-1])


def kernel_rows(leg, replays, limit):
    """rocprofv3 kernel statistics of one leg (a run of its own) -> [(name, calls, average us)] of the adamw kernels."""
    d = tempfile.mkdtemp(prefix="ema_ab_")
    try:
        child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"], leg, ROOT, replays, limit)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            sys.exit(f"rocprofv3 left no kernel_stats.csv under {d}")
        rows = list(csv.DictReader(open(files[0])))
    finally:
        shutil.rmtree(d, ignore_errors=True)
    return [(r["Name"], int(r["Calls"]), float(r["AverageNs"]) / 1e3) for r in rows if "adamw" in r["Name"]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", default=None, help="(internal) measure this one leg in this process: off | fused | lerp | dyn")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (leg parent)")
    ap.add_argument("--replays", type=int, default=700)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=150, help="time limit of one child process, seconds")
    ap.add_argument("--stats", action="store_true", help="also one rocprofv3 kernel-statistics run each of the legs dyn and fused")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_ab.txt"))
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, os.path.abspath(args.root), args.replays)
    legs = ([("parent", "off", os.path.abspath(args.parent))] if args.parent else []) + [("off", "off", ROOT), ("fused", "fused", ROOT), ("lerp", "lerp", ROOT)]
    times, losses, elements = {n: [] for n, _, _ in legs}, {}, 0
    for _ in range(args.rounds):
        for name, leg, root in legs:
            out = child([], leg, root, args.replays, args.limit)
            times[name].append(out["us_per_step"])
            losses[name] = out["last_loss"]
            elements = out.get("param_elements", elements)
    lines = ["Weight average (EMA) in the replayed training step: BASELINE config 2, bf16, one MI355X, graph.GraphedTrainStep, us per step; every figure",
             f"is a fresh process (capture, 50 warm-up replays, device events around {args.replays} replays), legs alternated over {args.rounds} rounds",
             "(scripts/ema_ab.py).  parent / off: no average; fused: ema_decay inside the AdamW launch; lerp: torch._foreach_lerp_ captured behind AdamW."]
    for name, v in times.items():
        mean = sum(v) / len(v)
        lines.append(f"  {name:<7} " + " / ".join(f"{t:.2f}" for t in v) + f"   mean {mean:.1f}, min-to-max {max(v) - min(v):.2f}   (last loss {losses[name]:.6f})")
    m = {n: sum(v) / len(v) for n, v in times.items()}
    spread = {n: max(v) - min(v) for n, v in times.items()}
    if "parent" in m:
        diff = m["off"] - m["parent"]
        lines.append(f"  off - parent = {diff:+.2f} us   (the legs' own min-to-max: parent {spread['parent']:.2f}, off {spread['off']:.2f}: "
                     + ("inside it" if abs(diff) <= max(spread["parent"], spread["off"]) else "OUTSIDE it") + ")")
    lines.append(f"  fused - off = {m['fused'] - m['off']:+.2f} us      lerp - off = {m['lerp'] - m['off']:+.2f} us      fused - lerp = {m['fused'] - m['lerp']:+.2f} us")
    lines.append(f"  byte estimate: {elements} parameter elements, {PARAM_BYTES_PER_ELEMENT[0]} -> {PARAM_BYTES_PER_ELEMENT[1]} bytes each in the AdamW launch "
                 f"({elements * PARAM_BYTES_PER_ELEMENT[0] / 1e6:.1f} -> {elements * PARAM_BYTES_PER_ELEMENT[1] / 1e6:.1f} MB): 9/7 of the launch's time, see the kernel rows")
    if args.stats:
        dev = {}
        for leg in ("dyn", "fused"):
            for name, calls, avg in kernel_rows(leg, 50, args.limit + 150):
                short = name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
                lines.append(f"  kernels, leg {leg:<5} (rocprofv3 --kernel-trace --stats, a run of its own): {short:<24} calls {calls:4d}  avg {avg:6.2f} us")
                if short.startswith("adamw_dev_kernel"):
                    dev[leg] = avg
        if len(dev) == 2:
            lines.append(f"  adamw_dev_kernel with the average - without = {dev['fused'] - dev['dyn']:+.2f} us ({dev['fused'] / dev['dyn']:.3f} x; "
                         f"9/7 of {dev['dyn']:.2f} us would be {dev['dyn'] * 9 / 7:.2f} us, {dev['dyn'] * 2 / 7:+.2f})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
