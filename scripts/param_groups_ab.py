"""What parameter groups cost per replayed training step, and what serving them all from one AdamW launch (HybridAdamW merge_groups) saves:
BASELINE config 2, bf16, one GPU, graph.GraphedTrainStep(dynamic_hyper=True) with a scheduler that moves every group's rate before every replay.

Legs, each measured in a fresh child process (its own import of the package, its own capture) under a time limit of its own, alternated
ROUNDS times; a child warms up, then puts device events around REPLAYS replays (scheduler step included).  The first abnormal exit of a
child ends the script.
  parent  (a) one group, HybridAdamW(model.parameters()), from the tree given by --parent (a built checkout of the parent commit)
  one     (b) the same from this tree: hyb_adamw_hyper_set + hyb_adamw_step_dev, as ever
  merged  (c) this tree, model.param_groups(layer_decay=0.75): 16 groups, one hyb_adamw_hyper_set_groups + one hyb_adamw_step_dev_groups
  split   (d) the same groups with merge_groups=False: 16 uploads, 16 AdamW launches and a counter launch -- what the parent would do with them

--stats adds one rocprofv3 --kernel-trace --stats run each of the legs one, merged and split (50 replays): the optimizer's kernels and the
number of launches per step.

    python scripts/param_groups_ab.py [--parent DIR] [--replays 600] [--rounds 3] [--stats] [--out profiles/param_groups_ab.txt]
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
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR = 1e-12          # (a vanishing rate: the step's cost does not depend on it)
LAYER_DECAY = 0.75
WARM = 52           # replays before the timed window
CFG2 = dict(batch=8, frames=16, size=224, d_model=512, num_heads=8, hidden_dim=2048)        # bench.py CONFIGS[2]


def worker(leg, root, replays):
    """One window of one leg in this process -> a JSON line {leg, us_per_step, last_loss, groups, advancing}."""
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
    if leg == "one":
        opt = P.HybridAdamW(list(model.parameters()), lr=LR)
    else:
        opt = P.HybridAdamW(model.param_groups(lr=LR, layer_decay=LAYER_DECAY), merge_groups=leg == "merged")
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda e: 1.0 / (1.0 + 1e-3 * e))          # a new rate for every group before every replay
    tr = P.GraphedTrainStep(model, P.HybridCrossEntropyLoss(), opt, x, y, dynamic_hyper=True)
    assert tr._fused_loss and tr.gs is not None

    def steps(n):
        with warnings.catch_warnings():                   # a replay is not an optimizer.step() call torch's scheduler could count
            warnings.simplefilter("ignore")
            for _ in range(n):
                tr.step()
                sched.step()
    steps(WARM)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    steps(replays)
    e1.record()
    torch.cuda.synchronize()
    res = {"leg": leg, "us_per_step": e0.elapsed_time(e1) * 1e3 / replays, "last_loss": float(tr.loss.item()), "groups": len(opt.param_groups),
           "advancing": bool(tr._advancing), "steps": tr._warm_steps + WARM + replays}
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
    """rocprofv3 kernel statistics of one leg (a run of its own) -> (steps taken, [(name, calls, average us)] of all kernels)."""
    d = tempfile.mkdtemp(prefix="param_groups_ab_")
    try:
        out = child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"], leg, ROOT, replays, limit)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            sys.exit(f"rocprofv3 left no kernel_stats.csv under {d}")
        rows = list(csv.DictReader(open(files[0])))
    finally:
        shutil.rmtree(d, ignore_errors=True)
    return out["steps"], [(r["Name"], int(r["Calls"]), float(r["AverageNs"]) / 1e3) for r in rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", default=None, help="(internal) measure this one leg in this process: one | merged | split")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (leg parent)")
    ap.add_argument("--replays", type=int, default=600)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=150, help="time limit of one child process, seconds")
    ap.add_argument("--stats", action="store_true", help="also one rocprofv3 kernel-statistics run each of the legs one, merged and split")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "param_groups_ab.txt"))
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, os.path.abspath(args.root), args.replays)
    legs = ([("parent", "one", os.path.abspath(args.parent))] if args.parent else []) + [(n, n, ROOT) for n in ("one", "merged", "split")]
    times, info = {n: [] for n, _, _ in legs}, {}
    for _ in range(args.rounds):
        for name, leg, root in legs:
            out = child([], leg, root, args.replays, args.limit)
            times[name].append(out["us_per_step"])
            info[name] = out
            print(f"{name}: {out['us_per_step']:.2f} us per step", file=sys.stderr, flush=True)
    lines = ["Parameter groups in the replayed training step: BASELINE config 2, bf16, one MI355X, graph.GraphedTrainStep(dynamic_hyper=True) with a",
             "LambdaLR that moves every group's rate before every replay, us per step (forward + backward + optimizer of 8 clips, upload and",
             f"scheduler step included); every figure is a fresh process (capture, {WARM} warm-up replays, device events around {args.replays} replays), legs",
             f"alternated over {args.rounds} rounds (scripts/param_groups_ab.py).  parent / one: one group; merged: model.param_groups(layer_decay={LAYER_DECAY}),",
             "one upload launch and one AdamW launch for all groups; split: the same groups with merge_groups=False, a launch per group."]
    for name, v in times.items():
        mean = sum(v) / len(v)
        lines.append(f"  {name:<7} " + " / ".join(f"{t:.2f}" for t in v) + f"   mean {mean:.1f}, min-to-max {max(v) - min(v):.2f}   ({info[name]['groups']} groups, "
                     f"the AdamW launch advances the counter: {info[name]['advancing']}, last loss {info[name]['last_loss']:.6f})")
    m = {n: sum(v) / len(v) for n, v in times.items()}
    spread = {n: max(v) - min(v) for n, v in times.items()}

    def against(a, b, what):
        diff = m[a] - m[b]
        return (f"  {a} - {b} = {diff:+.2f} us   {what} (the legs' own min-to-max: {b} {spread[b]:.2f}, {a} {spread[a]:.2f}: "
                + ("inside it" if abs(diff) <= max(spread[a], spread[b]) else "OUTSIDE it") + ")")
    if "parent" in m:
        lines.append(against("one", "parent", "the single-group step"))
    lines.append(against("merged", "one", "the price of the recipe"))
    lines.append(against("split", "merged", "what merging saves"))
    if args.stats:
        for leg in ("one", "merged", "split"):
            steps, rows = kernel_rows(leg, 50, args.limit + 150)
            total = sum(calls for _, calls, _ in rows)
            lines.append(f"  kernels, leg {leg:<6} (rocprofv3 --kernel-trace --stats, a run of its own, {steps} steps): {total} launches in all = {total / steps:.1f} per step")
            for name, calls, avg in rows:
                short = name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
                if any(s in short for s in ("adamw", "hyper_set", "ema_set")) or (calls >= steps and "elementwise" in short):
                    lines.append(f"      {short[:72]:<72} calls {calls:5d} = {calls / steps:5.2f} per step  avg {avg:6.2f} us")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
