"""What a MixTarget costs per replayed step, and whether the plain step moved: BASELINE config 2, bf16, one GPU, graph.GraphedTrainStep.

Legs, each measured in a fresh child process (its own import of the package, its own capture), alternated ROUNDS times; a child warms up,
then puts device events around REPLAYS replays:
  parent-plain  HybridCrossEntropyLoss() with a class-index target, from the tree given by --parent (a built checkout of the parent commit)
  plain         the same from this tree
  mix           this tree, y = MixTarget(y_a, y_b, lam) with per-clip lam, an exact 1 and an exact 0 (hybrid::temporal_ce_mix: the same
                launches, both targets and lam read in them)

    python scripts/mix_ab.py [--parent DIR] [--replays 700] [--rounds 3]                                  (part 1 of profiles/mix_ab.txt)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/mix_ab.py --worker mix --replays 50
                                                        (kernels per step; likewise --worker plain: part 3, profiles/mix_kernel_stats_*.csv)
profiles/mix_ab.txt holds this script's output, bench.py pairs of the two trees and the summary of the two kernel tables.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR = 1e-12          # (a vanishing rate: the step's cost does not depend on it)
CFG2 = dict(batch=8, frames=16, size=224, d_model=512, num_heads=8, hidden_dim=2048)        # bench.py CONFIGS[2]


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
    y = torch.randint(0, 8, (CFG2["batch"],), generator=g)
    if leg == "mix":
        lam = torch.rand(CFG2["batch"], generator=g)
        lam[1], lam[2] = 1.0, 0.0
        y = P.MixTarget(y.to(dev), y[torch.randperm(CFG2["batch"], generator=g)].to(dev), lam.to(dev))
    else:
        y = y.to(dev)
    tr = P.GraphedTrainStep(model, P.HybridCrossEntropyLoss(), P.HybridAdamW(model.parameters(), lr=LR), x, y)
    assert tr._fused_loss
    for _ in range(50):
        tr.step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        tr.step()
    e1.record()
    torch.cuda.synchronize()
    res = {"leg": leg, "us_per_step": e0.elapsed_time(e1) * 1e3 / replays, "last_loss": float(tr.loss.item())}
    tr.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", default=None, help="(internal) measure this one leg in this process: plain | mix")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (leg parent-plain)")
    ap.add_argument("--replays", type=int, default=700)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, os.path.abspath(args.root), args.replays)
    legs = ([("parent-plain", "plain", os.path.abspath(args.parent))] if args.parent else []) + [("plain", "plain", ROOT), ("mix", "mix", ROOT)]
    times, losses = {n: [] for n, _, _ in legs}, {}
    for _ in range(args.rounds):
        for name, leg, root in legs:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", leg, "--root", root, "--replays", str(args.replays)],
                               stdout=subprocess.PIPE, check=True, timeout=600, cwd=root)
            out = json.loads(r.stdout.decode().strip().splitlines()[-1])
            times[name].append(out["us_per_step"])
            losses[name] = out["last_loss"]
    print("Step time with a MixTarget: BASELINE config 2, bf16, one MI355X, graph.GraphedTrainStep, us per step; every figure is a fresh process")
    print(f"(capture, 50 warm-up replays, device events around {args.replays} replays), legs alternated over {args.rounds} rounds (scripts/mix_ab.py)")
    for name, v in times.items():
        mean = sum(v) / len(v)
        print(f"  {name:<13} " + " / ".join(f"{t:.2f}" for t in v) + f"   mean {mean:.1f}, min-to-max {max(v) - min(v):.2f}   (last loss {losses[name]:.6f})")
    m = {n: sum(v) / len(v) for n, v in times.items()}
    if "parent-plain" in m:
        print(f"  plain - parent-plain = {m['plain'] - m['parent-plain']:+.2f} us")
    print(f"  mix - plain = {m['mix'] - m['plain']:+.2f} us")


if __name__ == "__main__":
    main()
