"""What the loss options cost per replayed step: BASELINE config 2, bf16, one GPU, graph.GraphedTrainStep.

Legs, alternated ROUNDS times in one process after a warm-up of both, device events around REPLAYS replays each (a window of a second or
more at the default):
  plain  HybridCrossEntropyLoss()                                        (hybrid::temporal_ce, the benchmarked step)
  opts   HybridCrossEntropyLoss(weight, ignore_index, label_smoothing)   (hybrid::temporal_ce_opts: the same launches, the options ride in them)

    python scripts/loss_options_ab.py [--replays 800] [--rounds 4] [--legs plain,opts] [--out profiles/loss_options_step.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/loss_options_ab.py --legs opts --rounds 1 --replays 50 --out ''     (kernels per step)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import transformer_cnn_hybrid_network_for_video_processing_amd as P  # noqa: E402

LR = 1e-12          # (a vanishing rate: the step's cost does not depend on it)
CFG2 = dict(batch=8, frames=16, size=224, d_model=512, num_heads=8, hidden_dim=2048)        # bench.py CONFIGS[2]


def make(dev):
    torch.manual_seed(0)
    model = P.TransformerCNNHybrid(cnn_channels=(32, 64, 128, 256), d_model=CFG2["d_model"], num_heads=CFG2["num_heads"], num_layers=2,
                                   hidden_dim=CFG2["hidden_dim"], num_classes=8, dropout=0.0, compute_dtype="bf16").to(dev).train()
    return model, P.HybridAdamW(model.parameters(), lr=LR)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=800)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--legs", default="plain,opts")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_options_step.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(1000)
    x = torch.rand(CFG2["batch"], CFG2["frames"], 3, CFG2["size"], CFG2["size"], generator=g).to(dev)
    y = torch.randint(0, 8, (CFG2["batch"],), generator=g).to(dev)
    w = torch.rand(8, generator=g) + 0.25
    w[1] = 0.0
    y[0], y[-1] = 0, 5                                                            # a kept clip whose class carries weight, an ignored clip
    crits = {"plain": P.HybridCrossEntropyLoss(), "opts": P.HybridCrossEntropyLoss(weight=w, ignore_index=5, label_smoothing=0.1).to(dev)}
    names = [k for k in args.legs.split(",") if k]
    legs = {}
    for name in names:
        m, o = make(dev)
        legs[name] = P.GraphedTrainStep(m, crits[name], o, x, y)
        assert legs[name]._fused_loss

    def run(name, n):
        for _ in range(n):
            legs[name].step()

    for name in names:                                                            # warm-up of every leg
        run(name, 50)
    torch.cuda.synchronize()
    times = {k: [] for k in names}
    for _ in range(args.rounds):
        for name in names:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(name, args.replays)
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / args.replays)
    res = {"workload": "BASELINE config 2, bf16, 1 GPU, graph.GraphedTrainStep", "replays_per_window": args.replays, "rounds": args.rounds,
           "unit": "us per step",
           "legs": {k: {"runs_us": [round(t, 2) for t in v], "mean_us": round(sum(v) / len(v), 2), "spread_us": round(max(v) - min(v), 2),
                        "window_s": round(sum(v) / len(v) * args.replays * 1e-6, 2), "last_loss": float(legs[k].loss.item())}
                    for k, v in times.items()}}
    if "plain" in times and "opts" in times:
        res["opts_minus_plain_us"] = round(res["legs"]["opts"]["mean_us"] - res["legs"]["plain"]["mean_us"], 2)
    for tr in legs.values():
        tr.close()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
