"""What the classification meter costs behind a replayed forward: BASELINE config 2, bf16, one GPU, microseconds per evaluated batch.

Legs, each measured in a fresh child process (its own import of the package, its own capture) under a time limit of its own, alternated
ROUNDS times; a child warms up, then puts device events around REPLAYS batches.  The first abnormal exit of a child ends the script.
  predict  graph.GraphedPredict alone: the forward as one graph launch, nothing evaluated
  eval     graph.GraphedEval: the same forward with the meter's update launch (hyb_eval_metrics) captured behind it
  eager    GraphedPredict followed by the eager torch equivalent on its logits -- F.cross_entropy (sum and weight sum kept on the device),
           argmax / eq / sum, topk / eq / any / sum, bincount into a confusion matrix -- accumulated in device tensors, with no host read
The criterion carries class weights, ignore_index and label smoothing in both evaluating legs; top-k is top-5.

    python scripts/eval_bench.py [--replays 500] [--rounds 3] [--out profiles/eval_bench.txt]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG2 = dict(batch=8, frames=16, size=224, d_model=512, num_heads=8, hidden_dim=2048)        # bench.py CONFIGS[2]
LEGS = ("predict", "eval", "eager")
IGNORE, SMOOTHING, TOPK, CLASSES = 1, 0.1, 5, 8


def worker(leg, replays):
    """One window of one leg in this process -> a JSON line {leg, us_per_batch, ...}."""
    sys.path.insert(0, ROOT)
    import torch
    import torch.nn.functional as F
    import transformer_cnn_hybrid_network_for_video_processing_amd as P
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = P.TransformerCNNHybrid(cnn_channels=(32, 64, 128, 256), d_model=CFG2["d_model"], num_heads=CFG2["num_heads"], num_layers=2,
                                   hidden_dim=CFG2["hidden_dim"], num_classes=CLASSES, dropout=0.0, compute_dtype="bf16").to(dev).eval()
    g = torch.Generator(device="cpu").manual_seed(1000)
    x = torch.rand(CFG2["batch"], CFG2["frames"], 3, CFG2["size"], CFG2["size"], generator=g).to(dev)
    y = torch.randint(0, CLASSES, (CFG2["batch"],), generator=g).to(dev)
    w = torch.linspace(0.5, 1.5, CLASSES)
    crit = P.HybridCrossEntropyLoss(weight=w, ignore_index=IGNORE, label_smoothing=SMOOTHING).to(dev)
    meter = P.ClassificationMeter(CLASSES, topk=TOPK, criterion=crit)
    extra = {}
    if leg == "eval":
        ge = P.GraphedEval(model, x, y, meter)
        run = lambda: ge(x, y)
    else:
        gp = P.GraphedPredict(model, x)
        if leg == "predict":
            run = lambda: gp(x)
        else:
            num, den = torch.zeros((), device=dev), torch.zeros((), device=dev)
            counts = torch.zeros(3, dtype=torch.int64, device=dev)
            conf = torch.zeros(CLASSES * CLASSES, dtype=torch.float64, device=dev)
            wd = w.to(dev)

            def run():
                logits = gp(x)
                keep = y != IGNORE
                num.add_(F.cross_entropy(logits, y, weight=wd, ignore_index=IGNORE, label_smoothing=SMOOTHING, reduction="sum"))
                den.add_((wd[y] * keep).sum())
                pred = logits.argmax(1)
                counts[0].add_(keep.sum())
                counts[1].add_(((pred == y) & keep).sum())
                counts[2].add_(((logits.topk(TOPK, dim=1).indices == y[:, None]).any(1) & keep).sum())
                # (no read in this script; bincount itself sizes its output from the largest index, which it fetches to the host)
                conf.add_(torch.bincount(y * CLASSES + pred, weights=keep.double(), minlength=CLASSES * CLASSES))
    for _ in range(30):
        run()
    torch.cuda.synchronize()
    meter.reset()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        run()
    e1.record()
    torch.cuda.synchronize()
    if leg == "eval":
        out = meter.compute()
        extra = {"loss": out["loss"], "top1": out["top1"], "videos": out["videos"]}
    elif leg == "eager":
        extra = {"loss": float(num / den), "top1": float(counts[1]) / max(1, int(counts[0]))}
    print(json.dumps({"leg": leg, "us_per_batch": e0.elapsed_time(e1) * 1e3 / replays, **extra}))


def child(leg, replays, limit):
    """Run one leg as a fresh process under `timeout`; an abnormal exit (a fault, an abort, the time limit) ends the whole script."""
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--worker", leg, "--replays", str(replays)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, cwd=ROOT)
    if r.returncode != 0:
        sys.exit(f"leg {leg} ended with exit status {r.returncode}: stopping here, nothing more is started on the GPU")
    return json.loads([l for l in r.stdout.decode().strip().splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", default=None, help="(internal) measure this one leg in this process: " + " | ".join(LEGS))
    ap.add_argument("--replays", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=120, help="time limit of one child process, seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_bench.txt"))
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, args.replays)
    times, last = {n: [] for n in LEGS}, {}
    for _ in range(args.rounds):
        for leg in LEGS:
            out = child(leg, args.replays, args.limit)
            times[leg].append(out["us_per_batch"])
            last[leg] = out
    lines = ["Evaluation behind a replayed forward: BASELINE config 2 (8 clips of 16 frames 224 x 224), bf16, one MI355X, us per evaluated batch; every",
             f"figure is a fresh process (capture, 30 warm-up batches, device events around {args.replays} batches), legs alternated over {args.rounds} rounds",
             "(scripts/eval_bench.py).  predict: GraphedPredict alone; eval: GraphedEval (the meter launch in the graph); eager: GraphedPredict + the torch",
             "equivalent (cross_entropy, argmax, topk, bincount) accumulated on the device, no host read."]
    for leg in LEGS:
        v = times[leg]
        note = "" if leg == "predict" else f"   (loss {last[leg]['loss']:.6f}, top-1 {last[leg]['top1']:.4f})"
        lines.append(f"  {leg:<8} " + " / ".join(f"{t:.2f}" for t in v) + f"   mean {sum(v) / len(v):.1f}, min-to-max {max(v) - min(v):.2f}" + note)
    m = {n: sum(v) / len(v) for n, v in times.items()}
    lines.append(f"  eval - predict = {m['eval'] - m['predict']:+.2f} us      eager - predict = {m['eager'] - m['predict']:+.2f} us      "
                 f"eval - eager = {m['eval'] - m['eager']:+.2f} us")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
