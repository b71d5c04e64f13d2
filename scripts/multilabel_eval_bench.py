"""What the multi-label meter costs behind a replayed forward: BASELINE config 2, bf16, one GPU, microseconds per evaluated batch.

Legs, each measured in a fresh child process (its own import of the package, its own capture) under a time limit of its own, alternated
ROUNDS times; a child warms up, then puts device events around REPLAYS batches.  The first abnormal exit of a child ends the script.
  predict     graph.GraphedPredict alone: the forward as one graph launch, nothing evaluated
  classify    graph.GraphedEval with a ClassificationMeter (hyb_eval_metrics behind the forward): the yardstick for one meter launch
  multilabel  graph.GraphedEval with a MultiLabelMeter (hyb_eval_multilabel behind the forward, scores and labels appended to the bank)
  eager       GraphedPredict followed by the eager torch equivalent on its logits -- sigmoid, F.binary_cross_entropy_with_logits (sum),
              compare / sum for tp / fp / fn and exact matches, a slice copy of scores and labels into a preallocated bank -- accumulated
              in device tensors, with no host read
8 classes; the BCE criterion carries weight and pos_weight in both multi-label legs; the bank holds every video of the run.

    python scripts/multilabel_eval_bench.py [--replays 500] [--rounds 3] [--out profiles/multilabel_eval_bench.txt]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG2 = dict(batch=8, frames=16, size=224, d_model=512, num_heads=8, hidden_dim=2048)        # bench.py CONFIGS[2]
LEGS = ("predict", "classify", "multilabel", "eager")
CLASSES, THRESHOLD, WARM = 8, 0.5, 30


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
    B = CFG2["batch"]
    x = torch.rand(B, CFG2["frames"], 3, CFG2["size"], CFG2["size"], generator=g).to(dev)
    y = torch.randint(0, CLASSES, (B,), generator=g).to(dev)
    t = (torch.rand(B, CLASSES, generator=g) < 0.35).float().to(dev)
    w, pw = torch.linspace(0.5, 1.5, CLASSES), torch.linspace(2.0, 1.0, CLASSES)
    capacity = B * replays                                   # the timed window fills it exactly (the meter is reset after the warm-up)
    extra, meter = {}, None
    if leg == "classify":
        meter = P.ClassificationMeter(CLASSES, topk=5, criterion=P.HybridCrossEntropyLoss(weight=w, ignore_index=1, label_smoothing=0.1).to(dev))
        ge = P.GraphedEval(model, x, y, meter)
        run = lambda: ge(x, y)
    elif leg == "multilabel":
        meter = P.MultiLabelMeter(CLASSES, threshold=THRESHOLD, criterion=P.HybridBCEWithLogitsLoss(weight=w, pos_weight=pw).to(dev), capacity=capacity)
        ge = P.GraphedEval(model, x, t, meter)
        run = lambda: ge(x, t)
    else:
        gp = P.GraphedPredict(model, x)
        if leg == "predict":
            run = lambda: gp(x)
        else:
            num = torch.zeros((), device=dev)
            cells = torch.zeros(3, CLASSES, dtype=torch.int64, device=dev)
            exact = torch.zeros((), dtype=torch.int64, device=dev)
            bank_s = torch.zeros(capacity + B * WARM, CLASSES, device=dev)
            bank_l = torch.zeros(capacity + B * WARM, CLASSES, dtype=torch.uint8, device=dev)
            wd, pwd, yb, row = w.to(dev), pw.to(dev), t >= 0.5, [0]

            def run():
                logits = gp(x)
                s = torch.sigmoid(logits)
                num.add_(F.binary_cross_entropy_with_logits(logits, t, weight=wd, pos_weight=pwd, reduction="sum"))
                pred = s >= THRESHOLD
                cells[0].add_((pred & yb).sum(0))
                cells[1].add_((pred & ~yb).sum(0))
                cells[2].add_((~pred & yb).sum(0))
                exact.add_((pred == yb).all(1).sum())
                r = row[0] % bank_s.shape[0]                  # the host keeps the cursor: the eager form's slice copy needs it
                bank_s[r:r + B].copy_(s)
                bank_l[r:r + B].copy_(yb)
                row[0] += B
    for _ in range(WARM):
        run()
    torch.cuda.synchronize()
    if meter is not None:
        meter.reset()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        run()
    e1.record()
    torch.cuda.synchronize()
    if leg == "classify":
        out = meter.compute()
        extra = {"loss": out["loss"], "videos": out["videos"]}
    elif leg == "multilabel":
        out = meter.compute()
        extra = {"loss": out["loss"], "videos": out["videos"], "stored": out["stored"], "dropped": out["dropped"], "micro_f1": out["micro_f1"],
                 "mAP": out["mAP"]}
    elif leg == "eager":
        tp, fp, fn = (float(v) for v in cells.sum(1))
        extra = {"loss": float(num) / ((WARM + replays) * B * CLASSES), "micro_f1": 2 * tp / (2 * tp + fp + fn)}
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multilabel_eval_bench.txt"))
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, args.replays)
    times, last = {n: [] for n in LEGS}, {}
    for _ in range(args.rounds):
        for leg in LEGS:
            out = child(leg, args.replays, args.limit)
            times[leg].append(out["us_per_batch"])
            last[leg] = out
    lines = ["Multi-label evaluation behind a replayed forward: BASELINE config 2 (8 clips of 16 frames 224 x 224), bf16, one MI355X, 8 classes, us per",
             f"evaluated batch; every figure is a fresh process (capture, {WARM} warm-up batches, device events around {args.replays} batches), legs alternated over",
             f"{args.rounds} rounds (scripts/multilabel_eval_bench.py).  predict: GraphedPredict alone; classify: GraphedEval + ClassificationMeter (the parent",
             "commit's meter launch); multilabel: GraphedEval + MultiLabelMeter with a bank for the whole run; eager: GraphedPredict + the torch equivalent",
             "(sigmoid, BCE-with-logits sum, compares and sums, slice copies into a bank) accumulated on the device, no host read."]
    for leg in LEGS:
        v = times[leg]
        o = last[leg]
        note = ""
        if leg == "classify":
            note = f"   (loss {o['loss']:.6f})"
        elif leg == "multilabel":
            note = f"   (loss {o['loss']:.6f}, micro-F1 {o['micro_f1']:.4f}, mAP {o['mAP']:.4f}, stored {o['stored']}, dropped {o['dropped']})"
        elif leg == "eager":
            note = f"   (loss {o['loss']:.6f}, micro-F1 {o['micro_f1']:.4f})"
        lines.append(f"  {leg:<10} " + " / ".join(f"{t:.2f}" for t in v) + f"   mean {sum(v) / len(v):.1f}, min-to-max {max(v) - min(v):.2f}" + note)
    m = {n: sum(v) / len(v) for n, v in times.items()}
    lines.append(f"  classify - predict = {m['classify'] - m['predict']:+.2f} us      multilabel - predict = {m['multilabel'] - m['predict']:+.2f} us      "
                 f"eager - predict = {m['eager'] - m['predict']:+.2f} us      multilabel - eager = {m['multilabel'] - m['eager']:+.2f} us")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
