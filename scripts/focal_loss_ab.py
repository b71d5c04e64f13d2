"""What the focal and the asymmetric loss cost per replayed step, what fusing them saves, and whether the plain step moved: BASELINE
config 2, bf16, one GPU, graph.GraphedTrainStep.

Legs, each measured in a fresh child process (its own import of the package, its own capture, its own time limit), alternated ROUNDS
times; a child warms up, then puts device events around REPLAYS replays:
  parent-plain    HybridCrossEntropyLoss() with a class-index target, from the tree given by --parent (a built checkout of the parent commit)
  plain           the same from this tree
  focal           this tree, HybridFocalLoss(gamma=2) on class indices (hybrid::temporal_ce_focal)
  asym            this tree, HybridAsymmetricLoss() (gamma_neg 4, gamma_pos 0, clip 0.05) on a multi-hot fp32 [B, C] target (hybrid::temporal_ce_asym)
  focal-unfused   this tree, the same formula in eager torch behind forward_temporal (TorchFocal below), captured as the launches it makes
  asym-unfused    this tree, TorchAsymmetric below, likewise

    python scripts/focal_loss_ab.py [--parent DIR] [--replays 700] [--rounds 3]                      (part 1 of profiles/focal_loss_ab.txt)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/focal_loss_ab.py --worker focal --replays 50
                                     (kernels per step; likewise --worker plain / asym: profiles/focal_loss_kernel_stats_*.csv;
                                      --classes 64 puts the tail at its widest: part 3 of profiles/focal_loss_ab.txt)
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR = 1e-12          # (a vanishing rate: the step's cost does not depend on it)
CFG2 = dict(batch=8, frames=16, size=224, d_model=512, num_heads=8, hidden_dim=2048)        # bench.py CONFIGS[2]
LEGS = ("plain", "focal", "asym", "focal-unfused", "asym-unfused")
GAMMA, GAMMA_NEG, GAMMA_POS, CLIP = 2.0, 4.0, 0.0, 0.05


def torch_criteria():
    import torch

    class TorchFocal(torch.nn.Module):
        """mean_b (1 - p_y)^gamma (-log p_y), the usual eager recipe."""

        def forward(self, logits, y):
            logp = torch.log_softmax(logits, 1).gather(1, y[:, None])[:, 0]
            return ((1.0 - logp.exp()) ** GAMMA * -logp).mean()

    class TorchAsymmetric(torch.nn.Module):
        """The published asymmetric loss (logs clamped at 1e-8), divided by B C."""

        def forward(self, logits, t):
            p = torch.sigmoid(logits)
            q = (1.0 - p + CLIP).clamp(max=1.0)
            loss = t * torch.log(p.clamp(min=1e-8)) + (1.0 - t) * torch.log(q.clamp(min=1e-8))
            loss = loss * torch.pow(1.0 - p * t - q * (1.0 - t), GAMMA_POS * t + GAMMA_NEG * (1.0 - t))
            return -loss.mean()
    return TorchFocal(), TorchAsymmetric()


def worker(leg, root, replays, classes=8):
    """One window of one leg in this process -> a JSON line {leg, us_per_step, last_loss}."""
    sys.path.insert(0, root)
    import torch
    import transformer_cnn_hybrid_network_for_video_processing_amd as P
    assert os.path.realpath(os.path.dirname(os.path.dirname(P.__file__))) == os.path.realpath(root)
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = P.TransformerCNNHybrid(cnn_channels=(32, 64, 128, 256), d_model=CFG2["d_model"], num_heads=CFG2["num_heads"], num_layers=2,
                                   hidden_dim=CFG2["hidden_dim"], num_classes=classes, dropout=0.0, compute_dtype="bf16").to(dev).train()
    g = torch.Generator(device="cpu").manual_seed(1000)
    x = torch.rand(CFG2["batch"], CFG2["frames"], 3, CFG2["size"], CFG2["size"], generator=g).to(dev)
    y = torch.randint(0, classes, (CFG2["batch"],), generator=g)
    t = (torch.rand(CFG2["batch"], classes, generator=g) < 0.3).float()
    torch_focal, torch_asym = torch_criteria()
    if leg == "plain":
        crit, y = P.HybridCrossEntropyLoss(), y.to(dev)
    elif leg.startswith("focal"):
        crit, y = (P.HybridFocalLoss(gamma=GAMMA) if leg == "focal" else torch_focal), y.to(dev)
    else:
        crit = P.HybridAsymmetricLoss(gamma_neg=GAMMA_NEG, gamma_pos=GAMMA_POS, clip=CLIP) if leg == "asym" else torch_asym
        y = t.contiguous().to(dev)
    tr = P.GraphedTrainStep(model, crit, P.HybridAdamW(model.parameters(), lr=LR), x, y)
    assert tr._fused_loss == (not leg.endswith("unfused"))
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
    ap.add_argument("--worker", default=None, help="(internal) measure this one leg in this process: " + " | ".join(LEGS))
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (leg parent-plain)")
    ap.add_argument("--replays", type=int, default=700)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--classes", type=int, default=8, help="(with --worker) the number of classes, up to 64")
    ap.add_argument("--timeout", type=int, default=120, help="time limit of one child, seconds")
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, os.path.abspath(args.root), args.replays, args.classes)
    legs = ([("parent-plain", "plain", os.path.abspath(args.parent))] if args.parent else []) + [(n, n, ROOT) for n in LEGS]
    times, losses = {n: [] for n, _, _ in legs}, {}
    for _ in range(args.rounds):
        for name, leg, root in legs:
            # (a child that fails or runs into its limit ends the whole measurement: check=True / TimeoutExpired; the parent's tree runs its
            # own copy of the plain leg, which scripts/dense_loss_ab.py there provides)
            script = os.path.abspath(__file__) if root == ROOT else os.path.join(root, "scripts", "dense_loss_ab.py")
            r = subprocess.run([sys.executable, script, "--worker", leg, "--root", root, "--replays", str(args.replays)],
                               stdout=subprocess.PIPE, check=True, timeout=args.timeout, cwd=root)
            out = json.loads(r.stdout.decode().strip().splitlines()[-1])
            times[name].append(out["us_per_step"])
            losses[name] = out["last_loss"]
    print("Step time with the focal / asymmetric loss: BASELINE config 2, bf16, one MI355X, graph.GraphedTrainStep, us per step; every figure is a fresh")
    print(f"process (capture, 50 warm-up replays, device events around {args.replays} replays), legs alternated over {args.rounds} rounds (scripts/focal_loss_ab.py)")
    for name, v in times.items():
        mean = sum(v) / len(v)
        print(f"  {name:<14} " + " / ".join(f"{t:.2f}" for t in v) + f"   mean {mean:.1f}, min-to-max {max(v) - min(v):.2f}   (last loss {losses[name]:.6f})")
    m = {n: sum(v) / len(v) for n, v in times.items()}
    if "parent-plain" in m:
        print(f"  plain - parent-plain = {m['plain'] - m['parent-plain']:+.2f} us")
    for k in ("focal", "asym"):
        print(f"  {k} - plain = {m[k] - m['plain']:+.2f} us;  {k} - {k}-unfused = {m[k] - m[k + '-unfused']:+.2f} us")


if __name__ == "__main__":
    main()
