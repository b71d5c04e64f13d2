"""What HybridAdamW's non-finite guard (skip_nonfinite=True) costs per replayed training step, and whether the default step moved: BASELINE
config 2, bf16, one GPU, graph.GraphedTrainStep.

Legs, each measured in a fresh child process (its own import of the package, its own capture) under a time limit of its own, alternated
ROUNDS times; a child warms up, then puts device events around REPLAYS replays.  The first abnormal exit of a child ends the script.
  parent      (a) HybridAdamW(lr) from the tree given by --parent (a built checkout of the parent commit)
  off         (b) the same from this tree: the guard off, the plain launch (hyb_adamw_step)
  guard       (c) this tree, skip_nonfinite=True without clipping: the two norm launches run for the decision (hyb_grad_norm_guard), then
                  hyb_adamw_step_dev_guard
  clip        (d) this tree, max_grad_norm alone: hyb_grad_norm, hyb_adamw_step_dev
  clip_guard  (e) this tree, max_grad_norm with the guard: the same number of launches as (d), the guarded entry points

    python scripts/guard_ab.py [--parent DIR] [--replays 600] [--rounds 3] [--out profiles/guard_ab.txt]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR = 1e-12          # (a vanishing rate: the step's cost does not depend on it)
CLIP = 1.0
CFG2 = dict(batch=8, frames=16, size=224, d_model=512, num_heads=8, hidden_dim=2048)        # bench.py CONFIGS[2]
LEG_KW = {"off": {}, "guard": dict(skip_nonfinite=True), "clip": dict(max_grad_norm=CLIP), "clip_guard": dict(max_grad_norm=CLIP, skip_nonfinite=True)}


def worker(leg, root, replays):
    """One window of one leg in this process -> a JSON line {leg, us_per_step, last_loss, skipped}."""
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
    opt = P.HybridAdamW(list(model.parameters()), lr=LR, **LEG_KW[leg])
    tr = P.GraphedTrainStep(model, P.HybridCrossEntropyLoss(), opt, x, y)
    assert tr._fused_loss and tr.gs is not None
    for _ in range(52):
        tr.step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        tr.step()
    e1.record()
    torch.cuda.synchronize()
    res = {"leg": leg, "us_per_step": e0.elapsed_time(e1) * 1e3 / replays, "last_loss": float(tr.loss.item()),
           "skipped": int(tr.skipped_steps.item()) if "skip_nonfinite" in LEG_KW[leg] else None}
    tr.close()
    print(json.dumps(res))


def child(leg, root, replays, limit):
    """Run one leg as a fresh process under `timeout`; an abnormal exit (a fault, an abort, the time limit) ends the whole script."""
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--worker", leg, "--root", root, "--replays", str(replays)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, cwd=root)
    if r.returncode != 0:
        sys.exit(f"leg {leg} ({root}) ended with exit status {r.returncode}: stopping here, nothing more is started on the GPU")
    return json.loads([l for l in r.stdout.decode().strip().splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", default=None, help="(internal) measure this one leg in this process: off | guard | clip | clip_guard")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (leg parent)")
    ap.add_argument("--replays", type=int, default=600)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=150, help="time limit of one child process, seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guard_ab.txt"))
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, os.path.abspath(args.root), args.replays)
    legs = ([("parent", "off", os.path.abspath(args.parent))] if args.parent else []) + [(n, n, ROOT) for n in LEG_KW]
    times, losses, skipped = {n: [] for n, _, _ in legs}, {}, {}
    for _ in range(args.rounds):
        for name, leg, root in legs:
            out = child(leg, root, args.replays, args.limit)
            times[name].append(out["us_per_step"])
            losses[name], skipped[name] = out["last_loss"], out["skipped"]
    lines = ["The non-finite guard in the replayed training step: BASELINE config 2, bf16, one MI355X, graph.GraphedTrainStep, us per step (forward +",
             f"backward + optimizer of 8 clips); every figure is a fresh process (capture, 52 warm-up replays, device events around {args.replays} replays), legs",
             f"alternated over {args.rounds} rounds (scripts/guard_ab.py).  parent / off: hyb_adamw_step; guard: skip_nonfinite=True (hyb_grad_norm_guard +",
             f"hyb_adamw_step_dev_guard); clip: max_grad_norm={CLIP} (hyb_grad_norm + hyb_adamw_step_dev); clip_guard: both (the guarded entry points)."]
    for name, v in times.items():
        mean = sum(v) / len(v)
        lines.append(f"  {name:<11} " + " / ".join(f"{t:.2f}" for t in v) + f"   mean {mean:.1f}, min-to-max {max(v) - min(v):.2f}   (last loss {losses[name]:.6f}"
                     + ("" if skipped[name] is None else f", skipped steps {skipped[name]}") + ")")
    m = {n: sum(v) / len(v) for n, v in times.items()}
    spread = {n: max(v) - min(v) for n, v in times.items()}

    def against(a, b):
        diff = m[a] - m[b]
        return (f"  {a} - {b} = {diff:+.2f} us   (the legs' own min-to-max: {b} {spread[b]:.2f}, {a} {spread[a]:.2f}: "
                + ("inside it" if abs(diff) <= max(spread[a], spread[b]) else "OUTSIDE it") + ")")
    if "parent" in m:
        lines.append(against("off", "parent"))
    lines.append(against("clip_guard", "clip"))
    lines.append(against("guard", "off"))
    lines.append(against("clip", "off"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
