"""What gradient accumulation costs per replayed micro-step, fused into the optimizer launches against the unfused alternative, and whether
the default step moved: BASELINE config 2, bf16, one GPU, graph.GraphedTrainStep.

Legs, each measured in a fresh child process (its own import of the package, its own capture) under a time limit of its own, alternated
ROUNDS times; a child warms up, then puts device events around REPLAYS replays (= micro-steps).  The first abnormal exit of a child ends
the script.
  parent   (a) HybridAdamW(lr) from the tree given by --parent (a built checkout of the parent commit)
  k1       (b) the same from this tree: accumulation_steps = 1, the plain launch (hyb_adamw_step)
  k4       (c) this tree, GraphedTrainStep(accumulation_steps=4): three replays ending in hyb_grad_accumulate, the fourth in
               hyb_adamw_step_dev_acc
  unfused  (d) this tree, the same two graphs with torch._foreach_add_ into the accumulators on all four micro-steps, on the fourth
               torch._foreach_mul_(1 / 4), the plain device AdamW launch (hyb_adamw_step_dev) on the scaled sum and torch._foreach_zero_

    python scripts/accum_ab.py [--parent DIR] [--replays 600] [--rounds 3] [--out profiles/accum_ab.txt]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR = 1e-12          # (a vanishing rate: the step's cost does not depend on it)
K = 4
CFG2 = dict(batch=8, frames=16, size=224, d_model=512, num_heads=8, hidden_dim=2048)        # bench.py CONFIGS[2]
# bytes per parameter element: plain AdamW (p, m, v in and out + g in); the accumulate launch (acc in and out + g in); the accumulated
# AdamW launch (+ acc in and out); unfused: add (3) on every micro-step, then mul (2) + AdamW (7) + zero (1) on the k-th
BYTES = {"adamw": 7 * 4, "accumulate": 3 * 4, "adamw_acc": 9 * 4, "unfused_update": (3 + 2 + 7 + 1) * 4}


def worker(leg, root, replays):
    """One window of one leg in this process -> a JSON line {leg, us_per_micro_step, last_loss}."""
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
    kw = {}
    if leg == "k4":
        opt = P.HybridAdamW(params, lr=LR)
        kw = dict(accumulation_steps=K, warmup=K)
    elif leg == "unfused":
        class Unfused(P.HybridAdamW):
            """Accumulation as passes of their own around the plain device AdamW launch, captured into the same two graphs."""
            sums = [torch.zeros_like(p) for p in params]

            def accumulate(self):
                torch._foreach_add_(self.sums, [p.grad for p in params])

            def step(self, closure=None):
                grads = [p.grad for p in params]
                torch._foreach_add_(self.sums, grads)
                torch._foreach_mul_(self.sums, 1.0 / K)
                for p, s in zip(params, self.sums):
                    p.grad = s
                self._accum_k = 1                      # the plain device path (set_dynamic_hyper): hyb_adamw_step_dev on the scaled sum
                try:
                    loss = super().step(closure)
                finally:
                    self._accum_k = K
                    for p, gr in zip(params, grads):
                        p.grad = gr
                torch._foreach_zero_(self.sums)
                return loss
        opt = Unfused(params, lr=LR)
        opt.set_dynamic_hyper(True)
        kw = dict(accumulation_steps=K, warmup=K)
    else:
        opt = P.HybridAdamW(params, lr=LR)
    tr = P.GraphedTrainStep(model, P.HybridCrossEntropyLoss(), opt, x, y, **kw)
    assert tr._fused_loss and tr.gs is not None
    assert replays % K == 0
    for _ in range(52):
        tr.step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        tr.step()
    e1.record()
    torch.cuda.synchronize()
    res = {"leg": leg, "us_per_micro_step": e0.elapsed_time(e1) * 1e3 / replays, "last_loss": float(tr.loss.item()),
           "param_elements": sum(p.numel() for p in params)}
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
    ap.add_argument("--worker", default=None, help="(internal) measure this one leg in this process: k1 | k4 | unfused")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (leg parent)")
    ap.add_argument("--replays", type=int, default=600)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=150, help="time limit of one child process, seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accum_ab.txt"))
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, os.path.abspath(args.root), args.replays)
    legs = ([("parent", "k1", os.path.abspath(args.parent))] if args.parent else []) + [("k1", "k1", ROOT), ("k4", "k4", ROOT), ("unfused", "unfused", ROOT)]
    times, losses, elements = {n: [] for n, _, _ in legs}, {}, 0
    for _ in range(args.rounds):
        for name, leg, root in legs:
            out = child(leg, root, args.replays, args.limit)
            times[name].append(out["us_per_micro_step"])
            losses[name] = out["last_loss"]
            elements = out.get("param_elements", elements)
    lines = ["Gradient accumulation in the replayed training step: BASELINE config 2, bf16, one MI355X, graph.GraphedTrainStep, us per MICRO-step (one",
             f"forward + backward of 8 clips); every figure is a fresh process (capture, 52 warm-up replays, device events around {args.replays} replays), legs",
             f"alternated over {args.rounds} rounds (scripts/accum_ab.py).  parent / k1: no accumulation, every replay ends in AdamW; k4: accumulation_steps = {K},",
             "fused (hyb_grad_accumulate x 3, then hyb_adamw_step_dev_acc); unfused: _foreach_add_ x 4, _foreach_mul_, hyb_adamw_step_dev, _foreach_zero_."]
    for name, v in times.items():
        mean = sum(v) / len(v)
        lines.append(f"  {name:<8} " + " / ".join(f"{t:.2f}" for t in v) + f"   mean {mean:.1f}, min-to-max {max(v) - min(v):.2f}   (last loss {losses[name]:.6f})")
    m = {n: sum(v) / len(v) for n, v in times.items()}
    spread = {n: max(v) - min(v) for n, v in times.items()}
    if "parent" in m:
        diff = m["k1"] - m["parent"]
        lines.append(f"  k1 - parent = {diff:+.2f} us   (the legs' own min-to-max: parent {spread['parent']:.2f}, k1 {spread['k1']:.2f}: "
                     + ("inside it" if abs(diff) <= max(spread["parent"], spread["k1"]) else "OUTSIDE it") + ")")
    base = "parent" if "parent" in m else "k1"
    lines.append(f"  k4: {m['k4']:.1f} us per micro-step, {K * m['k4']:.1f} us per optimizer step of {K} micro-batches; per micro-step - {base} = {m['k4'] - m[base]:+.2f} us")
    lines.append(f"  unfused: {m['unfused']:.1f} us per micro-step, {K * m['unfused']:.1f} us per optimizer step; k4 - unfused = {m['k4'] - m['unfused']:+.2f} us per micro-step, "
                 f"{K * (m['k4'] - m['unfused']):+.2f} us per optimizer step")
    mb = lambda b: elements * b / 1e6
    fused = ((K - 1) * BYTES["accumulate"] + BYTES["adamw_acc"]) / K
    unfused = ((K - 1) * BYTES["accumulate"] + BYTES["unfused_update"]) / K
    lines.append(f"  byte estimate, {elements} parameter elements, optimizer-side traffic per micro-step: plain AdamW {mb(BYTES['adamw']):.1f} MB; k4 fused "
                 f"({K - 1} x {BYTES['accumulate']} + {BYTES['adamw_acc']}) / {K} = {fused:.1f} B per element, {mb(fused):.1f} MB; unfused "
                 f"({K - 1} x {BYTES['accumulate']} + {BYTES['unfused_update']}) / {K} = {unfused:.1f} B per element, {mb(unfused):.1f} MB")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
