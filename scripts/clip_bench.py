"""What gradient clipping and device-side hyper-parameters cost per replayed step: BASELINE config 2, bf16, one GPU, graph.GraphedTrainStep.

Legs, alternated ROUNDS times in one process, device events around REPLAYS replays each:
  a  the default step (no clipping, hyper-parameters by value in the captured AdamW launch)
  b  dynamic_hyper=True, a new learning rate before every step (one hyb_adamw_hyper_set launch per step + hyb_adamw_step_dev)
  c  b + max_grad_norm (hyb_grad_norm + the clip coefficient applied inside the AdamW launch)
  d  what one would write without it: a GraphedTrainStep whose piece C calls torch.nn.utils.clip_grad_norm_(params, c, foreach=True)
     before optimizer.step() (hyper-parameters by value, as a)
If torch's chain cannot be captured on this build, c and d are timed as EAGER steps instead and the JSON says so.

    python scripts/clip_bench.py [--replays 200] [--rounds 3] [--legs abcd] [--out profiles/clip_bench.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/clip_bench.py --legs c --rounds 1 --replays 50 --out ''     (the two kernels' times)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import transformer_cnn_hybrid_network_for_video_processing_amd as P  # noqa: E402

LR = 1e-12
CFG2 = dict(batch=8, frames=16, size=224, d_model=512, num_heads=8, hidden_dim=2048)        # bench.py CONFIGS[2]


def make(dev, **opt_kw):
    torch.manual_seed(0)
    model = P.TransformerCNNHybrid(cnn_channels=(32, 64, 128, 256), d_model=CFG2["d_model"], num_heads=CFG2["num_heads"], num_layers=2,
                                   hidden_dim=CFG2["hidden_dim"], num_classes=8, dropout=0.0, compute_dtype="bf16").to(dev).train()
    # (a vanishing rate: the step's cost does not depend on it, and over 1000+ steps on ONE batch any real rate fits it until the norm falls below
    # the threshold and clipping is no longer active)
    return model, P.HybridAdamW(model.parameters(), lr=LR, **opt_kw)


class TorchClipStep(P.GraphedTrainStep):
    """Leg d: torch's own clipping chain captured in front of the optimizer launch."""

    def __init__(self, *a, clip, **kw):
        self._clip = clip
        super().__init__(*a, **kw)

    def _piece_c(self):
        self.torch_norm = torch.nn.utils.clip_grad_norm_(self.t_params + self.b_params, self._clip, foreach=True)
        super()._piece_c()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--legs", default="abcd")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(1000)
    x = torch.rand(CFG2["batch"], CFG2["frames"], 3, CFG2["size"], CFG2["size"], generator=g).to(dev)
    y = torch.randint(0, 8, (CFG2["batch"],), generator=g).to(dev)
    crit = P.HybridCrossEntropyLoss()

    # the threshold: half of the first step's gradient norm, so that clipping is active
    m0, _ = make(dev)
    crit(m0(x), y).backward()
    clip = 0.5 * float(torch.linalg.vector_norm(torch.stack([p.grad.double().norm() for p in m0.parameters()])).item())
    nparam = sum(p.numel() for p in m0.parameters())
    del m0

    legs, notes = {}, {}
    if "a" in args.legs:
        m, o = make(dev)
        legs["a"] = (P.GraphedTrainStep(m, crit, o, x, y), o, False)
    if "b" in args.legs:
        m, o = make(dev)
        legs["b"] = (P.GraphedTrainStep(m, crit, o, x, y, dynamic_hyper=True), o, True)
    graphed_cd = True
    if "d" in args.legs:
        m, o = make(dev)
        try:
            legs["d"] = (TorchClipStep(m, crit, o, x, y, clip=clip), o, False)
        except Exception as e:                                                  # noqa: BLE001 (reported)
            graphed_cd = False
            notes["d"] = f"torch's clip_grad_norm_ chain could not be captured ({type(e).__name__}: {str(e)[:160]}); c and d timed as eager steps"
            torch.cuda.synchronize()
    if "c" in args.legs and graphed_cd:
        m, o = make(dev, max_grad_norm=clip)
        legs["c"] = (P.GraphedTrainStep(m, crit, o, x, y, dynamic_hyper=True), o, True)

    def eager_leg(torch_clip):
        m, o = make(dev, **({} if torch_clip else {"max_grad_norm": clip}))

        def step():
            o.zero_grad(set_to_none=True)
            loss = crit(m(x), y)
            loss.backward()
            if torch_clip:
                torch.nn.utils.clip_grad_norm_(m.parameters(), clip, foreach=True)
            o.step()
            return loss
        return step
    eager = {}
    if not graphed_cd:
        eager = {k: eager_leg(k == "d") for k in "cd" if k in args.legs}

    def run(name, n):
        if name in eager:
            for _ in range(n):
                eager[name]()
            return
        tr, o, moving = legs[name]
        for k in range(n):
            if moving:
                o.param_groups[0]["lr"] = LR * (1.0 + 1e-3 * ((k % 1000) + 1))       # a new rate every step: sync_hyper uploads every time
            tr.step()

    names = [k for k in "abcd" if k in legs or k in eager]
    for name in names:                                                         # warm-up of every leg
        run(name, 20)
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
    res = {"workload": "BASELINE config 2, bf16, 1 GPU, " + ("graph.GraphedTrainStep" if graphed_cd else "a/b graphed, c/d EAGER steps"),
           "replays_per_leg": args.replays, "rounds": args.rounds, "parameters": nparam, "max_grad_norm": clip, "unit": "us per step",
           "legs": {k: {"runs_us": [round(t, 2) for t in v], "mean_us": round(sum(v) / len(v), 2)} for k, v in times.items()}, "notes": notes}
    mean = {k: v["mean_us"] for k, v in res["legs"].items()}
    if "a" in mean:
        res["delta_vs_a_us"] = {k: round(mean[k] - mean["a"], 2) for k in mean if k != "a"}
    if "c" in legs:
        tr, o, _ = legs["c"]
        res["leg_c_last_norm"], res["leg_c_last_coef"] = float(tr.grad_norm.item()), float(o.clip_coef.item())
    if "d" in legs:
        res["leg_d_last_norm"] = float(legs["d"][0].torch_norm.item())
    for tr, _, _ in legs.values():
        tr.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
