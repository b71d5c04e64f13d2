"""What the inference path buys: BASELINE config 2 (B = 8, T = 16, 224 x 224, default model), one GPU, modes bf16 and mixed.

Three contenders per mode on the SAME model and clips, in ONE process, each warmed up, then alternated ROUNDS times with device events
around CALLS calls each:
  a  model.eval() + torch.no_grad() forward -- the training forward's kernels and buffers with BatchNorm's running statistics
  b  model.predict(x)                        -- hybrid::backbone_infer (conv + BatchNorm + ReLU + MaxPool in one kernel per stage) + hybrid::temporal
  c  GraphedPredict                          -- b replayed as one hipGraph (the copy of the clip into the static buffer included)
plus torch.cuda.max_memory_allocated of one a call and one b call (each from a reset peak after its warm-up) and the largest logits
difference between a and b.  One JSON: per contender the per-round mean call times in microseconds, their median and spread (max - min).

    python scripts/infer_bench.py [--calls 200] [--rounds 5] [--modes bf16,mixed] [--out profiles/infer_bench.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/infer_bench.py --trace a|b --modes bf16 --calls 20      (one contender's kernels)
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import transformer_cnn_hybrid_network_for_video_processing_amd as P  # noqa: E402

CFG2 = dict(batch=8, frames=16, size=224)        # bench.py CONFIGS[2]; the model's defaults are that config's


def make(mode, dev):
    torch.manual_seed(0)
    model = P.TransformerCNNHybrid(compute_dtype=mode).to(dev).eval()
    g = torch.Generator(device="cpu").manual_seed(1000)
    x = torch.rand(CFG2["batch"], CFG2["frames"], 3, CFG2["size"], CFG2["size"], generator=g).to(dev)
    return model, x


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls          # microseconds per call


def peak(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--modes", default="bf16,mixed")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--trace", default="", help="a or b: run only that contender (for a kernel trace), no JSON")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "infer_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("infer_bench.py measures on the GPU; none is visible")
    dev = torch.device("cuda", 0)
    result = {"config": dict(CFG2, model="TransformerCNNHybrid() defaults"), "calls_per_round": args.calls, "rounds": args.rounds,
              "device": torch.cuda.get_device_name(0), "unit": "microseconds per call (device events around `calls_per_round` calls)", "modes": {}}
    for mode in [m for m in args.modes.split(",") if m]:
        model, x = make(mode, dev)

        def eval_fwd():
            with torch.no_grad():
                return model(x)

        def predict():
            return model.predict(x)

        if args.trace:
            fn = {"a": eval_fwd, "b": predict}[args.trace]
            for _ in range(args.calls):
                fn()
            torch.cuda.synchronize()
            continue
        graphed = P.GraphedPredict(model, x)
        legs = {"a_eval_forward": eval_fwd, "b_predict": predict, "c_graphed_predict": lambda: graphed(x)}
        for fn in legs.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        la, lb = eval_fwd().float(), predict().float()
        times = {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, fn in legs.items():                 # alternating: a, b, c, a, b, c, ...
                times[k].append(timed(fn, args.calls))
        graphed.close()
        r = {}
        for k, t in times.items():
            r[k] = {"per_round_us": [round(v, 2) for v in t], "median_us": round(statistics.median(t), 2), "spread_us": round(max(t) - min(t), 2)}
        a, b, c = (r[k]["median_us"] for k in ("a_eval_forward", "b_predict", "c_graphed_predict"))
        r["predict_saves_us"] = round(a - b, 2)
        r["graphed_predict_saves_us"] = round(a - c, 2)
        r["predict_faster_than_eval_by_more_than_its_spread"] = bool(a - b > r["a_eval_forward"]["spread_us"])
        r["logits_max_abs_diff_predict_vs_eval"] = float((la - lb).abs().max())
        r["logits_max_abs"] = float(la.abs().max())
        pa, pb = peak(eval_fwd), peak(predict)
        r["max_memory_allocated_MB"] = {"a_eval_forward": round(pa / 1e6, 1), "b_predict": round(pb / 1e6, 1), "saved": round((pa - pb) / 1e6, 1)}
        from transformer_cnn_hybrid_network_for_video_processing_amd import ops
        h = CFG2["size"]
        r["fused_stages"] = [bool(ops.conv3x3_pool_fused(model._dt, h >> s, ops.pad_channels(ci), ops.pad_channels(co)))
                             for s, (ci, co) in enumerate(((32, 64), (64, 128), (128, 256)), start=1)]
        result["modes"][mode] = r
        print(f"{mode}: eval forward {a:.1f} us (spread {r['a_eval_forward']['spread_us']:.1f}), predict {b:.1f} us, graphed predict {c:.1f} us; "
              f"peak memory {pa / 1e6:.0f} -> {pb / 1e6:.0f} MB", file=sys.stderr)
        del model, x, graphed
        torch.cuda.empty_cache()
    if args.trace:
        return
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
