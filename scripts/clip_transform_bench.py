"""What the device-side clip augmentation kernel (hyb_clips_u8_transform) costs, on its own and under the training step.

Kernel legs, 8 clips x 16 output frames, alternated ROUNDS times in one process, device events around LAUNCHES launches each:
  a  the existing ToTensor kernel (hyb_frames_u8hwc_to_f32chw) at 224 x 224
  b  the new kernel with identity rows, 224 x 224 -> 224 x 224 (moves the same bytes as a)
  c  random crops (ClipTransform's RandomResizedCrop rows) of a 256 x 256 source -> 224 x 224, with flip and normalisation
  d  c with Tin = 32 -> Tout = 16, stride 2
Per leg: us per launch, the algorithmic bytes (dst bytes + the crops' source bytes, from the shapes and the rows), GB/s, round-to-round spread.

Pipeline legs, BASELINE config 2, bf16, one GPU: clips/s of ClipPipeline -> GraphedTrainStep (load + step per batch), alternated:
  plain      uint8 224 x 224 batches, ToTensor on the copy stream (today's path)
  transform  uint8 256 x 256 batches, ClipTransform(224, mean, std) on the copy stream -- the kernel co-runs with the step

    python scripts/clip_transform_bench.py [--launches 200] [--rounds 3] [--steps 100] [--no-pipeline] [--out profiles/clip_transform_bench.json]
"""
import argparse
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import transformer_cnn_hybrid_network_for_video_processing_amd as P  # noqa: E402
from transformer_cnn_hybrid_network_for_video_processing_amd._lib import lib  # noqa: E402

B, TOUT, C, SIZE = 8, 16, 3, 224
IMAGENET = dict(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
CFG2 = dict(d_model=512, num_heads=8, hidden_dim=2048)        # bench.py CONFIGS[2]


def kernel_legs(dev):
    """-> {name: (launch(), algorithmic bytes)}"""
    g = torch.Generator(device="cpu").manual_seed(7)
    out = torch.empty(B, TOUT, C, SIZE, SIZE, device=dev)
    dst_bytes = out.numel() * 4
    s224 = torch.randint(0, 256, (B, TOUT, SIZE, SIZE, C), dtype=torch.uint8, generator=g).to(dev)
    s256 = torch.randint(0, 256, (B, TOUT, 256, 256, C), dtype=torch.uint8, generator=g).to(dev)
    s256_t32 = torch.randint(0, 256, (B, 32, 256, 256, C), dtype=torch.uint8, generator=g).to(dev)
    ident = torch.tensor([[0, 0, SIZE, SIZE, 0, 0, 1, 0]] * B, dtype=torch.int32, device=dev)
    tr_c = P.ClipTransform(SIZE, seed=1, **IMAGENET)
    tr_d = P.ClipTransform(SIZE, frames=TOUT, frame_stride=(2, 2), seed=1, **IMAGENET)
    rows_c, rows_d = tr_c.sample(B, TOUT, 256, 256), tr_d.sample(B, 32, 256, 256)
    mi = torch.from_numpy(tr_c.mean_invstd(C)).to(dev)
    dev_c, dev_d = torch.from_numpy(rows_c).to(dev), torch.from_numpy(rows_d).to(dev)

    def crop_bytes(rows):
        return int(sum(TOUT * int(r[2]) * int(r[3]) * C for r in rows))

    def st():
        return torch.cuda.current_stream().cuda_stream
    return {
        "a": (lambda: lib.call("hyb_frames_u8hwc_to_f32chw", s224, out, B * TOUT, SIZE, SIZE, C, st()), dst_bytes + s224.numel()),
        "b": (lambda: lib.call("hyb_clips_u8_transform", s224, ident, None, out, B, TOUT, SIZE, SIZE, C, TOUT, SIZE, SIZE, st()),
              dst_bytes + s224.numel()),
        "c": (lambda: lib.call("hyb_clips_u8_transform", s256, dev_c, mi, out, B, TOUT, 256, 256, C, TOUT, SIZE, SIZE, st()),
              dst_bytes + crop_bytes(rows_c)),
        "d": (lambda: lib.call("hyb_clips_u8_transform", s256_t32, dev_d, mi, out, B, 32, 256, 256, C, TOUT, SIZE, SIZE, st()),
              dst_bytes + crop_bytes(rows_d)),
    }


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n          # us per call


def spread(v):
    return round((max(v) - min(v)) / (sum(v) / len(v)), 4)


def pipeline_legs(dev, steps, rounds):
    torch.manual_seed(0)
    crit = P.HybridCrossEntropyLoss()
    g = torch.Generator(device="cpu").manual_seed(1000)
    x0 = torch.rand(B, TOUT, C, SIZE, SIZE, generator=g).to(dev)
    y0 = torch.randint(0, 8, (B,), generator=g).to(dev)
    model = P.TransformerCNNHybrid(cnn_channels=(32, 64, 128, 256), num_layers=2, num_classes=8, dropout=0.0, compute_dtype="bf16", **CFG2).to(dev).train()
    trainer = P.GraphedTrainStep(model, crit, P.HybridAdamW(model.parameters(), lr=1e-12), x0, y0)
    total = rounds * (steps + 5) + 8
    pipes = {
        "plain": iter(P.ClipPipeline(itertools.islice(iter(P.SyntheticClipSource(B, TOUT, SIZE, seed=1000, distinct=3)), total), device=dev)),
        "transform": iter(P.ClipPipeline(itertools.islice(iter(P.SyntheticClipSource(B, TOUT, 256, seed=1000, distinct=3)), total), device=dev,
                                         transform=P.ClipTransform(SIZE, seed=0, **IMAGENET))),
    }

    def step(name):
        xb, yb = next(pipes[name])
        trainer.load(xb, yb)
        return trainer.step()
    for name in pipes:
        for _ in range(5):
            step(name)
    torch.cuda.synchronize()
    us = {k: [] for k in pipes}
    for _ in range(rounds):
        for name in pipes:
            us[name].append(timed(lambda: step(name), steps))
    res = {k: {"runs_clips_per_s": [round(B * 1e6 / t, 1) for t in v], "mean_clips_per_s": round(B * 1e6 / (sum(v) / len(v)), 1),
               "mean_ms_per_step": round(sum(v) / len(v) / 1e3, 4), "spread": spread(v)} for k, v in us.items()}
    for p in pipes.values():            # drain, so that no slot is left in flight
        for _ in p:
            pass
    trainer.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--no-pipeline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_transform_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_transform_bench.py measures on the GPU: no device visible")
    dev = torch.device("cuda", 0)
    legs = kernel_legs(dev)
    for fn, _ in legs.values():
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in legs}
    for _ in range(args.rounds):
        for name, (fn, _) in legs.items():
            us[name].append(timed(fn, args.launches))
    res = {"device": torch.cuda.get_device_name(0), "shape": f"{B} clips x {TOUT} output frames x {C} x {SIZE} x {SIZE} fp32", "launches_per_leg": args.launches,
           "rounds": args.rounds, "kernel_legs": {}}
    for name, v in us.items():
        mean = sum(v) / len(v)
        res["kernel_legs"][name] = {"runs_us": [round(t, 2) for t in v], "mean_us": round(mean, 2), "algorithmic_bytes": legs[name][1],
                                    "GB_per_s": round(legs[name][1] / mean / 1e3, 1), "spread": spread(v)}
    if not args.no_pipeline:
        res["pipeline_config2_bf16"] = pipeline_legs(dev, args.steps, args.rounds)
        res["pipeline_steps_per_leg"] = args.steps
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
