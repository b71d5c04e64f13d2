"""What colour jitter, Gaussian noise and random erasing cost inside the clip augmentation kernel (hyb_clips_u8_transform_photo), next to the
kernel without them and next to the same augmentations as eager torch ops on the fp32 clip.

The method of scripts/mix_bench.py: 8 clips x 16 frames of 256 x 256 -> 224 x 224, ClipTransform's random crops with flip and normalisation; legs
alternated ROUNDS times in one process, device events around LAUNCHES launches each.  The plain kernel in the same run is the yardstick:
  plain        hyb_clips_u8_transform
  identity     hyb_clips_u8_transform_photo, every photo row the identity (the same work through the new kernel)
  bright_sat   brightness and saturation factors != 1 on every clip
  contrast     a contrast factor != 1 on every clip; luma_sums is the hyb_clips_u8_luma_sums launch it needs, timed on its own
  noise        sigma 0.1 on every clip: two hashes, one log, one sqrt, one cosine per element
  erase        a RandomErasing box on every clip, "pixel" mode
  all          everything above at once (the contrast leg's luma launch not included: add luma_sums)
  all_mixup    ... with every clip blended with its partner: both clips go through the whole chain
  eager        plain + the eager torch equivalents of `all` on the fp32 clip: mul_/clamp_ for brightness, the contrast and saturation lerps
               with their clamps, randn_like noise, a masked fill -- what a user has to run without the fused kernel
Then ClipPipeline -> GraphedTrainStep clips/s with a photometric transform and without (--no-train skips it).

    python scripts/photo_bench.py [--launches 200] [--rounds 3] [--steps 100] [--no-train] [--out profiles/photo_bench.json]
"""
import argparse
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import transformer_cnn_hybrid_network_for_video_processing_amd as P  # noqa: E402
from transformer_cnn_hybrid_network_for_video_processing_amd._lib import lib  # noqa: E402

B, TOUT, C, SIZE, SRC = 8, 16, 3, 224, 256
IMAGENET = dict(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
CFG2 = dict(d_model=512, num_heads=8, hidden_dim=1024)
ON = {
    "bright_sat": dict(brightness=0.4, saturation=0.4),
    "contrast": dict(contrast=0.4),
    "noise": dict(noise_std=0.1),
    "erase": dict(erase_prob=1.0, erase_mode="pixel"),
    "all": dict(brightness=0.4, contrast=0.4, saturation=0.4, noise_std=0.1, erase_prob=1.0, erase_mode="pixel"),
}


def legs(dev):
    """-> {name: launch()}"""
    g = torch.Generator(device="cpu").manual_seed(7)
    out = torch.empty(B, TOUT, C, SIZE, SIZE, device=dev)
    src = torch.randint(0, 256, (B, TOUT, SRC, SRC, C), dtype=torch.uint8, generator=g).to(dev)
    tr = P.ClipTransform(SIZE, seed=1, **IMAGENET)
    drows = torch.from_numpy(tr.sample(B, TOUT, SRC, SRC)).to(dev)
    mi = torch.from_numpy(tr.mean_invstd(C)).to(dev)
    mixup = torch.from_numpy(P.ClipTransform(SIZE, seed=1, mixup_alpha=0.8).sample_mix(B, SIZE, SIZE)[0]).to(dev)
    rows = {"identity": P.ClipTransform(SIZE, seed=1).sample_photo(B, TOUT, SIZE, SIZE)}
    for name, kw in ON.items():
        rows[name] = P.ClipTransform(SIZE, seed=1, **kw).sample_photo(B, TOUT, SIZE, SIZE)
    dphoto = {k: torch.from_numpy(v).to(dev) for k, v in rows.items()}
    sums = torch.empty(B, TOUT, dtype=torch.int64, device=dev)

    def st():
        return torch.cuda.current_stream().cuda_stream

    def luma():
        lib.call("hyb_clips_u8_luma_sums", src, drows, sums, B, TOUT, SRC, SRC, C, TOUT, st())

    def plain():
        lib.call("hyb_clips_u8_transform", src, drows, mi, out, B, TOUT, SRC, SRC, C, TOUT, SIZE, SIZE, st())

    def photo(name, mix=None, with_sums=False):
        return lambda: lib.call("hyb_clips_u8_transform_photo", src, drows, mix, dphoto[name], sums if with_sums else None, mi, out, B, TOUT, SRC, SRC,
                                C, TOUT, SIZE, SIZE, st())
    luma()                                                       # the contrast legs read it
    # the eager equivalents work on the [0,1] clip, then normalise: the plain kernel without mean/std, then torch ops
    f = torch.from_numpy(rows["all"][:, :3].copy().view(np.float32)).to(dev).view(B, 3, 1, 1, 1, 1)
    w = torch.tensor([0.2989, 0.587, 0.114], device=dev).view(1, 1, C, 1, 1)
    mean, invstd = mi[0].view(1, 1, C, 1, 1), mi[1].view(1, 1, C, 1, 1)
    mask = torch.zeros(B, 1, 1, SIZE, SIZE, dtype=torch.bool, device=dev)
    for b, (y0, x0, h, wd) in enumerate(rows["all"][:, 8:12].tolist()):
        mask[b, :, :, y0:y0 + h, x0:x0 + wd] = True

    def eager():
        lib.call("hyb_clips_u8_transform", src, drows, None, out, B, TOUT, SRC, SRC, C, TOUT, SIZE, SIZE, st())
        out.mul_(f[:, 0]).clamp_(0, 1)
        mu = (out * w).sum(2, keepdim=True).mean((1, 3, 4), keepdim=True)
        out.mul_(f[:, 1]).add_((1 - f[:, 1]) * mu).clamp_(0, 1)
        lum = (out * w).sum(2, keepdim=True)
        out.mul_(f[:, 2]).add_((1 - f[:, 2]) * lum).clamp_(0, 1)
        out.add_(torch.randn_like(out), alpha=0.1).clamp_(0, 1)
        out.sub_(mean).mul_(invstd)
        torch.where(mask, torch.randn_like(out), out, out=out)
    return {"plain": plain, "identity": photo("identity"), "bright_sat": photo("bright_sat"), "contrast": photo("contrast", with_sums=True),
            "luma_sums": luma, "noise": photo("noise"), "erase": photo("erase"), "all": photo("all", with_sums=True),
            "all_mixup": photo("all", mix=mixup, with_sums=True), "eager": eager}, {"erase_boxes": rows["all"][:, 8:12].tolist()}


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n          # us per call


def pipeline_legs(dev, steps, rounds):
    """ClipPipeline -> GraphedTrainStep on config-2-sized clips, the method of scripts/clip_transform_bench.py: clips per second of the whole
    loop, input pipeline included, with the plain transform and with every photometric option on; the two legs alternate."""
    torch.manual_seed(0)
    crit = P.HybridCrossEntropyLoss()
    g = torch.Generator(device="cpu").manual_seed(1000)
    x0 = torch.rand(B, TOUT, C, SIZE, SIZE, generator=g).to(dev)
    y0 = torch.randint(0, 8, (B,), generator=g).to(dev)
    model = P.TransformerCNNHybrid(cnn_channels=(32, 64, 128, 256), num_layers=2, num_classes=8, dropout=0.0, compute_dtype="bf16", **CFG2).to(dev).train()
    trainer = P.GraphedTrainStep(model, crit, P.HybridAdamW(model.parameters(), lr=1e-12), x0, y0)
    total = rounds * (steps + 5) + 8

    def pipe(**kw):
        return iter(P.ClipPipeline(itertools.islice(iter(P.SyntheticClipSource(B, TOUT, SRC, seed=1000, distinct=3)), total), device=dev,
                                   transform=P.ClipTransform(SIZE, seed=0, **IMAGENET, **kw)))
    pipes = {"plain": pipe(), "photometric": pipe(**ON["all"])}

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
               "spread": round((max(v) - min(v)) / (sum(v) / len(v)), 4)} for k, v in us.items()}
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
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "photo_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("photo_bench.py measures on the GPU: no device visible")
    dev = torch.device("cuda", 0)
    L, info = legs(dev)
    for fn in L.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in L}
    for _ in range(args.rounds):
        for name, fn in L.items():
            us[name].append(timed(fn, args.launches))
    res = {"device": torch.cuda.get_device_name(0), "shape": f"{B} clips x {TOUT} frames, {SRC} x {SRC} uint8 -> {C} x {SIZE} x {SIZE} fp32",
           "launches_per_leg": args.launches, "rounds": args.rounds, "legs": {}, **info}
    for name, v in us.items():
        mean = sum(v) / len(v)
        res["legs"][name] = {"runs_us": [round(t, 2) for t in v], "mean_us": round(mean, 2), "vs_plain": round(mean / (sum(us["plain"]) / len(us["plain"])), 3),
                             "spread": round((max(v) - min(v)) / mean, 4)}
    if not args.no_train:
        res["pipeline_to_train_step"] = pipeline_legs(dev, args.steps, args.rounds)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
