"""What RandAugment's ops and the hue shift cost inside the clip augmentation kernel (hyb_clip_aug_u8_transform), next to the kernels without them and
next to the same augmentations as eager torch ops on the fp32 clip.

The protocol of scripts/photo_bench.py: 8 clips x 16 frames of 256 x 256 -> 224 x 224, ClipTransform's random crops with flip and normalisation; legs
alternated ROUNDS times in one process, device events around LAUNCHES launches each.  No time is fixed in advance: every leg is reported in us per
launch with its min-to-max over the rounds.
  plain            hyb_clips_u8_transform
  photo_identity   hyb_clips_u8_transform_photo, every photo row the identity
  aug_identity     hyb_clip_aug_u8_transform, every aug row the identity, no photo rows (the same work through the new kernel)
  geometry         a rotation, a shear and a translation folded into M on every clip, an empty program
  program_n2       Brightness, Color on every clip;   program_n4: Brightness, Color, Posterize, Solarize
  hue              one Hue step on every clip
  rand_m7_n4       rows drawn by ClipTransform("rand-m7-n4-mstd0.5", hue=0.1) with Mixup and random erasing ("pixel"): both clips of a pair go through
                   the whole chain; luma_sums, the launch a Contrast step needs, is timed on its own
The comparison that decides is the plain kernel followed by the eager torch equivalents on the fp32 clip -- what a user has to run without the fused
kernel:
  eager_geometry   plain (no mean / std) + affine_grid / grid_sample (bilinear, a second resampling), a second grid_sample of ones for the fill, normalise
  eager_program_n4 plain + the four steps as elementwise ops + normalise
  eager_hue        plain + torchvision's adjust_hue arithmetic as elementwise ops + normalise
  eager_geometry_program_n4   both
Then ClipPipeline -> GraphedTrainStep clips/s at config 2 with the option and without (--no-train skips it).

    python scripts/randaug_bench.py [--launches 200] [--rounds 3] [--steps 100] [--no-train] [--out profiles/randaug_bench.json]
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
import torch.nn.functional as F  # noqa: E402

import transformer_cnn_hybrid_network_for_video_processing_amd as P  # noqa: E402
from transformer_cnn_hybrid_network_for_video_processing_amd._lib import lib  # noqa: E402

B, TOUT, C, SIZE, SRC = 8, 16, 3, 224, 256
IMAGENET = dict(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
CFG2 = dict(d_model=512, num_heads=8, hidden_dim=1024)
RAND = dict(randaugment="rand-m7-n4-mstd0.5", hue=0.1)
BITS, THR, FB, FC = 4, 128, 1.3, 0.7


def _bits(x):
    return int(np.float32(x).view(np.int32))


def aug_rows(prog=(), M=None, fill=(0.485, 0.456, 0.406)):
    rows = np.zeros((B, 32), dtype=np.int32)
    rows[:, 0], rows[:, 1] = int(M is not None), len(prog)
    for i, (op, arg) in enumerate(prog):
        rows[:, 2 + 2 * i], rows[:, 3 + 2 * i] = op, arg
    rows[:, 18:24] = np.asarray((1, 0, 0, 0, 1, 0) if M is None else M, dtype=np.float32).view(np.int32)
    rows[:, 24:27] = np.asarray(fill, dtype=np.float32).view(np.int32)
    return rows


def eager_hue(x, h):
    """torchvision's adjust_hue on a float [..., 3, H, W] clip (channel axis 2 of [B,T,C,H,W])."""
    r, g, b = x.unbind(2)
    mx, mn = x.amax(2), x.amin(2)
    eq = mx == mn
    cr = mx - mn
    ones = torch.ones_like(mx)
    s = cr / torch.where(eq, ones, mx)
    d = torch.where(eq, ones, cr)
    rc, gc, bc = (mx - r) / d, (mx - g) / d, (mx - b) / d
    hr = (mx == r) * (bc - gc)
    hg = ((mx == g) & (mx != r)) * (2.0 + rc - bc)
    hb = ((mx != g) & (mx != r)) * (4.0 + gc - rc)
    hh = torch.fmod((hr + hg + hb) / 6.0 + 1.0, 1.0)
    hh = (hh + h) % 1.0
    i = torch.floor(hh * 6.0)
    f = hh * 6.0 - i
    i = i.to(torch.int32) % 6
    p = (mx * (1.0 - s)).clamp_(0, 1)
    q = (mx * (1.0 - s * f)).clamp_(0, 1)
    t = (mx * (1.0 - s * (1.0 - f))).clamp_(0, 1)
    mask = i.unsqueeze(2) == torch.arange(6, device=x.device).view(1, 1, 6, 1, 1)
    a1, a2, a3 = torch.stack((mx, q, p, p, t, mx), 2), torch.stack((t, mx, mx, q, p, p), 2), torch.stack((p, p, t, mx, mx, q), 2)
    return torch.stack(((mask * a1).sum(2), (mask * a2).sum(2), (mask * a3).sum(2)), 2)


def legs(dev):
    """-> {name: launch()}"""
    g = torch.Generator(device="cpu").manual_seed(7)
    out = torch.empty(B, TOUT, C, SIZE, SIZE, device=dev)
    src = torch.randint(0, 256, (B, TOUT, SRC, SRC, C), dtype=torch.uint8, generator=g).to(dev)
    tr = P.ClipTransform(SIZE, seed=1, **IMAGENET)
    drows = torch.from_numpy(tr.sample(B, TOUT, SRC, SRC)).to(dev)
    mi = torch.from_numpy(tr.mean_invstd(C)).to(dev)
    M3 = P.ClipTransform._affine("Rotate", 21.0, SIZE, SIZE) @ P.ClipTransform._affine("ShearX", 0.21, SIZE, SIZE) @ \
        P.ClipTransform._affine("TranslateY", 0.1, SIZE, SIZE)
    M = M3[:2].reshape(6)
    n2 = [(2, _bits(FB)), (4, _bits(FC))]
    n4 = n2 + [(5, BITS), (6, THR)]
    full = P.ClipTransform(SIZE, seed=1, mixup_alpha=0.8, erase_prob=1.0, erase_mode="pixel", **IMAGENET, **RAND)
    rows = {"aug_identity": aug_rows(), "geometry": aug_rows(M=M), "program_n2": aug_rows(n2), "program_n4": aug_rows(n4), "hue": aug_rows([(8, _bits(0.1))]),
            "rand_m7_n4": full.sample_aug(B, SIZE, SIZE)}
    daug = {k: torch.from_numpy(v).to(dev) for k, v in rows.items()}
    photo_id = torch.from_numpy(P.ClipTransform(SIZE, seed=1).sample_photo(B, TOUT, SIZE, SIZE)).to(dev)
    photo_full = torch.from_numpy(full.sample_photo(B, TOUT, SIZE, SIZE)).to(dev)
    mixup = torch.from_numpy(full.sample_mix(B, SIZE, SIZE)[0]).to(dev)
    sums = torch.empty(B, TOUT, dtype=torch.int64, device=dev)

    def st():
        return torch.cuda.current_stream().cuda_stream

    def luma():
        lib.call("hyb_clips_u8_luma_sums", src, drows, sums, B, TOUT, SRC, SRC, C, TOUT, st())

    def plain(norm=mi):
        lib.call("hyb_clips_u8_transform", src, drows, norm, out, B, TOUT, SRC, SRC, C, TOUT, SIZE, SIZE, st())

    def photo_identity():
        lib.call("hyb_clips_u8_transform_photo", src, drows, None, photo_id, None, mi, out, B, TOUT, SRC, SRC, C, TOUT, SIZE, SIZE, st())

    def aug(name, mix=None, photo=None, with_sums=False):
        return lambda: lib.call("hyb_clip_aug_u8_transform", src, drows, mix, photo, daug[name], sums if with_sums else None, mi, out, B, TOUT, SRC, SRC,
                                C, TOUT, SIZE, SIZE, st())
    luma()
    # ---- the eager equivalents work on the [0,1] clip, then normalise: the plain kernel without mean / std, then torch ops
    w = torch.tensor([0.2989, 0.587, 0.114], device=dev).view(1, 1, C, 1, 1)
    mean, invstd = mi[0].view(1, 1, C, 1, 1), mi[1].view(1, 1, C, 1, 1)
    a, b, c, d, e, f = (float(v) for v in M)
    S = float(SIZE)
    # pixel-centre coordinates -> affine_grid's normalised ones (align_corners=False), square frames
    theta = torch.tensor([[a, b, a + b + 2 * c / S - 1], [d, e, d + e + 2 * f / S - 1]], device=dev).expand(B * TOUT, 2, 3).contiguous()
    ones = torch.ones(B * TOUT, 1, SIZE, SIZE, device=dev)
    fill = mean.view(1, C, 1, 1)

    def e_geometry():
        grid = F.affine_grid(theta, (B * TOUT, C, SIZE, SIZE), align_corners=False)
        x = F.grid_sample(out.view(B * TOUT, C, SIZE, SIZE), grid, mode="bilinear", padding_mode="zeros", align_corners=False)
        cover = F.grid_sample(ones, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
        out.copy_((x + (1 - cover) * fill).view_as(out))

    def e_program():
        out.mul_(FB).clamp_(0, 1)
        lum = (out * w).sum(2, keepdim=True)
        out.mul_(FC).add_((1 - FC) * lum).clamp_(0, 1)
        q = (out * 255 + 0.5).floor_().to(torch.int32).bitwise_and_(~((1 << (8 - BITS)) - 1))
        out.copy_(q).div_(255)
        out.copy_(torch.where(q >= THR, 1 - out, out))

    def normalise():
        out.sub_(mean).mul_(invstd)

    def eager(*steps):
        def run():
            plain(None)
            for s in steps:
                s()
            normalise()
        return run
    return {"plain": plain, "photo_identity": photo_identity, "aug_identity": aug("aug_identity"), "geometry": aug("geometry"),
            "program_n2": aug("program_n2"), "program_n4": aug("program_n4"), "hue": aug("hue"), "luma_sums": luma,
            "rand_m7_n4": aug("rand_m7_n4", mix=mixup, photo=photo_full, with_sums=True),
            "eager_geometry": eager(e_geometry), "eager_program_n4": eager(e_program), "eager_hue": eager(lambda: out.copy_(eager_hue(out, 0.1))),
            "eager_geometry_program_n4": eager(e_geometry, e_program)}, {"rand_rows_geometric": int(rows["rand_m7_n4"][:, 0].sum()),
                                                                          "rand_rows_steps": rows["rand_m7_n4"][:, 1].tolist()}


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n          # us per call


def pipeline_legs(dev, steps, rounds):
    """ClipPipeline -> GraphedTrainStep on config-2-sized clips, the method of scripts/photo_bench.py: clips per second of the whole loop, input
    pipeline included, with the plain transform and with RandAugment and the hue shift on; the two legs alternate."""
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
    pipes = {"plain": pipe(), "randaugment": pipe(**RAND)}

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "randaug_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("randaug_bench.py measures on the GPU: no device visible")
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
    base = sum(us["plain"]) / len(us["plain"])
    for name, v in us.items():
        mean = sum(v) / len(v)
        res["legs"][name] = {"runs_us": [round(t, 2) for t in v], "mean_us": round(mean, 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2),
                             "vs_plain": round(mean / base, 3)}
    m = {k: v["mean_us"] for k, v in res["legs"].items()}
    res["fused_vs_eager"] = {"geometry": round(m["eager_geometry"] / m["geometry"], 2), "program_n4": round(m["eager_program_n4"] / m["program_n4"], 2),
                             "hue": round(m["eager_hue"] / m["hue"], 2)}
    res["slower_than_eager"] = [k for k, v in res["fused_vs_eager"].items() if v < 1.0]
    if not args.no_train:
        res["pipeline_to_train_step"] = pipeline_legs(dev, args.steps, args.rounds)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
