"""What the input side of multi-view evaluation costs: V views per clip from ONE copy of the source bytes (hyb_clips_u8_transform_views), next to
what had to be done without it -- replicate every uint8 clip V times on the host and run the plain kernel (hyb_clips_u8_transform).

Workload: 8 source clips of 32 frames, 256 x 340 x 3 uint8 -> 16 frames of 224 x 224, V = 30 (10 temporal windows x 3 spatial crops,
ClipTransform(224, train=False, frames=16, eval_views=(10, 3), eval_crop=224/256) with mean/std), i.e. 240 fp32 clips per batch.
The method of scripts/mix_bench.py: the legs alternated ROUNDS times in one process, each leg on buffers of its own.
  a        one pinned H2D copy of the 8 clips and of the 240 rows, then the views launch
  b        the host replicates the 8 clips to 240 in pinned memory, one H2D copy of those and of the rows, then the plain kernel on the same 240 rows
  b_copy   leg b without the host's replication (the pinned 240 clips are already there): its H2D copy and kernel alone
  c_views  the views kernel alone, device events around LAUNCHES launches
  c_plain  the plain kernel alone on the replicated input, same rows, same output
Legs a / b / b_copy are wall-clock per batch, synchronised at the end of every batch (they include host work and PCIe); legs c are device time.
Per leg: us per batch of every round, their mean and the round-to-round spread (max - min) / mean.  The outputs of the two kernels are compared
with torch.equal before anything is timed.

    python scripts/views_bench.py [--batches 5] [--launches 20] [--rounds 3] [--out profiles/views_bench.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import transformer_cnn_hybrid_network_for_video_processing_amd as P  # noqa: E402
from transformer_cnn_hybrid_network_for_video_processing_amd._lib import lib  # noqa: E402

B, TIN, HIN, WIN, C, TOUT, SIZE, K, S = 8, 32, 256, 340, 3, 16, 224, 10, 3
V = K * S
IMAGENET = dict(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))


def legs(dev):
    g = torch.Generator(device="cpu").manual_seed(7)
    tr = P.ClipTransform(SIZE, train=False, frames=TOUT, eval_views=(K, S), eval_crop=SIZE / 256, **IMAGENET)
    assert tr.views == V
    host_rows = torch.from_numpy(tr.sample_views(B, TIN, HIN, WIN)).pin_memory()
    mi = torch.from_numpy(tr.mean_invstd(C)).to(dev)
    host = torch.randint(0, 256, (B, TIN, HIN, WIN, C), dtype=torch.uint8, generator=g).pin_memory()
    host_rep = torch.empty((B * V, TIN, HIN, WIN, C), dtype=torch.uint8).pin_memory()
    # every leg its own device buffers
    dev_a, rows_a, out_a = torch.empty_like(host, device=dev), torch.empty_like(host_rows, device=dev), torch.empty(B * V, TOUT, C, SIZE, SIZE, device=dev)
    dev_b, rows_b, out_b = torch.empty_like(host_rep, device=dev), torch.empty_like(host_rows, device=dev), torch.empty_like(out_a)
    dev_c, rows_c, out_cv, out_cp = host.to(dev), host_rows.to(dev), torch.empty_like(out_a), torch.empty_like(out_a)

    def st():
        return torch.cuda.current_stream().cuda_stream

    def views(src, rows, out):
        lib.call("hyb_clips_u8_transform_views", src, rows, mi, out, B, V, TIN, HIN, WIN, C, TOUT, SIZE, SIZE, st())

    def plain(src, rows, out):
        lib.call("hyb_clips_u8_transform", src, rows, mi, out, B * V, TIN, HIN, WIN, C, TOUT, SIZE, SIZE, st())

    def replicate():
        host_rep.view(B, V, TIN, HIN, WIN, C).copy_(host.unsqueeze(1).expand(B, V, TIN, HIN, WIN, C))

    def leg_a():
        dev_a.copy_(host, non_blocking=True)
        rows_a.copy_(host_rows, non_blocking=True)
        views(dev_a, rows_a, out_a)

    def leg_b_copy():
        dev_b.copy_(host_rep, non_blocking=True)
        rows_b.copy_(host_rows, non_blocking=True)
        plain(dev_b, rows_b, out_b)

    def leg_b():
        replicate()
        leg_b_copy()

    # the two routes write the same bits
    leg_a()
    leg_b()
    dev_rep = dev_b                                                  # leg c's replicated input: leg b's device copy, left as it is
    views(dev_c, rows_c, out_cv)
    plain(dev_rep, rows_c, out_cp)
    torch.cuda.synchronize()
    assert torch.equal(out_a, out_b) and torch.equal(out_cv, out_cp) and torch.equal(out_a, out_cv)
    wall = {"a": leg_a, "b": leg_b, "b_copy": leg_b_copy}
    device = {"c_views": lambda: views(dev_c, rows_c, out_cv), "c_plain": lambda: plain(dev_rep, rows_c, out_cp)}
    info = {"h2d_bytes": {"a": host.numel() + host_rows.numel() * 4, "b": host_rep.numel() + host_rows.numel() * 4}, "dst_bytes": out_a.numel() * 4}
    return wall, device, info


def timed_wall(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
        torch.cuda.synchronize()                  # a batch is done when its clips are there
    return (time.perf_counter() - t0) * 1e6 / n   # us per batch


def timed_device(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n          # us per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "views_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("views_bench.py measures on the GPU: no device visible")
    dev = torch.device("cuda", 0)
    wall, device, info = legs(dev)
    for fn in device.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in (*wall, *device)}
    for _ in range(args.rounds):
        for name, fn in wall.items():
            us[name].append(timed_wall(fn, args.batches))
        for name, fn in device.items():
            us[name].append(timed_device(fn, args.launches))
    res = {"device": torch.cuda.get_device_name(0),
           "shape": f"{B} clips x {TIN} frames, {HIN} x {WIN} x {C} uint8 -> {B * V} clips x {TOUT} frames, {C} x {SIZE} x {SIZE} fp32 (V = {K} x {S})",
           "batches_per_wall_leg": args.batches, "launches_per_device_leg": args.launches, "rounds": args.rounds, "legs": {}, **info}
    for name, v in us.items():
        mean = sum(v) / len(v)
        res["legs"][name] = {"runs_us": [round(t, 1) for t in v], "mean_us": round(mean, 1), "min_to_max_us": round(max(v) - min(v), 1),
                             "spread": round((max(v) - min(v)) / mean, 4)}
    L = res["legs"]
    res["h2d_bytes_ratio_a_over_b"] = round(info["h2d_bytes"]["a"] / info["h2d_bytes"]["b"], 5)
    res["a_over_b"] = round(L["a"]["mean_us"] / L["b"]["mean_us"], 4)
    res["a_over_b_copy"] = round(L["a"]["mean_us"] / L["b_copy"]["mean_us"], 4)
    res["c_views_over_c_plain"] = round(L["c_views"]["mean_us"] / L["c_plain"]["mean_us"], 4)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
