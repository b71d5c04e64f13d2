"""Per conv stage of config 2 (bf16), over the training steps of a rocprofv3 kernel_trace.csv:  python scripts/stage_pairs.py <kernel_trace.csv> <tag>

Duration of the forward conv, of the launch that makes the pooled map (two launches later: bn_relu_pool_fwd or bn_relu_apply_pooled) and of
their sum: median, min, max.  The first eight steps (eager, capture, warm-up) are dropped."""
import csv, statistics, sys
rows = list(csv.DictReader(open(sys.argv[1])))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
KEYS = {"stage2": "conv3x3_k32_kernel<2, 2, 1, true", "stage3": "conv3x3_v2_kernel<4, 2, 2, 1, 4, true", "stage4": "conv3x3_v2_kernel<4, 4, 2, 1, 6, true"}
for st, key in KEYS.items():
    conv, post, both, names = [], [], [], set()
    for i, r in enumerate(rows):
        if key in r["Kernel_Name"] and i + 2 < len(rows):
            p = rows[i + 2]
            if "bn_relu_pool_fwd" not in p["Kernel_Name"] and "bn_relu_apply_pooled" not in p["Kernel_Name"]:
                continue
            names.add(p["Kernel_Name"].split("(")[0][-40:])
            conv.append(dur(r)); post.append(dur(p)); both.append(dur(r) + dur(p))
    conv, post, both = conv[8:], post[8:], both[8:]          # drop the eager / capture / warm-up steps
    f = lambda v: f"median {statistics.median(v):6.1f} min {min(v):6.1f} max {max(v):6.1f}"
    print(f"{sys.argv[2]:>8} {st} n={len(both):3d}  conv {f(conv)} | post {f(post)} | conv+post {f(both)}  [{','.join(sorted(names))}]")
