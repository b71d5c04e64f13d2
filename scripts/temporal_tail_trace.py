"""Which cases of tests/test_gpu_temporal.py take the fused temporal tail: the evidence behind that file's "in" / "out" column.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 scripts/temporal_tail_trace.py run [MODE]
    python3 scripts/temporal_tail_trace.py report DIR/.../*_kernel_trace.csv [MODE] > profiles/temporal_tail_dispatch.txt

`run` calls hybrid::temporal_ce forward + backward ONCE per case, in table order, and nothing else from the library.  Every such call starts
with exactly one global-average-pool launch (gap_fwd_kernel), so `report` cuts the trace, sorted by start time, at those launches: one
segment per case.  It lists per case whether temporal_tail_fwd_kernel / temporal_tail_bwd_kernel are in the segment and, where they are not,
that the separate head / LayerNorm launches are; it exits non-zero when a case is on the other side than the table says."""
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def cases():
    import test_gpu_temporal as T
    return T, list(T.CASES.items()) + [("C65", T.C65)]


def run(mode):
    import torch
    T, table = cases()
    for name, c in table:
        m = T._model(c, mode)
        if name == "C65":                  # the forward only: its backward is refused (hyb_head_bwd takes at most 64 classes)
            y, mask = T._inputs(c)[2:]
            h = T._pooled(c, mode)
            with torch.no_grad():
                m.forward_temporal_loss((h.bfloat16() if mode in T._H_BF16 else h).cuda(), c.B, y.cuda(), None)
        else:
            T._run(m, c, mode, fused_loss=True)
        torch.cuda.synchronize()
        print("ran", name, flush=True)


def report(path, mode):
    T, table = cases()
    with open(path, newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    segs = []
    for r in rows:
        k = r["Kernel_Name"]
        if "gap_fwd_kernel" in k:
            segs.append([])
        if segs:
            segs[-1].append(k)
    if len(segs) != len(table):
        sys.exit(f"{len(segs)} global-average-pool launches for {len(table)} cases")
    print(f"# hybrid::temporal_ce forward + backward, one call per case of tests/test_gpu_temporal.py, mode {mode}: kernels of the fused tail per call")
    print(f"# {'case':6s} {'B':>3s} {'S':>3s} {'D':>5s} {'L':>2s} {'cls':>3s}  table  tail_fwd  tail_bwd  head_fwd  head_bwd  launches")
    bad = []
    for (name, c), seg in zip(table, segs):
        n = {k: sum(k in s for s in seg) for k in ("temporal_tail_fwd_kernel", "temporal_tail_bwd_kernel", "head_fwd_kernel", "head_bwd_d")}
        took = n["temporal_tail_fwd_kernel"] == 1 and (name == "C65" or n["temporal_tail_bwd_kernel"] == 1)
        none = n["temporal_tail_fwd_kernel"] == 0 and n["temporal_tail_bwd_kernel"] == 0 and n["head_fwd_kernel"] == 1
        if not ((c.tail == "in" and took and n["head_fwd_kernel"] == 0 and n["head_bwd_d"] == 0) or (c.tail == "out" and none)):
            bad.append(name)
        print(f"  {name:6s} {c.B:3d} {c.S:3d} {c.D:5d} {c.L:2d} {c.classes:3d}  {c.tail:5s}  {n['temporal_tail_fwd_kernel']:8d}  {n['temporal_tail_bwd_kernel']:8d}  "
              f"{n['head_fwd_kernel']:8d}  {n['head_bwd_d']:8d}  {len(seg):8d}")
    print("# (C65: forward only -- its backward is refused by hyb_head_bwd's argument check)")
    if bad:
        sys.exit("on the other side than the table says: " + ", ".join(bad))
    print("# every case is on the side the table says")


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "run":
        run(sys.argv[2] if len(sys.argv) > 2 else "fp32")
    elif len(sys.argv) >= 3 and sys.argv[1] == "report":
        report(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else "fp32")
    else:
        sys.exit(__doc__)
