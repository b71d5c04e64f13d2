"""HybridAdamW against another tree's HybridAdamW (the parent commit's), bit for bit: the same tensor lists through the same configurations
with fixed seeds, three optimizer steps each, and per (tensor list, configuration) one line -- the library calls made, in order, and a
sha256 over everything the optimizer owns afterwards (parameters, both moments, the averages, the accumulators, norm_out, the guard block,
the counter).  The two trees' lines must be equal.

Tensor lists: those of tests/test_gpu_optim_slices.py (one full slice of each launch variant's table, and one tensor more) and the nine
tensors of tests/test_gpu_optim.py (odd sizes; the last one 4 bytes off a 16-byte boundary).
Configurations: by-value, dynamic, clipped, the average with warm-up, k = 2 with and without clipping, the guard with and without clipping,
a non-finite step under the guard, accumulators bound from outside (no gradient tensors), and three parameter groups merged and split, each
with the average / accumulating / guarded.  The learning rate is halved after every step, so the uploads are part of the sequence.

A worker runs in a given tree as a fresh child process under `timeout`; an abnormal exit ends the script with nothing more started.

    python scripts/optim_step_compare.py --parent DIR [--out profiles/optim_step_state_compare.txt]"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 3


def tensor_lists():
    lists = {}
    for capacity in (80, 76, 72, 64):
        for extra in (0, 1):
            sizes = [5] * (capacity + extra)
            sizes[capacity - 1 + extra] = 4097
            lists[f"{capacity + extra} tensors"] = sizes
    lists["9 tensors"] = [512 * 512, 2048 * 512, 8, 3, 1000, 4097, 32 * 27, 1, 1025]
    return lists


def configurations():
    cfgs = [("by-value", {}), ("dynamic", dict(dynamic=True)), ("clipped", dict(max_grad_norm=1.0)),
            ("average, warm-up", dict(ema_decay=0.99, ema_warmup=True)),
            ("k = 2", dict(accumulation_steps=2)), ("k = 2, clipped", dict(accumulation_steps=2, max_grad_norm=1.0)),
            ("guard", dict(skip_nonfinite=True)), ("guard, clipped", dict(skip_nonfinite=True, max_grad_norm=1.0)),
            ("guard, clipped, step 2 not finite", dict(skip_nonfinite=True, max_grad_norm=1.0, poison=1)),
            ("k = 2, accumulators bound, no gradients", dict(accumulation_steps=2, bind=True))]
    for merge in (True, False):
        for what, kw in (("average", dict(ema_decay=0.9)), ("k = 2", dict(accumulation_steps=2)), ("guard", dict(skip_nonfinite=True))):
            cfgs.append((f"three groups {'merged' if merge else 'split'}, {what}", dict(kw, groups=3, merge_groups=merge, dynamic=True)))
    return cfgs


def offset_copy(torch, t):
    base = torch.empty(t.numel() + 1, device="cuda")
    v = base[1:]
    v.copy_(t)
    return v


def run(torch, P, lib, sizes, kw, seed):
    kw = dict(kw)
    dynamic, poison, bind, ngroups = kw.pop("dynamic", False), kw.pop("poison", None), kw.pop("bind", False), kw.pop("groups", 1)
    k = kw.get("accumulation_steps", 1)
    odd = len(sizes) == 9                                   # the nine-tensor list: its last tensor (and gradient) 4 bytes off alignment
    g = torch.Generator().manual_seed(seed)
    new = lambda n, last: offset_copy(torch, torch.randn(n, generator=g).cuda()) if odd and last else torch.randn(n, generator=g).cuda()      # noqa: E731
    ps = [torch.nn.Parameter(new(n, i == len(sizes) - 1)) for i, n in enumerate(sizes)]
    groups = [dict(params=ps[i::ngroups], lr=1e-3 * (i + 1), weight_decay=1e-2 * i, betas=(0.9 - 0.1 * i, 0.999)) for i in range(ngroups)]
    opt = P.HybridAdamW(groups, **kw)
    opt.set_dynamic_hyper(dynamic)
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    advance = ngroups == 1 or kw.get("merge_groups", True)   # (split groups: several calls end the step, the counter is advanced here)
    opt.set_step_counter(counter, advance=advance)
    bound = [torch.zeros(n, device="cuda") for n in sizes] if bind else None
    if bind:
        opt._bind_accumulators(ps, bound, no_grad=True)
    calls = []
    orig = lib.call
    lib.call = lambda name, *args: (calls.append(name), orig(name, *args))[1]
    try:
        for s in range(STEPS):
            for j in range(k):
                for i, p in enumerate(ps):
                    p.grad = new(p.numel(), i == len(ps) - 1) * (10.0 ** (s - 1))
                if poison == s and j == k - 1:
                    ps[len(ps) // 2].grad[0] = float("inf")
                if bind:                                    # whoever binds the accumulators adds every micro-batch's gradient itself
                    for a, p in zip(bound, ps):
                        a += p.grad
                if j < k - 1:
                    if not bind:
                        opt.accumulate()
                    counter.add_(1)
            opt.step()
            if not advance:
                counter.add_(1)
            for group in opt.param_groups:
                group["lr"] *= 0.5
    finally:
        lib.call = orig
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for p in ps:
        st = opt.state[p]
        for t in (p.data, st["exp_avg"], st["exp_avg_sq"], st.get("ema"), opt._acc.get(p)):
            if t is not None:
                h.update(t.detach().cpu().contiguous().numpy().tobytes())
    for t in (opt._norm_out, opt._guard, counter):
        if t is not None:
            h.update(t.cpu().numpy().tobytes())
    return calls, h.hexdigest()


def worker(root):
    sys.path.insert(0, root)
    import torch
    import transformer_cnn_hybrid_network_for_video_processing_amd as P
    from transformer_cnn_hybrid_network_for_video_processing_amd._lib import lib
    assert os.path.realpath(os.path.dirname(os.path.dirname(P.__file__))) == os.path.realpath(root)
    for li, (lname, sizes) in enumerate(tensor_lists().items()):
        for ci, (cname, kw) in enumerate(configurations()):
            calls, digest = run(torch, P, lib, sizes, kw, 1000 * li + ci)
            print(json.dumps({"list": lname, "config": cname, "calls": calls, "sha256": digest}), flush=True)


def child(root, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--worker", "--root", root]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, cwd=root)
    if r.returncode != 0:
        sys.exit(f"the worker in {root} ended with exit status {r.returncode}: stopping here, nothing more is started on the GPU")
    return [json.loads(l) for l in r.stdout.decode().splitlines() if l.startswith("{")]


def runs(calls):
    out = []
    for c in calls:
        if out and out[-1][0] == c:
            out[-1][1] += 1
        else:
            out.append([c, 1])
    return " ".join(c.replace("hyb_", "") + (f" x{n}" if n > 1 else "") for c, n in out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true", help="(internal) run every list through every configuration in this process")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--limit", type=int, default=300, help="time limit of one worker, seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_step_state_compare.txt"))
    args = ap.parse_args()
    if args.worker:
        return worker(os.path.abspath(args.root))
    if not args.parent:
        ap.error("--parent DIR is required")
    theirs, ours = child(os.path.abspath(args.parent), args.limit), child(ROOT, args.limit)
    lines = ["HybridAdamW, the parent commit's tree against this one (scripts/optim_step_compare.py): per tensor list and configuration, three optimizer",
             "steps with fixed seeds in a fresh process per tree; the library calls in order (hyb_ left out, repeats as xN) and a sha256 over",
             "parameters, both moments, averages, accumulators, norm_out, the guard block and the counter.  EQUAL: calls and digest are the parent's."]
    differ = len(theirs) != len(ours)
    for a, b in zip(theirs, ours):
        same = a == b
        differ |= not same
        lines.append(f"  {'EQUAL ' if same else 'DIFFER'}  {b['list']:<10}  {b['config']:<40}  sha256 {b['sha256'][:16]}  {runs(b['calls'])}")
        if not same:
            lines.append(f"          parent: sha256 {a['sha256'][:16]}  {runs(a['calls'])}")
    lines.append(f"{len(ours)} runs in this tree, {len(theirs)} in the parent's: " + ("DIFFERENCES" if differ else "all equal"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(args.out, "w") as f:
        f.write(text)
    sys.exit(3 if differ else 0)                             # (1: a worker ended abnormally)


if __name__ == "__main__":
    main()
