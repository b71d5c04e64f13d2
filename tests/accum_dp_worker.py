"""Worker of tests/test_gpu_accum_dp.py (launched by torch.distributed.run, 2 ranks sharing cuda:0, gloo): gradient accumulation with data
parallelism, k = 2 micro-batches per optimizer step, STEPS optimizer steps (the first is GraphedTrainStep's warm-up) --
  A: graph.GraphedTrainStep(accumulation_steps=2): the buckets are the accumulators, the all-reduces are issued on the k-th micro-step only;
  B: eager -- per rank acc += g with torch ops in micro-batch order in one flat buffer, ONE all-reduce of acc with the op and scale
     GraphedTrainStep uses, G = acc * inv_k with a torch op, a plain device-path HybridAdamW step on G --
from the same weights, on the same per-rank micro-batches.  Parameters and BatchNorm buffers must end BIT-equal between A and B on every
rank, and equal across ranks.  The worker counts dist.all_reduce calls: A issues exactly 2 per optimizer step (one per bucket), not per
micro-step, and leaves both buckets all zero after the update.  Dropout off: the two runs must not depend on the seed counter."""
import hashlib, os, sys
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import transformer_cnn_hybrid_network_for_video_processing_amd as P
from transformer_cnn_hybrid_network_for_video_processing_amd import ops

K, STEPS = 2, 3
dist.init_process_group(backend="gloo")
rank, world = dist.get_rank(), dist.get_world_size()
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
kw = dict(cnn_channels=(32, 64), d_model=64, num_heads=4, num_layers=1, hidden_dim=128, dropout=0.0)

reduces = [0]
_all_reduce = dist.all_reduce


def counting_all_reduce(*a, **k):
    reduces[0] += 1
    return _all_reduce(*a, **k)


dist.all_reduce = counting_all_reduce


def make():
    torch.manual_seed(0)
    m = P.TransformerCNNHybrid(**kw).to(dev).train()
    for a in m.encoder.attention_layers:
        a.dropoutLayer.p = 0.0
    return m


g = torch.Generator().manual_seed(1000 + rank)                    # rank r seeds its own clips
batches = [(torch.rand(2, 4, 3, 32, 32, generator=g).to(dev), torch.randint(0, 8, (2,), generator=g).to(dev)) for _ in range(K)]
crit = P.HybridCrossEntropyLoss()

# A: replayed graphs; the constructor takes `warmup` real micro-steps (one optimizer step) on batches[0]
ma = make()
oa = P.HybridAdamW(ma.parameters(), lr=1e-3)
tr = P.GraphedTrainStep(ma, crit, oa, *batches[0], warmup=K, accumulation_steps=K)
assert tr.steps_done() == 1 and tr.micro_steps_done() == K and tr.gs is None
per_step, zero_after, update_flags = [], [], []
for _ in range(STEPS - 1):
    before = reduces[0]
    for x, y in batches:
        tr.load(x, y)
        la = tr.step()
        update_flags.append(tr.is_update_step)
    per_step.append(reduces[0] - before)
    torch.cuda.synchronize()
    zero_after.append(not bool(tr.t_bucket.view(torch.int32).any()) and not bool(tr.b_bucket.view(torch.int32).any()))
assert tr.steps_done() == STEPS and tr.micro_steps_done() == STEPS * K
fb_refused = False
try:
    tr.fwd_bwd()
except RuntimeError:
    fb_refused = True
avg = tr._avg
pa = {n: p.detach().clone() for n, p in ma.named_parameters()}
ba = {n: b.detach().clone() for n, b in ma.named_buffers()}
tr.close()
ops.set_step_counter(None)

# B: eager reference
mb = make()
ob = P.HybridAdamW(mb.parameters(), lr=1e-3)
ob.set_dynamic_hyper(True)
params = list(mb.parameters())
flat = torch.zeros(sum(p.numel() for p in params), device=dev)
inv_k = float(torch.tensor(1.0 / K, dtype=torch.float64).float())
for s in range(STEPS):
    flat.zero_()
    for x, y in ([batches[0]] * K if s == 0 else batches):
        ob.zero_grad(set_to_none=True)
        lb = crit(mb(x), y)
        lb.backward()
        flat += torch.cat([p.grad.reshape(-1) for p in params])
    _all_reduce(flat, op=dist.ReduceOp.AVG if avg else dist.ReduceOp.SUM)
    if not avg:
        flat.mul_(1.0 / world)
    G = flat * inv_k
    off = 0
    for p in params:
        p.grad = G[off:off + p.numel()].view_as(p)
        off += p.numel()
    ob.step()
torch.cuda.synchronize()

bad = [n for n, p in mb.named_parameters() if not torch.equal(p.detach(), pa[n])]
bad += [n for n, b in mb.named_buffers() if not torch.equal(b.detach(), ba[n])]
h = hashlib.sha256()
for n, p in sorted(pa.items()):
    h.update(p.cpu().numpy().tobytes())
digest = h.hexdigest()
digests = [None] * world
dist.all_gather_object(digests, digest)
moved = max((pa[n] - p0).abs().max().item() for (n, p0) in make().named_parameters())
flags_ok = update_flags == [False, True] * (STEPS - 1)
print(f"ACDP rank {rank}: mismatching tensors {bad}; loss graph {float(la):.6f} eager {float(lb.detach()):.6f}; digest {digest[:16]}; "
      f"all ranks equal {len(set(digests)) == 1}; all-reduces per optimizer step {per_step}; buckets zero after update {zero_after}; "
      f"update flags ok {flags_ok}; fwd_bwd refused {fb_refused}; max parameter change {moved:.3e}", flush=True)
ok = (not bad and len(set(digests)) == 1 and moved > 0 and float(la) == float(lb.detach()) and per_step == [2] * (STEPS - 1)
      and all(zero_after) and flags_ok and fb_refused)
dist.destroy_process_group()
sys.exit(0 if ok else 1)
