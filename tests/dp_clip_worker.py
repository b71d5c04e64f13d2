"""Worker of tests/test_gpu_clip_lr.py::test_data_parallel_clipping_and_schedule_graph_equals_eager (launched by torch.distributed.run, 2 ranks
sharing cuda:0, gloo) -- the sibling of tests/dp_equiv_worker.py with gradient-norm clipping and a warm-up schedule switched on:
  A: graph.GraphedTrainStep (the norm is taken in piece C over the AVERAGED gradients in the flat buckets; the hyper-parameters are uploaded
     in front of every replay), and
  B: the eager step with dp.GradAllReducer and the same HybridAdamW(max_grad_norm) + scheduler --
from the same weights, on the same per-rank shard.  The norm kernel's bits do not depend on the gradients' alignment, so both form the same
norm of the same averaged gradients: the parameters must end BIT-equal, on every rank, and equal across ranks, with clipping active."""
import hashlib, math, os, sys, warnings
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import transformer_cnn_hybrid_network_for_video_processing_amd as P
from transformer_cnn_hybrid_network_for_video_processing_amd import ops
from transformer_cnn_hybrid_network_for_video_processing_amd.dp import GradAllReducer

K, WARM = 4, 1
dist.init_process_group(backend="gloo")
rank, world = dist.get_rank(), dist.get_world_size()
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
kw = dict(cnn_channels=(32, 64, 128, 256), d_model=128, num_heads=4, num_layers=2, hidden_dim=256, dropout=0.0)


def make():
    torch.manual_seed(0)
    m = P.TransformerCNNHybrid(**kw).to(dev).train()
    for a in m.encoder.attention_layers:
        a.dropoutLayer.p = 0.0
    return m


def lam(e):
    return min(1.0, (e + 1) / 4.0)


g = torch.Generator().manual_seed(1000 + rank)
x = torch.rand(2, 4, 3, 112, 112, generator=g).to(dev)
y = torch.randint(0, 8, (2,), generator=g).to(dev)
crit = P.HybridCrossEntropyLoss()

# the clip threshold: half the norm of the first step's averaged gradients (the same number on every rank).  The peak rate is 1e-5: at 1e-3 the
# norm on this fixed shard halves within the first step (24.3 -> 10.3, measured; at 1e-4 within five) and clipping would stop being active
m0 = make()
red0 = GradAllReducer(m0)
crit(m0(x), y).backward()
red0.finalize()
torch.cuda.synchronize()
c = torch.tensor([0.5 * math.sqrt(sum((p.grad.double() ** 2).sum().item() for p in m0.parameters()))], dtype=torch.float64)
dist.broadcast(c, src=0)
C = float(c.item())
del m0, red0

# A: replayed graphs; the constructor takes WARM real steps at the construction-time rate
ma = make()
oa = P.HybridAdamW(ma.parameters(), lr=1e-5, max_grad_norm=C)
sa = torch.optim.lr_scheduler.LambdaLR(oa, lam)
tr = P.GraphedTrainStep(ma, crit, oa, x, y, warmup=WARM, dynamic_hyper=True)
norms_a = []
for _ in range(K):
    la = tr.step()
    norms_a.append(tr.grad_norm.item())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sa.step()
assert tr.steps_done() == WARM + K
torch.cuda.synchronize()
pa = {n: p.detach().clone() for n, p in ma.named_parameters()}
ba = {n: b.detach().clone() for n, b in ma.named_buffers()}
tickets = int(oa._ticket.item()) if oa._ticket is not None else 0
tr.close()
ops.set_step_counter(None)

# B: eager step + GradAllReducer, WARM steps at the first rate before the scheduler starts
mb = make()
ob = P.HybridAdamW(mb.parameters(), lr=1e-5, max_grad_norm=C)
sb = torch.optim.lr_scheduler.LambdaLR(ob, lam)
red = GradAllReducer(mb)
norms_b = []
for k in range(WARM + K):
    ob.zero_grad(set_to_none=True)
    lb = crit(mb(x), y)
    lb.backward()
    red.finalize()
    ob.step()
    if k >= WARM:
        norms_b.append(ob.grad_norm.item())
        sb.step()
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
clipped = all(n > C for n in norms_a) and all(math.isfinite(n) for n in norms_a)
print(f"DPCLIP rank {rank}: mismatching tensors {bad}; loss graph {float(la):.6f} eager {float(lb.detach()):.6f}; digest {digest[:16]}; "
      f"all ranks equal {len(set(digests)) == 1}; clipped every step {clipped}; norms graph {norms_a} eager {norms_b} threshold {C:.6g}; "
      f"ticket {tickets}; max parameter change {moved:.3e}", flush=True)
ok = (not bad and len(set(digests)) == 1 and moved > 0 and float(la) == float(lb.detach()) and clipped and norms_a == norms_b and tickets == 0)
dist.destroy_process_group()
sys.exit(0 if ok else 1)
