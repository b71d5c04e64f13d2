"""Worker of tests/test_gpu_nonfinite_guard_dp.py (launched by torch.distributed.run, 2 ranks, gloo; rank r on cuda:r, or both on cuda:0
where there is one device): HybridAdamW(skip_nonfinite=True) under GraphedTrainStep with data parallelism, k = argv[1] micro-batches per
optimizer step.  After the warm-up step: one optimizer step in which ONLY rank 1's first micro-batch is poisoned (a NaN mixing weight in its
MixTarget: read at replay time, the forward pass stays clean), then one clean step.  The norm is taken over the all-reduced buckets, so both
ranks must take the same decision without another collective: both report the skip, the parameters stay bit-equal to what they were and
equal across ranks, the buckets (the accumulators when k > 1) are all zero afterwards, and the clean step applies on both ranks."""
import hashlib, os, sys
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import transformer_cnn_hybrid_network_for_video_processing_amd as P

K = int(sys.argv[1])
dist.init_process_group(backend="gloo")
rank, world = dist.get_rank(), dist.get_world_size()
dev = torch.device("cuda", rank % torch.cuda.device_count())
torch.cuda.set_device(dev)
kw = dict(cnn_channels=(32, 64), d_model=64, num_heads=4, num_layers=1, hidden_dim=128, dropout=0.0)

torch.manual_seed(0)
model = P.TransformerCNNHybrid(**kw).to(dev).train()
for a in model.encoder.attention_layers:
    a.dropoutLayer.p = 0.0

g = torch.Generator().manual_seed(2000 + rank)                    # rank r seeds its own clips
batches = []
for _ in range(K):
    x = torch.rand(2, 2, 3, 32, 32, generator=g).to(dev)
    y = P.MixTarget(torch.randint(0, 8, (2,), generator=g).to(dev), torch.randint(0, 8, (2,), generator=g).to(dev), torch.rand(2, generator=g).to(dev))
    batches.append((x, y))
crit = P.HybridCrossEntropyLoss()
opt = P.HybridAdamW(model.parameters(), lr=1e-3, max_grad_norm=0.5, skip_nonfinite=True)
tr = P.GraphedTrainStep(model, crit, opt, *batches[0], warmup=K, accumulation_steps=K)
assert tr.gs is None and tr.steps_done() == 1


def digest():
    h = hashlib.sha256()
    for _, p in sorted(model.named_parameters()):
        h.update(p.detach().cpu().numpy().tobytes())
    out = [None] * world
    dist.all_gather_object(out, h.hexdigest())
    return out


def optimizer_step(poison):
    for j, (x, y) in enumerate(batches):
        if poison and j == 0 and rank == 1:
            lam = y.lam.clone()
            lam[0] = float("nan")
            y = P.MixTarget(y.y_a, y.y_b, lam)
        tr.load(x, y)
        tr.step()
    assert tr.is_update_step
    torch.cuda.synchronize()


params = list(model.parameters())
before = [p.detach().clone() for p in params]
moments = [opt.state[p]["exp_avg"].clone() for p in params]
optimizer_step(True)
skipped = (int(tr.skipped_steps.item()), int(opt.last_step_skipped.item()))
unchanged = all(torch.equal(p.detach().view(torch.int32), q.view(torch.int32)) for p, q in zip(params, before)) and \
    all(torch.equal(opt.state[p]["exp_avg"], q) for p, q in zip(params, moments))
norm_finite = bool(torch.isfinite(tr.grad_norm))
equal_after_skip = len(set(digest())) == 1
buckets_zero = not bool(tr.t_bucket.view(torch.int32).any()) and not bool(tr.b_bucket.view(torch.int32).any())
steps = tr.steps_done()

optimizer_step(False)
applied = int(opt.last_step_skipped.item()) == 0 and int(tr.skipped_steps.item()) == 1 and \
    all(bool(torch.isfinite(p).all()) for p in params) and any(not torch.equal(p.detach(), q) for p, q in zip(params, before))
equal_after_clean = len(set(digest())) == 1
tr.sync_optimizer_state()
step_counts = sorted({int(opt.state[p]["step"]) for p in params})
tr.close()

print(f"NFDP rank {rank} k {K}: skipped {skipped}; parameters unchanged {unchanged}; norm finite {norm_finite}; ranks equal after the skip "
      f"{equal_after_skip}; buckets zero {buckets_zero}; steps done {steps}; clean step applied {applied}; ranks equal after it "
      f"{equal_after_clean}; step counts {step_counts}", flush=True)
ok = (skipped == (1, 1) and unchanged and not norm_finite and equal_after_skip and (buckets_zero or K == 1) and steps == 2 and applied
      and equal_after_clean and step_counts == [2])
dist.destroy_process_group()
sys.exit(0 if ok else 1)
