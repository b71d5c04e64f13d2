"""The training step as replayed hipGraphs: zero_grad -> forward -> cross-entropy -> backward -> (gradient all-reduce) -> AdamW.

Why: the step is ~70 small-to-medium kernel launches; issued eagerly they cost the host 1.4 ms of Python + launch time for ~1.6 ms
of GPU work (scripts/host_jitter.py), so any kernel speed-up beyond ~15 % -- and any slower host, e.g. 8 ranks sharing one
machine -- would leave the GPU waiting.  Captured once (torch.cuda.graphs = HIP stream capture) the step is one graph launch (three with data parallelism).

The reference has nothing comparable (single process, eager); this is host-side scheduling only: the
kernels, their order and their arithmetic are exactly those of the eager step, so results are bit-identical to eager for the
same dropout seeds.

What makes capture legal here
  * every buffer an operator needs is a torch allocation made during capture (graph-private pool): nothing is allocated or
    freed by the library, and no call synchronises;
  * step-dependent scalars live on the device: the kernels add a device counter to their by-value dropout seed, and AdamW forms
    its bias corrections from state['step'] + counter on the device (hyb_*'s seed_inc / step_inc arguments).  The counter is
    advanced inside the last graph, so every replay is a new step with new masks.  With dynamic_hyper=True (or max_grad_norm set on the
    optimizer, or ema_decay: the weight average the AdamW launch then keeps, its decay and warm-up flag read from the device as well)
    AdamW's hyper-parameters live on the device too: step() uploads what changed (optimizer.sync_hyper(), never captured)
    before it replays, so a torch.optim.lr_scheduler works across replays, and the gradient norm is taken and applied inside piece C --
    with data parallelism over the averaged gradients in the buckets, as DistributedDataParallel + clip_grad_norm_ would;
  * a HybridCrossEntropyLoss with options (class weights, ignore_index, label smoothing) stays inside the temporal part's launches: the
    weights are read from the criterion's ``weight`` buffer when a replay runs, so an in-place update of that buffer is picked up by the
    next replay; ignore_index and label_smoothing travel by value, and step() refuses a change of either after capture;
  * a MixTarget (the labels of a Mixup / CutMix batch) is three static tensors: both targets and lam are read from device memory when a
    replay runs, so load() brings new labels and new mixing weights without a recapture, and the loss stays in the same launches;
  * a dense target (floating [B, C]: class probabilities under a HybridCrossEntropyLoss, binary targets under a HybridBCEWithLogitsLoss) is
    one static tensor read from device memory when a replay runs, as are the criterion's weight / pos_weight buffers; the loss stays in
    the same launches (hybrid::temporal_ce_dense), and load() refuses a target of another form than the one captured;
  * a HybridFocalLoss (class indices) and a HybridAsymmetricLoss (a dense target) ride the same way (hybrid::temporal_ce_focal /
    hybrid::temporal_ce_asym): targets and the weight / pos_weight buffers are read when a replay runs, the exponents and clip travel by
    value, and step() refuses a change of them after capture;
  * BatchNorm running statistics are updated in place by the captured statistics kernels (hybrid::backbone_);
  * with HybridAdamW(skip_nonfinite=True) a replay whose gradients are not finite changes nothing in the model: the captured norm launch
    decides, the captured AdamW launch reads the decision (optim.py).  The counter advances all the same -- the next replay draws new
    dropout masks -- and the AdamW launch subtracts the device's count of skipped steps from its step number.  The guard is part of the
    captured launches (and active in the warm-up steps): a toggle after capture is refused.  Not rolled back: the BatchNorm statistics.

Data parallelism (world > 1): the backward pass is captured in two pieces so that the gradient all-reduce of the temporal part
(25 of the 27 MB) runs -- eagerly, on the collective's own stream, outside any graph, so any torch.distributed backend works --
while the CNN backbone's backward graph executes:

    graph A: forward, loss, backward of head + encoder + token projection  -> their gradients in the "temporal" bucket
    all_reduce(temporal bucket, async)                                      [RCCL / xGMI]
    graph B: backward of the conv stages                                   -> their gradients in the "backbone" bucket
    all_reduce(backbone bucket, async); wait both
    graph C: AdamW over all parameters (gradients = views of the buckets), step counter += 1

With one rank there is nothing to exchange and no bucket: the gradient tensors produced under capture live at fixed addresses in
the graphs' private pool, so they are bound to ``p.grad`` and AdamW reads them in place (saves the two pack copies, ~25 us); and the
whole step is one graph (A, B and C captured back to back: every graph launch leaves the GPU idle for ~8 us, scripts/step_trace.py).

Gradient accumulation (accumulation_steps = k > 1): one optimizer step over k calls of step(), each a micro-batch brought by load().
  * ONE device counter, counting MICRO-steps: the dropout-seed kernels use it as ever, so every micro-batch draws its own masks; the AdamW
    launch derives its step number as counter / k (hyb_adamw_step_dev_acc) and, on update steps, advances the counter through its ticket;
    the other micro-steps end in a `counter += 1`.
  * One rank: a second graph holds A + B + one hyb_grad_accumulate launch (acc += g) + the counter increment; the single graph ends in
    the AdamW launch that reads its own gradients and the accumulators together, steps on (acc + g) / k and leaves acc zeroed.  step()
    replays the former k - 1 times, then the latter.  +4 bytes per parameter of memory.
  * World > 1: the buckets ARE the accumulators (no extra memory).  A and B bind their gradients as on one rank; after each, one eager
    hyb_grad_accumulate adds them into the bucket views.  The all-reduces are issued on the k-th micro-step only -- the equivalent of
    DistributedDataParallel.no_sync() -- and graph C steps on bucket / k with no gradient tensors, which leaves the buckets zeroed.
    Limitation: fwd_bwd() is refused with k > 1 and world > 1 (graphs A and B no longer fill the buckets by themselves).
"""
import os

import torch
import torch.distributed as dist

from . import ops
from .meter import MultiLabelMeter
from .modules import HybridAsymmetricLoss, HybridFocalLoss


class GraphedTrainStep:
    _guard_on = False                # set by the constructor: whether the captured optimizer launches are the guarded ones
    _merge_on = None                 # set by the constructor: the optimizer's merge_groups at capture (None: nothing captured, nothing to hold it to)

    def __init__(self, model, criterion, optimizer, x, y, mask=None, process_group=None, warmup=3, dynamic_hyper=False, accumulation_steps=1):
        if not (hasattr(model, "forward_backbone") and hasattr(model, "forward_temporal")):
            raise TypeError("GraphedTrainStep drives a TransformerCNNHybrid")
        if not hasattr(optimizer, "set_step_counter"):
            raise TypeError("GraphedTrainStep needs HybridAdamW (its step number lives on the device)")
        self.model, self.criterion, self.optimizer = model, criterion, optimizer
        # micro-batches per optimizer step: captured by value (the number of replays per update, k inside the AdamW launch)
        k = accumulation_steps
        if not isinstance(k, int) or isinstance(k, bool) or k < 1:
            raise ValueError("accumulation_steps must be an int >= 1")
        if k != 1 or getattr(optimizer, "accumulation_steps", 1) != 1:
            if not hasattr(optimizer, "set_accumulation"):
                raise TypeError("GraphedTrainStep: accumulation_steps > 1 needs HybridAdamW (the accumulated step is its AdamW launch)")
            if optimizer.accumulation_steps not in (1, k):
                raise ValueError(f"GraphedTrainStep: accumulation_steps={k}, but the optimizer was given {optimizer.accumulation_steps}")
            if max(1, warmup) % k:
                raise ValueError(f"GraphedTrainStep: warmup counts micro-steps and must be a multiple of accumulation_steps ({warmup} is no "
                                 f"multiple of {k}): the captured step starts at an optimizer-step boundary")
            optimizer.set_accumulation(k)
        self._k = k
        self._micro = 0              # micro-steps taken since the last optimizer step (host side; the device counter holds the total)
        self.is_update_step = False  # True after a step() that ran AdamW (with accumulation_steps == 1: after every step())
        if dynamic_hyper:
            optimizer.set_dynamic_hyper(True)
        # what the captured AdamW launch is bound to: the device path reads its hyper-parameters when it runs; the plain launch carries
        # them by value, so a later change would be lost silently -- step() refuses it instead
        self._dev_hyper = optimizer.uses_device_hyper()
        self._clipping = any(g.get("max_grad_norm") is not None for g in optimizer.param_groups)
        # which groups' captured AdamW launch also keeps the weight average (hyb_adamw_step_dev_ema): a kernel variant, fixed by the capture
        self._ema_on = [g.get("ema_decay") is not None for g in optimizer.param_groups]
        # whether the captured norm and AdamW launches are the guarded ones (skip_nonfinite): entry points, fixed by the capture
        self._guard_on = bool(getattr(optimizer, "skip_nonfinite", False))
        self._captured_hyper = self._hyper_now()
        from .modules import HybridAsymmetricLoss, HybridBCEWithLogitsLoss, HybridCrossEntropyLoss, HybridFocalLoss
        self._fused_loss = (type(criterion) in (HybridCrossEntropyLoss, HybridBCEWithLogitsLoss, HybridFocalLoss, HybridAsymmetricLoss)
                            and hasattr(model, "forward_temporal_loss")
                            and os.environ.get("HYB_FUSED_LOSS", "1") != "0")       # (=0: A/B, the criterion as its own two launches)
        # the captured loss launch carries ignore_index and label_smoothing by value (the class weights are read from the criterion's buffer
        # when a replay runs, so an in-place update of criterion.weight is picked up); a later change is refused like an optimizer's (_check_hyper)
        if type(criterion) is HybridAsymmetricLoss and hasattr(model, "head"):
            criterion._check_weight(model.head.weight.shape[0], x.device)         # (sigmoid_focal's two vectors exist before their addresses are noted)
        self._captured_loss_opts = self._loss_opts_now()
        self.group = process_group
        self.world = dist.get_world_size(process_group) if dist.is_available() and dist.is_initialized() else 1
        dev = x.device
        from .modules import MixTarget
        self._mix = isinstance(y, MixTarget)
        if self._mix and not hasattr(criterion, "has_options"):
            raise TypeError("a MixTarget needs a HybridCrossEntropyLoss criterion")
        # a dense target (floating [B, C]: class probabilities, or the binary targets of a HybridBCEWithLogitsLoss) is one static tensor like
        # the class indices, read from device memory when a replay runs; load() keeps to the form captured
        self._dense = not self._mix and y.is_floating_point()
        # static inputs: copy new batches in with load() (a MixTarget: static copies of all three tensors)
        self.x, self.y = x.clone(), MixTarget(*(t.clone() for t in y)) if self._mix else y.clone()
        self.mask = mask.clone() if mask is not None else None
        self.counter = torch.zeros(1, dtype=torch.int64, device=dev)
        self._one = None
        self.t_params = [p for p in model.temporal_parameters() if p.requires_grad]
        self.b_params = [p for p in model.backbone_parameters() if p.requires_grad]
        if len(self.t_params) + len(self.b_params) != sum(1 for p in model.parameters() if p.requires_grad):
            raise RuntimeError("model has trainable parameters outside its backbone and temporal parts")
        self.t_bucket, self.t_views = self._bucket(self.t_params) if self.world > 1 else (None, None)
        self.b_bucket, self.b_views = self._bucket(self.b_params) if self.world > 1 else (None, None)
        self._avg = self.world > 1 and dist.get_backend(process_group) == "nccl" and hasattr(dist.ReduceOp, "AVG")
        if self.world > 1:                                     # same start on every rank
            with torch.no_grad():
                for t in list(model.parameters()) + list(model.buffers()):
                    dist.broadcast(t.data, src=0, group=process_group)

        ops.set_step_counter(self.counter)
        # one parameter group, or several that the optimizer serves from one launch (merge_groups, fixed by the capture): the AdamW launch
        # itself advances the counter (no separate `counter += 1` launch per step)
        self._merge_on = bool(getattr(optimizer, "merge_groups", False))
        self._advancing = (sum(1 for g in optimizer.param_groups if any(p.requires_grad for p in g["params"])) == 1
                           or (hasattr(optimizer, "merges_groups") and optimizer.merges_groups()))
        optimizer.set_step_counter(self.counter, advance=self._advancing)
        self._captured = False                                 # (world > 1, k > 1: the eager accumulate launches' tables are kept from then on)
        if self.world > 1 and k == 1:
            for p, v in zip(self.t_params + self.b_params, self.t_views + self.b_views):
                p.grad = v                                     # AdamW reads the (all-reduced) buckets in place
        elif self.world > 1:                                   # the buckets are the accumulators; AdamW gets no gradient tensors
            optimizer._bind_accumulators(self.t_params + self.b_params, self.t_views + self.b_views, no_grad=True)
        elif k > 1:
            optimizer.accum_init()                             # eagerly, zeroed: a captured launch must not be the one that creates them
        # warm-up on a side stream (lazy initialisation, allocator steady state), then capture
        side = torch.cuda.Stream(device=dev)
        cap = torch.cuda.Stream(device=dev)                    # every capture below runs on this stream
        if self._fused_loss:
            # the fused loss keeps a ticket word between its workgroups that must be zero before the first call and that no graph zeroes:
            # the buffers of both streams are created and zeroed here, eagerly, and kept (ops._ce_scratch refuses to create one under capture)
            nclips = x.shape[0]
            self._ce_scratch = [ops.prepare_ce_scratch(nclips, dev, st) for st in (side, cap)]
            cap.wait_stream(torch.cuda.current_stream(dev))
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for i in range(max(1, warmup)):
                update = (i + 1) % k == 0
                self._piece_a(); self._accumulate_bucket("t")
                if update:
                    self._reduce_wait(self._reduce(self.t_bucket))
                self._piece_b(); self._accumulate_bucket("b")
                if update:
                    self._reduce_wait(self._reduce(self.b_bucket))
                    self._piece_c()
                else:
                    self._piece_acc()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        self._warm_steps = max(1, warmup)
        self.ga, self.gb, self.gc_ = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.ga, stream=cap):
            self._piece_a()
        with torch.cuda.graph(self.gb, pool=self.ga.pool(), stream=cap):
            self._piece_b()
        self.gs = self.gm = None
        self.is_update_step = True
        params = self.t_params + self.b_params
        if self.world == 1 and os.environ.get("HYB_GRAPH_SINGLE", "1") != "0":      # (=0: A/B switch, the three-graph form)
            # one rank: nothing happens between the pieces, so the whole step is ALSO captured as one graph (every graph launch leaves the
            # GPU idle for ~8 us: two launches fewer per step).  Graphs A + B stay for fwd_bwd(); the two captures have their own gradient
            # tensors, and p.grad is re-bound to the set the last call wrote.
            self._grads_fb, self._loss_fb = [p.grad for p in params], self.loss
            self.gs = torch.cuda.CUDAGraph()
            # (its own memory pool: in A/B's pool the loss and gradient tensors step() returns could sit in blocks that A/B use as scratch,
            # and a later fwd_bwd() would overwrite them -- ADVICE r3)
            with torch.cuda.graph(self.gs, stream=cap):
                self._piece_a(); self._piece_b(); self._piece_c()
            self._grads_step, self._loss_step, self._logits_step = [p.grad for p in params], self.loss, self.logits
            self._bound = "step"
            if k > 1:
                # micro-batches 1 .. k - 1: A + B + the accumulate launch (+ counter += 1), in a pool of its own for the reason gs has one
                self.gm = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self.gm, stream=cap):
                    self._piece_a(); self._piece_b(); self._piece_acc()
                self._grads_micro, self._loss_micro, self._logits_micro = [p.grad for p in params], self.loss, self.logits
                self._bound = "micro"
        else:
            with torch.cuda.graph(self.gc_, pool=self.ga.pool(), stream=cap):
                self._piece_c()
            if k > 1:                                          # what ends a micro-step that is no update (world > 1: the accumulation was eager)
                self.gm = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self.gm, pool=self.ga.pool(), stream=cap):
                    self._piece_acc()
        self._captured = True
        # the captures above did not execute: the state is still "after the warm-up steps"

    def _hyper_now(self):
        """Per group, as the optimizer itself states it: (the row of its device block less the clip value, whether it clips, what its launch
        carries by value besides)."""
        opt = self.optimizer
        return [(opt._group_hyper(g)[:5], g.get("max_grad_norm") is not None, opt._by_value(g)) for g in opt.param_groups]

    def _loss_opts_now(self):
        """[(name, value)]: what the criterion's captured launches carry by value and the addresses of the buffers they read, as the criterion
        itself lists them (modules._Criterion._captured); None for a criterion that is not one of this package's."""
        captured = getattr(self.criterion, "_captured", None)
        return captured() if captured is not None else None

    def _check_hyper(self):
        """In front of every replay.  Device path: upload what changed.  Plain path: a few comparisons per group (the host is the step's pacemaker
        between graph launches, so this stays allocation-free) -- a changed value must not be lost silently."""
        if bool(getattr(self.optimizer, "skip_nonfinite", False)) != self._guard_on:
            raise RuntimeError("GraphedTrainStep: skip_nonfinite was switched on or off after capture; the captured norm and AdamW launches are "
                               "(not) the guarded ones -- set it on the optimizer before constructing GraphedTrainStep")
        if self._merge_on is not None and bool(getattr(self.optimizer, "merge_groups", False)) != self._merge_on:
            raise RuntimeError("GraphedTrainStep: merge_groups was switched on or off after capture; the captured AdamW launches are (not) the "
                               "one launch over all parameter groups -- set it on the optimizer before constructing GraphedTrainStep")
        now = self._loss_opts_now()
        if now != self._captured_loss_opts:
            what = [name for (name, a), (_, b) in zip(now, self._captured_loss_opts) if a != b]
            raise RuntimeError(f"GraphedTrainStep: the criterion's {', '.join(what)} changed after capture, but the captured loss launch carries "
                               "the old value -- construct a new GraphedTrainStep (an in-place update of criterion.weight needs none: the "
                               "buffer is read at replay time)")
        if [g.get("ema_decay") is not None for g in self.optimizer.param_groups] != self._ema_on:
            raise RuntimeError("GraphedTrainStep: ema_decay was switched on or off after capture; the captured AdamW launch does (not) keep the "
                               "average -- set it on the optimizer before constructing GraphedTrainStep (its value may change at any time)")
        if self._captured_hyper[0][2]:                         # (an optimizer whose launch carries something by value: HybridSGD's nesterov)
            for g, c in zip(self.optimizer.param_groups, self._captured_hyper):
                now = self.optimizer._by_value(g)
                if now != c[2]:
                    what = [name for (name, a), (_, b) in zip(now, c[2]) if a != b]
                    raise RuntimeError(f"GraphedTrainStep: the optimizer's {', '.join(what)} changed after capture, but it travels by value in the "
                                       "captured step launch -- construct a new GraphedTrainStep")
        if self._dev_hyper:
            if any((g.get("max_grad_norm") is not None) != self._clipping for g in self.optimizer.param_groups):
                raise RuntimeError("GraphedTrainStep: max_grad_norm was switched on or off after capture; the norm launch is (not) part of the "
                                   "captured step -- set it on the optimizer before constructing GraphedTrainStep")
            self.optimizer.sync_hyper()                        # on the current stream, in front of the replay; uploads only what changed
            return
        for g, c in zip(self.optimizer.param_groups, self._captured_hyper):
            if self.optimizer._group_hyper(g)[:5] != c[0] or (g.get("max_grad_norm") is not None) != c[1]:
                raise RuntimeError("GraphedTrainStep: an optimizer hyper-parameter (lr, betas, eps, weight_decay, max_grad_norm) changed after "
                                   "capture, but the captured AdamW launch carries the old value -- construct with dynamic_hyper=True to use "
                                   "schedulers (and set max_grad_norm before constructing)")

    @property
    def grad_norm(self):
        """optimizer.grad_norm: the device scalar holding the last step's unclipped total gradient norm (max_grad_norm set)."""
        return self.optimizer.grad_norm

    @property
    def skipped_steps(self):
        """optimizer.skipped_steps: the device scalar counting the optimizer steps the non-finite guard has skipped (skip_nonfinite=True)."""
        return self.optimizer.skipped_steps

    def _check_accumulation(self):
        if self.optimizer.accumulation_steps != self._k:
            raise RuntimeError(f"GraphedTrainStep: the optimizer's accumulation_steps changed after capture ({self._k} -> "
                               f"{self.optimizer.accumulation_steps}); the captured launches carry k and step() the number of replays per "
                               "update -- construct a new GraphedTrainStep")

    def _bind(self, which):
        if self.gs is not None and self._bound != which:
            for p, g in zip(self.t_params + self.b_params, {"step": self._grads_step, "fb": self._grads_fb}.get(which) or self._grads_micro):
                p.grad = g
            self._bound = which

    @staticmethod
    def _bucket(params):
        total = sum(p.numel() for p in params)
        flat = torch.zeros(max(total, 1), dtype=torch.float32, device=params[0].device if params else "cuda")
        views, off = [], 0
        for p in params:
            views.append(flat[off:off + p.numel()].view_as(p))
            off += p.numel()
        return flat, views

    # ---- the three pieces (identical code runs eagerly in the warm-up and under capture) -------------------------------
    def _piece_a(self, bind=True):
        h, B = self.model.forward_backbone(self.x)
        if self._fused_loss:                                   # the loss rides in the temporal part's last launch, its backward in the backward's first
            loss, logits = self.model.forward_temporal_loss(h, B, self.y, self.mask, self.criterion)
        else:
            logits = self.model.forward_temporal(h, B, self.mask)
            loss = self.criterion(logits, self.y)
        self.logits = logits.detach()
        if self._one is None:                                  # d(loss)/d(loss): a constant, not a fill launch per step
            self._one = torch.ones_like(loss)
        grads = torch.autograd.grad(loss, [h] + self.t_params, grad_outputs=self._one)
        self._h, self._gh = h, grads[0]
        self._deliver(self.t_params, self.t_views, grads[1:], bind)
        self.loss = loss.detach()

    def _piece_b(self, bind=True):
        grads = torch.autograd.grad(self._h, self.b_params, grad_outputs=self._gh)
        self._deliver(self.b_params, self.b_views, grads, bind)
        self._h = self._gh = None

    def _deliver(self, params, views, grads, bind):
        if views is not None and self._k == 1:
            torch._foreach_copy_(views, list(grads))
        elif bind:                                             # one rank: the captured gradient tensors themselves (static addresses)
            for p, g in zip(params, grads):
                p.grad = g

    def _piece_c(self):
        if self.world > 1 and not self._avg:
            self.t_bucket.mul_(1.0 / self.world)
            self.b_bucket.mul_(1.0 / self.world)
        self.optimizer.step()
        if not self._advancing:
            self.counter.add_(1)

    def _piece_acc(self):
        """What ends a micro-batch that is no update: acc += g (one rank; with world > 1 _accumulate_bucket has done it) and counter += 1."""
        if self.world == 1:
            self.optimizer.accumulate()
        self.counter.add_(1)

    def _accumulate_bucket(self, which):
        """World > 1 with accumulation: one eager hyb_grad_accumulate, bucket views += the gradients graph A (or B) has just written."""
        if self.world == 1 or self._k == 1:
            return
        params, views = (self.t_params, self.t_views) if which == "t" else (self.b_params, self.b_views)
        if params:                                             # (the optimizer keeps the table only once the captures are done)
            self.optimizer._accumulate_into(("bucket", which), params, views, keep=self._captured)

    def _reduce(self, bucket):
        if self.world == 1:
            return None
        return dist.all_reduce(bucket, op=dist.ReduceOp.AVG if self._avg else dist.ReduceOp.SUM, group=self.group, async_op=True)

    @staticmethod
    def _reduce_wait(work):
        if work is not None:
            work.wait()

    # ---- public ---------------------------------------------------------------------------------------------------------
    def load(self, x, y, mask=None):
        """Copy the next batch into the static input buffers (same shapes as at construction; y a MixTarget exactly when it was one there, a
        dense floating [B, C] target exactly when it was one there)."""
        from .modules import MixTarget
        if isinstance(y, MixTarget) != self._mix:
            raise TypeError("GraphedTrainStep was captured with " + ("a MixTarget: load() needs one too" if self._mix else
                            "a dense target: a MixTarget needs a step constructed with one" if self._dense else
                            "a class-index tensor: a MixTarget needs a step constructed with one"))
        if not self._mix and y.is_floating_point() != self._dense:
            raise TypeError("GraphedTrainStep was captured with " + ("a dense target: load() needs a floating [B,C] target too" if self._dense else
                            "a class-index tensor: a dense target needs a step constructed with one"))
        self.x.copy_(x, non_blocking=True)
        if self._mix:
            for dst, src in zip(self.y, y):
                dst.copy_(src, non_blocking=True)
        else:
            self.y.copy_(y, non_blocking=True)
        if mask is not None:
            self.mask.copy_(mask, non_blocking=True)

    def step(self):
        """One training step; returns the (device) loss tensor of this step -- reading it synchronises."""
        self._check_hyper()
        if self._k > 1:
            return self._micro_step()
        if self.gs is not None:
            self._bind("step")
            self.gs.replay()
            self.loss = self._loss_step
            return self.loss
        self.ga.replay()
        w1 = self._reduce(self.t_bucket)                       # rides under graph B
        self.gb.replay()
        w2 = self._reduce(self.b_bucket)
        self._reduce_wait(w1)
        self._reduce_wait(w2)
        self.gc_.replay()
        return self.loss

    def _micro_step(self):
        """step() with accumulation_steps = k > 1: micro-batches 1 .. k - 1 accumulate, the k-th runs AdamW; returns this micro-batch's loss."""
        self._check_accumulation()
        update = self._micro == self._k - 1
        if self.gs is not None:
            self._bind("step" if update else "micro")
            (self.gs if update else self.gm).replay()
            self.loss, self.logits = (self._loss_step, self._logits_step) if update else (self._loss_micro, self._logits_micro)
        else:
            self.ga.replay()
            self._accumulate_bucket("t")
            w1 = self._reduce(self.t_bucket) if update else None     # the k-th micro-step only; rides under graph B
            self.gb.replay()
            self._accumulate_bucket("b")
            if update:
                w2 = self._reduce(self.b_bucket)
                self._reduce_wait(w1)
                self._reduce_wait(w2)
                self.gc_.replay()
            else:
                self.gm.replay()
        self._micro = 0 if update else self._micro + 1
        self.is_update_step = update
        return self.loss

    def fwd_bwd(self):
        """Forward + loss + backward (+ all-reduce) only: no optimizer, the step counter does not advance.  With accumulation_steps > 1:
        refused between the micro-batches of one optimizer step, and always with world > 1 (see the module docstring)."""
        if self._k > 1:
            self._check_accumulation()
            if self.world > 1:
                raise RuntimeError("GraphedTrainStep.fwd_bwd() is not available with accumulation_steps > 1 and data parallelism: graphs A and "
                                   "B no longer fill the buckets by themselves")
            if self._micro:
                raise RuntimeError(f"GraphedTrainStep.fwd_bwd() in the middle of an accumulated step ({self._micro} of {self._k} micro-batches "
                                   "taken): finish the optimizer step first")
        self._bind("fb")
        self.ga.replay()
        w1 = self._reduce(self.t_bucket)
        self.gb.replay()
        w2 = self._reduce(self.b_bucket)
        self._reduce_wait(w1)
        self._reduce_wait(w2)
        if self.gs is not None:
            self.loss = self._loss_fb
        return self.loss

    def eager_fwd_bwd(self):
        """The same forward + backward issued launch by launch (for per-kernel event timing, which needs live launches)."""
        self._piece_a(bind=False)
        self._piece_b(bind=False)
        return self.loss

    def steps_done(self):
        """Optimizer steps taken through this object, warm-up included (reads the device counter: synchronises)."""
        return int(self.counter.item()) // self._k

    def micro_steps_done(self):
        """Micro-steps (forward + backward passes) taken through this object, warm-up included; = steps_done() with accumulation_steps 1."""
        return int(self.counter.item())

    def sync_optimizer_state(self):
        """Fold the device step counter into the optimizer's Python-side state (before state_dict()), less the steps the non-finite guard
        skipped: `step` counts applied updates.  Both device counts are zeroed.  Refused between the micro-batches of one optimizer step:
        the accumulators then hold a partial sum that no state dict carries."""
        if self._micro:
            raise RuntimeError(f"GraphedTrainStep.sync_optimizer_state() in the middle of an accumulated step ({self._micro} of {self._k} "
                               "micro-batches taken): finish the optimizer step first")
        n = self.steps_done()
        if hasattr(self.optimizer, "_take_skipped"):
            n -= self.optimizer._take_skipped()
        for st in self.optimizer.state.values():
            if "step" in st:
                st["step"] = int(st["step"]) + n
        self.counter.zero_()

    def close(self):
        ops.set_step_counter(None)
        self.optimizer.set_step_counter(None)


class GraphedPredict:
    """``model.predict(x, mask)`` captured once as a hipGraph on static buffers: ``__call__(x)`` copies the clip batch in and replays.

    Inference at small batch is launch-bound like the training step (about twenty launches and four operator calls of host work per
    forward); replayed, it is one graph launch.  Same kernels, same order, same arithmetic as eager ``predict``: bit-identical results.
    The graph is a single chain on one stream.  Capture discipline as GraphedTrainStep: warm up first on a side stream (lazy
    initialisation, allocator steady state), every buffer is a torch allocation (the static inputs outside the capture, the operators'
    workspaces in the graph's private pool), nothing under capture relies on a zero-filled buffer.  The returned logits tensor is the
    graph's static output: the next call overwrites it (clone to keep).  The weights are read at replay time, so a later
    ``load_state_dict`` into the same parameters is picked up; changing shapes, dtype or structure needs a new GraphedPredict."""

    def __init__(self, model, x, mask=None, warmup=3):
        if not hasattr(model, "predict"):
            raise TypeError("GraphedPredict drives a TransformerCNNHybrid")
        if not x.is_cuda:
            raise RuntimeError("GraphedPredict needs the model and the clip batch on a cuda (ROCm) device; there is no CPU fallback")
        self.model = model
        dev = x.device
        self.x = x.detach().float().clone()                   # static inputs
        self.mask = mask.detach().clone() if mask is not None else None
        side = torch.cuda.Stream(device=dev)
        cap = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(max(1, warmup)):
                model.predict(self.x, self.mask)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=cap):
            self.logits = model.predict(self.x, self.mask)

    def __call__(self, x, mask=None):
        if self.graph is None:
            raise RuntimeError("GraphedPredict is closed")
        if x.shape != self.x.shape:
            raise ValueError(f"GraphedPredict was captured for clips of shape {tuple(self.x.shape)}, got {tuple(x.shape)}")
        self.x.copy_(x, non_blocking=True)
        if mask is not None:
            if self.mask is None:
                raise ValueError("GraphedPredict was captured without a mask")
            self.mask.copy_(mask, non_blocking=True)
        self.graph.replay()
        return self.logits

    def close(self):
        """Release the graph and its private memory pool."""
        if self.graph is not None:
            self.graph.reset()
        self.graph = self.logits = None


class GraphedEval:
    """``model.evaluate(x, y, meter, mask, views)`` captured once as a hipGraph: predict plus the meter's update launch (hyb_eval_metrics)
    on static buffers.  ``__call__(x, y)`` copies the batch in and replays; nothing synchronises until ``meter.compute()``.

    The discipline is GraphedPredict's: static ``x``, ``y`` and ``mask``, warm-up on a side stream, then one capture on a stream of its own.
    The meter's state exists before the capture (the meter creates it eagerly) and the captured launch adds into it in place, so every
    replay accumulates.  The warm-up calls update the meter like any other call, and their batches must not remain in it: the meter is
    RESET after the warm-up, before the capture -- a freshly built GraphedEval leaves the meter zeroed, whatever it held before.
    The logits are bit-identical to GraphedPredict's on the same input, and the returned tensor is the graph's static output (clone to keep).
    The criterion's class weights are read from its ``weight`` buffer when a replay runs (an in-place update reaches the next replay);
    ``ignore_index`` and ``label_smoothing`` travel by value in the captured launch, and a change of either after capture is refused, as
    GraphedTrainStep refuses it.  Works unchanged with the weight-average twin ``optimizer.ema_model(model)``.
    With a ``meter.MultiLabelMeter`` the captured launch is hyb_eval_multilabel and the static ``y`` is fp32 [B, C].  Nothing travels by
    value: the criterion's ``weight`` and ``pos_weight`` buffers and the meter's ``threshold`` buffer are captured by address, so an in-place
    update of any of them reaches the next replay and a REPLACED buffer is refused.  The reset after the warm-up zeroes the bank's cursor
    too: a freshly built GraphedEval leaves an empty bank, and every replay appends behind the cursor on the device.
    The other criteria need no further argument: a meter with a HybridFocalLoss captures hyb_eval_metrics_focal, a floating ``y`` [B, C]
    (soft targets; the static ``y`` is fp32 [B, C]) hyb_eval_metrics_soft, a MultiLabelMeter with a HybridAsymmetricLoss
    hyb_eval_multilabel_asym.  ``gamma``, ``gamma_pos``, ``gamma_neg``, ``clip`` and ``label_smoothing`` travel by value in the captured launch
    and a change after capture is refused by name, like ``ignore_index``; the buffers are captured by address as above."""

    def __init__(self, model, x, y, meter, mask=None, views=1, warmup=3):
        if not hasattr(model, "evaluate"):
            raise TypeError("GraphedEval drives a TransformerCNNHybrid")
        if not x.is_cuda:
            raise RuntimeError("GraphedEval needs the model and the clip batch on a cuda (ROCm) device; there is no CPU fallback")
        self.model, self.meter, self.views = model, meter, views
        dev = x.device
        self.x = x.detach().float().clone()                   # static inputs
        self._multilabel = isinstance(meter, MultiLabelMeter)
        self.y = y.detach().float().clone() if self._multilabel else y.detach().clone()     # multi-label: the static y is fp32 [B, C]
        self._soft = not self._multilabel and self.y.is_floating_point()                   # soft targets: the static y is fp32 [B, C] too
        self._by_name = self._soft or isinstance(meter.criterion, (HybridFocalLoss, HybridAsymmetricLoss))
        self.mask = mask.detach().clone() if mask is not None else None
        self._captured_loss_opts = self._loss_opts_now()
        side = torch.cuda.Stream(device=dev)
        cap = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(max(1, warmup)):
                model.evaluate(self.x, self.y, meter, self.mask, views)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        meter.reset()                                          # the warm-up batches do not stay in the meter
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=cap):
            self.logits = model.evaluate(self.x, self.y, meter, self.mask, views)
        # the capture did not execute: the meter is still zeroed

    def _loss_opts_now(self):
        """What the captured meter launch carries by value or by address: (ignore_index, label_smoothing, the weight buffer's address); with
        a MultiLabelMeter the addresses of the criterion's weight and pos_weight buffers and of the meter's threshold buffer."""
        c = self.meter.criterion
        if self._by_name:
            return self._loss_opts_by_name(c)
        if self._multilabel:
            return tuple(None if t is None else t.data_ptr() for t in (*self.meter.loss_options(), self.meter.threshold))
        if c is None:
            return None
        return (c.ignore_index, c.label_smoothing, c.weight.data_ptr() if c.weight is not None else None)

    def _loss_opts_by_name(self, c):
        """The focal, soft-target and asymmetric launches: ((name, value), ..) of every scalar the captured launch carries by value and of
        every buffer it reads by address."""
        def address(t):
            return None if t is None else t.data_ptr()
        if self._multilabel:
            return (("gamma_pos", c.gamma_pos), ("gamma_neg", c.gamma_neg), ("clip", c.clip), ("weight buffer", address(c.weight)),
                    ("pos_weight buffer", address(c.pos_weight)), ("meter's threshold buffer", address(self.meter.threshold)))
        if c is None:
            return ()
        scalar = ("label_smoothing", c.label_smoothing) if self._soft else ("gamma", c.gamma)
        return (("ignore_index", c.ignore_index), scalar, ("weight buffer", address(c.weight)))

    def _check_loss_opts(self):
        now = self._loss_opts_now()
        if now != self._captured_loss_opts and self._by_name:
            what = [n for (n, a), (_, b) in zip(now, self._captured_loss_opts) if a != b] or ["criterion itself"]
            raise RuntimeError(f"GraphedEval: {', '.join(what)} changed after capture, but the captured meter launch carries the old value (a "
                               "scalar) or reads the old address (a buffer that was replaced, not updated in place) -- construct a new "
                               "GraphedEval (an in-place update of a buffer needs none: it is read at replay time)")
        if now != self._captured_loss_opts and self._multilabel:
            what = [n for n, a, b in zip(("criterion's weight buffer", "criterion's pos_weight buffer", "meter's threshold buffer"), now,
                                         self._captured_loss_opts) if a != b]
            raise RuntimeError(f"GraphedEval: the {', the '.join(what)} was replaced after capture, but the captured meter launch reads the old "
                               "address -- construct a new GraphedEval (an in-place update needs none: the buffers are read at replay time)")
        if now != self._captured_loss_opts:
            what = [n for n, a, b in zip(("ignore_index", "label_smoothing", "the weight buffer (replaced, not updated in place)"),
                                         now or (None,) * 3, self._captured_loss_opts or (None,) * 3) if a != b] or ["criterion itself"]
            raise RuntimeError(f"GraphedEval: the criterion's {', '.join(what)} changed after capture, but the captured meter launch carries "
                               "the old value -- construct a new GraphedEval (an in-place update of criterion.weight needs none: the "
                               "buffer is read at replay time)")

    def __call__(self, x, y, mask=None):
        if self.graph is None:
            raise RuntimeError("GraphedEval is closed")
        if x.shape != self.x.shape or y.shape != self.y.shape:
            raise ValueError(f"GraphedEval was captured for clips of shape {tuple(self.x.shape)} and targets {tuple(self.y.shape)}, got "
                             f"{tuple(x.shape)} and {tuple(y.shape)}")
        self._check_loss_opts()
        self.x.copy_(x, non_blocking=True)
        self.y.copy_(y, non_blocking=True)
        if mask is not None:
            if self.mask is None:
                raise ValueError("GraphedEval was captured without a mask")
            self.mask.copy_(mask, non_blocking=True)
        self.graph.replay()
        return self.logits

    def close(self):
        """Release the graph and its private memory pool (the meter and its state stay)."""
        if self.graph is not None:
            self.graph.reset()
        self.graph = self.logits = None
