"""Fused AdamW: the optimizer step that follows the hot path in the reference harnesses
(`optim.AdamW(model.parameters(), lr)`, Model.py:153 / FCT.py:305), as ONE HIP launch over all parameter tensors
(`hyb_adamw_step`).  Same constructor defaults and update rule as `torch.optim.AdamW` (betas (0.9, 0.999), eps 1e-8,
weight_decay 1e-2, amsgrad/maximize off); state-dict keys (`step`, `exp_avg`, `exp_avg_sq`) follow torch's so checkpoints
interchange.  CUDA fp32 parameters only -- there is no CPU fallback.

What a training run needs on top of that, all built on hyper-parameters that live in DEVICE memory (`double hyper[groups, 6]`; the C side
of each is described in include/hybrid_hip.h):
  * `max_grad_norm=c`: `torch.nn.utils.clip_grad_norm_(params, c)` fused into the step -- one bit-reproducible launch forms the global L2
    norm of all gradients and the clip coefficient, the AdamW launch scales every gradient element by it;
  * `set_dynamic_hyper(True)`: the AdamW launch reads lr / betas / eps / weight_decay from the device block, so a launch captured into a
    hipGraph follows `param_groups[i]["lr"] = ...` -- i.e. any `torch.optim.lr_scheduler` -- after a `sync_hyper()`, which `step()`
    (eager) and `GraphedTrainStep.step()` (before the replay) call;
  * `ema_decay=d`: an exponential moving average of the weights (timm's ModelEma, swa_utils.AveragedModel) kept by the AdamW launch itself:
    `state[p]["ema"] <- d * ema + (1 - d) * p_new` where the launch holds `p_new` in a register -- no second pass over the weights, no
    extra launch.  `ema_warmup=True` uses `min(d, (1 + n) / (10 + n))` after n earlier steps.  Both live in a device block
    (`double [groups, 2]`), so a captured step follows a decay changed between replays.  `ema_model(model)` gives a twin module whose
    parameters ARE the averages, for `predict` / `GraphedPredict`.  The average follows only parameters that are stepped: a parameter
    without a gradient keeps its old average.
  * `accumulation_steps=k`: one optimizer step over k micro-batches.  After each of the first k - 1 backward passes `accumulate()` adds
    every `.grad` into an fp32 accumulator; `step()` after the k-th steps on `(acc + grad) * (1 / k)` and leaves the accumulators zeroed,
    all inside the AdamW launch (the norm of a clipped step is taken over the same mean): no separate sum, scale or memset pass.  The
    accumulators are zero at every optimizer-step boundary, so they are neither state nor part of the state dict.
  * `skip_nonfinite=True`: an optimizer step whose global gradient norm is not finite -- a NaN or infinite gradient element, or finite ones
    whose sum of squares overflows fp32 (a single 1e20: deliberate) -- leaves parameters, both moments and the weight average exactly as
    they were, and is counted, all on the device: the norm launch's final workgroup writes `{skip_now, skipped_total}` into a device block,
    the AdamW launch reads it and, on a skip, makes no store to the model; it still zeroes the accumulators and advances the device step
    counter.  What GradScaler.step does, with no host read: it works inside a replayed hipGraph.  Bias correction and the average's
    warm-up go by the number of APPLIED updates, so the run continues as if the batch had never been seen.  With max_grad_norm the norm
    is taken anyway and the guard adds no launch; without, the guard runs the norm launches for its decision (coefficient 1).  With finite
    gradients every step is bit-identical to the unguarded one.  `skipped_steps` / `last_step_skipped` are device scalars; on a skipped
    step `grad_norm` holds the non-finite norm and `clip_coef` is unspecified.  In eager use `state[p]["step"]` counts ATTEMPTED steps
    until `fold_skipped()` (one host read; `state_dict()` calls it) subtracts the device count, so saved steps are applied-update
    counts.  Out of scope: BatchNorm running statistics are updated by the forward pass and are not rolled back (an inf activation
    reaches them, as in torch), and a learning-rate scheduler stepped by the host is not held back on a skipped step (as with GradScaler).
  * `merge_groups=True` (the default): on the device path ONE AdamW launch serves the tensors of all parameter groups (the tensor table
    carries each tensor's group, and a workgroup reads that group's row of the device blocks), `accumulate()` is one launch and
    `sync_hyper()` uploads all changed groups with one -- so no-decay groups and a per-layer learning rate
    (`TransformerCNNHybrid.param_groups`) cost no launch per group, and an advancing step counter works with them.  Bit for bit the
    per-group launches' result.  It applies when more than one group has gradients, all of them keep a weight average or none does, they
    share the step number and there are at most 255 groups; otherwise, and on the plain by-value path, every group is a launch of its
    own as before.  An attribute like `skip_nonfinite`, neither a group key nor state.

How a step is put together.  `_plan` decides once per call which groups are live and whether one call serves them all; each resulting
launch unit is a `_Unit` record -- the pointer tables of its tensors, built (and cached while no tensor moves) by `_unit`, the one builder
behind `step()`, `accumulate()` and GraphedTrainStep's eager accumulate.  `step()` is then `_prepare` (state, tables, step numbers),
`_norm` (one call, named by `_norm_symbol`) and `_launch` (one call per unit: `_step_symbol` names the entry point, `_STEP_ARGS` lists its
arguments by the names of the record's fields).

`HybridLAMB` (at the end of the file) is the same optimizer with layer-wise trust ratios: its `_launch` is two calls per unit, the trust
pass and the step that reads it.  `HybridSGD` and `HybridLARS` (after it) are the same optimizer again with torch.optim.SGD's rule: one
state tensor (`_STATE`), a hyper row of their own (`_group_hyper`) and a `_launch` that calls hyb_sgd_step_dev."""
import copy
import ctypes
from typing import NamedTuple

import torch

from ._lib import lib, ptr_array
from .ops import _stream


class _Unit(NamedTuple):
    """A launch unit: the tensors ONE library call serves -- the stepped parameters of one group (key: its index) or of all live groups
    (key "all") -- as the host arrays the call takes.  A column the unit does not carry is None."""
    key: object          # where the unit is cached
    first: int           # index of the unit's first group (whose hyper row an ungrouped call reads)
    params: list
    layout: list         # the group index of every tensor (None: accumulate() does not care)
    addrs: list          # per tensor, the addresses of its columns: the unit is valid while they and the layout stay
    n: int
    numel: object        # long long [n]
    p: object            # the pointer arrays: parameters, exp_avg, exp_avg_sq, ...
    m: object
    v: object
    ema: object          # ... the weight averages, the accumulators, ...
    acc: object
    group: object        # ... and unsigned char [n], the layout as a merged call takes it (None: a call for one group)


# the arguments of each device-path step entry point, in order (the stream follows): fields of the unit, or names _launch defines
_STEP_ARGS = {
    "hyb_adamw_step_dev": "n p grads m v numel hyper step counter ticket clip",
    "hyb_adamw_step_dev_ema": "n p grads m v ema numel hyper ema_hyper step counter ticket clip",
    "hyb_adamw_step_dev_acc": "n p grads m v acc ema numel hyper ema_hyper k step counter ticket clip",
    "hyb_adamw_step_dev_guard": "n p grads m v acc ema numel hyper ema_hyper k step counter ticket clip guard",
    "hyb_adamw_step_dev_groups": "n p grads m v acc ema numel group groups hyper ema_hyper k step counter ticket clip guard",
    "hyb_lamb_step_dev": "n p grads m v acc ema numel group groups hyper ema_hyper k step counter ticket clip guard trust",
    "hyb_lamb_trust": "n p grads m v acc numel group groups hyper k step counter clip guard always_adapt partials trust",
    "hyb_sgd_step_dev": "n p grads m acc ema numel group groups hyper ema_hyper k step counter ticket clip guard nesterov trust",
    "hyb_lars_trust": "n p grads acc numel group groups hyper k clip guard trust_coeff always_adapt partials trust",
}
_STEP_ARGS = {name: tuple(fields.split()) for name, fields in _STEP_ARGS.items()}


def _step_symbol(merged, guard, accum, ema):
    """The entry point of a device-path step: the first of merged / guarded / accumulating / averaging that holds names it (each of the
    earlier ones takes all the later ones' arguments)."""
    return "hyb_adamw_step_dev" + ("_groups" if merged else "_guard" if guard else "_acc" if accum else "_ema" if ema else "")


def _norm_symbol(guard, accum):
    return "hyb_grad_norm" + ("_acc" if accum else "") + ("_guard" if guard else "")


def _no_capture(what, remedy, why=""):
    """Device memory that must be zero (or hold a value) before its first captured use is created eagerly: a buffer born while its stream
    captures is written only by that one graph (a replay of another graph would meet whatever it held before), so that is refused."""
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError(f"HybridAdamW: {what} does not exist yet and cannot be created under stream capture {why}-- {remedy}")


class HybridAdamW(torch.optim.Optimizer):
    _STATE = ("exp_avg", "exp_avg_sq")     # the state tensors of the update rule, in the order of the unit's columns m, v (HybridSGD: one)

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None, ema_decay=None, ema_warmup=False,
                 accumulation_steps=1, skip_nonfinite=False, merge_groups=True):
        if lr < 0.0 or eps < 0.0 or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0 or weight_decay < 0.0:
            raise ValueError("invalid AdamW hyper-parameter")
        self._setup(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay), max_grad_norm, ema_decay, ema_warmup, accumulation_steps,
                    skip_nonfinite, merge_groups)

    def _setup(self, params, rule, max_grad_norm, ema_decay, ema_warmup, accumulation_steps, skip_nonfinite, merge_groups):
        """Everything of the constructor that does not depend on the update rule; `rule`: the rule's own (checked) group defaults."""
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError("max_grad_norm must be None (no clipping) or > 0")
        if ema_decay is not None and not 0.0 <= float(ema_decay) < 1.0:
            raise ValueError("ema_decay must be None (no average) or in [0, 1)")
        # three constructor arguments that are attributes -- neither a param-group key nor state (the accumulators are zero between steps;
        # merge_groups says which launches serve the groups, not what they compute); checked before the base class touches anything
        self._accum_k = self._checked("accumulation_steps", accumulation_steps)
        self._skip_nonfinite = self._checked("skip_nonfinite", skip_nonfinite)
        self._merge_groups = self._checked("merge_groups", merge_groups)
        self._guard = None           # device int64 [2]: skip_now (the last guarded step was skipped), skipped_total (since the last fold)
        # max_grad_norm sits in the groups only so that it travels in the state dict: clipping is global, every group carries the same value;
        # ema_decay / ema_warmup are per group (None: that group takes the launch without the average)
        super().__init__(params, dict(rule, max_grad_norm=max_grad_norm, ema_decay=ema_decay, ema_warmup=bool(ema_warmup)))
        self._tables = {}            # unit key -> the _Unit of step(), cached while the tensors' addresses stay
        self._step_counter = None    # device int64 [1]: the kernel uses step + counter (captured launches, graph.GraphedTrainStep)
        self._advance = False
        self._ticket = None          # device uint32 [1], this optimizer's own: the advancing launch counts its finished workgroups there
        self._dynamic = False        # set_dynamic_hyper(): take the device path even without clipping
        self._hyper = None           # device double [groups, 6]: lr, beta1, beta2, eps, weight_decay, max_grad_norm (0 = off) per group
        self._hyper_sent = {}        # per group: the values last uploaded (sync_hyper uploads on change only)
        self._norm_out = None        # device fp32 [2]: the last step's unclipped total gradient norm, its clip coefficient
        self._partials = None        # (numels, device fp32 [chunks], host numel array): hyb_grad_norm's per-chunk sums of squares
        self._ema_hyper = None       # device double [groups, 2]: ema_decay, ema_warmup (0 / 1) per group; created with _hyper
        self._ema_sent = {}          # per group: the (decay, warmup) last uploaded
        self._acc = {}               # parameter -> its fp32 gradient accumulator (16-byte aligned; zero at every optimizer-step boundary)
        self._acc_flat = []          # the flat buffers the accumulators created here are views of
        self._acc_tables = {}        # unit key -> the _Unit (parameters and accumulators only) of accumulate()
        self._acc_only = False       # _bind_accumulators(no_grad=True): the accumulators hold the whole sum, step() passes no gradients

    @staticmethod
    def _checked(name, value):
        """accumulation_steps: an int >= 1; skip_nonfinite, merge_groups: a bool."""
        if name == "accumulation_steps":
            if not isinstance(value, int) or isinstance(value, bool) or value < 1:
                raise ValueError("accumulation_steps must be an int >= 1")
        elif not isinstance(value, bool):
            raise ValueError(f"{name} must be a bool")
        return value

    accumulation_steps = property(lambda self: self._accum_k)
    skip_nonfinite = property(lambda self: self._skip_nonfinite)
    merge_groups = property(lambda self: self._merge_groups)

    def set_accumulation(self, k):
        """Micro-batches per optimizer step from now on (1: plain steps).  Change it only at an optimizer-step boundary: step() divides
        whatever the accumulators hold, plus the current gradients, by the k in force when it runs."""
        self._accum_k = self._checked("accumulation_steps", k)

    def set_skip_nonfinite(self, flag):
        """Switch the non-finite guard on or off between steps.  Switching folds the device's count of skipped steps first (fold_skipped():
        one host read), since only guarded launches subtract it from the step number."""
        if self._checked("skip_nonfinite", flag) != self._skip_nonfinite:
            self.fold_skipped()
            self._skip_nonfinite = flag

    def set_merge_groups(self, flag):
        """Switch the one-launch step over all parameter groups on or off between steps (the cached pointer tables go with it)."""
        if self._checked("merge_groups", flag) != self._merge_groups:
            self._merge_groups = flag
            self._tables.clear()
            self._acc_tables.clear()

    def _plan(self, stepped):
        """(merged, units) for the parameters for which stepped(p) holds.  A group with one is live; units lists what each library call
        serves as (table key, indices of its groups).  merged: ONE hyb_adamw_step_dev_groups call serves every live group (key "all") -- the
        device path, more than one live group, all of them with the average or all without, one step number, at most 255 groups;
        otherwise one call per live group (key: its index)."""
        groups = self.param_groups
        live = [gi for gi, g in enumerate(groups) if any(stepped(p) for p in g["params"])]
        merged = (self._merge_groups and len(groups) <= 255 and self.uses_device_hyper() and len(live) > 1
                  and len({self._group_ema(groups[gi]) is not None for gi in live}) == 1
                  and len({int(self.state.get(p, {}).get("step", 0)) for gi in live for p in groups[gi]["params"] if stepped(p)}) == 1)
        return merged, ([("all", live)] if merged else [(gi, [gi]) for gi in live])

    def merges_groups(self):
        """Whether step() will serve all parameter groups from one AdamW launch, judged by requires_grad (for a caller that captures
        step() before any gradient exists, GraphedTrainStep): an advancing step counter is then allowed with several groups."""
        return self._plan(lambda p: p.requires_grad)[0]

    def _device(self):
        dev = self.param_groups[0]["params"][0].device
        if dev.type != "cuda":
            raise RuntimeError("HybridAdamW: contiguous fp32 CUDA parameters only (no CPU fallback)")
        return dev

    def _guard_block(self):
        """The guard block, created and zeroed eagerly (_no_capture)."""
        if self._guard is None:
            _no_capture("the non-finite guard's device block", "call sync_hyper() (or take one eager step()) with skip_nonfinite on before capturing")
            self._guard = torch.zeros(2, dtype=torch.int64, device=self._device())
        return self._guard

    @property
    def skipped_steps(self):
        """Device int64 scalar: optimizer steps skipped by the guard since the last fold_skipped().  Reading it synchronises; holding it
        does not."""
        return self._guard_block()[1]

    @property
    def last_step_skipped(self):
        """Device int64 scalar, 0 or 1: whether the last guarded step was skipped."""
        return self._guard_block()[0]

    def _take_skipped(self):
        """The device's count of skipped steps, which is zeroed (one host read).  0 without a guard block."""
        if self._guard is None:
            return 0
        n = int(self._guard[1].item())
        if n:
            self._guard[1:].zero_()
        return n

    def fold_skipped(self):
        """Subtract the device's count of skipped steps from every stepped parameter's `step` and zero it: `step` then counts applied
        updates.  The step number the kernel forms (step - skipped) is the same before and after.  One host read.  Returns the count."""
        n = self._take_skipped()
        if n:
            for st in self.state.values():
                if "step" in st:
                    st["step"] = int(st["step"]) - n
        return n

    def state_dict(self):
        """(A guarded optimizer folds the skipped steps first: saved `step` values are applied-update counts, as torch.optim.AdamW's.)"""
        self.fold_skipped()
        return super().state_dict()

    def set_step_counter(self, counter, advance=False):
        """With a device counter the step number used by the kernel is state['step'] + counter, read on the device: one captured
        launch then serves every replay of a hipGraph.  advance=True: step() also adds 1 to the counter (inside the AdamW launch, after
        every workgroup has read it) -- the caller then needs no separate `counter += 1` launch; ONE call must then end the step: every
        parameter in one group, or several groups that step() merges (merges_groups())."""
        self._step_counter = counter
        self._advance = bool(advance) and counter is not None
        if self._advance and (self._ticket is None or self._ticket.device != counter.device):
            self._ticket = torch.zeros(1, dtype=torch.int32, device=counter.device)

    def set_dynamic_hyper(self, flag=True):
        """True: step() launches hyb_adamw_step_dev, which reads the hyper-parameters from device memory when it runs -- needed for a
        captured step that must follow a learning-rate schedule.  (With max_grad_norm set the device path is taken anyway.)"""
        self._dynamic = bool(flag)

    def uses_device_hyper(self):
        """(The average always takes the device path: its decay is read on the device, so a change between replays is picked up.)"""
        return self._dynamic or self._accum_k > 1 or self._skip_nonfinite or any(g.get("max_grad_norm") is not None or g.get("ema_decay") is not None for g in self.param_groups)

    @staticmethod
    def _group_ema(group):
        """None (no average; also a group loaded from a torch.optim.AdamW state dict, which lacks the key), or (decay, warmup as 0.0 / 1.0)."""
        d = group.get("ema_decay")
        if d is None:
            return None
        if not 0.0 <= float(d) < 1.0:
            raise ValueError("ema_decay must be None (no average) or in [0, 1)")
        return (float(d), 1.0 if group.get("ema_warmup") else 0.0)

    def _clip_value(self):
        vals = {None if g.get("max_grad_norm") is None else float(g["max_grad_norm"]) for g in self.param_groups}
        if len(vals) != 1:
            raise RuntimeError("HybridAdamW: clipping is global over all groups -- every param group must carry the same max_grad_norm")
        c = vals.pop()
        if c is not None and not c > 0.0:
            raise ValueError("max_grad_norm must be None (no clipping) or > 0")
        return c

    def _device_buffers(self):
        """The hyper blocks and norm_out, created and zeroed eagerly (_no_capture)."""
        if self._hyper is None or self._hyper.shape[0] != len(self.param_groups):
            _no_capture("the device hyper-parameter block", "call sync_hyper() (or take one eager step()) before capturing")
            dev = self._device()
            self._hyper = torch.zeros(len(self.param_groups), 6, dtype=torch.float64, device=dev)
            self._hyper_sent = {}
            self._ema_hyper = torch.zeros(len(self.param_groups), 2, dtype=torch.float64, device=dev)
            self._ema_sent = {}
            if self._norm_out is None or self._norm_out.device != dev:
                self._norm_out = torch.zeros(2, dtype=torch.float32, device=dev)
        if self._skip_nonfinite:
            self._guard_block()
        return self._hyper

    def _group_hyper(self, group):
        b1, b2 = group["betas"]
        c = group.get("max_grad_norm")             # (groups loaded from a torch.optim.AdamW state dict lack the key)
        return (float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]), 0.0 if c is None else float(c))

    def _by_value(self, group):
        """((name, value), ...): what a captured step launch of this group carries by value besides its hyper-parameters -- a change after
        capture cannot be followed, and GraphedTrainStep refuses it by name.  Nothing here (HybridSGD: nesterov)."""
        return ()

    def sync_hyper(self):
        """Upload every group's (lr, betas, eps, weight_decay, max_grad_norm), and (ema_decay, ema_warmup) where the group keeps an average,
        that differs from what the device holds (one tiny launch on the current stream for all changed groups, hyb_adamw_hyper_set_groups;
        the per-group calls where a single group changed, merge_groups is off or there are more than 255; the host never waits).  Must NOT be captured: the
        values travel as kernel arguments, a captured upload would put the capture-time values back at every replay."""
        hyper = self._device_buffers()
        changed = {gi: vals for gi, vals in enumerate(map(self._group_hyper, self.param_groups)) if self._hyper_sent.get(gi) != vals}
        ema_changed = {gi: ema for gi, ema in enumerate(map(self._group_ema, self.param_groups)) if ema is not None and self._ema_sent.get(gi) != ema}
        rows = sorted(changed.keys() | ema_changed.keys())
        if not rows:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("HybridAdamW.sync_hyper() under stream capture: upload the hyper-parameters before capturing")
        if self._merge_groups and len(rows) > 1 and len(self.param_groups) <= 255:
            lib.call("hyb_adamw_hyper_set_groups", hyper, self._ema_hyper, len(self.param_groups),
                     len(changed), (ctypes.c_ubyte * len(changed))(*changed), (ctypes.c_double * (6 * len(changed)))(*[v for vals in changed.values() for v in vals]),
                     len(ema_changed), (ctypes.c_ubyte * len(ema_changed))(*ema_changed),
                     (ctypes.c_double * (2 * len(ema_changed)))(*[v for ema in ema_changed.values() for v in ema]), _stream())
        else:
            for gi in rows:
                if gi in changed:
                    lib.call("hyb_adamw_hyper_set", hyper[gi], *changed[gi], _stream())
                if gi in ema_changed:
                    lib.call("hyb_adamw_ema_set", self._ema_hyper[gi], *ema_changed[gi], _stream())
        self._hyper_sent.update(changed)
        self._ema_sent.update(ema_changed)

    @property
    def grad_norm(self):
        """Device fp32 scalar: the unclipped total L2 norm of the last clipped step's gradients (what clip_grad_norm_ returns).  Reading it
        synchronises; holding it does not."""
        self._device_buffers()
        return self._norm_out[0]

    @property
    def clip_coef(self):
        """Device fp32 scalar: the coefficient the last clipped step multiplied its gradients by (1 = not clipped)."""
        self._device_buffers()
        return self._norm_out[1]

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._tables.clear()
        if self._guard is not None:                 # loaded `step` values are applied-update counts: nothing is left to subtract
            self._guard[1:].zero_()
        for st in self.state.values():              # torch casts loaded state to the parameter's dtype/device; keep the layout the kernel needs
            for k in self._STATE + ("ema",):
                if st.get(k) is not None:
                    st[k] = st[k].to(torch.float32).contiguous()
            if "step" in st and torch.is_tensor(st["step"]):
                st["step"] = int(st["step"].item())

    def _new_ema(self, p):
        if p.is_cuda:
            _no_capture("a parameter's weight average", "call ema_init() (or take one eager step()) before capturing")
        return p.detach().clone()

    @torch.no_grad()
    def ema_init(self):
        """Create the average of every parameter of every group with an ema_decay that has none yet, as a copy of the parameter's current
        value.  step() does the same for a parameter the first time it steps it (the value BEFORE that step, as a deep copy of the model
        taken before training); call this to start all averages at once, e.g. before capturing, or for parameters that get gradients later."""
        for group in self.param_groups:
            if group.get("ema_decay") is None:
                continue
            for p in group["params"]:
                st = self.state[p]
                if "ema" not in st:
                    st["ema"] = self._new_ema(p)

    def ema_model(self, model):
        """A twin of `model` (an nn.Module holding this optimizer's parameters) for evaluating the averaged weights while training goes on:
        a deep copy of the module structure in which
          * every parameter this optimizer averages IS its `state[p]["ema"]` tensor (same memory: nothing is copied, now or per use),
          * every other parameter is the live parameter's memory, and every buffer is the live model's buffer itself (BatchNorm running
            statistics are averages already, and always current),
          * every parameter has requires_grad=False.
        `twin.predict(x)` and `GraphedPredict(twin, x)` read whatever the averages hold when they run.  load_state_dict() replaces the
        state tensors: build a new twin after it.  Raises if an averaged parameter has no average yet (step() or ema_init() first)."""
        averaged = {}
        for group in self.param_groups:
            if group.get("ema_decay") is None:
                continue
            for p in group["params"]:
                e = self.state[p].get("ema") if p in self.state else None
                if e is None:
                    raise RuntimeError("HybridAdamW.ema_model: a parameter of a group with ema_decay has no average yet -- take a step() or "
                                       "call ema_init() first")
                averaged[id(p)] = e
        memo = {}
        for p in model.parameters():
            memo[id(p)] = torch.nn.Parameter(averaged.get(id(p), p.detach()), requires_grad=False)
        for b in model.buffers():
            memo[id(b)] = b
        return copy.deepcopy(model, memo)

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        if hasattr(self, "_tables"):
            self._tables.clear()
            self._acc_tables.clear()

    # ---- launch units -------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _unit(cache, key, first, params, layout=None, merged=False, **columns):
        """The _Unit of `params` with the given columns (p, m, v, ema, acc: one tensor per parameter, or None), from cache[key] if it is
        still valid -- every tensor of every column is where it was (load_state_dict() / a rollback replaces the moments and the averages
        with new allocations, the old ones may already be freed) and in the group it was in -- else built and cached (cache None: not kept)."""
        addrs = list(zip(*[[t.data_ptr() for t in col] for col in columns.values() if col is not None]))
        u = None if cache is None else cache.get(key)
        if u is None or u.addrs != addrs or u.layout != layout:
            arrays = dict.fromkeys(("p", "m", "v", "ema", "acc"))
            arrays.update((name, ptr_array([t.data_ptr() for t in col])) for name, col in columns.items() if col is not None)
            u = _Unit(key, first, params, layout, addrs, len(params), (ctypes.c_longlong * len(params))(*[p.numel() for p in params]),
                      group=(ctypes.c_ubyte * len(params))(*layout) if merged else None, **arrays)
            if cache is not None:
                cache[key] = u
        return u

    # ---- gradient accumulation --------------------------------------------------------------------------------------------------------
    def _new_accumulators(self, params):
        """Zeroed accumulators for `params`, views of ONE flat buffer, each starting on a multiple of 4 elements (16 bytes)."""
        if not params:
            return
        if params[0].is_cuda:
            _no_capture("a parameter's gradient accumulator", "call accum_init() before capturing",
                        "(it must be zero before the first micro-batch, and a buffer born in a capture is zeroed by that graph only) ")
        for p in params:
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                raise RuntimeError("HybridAdamW: contiguous fp32 CUDA parameters only (no CPU fallback)")
        offs, total = [], 0
        for p in params:
            offs.append(total)
            total += (p.numel() + 3) // 4 * 4
        flat = torch.zeros(max(total, 4), dtype=torch.float32, device=params[0].device)
        self._acc_flat.append(flat)
        for p, o in zip(params, offs):
            self._acc[p] = flat[o:o + p.numel()].view(p.shape)

    def _accumulators(self, params):
        self._new_accumulators([p for p in params if p not in self._acc])
        return [self._acc[p] for p in params]

    @torch.no_grad()
    def accum_init(self):
        """Create (zeroed) the accumulator of every parameter that has none yet.  accumulate() and step() do the same on first eager use;
        call this before capturing either, or to make the one allocation up front."""
        for group in self.param_groups:
            self._new_accumulators([p for p in group["params"] if p not in self._acc])

    def _bind_accumulators(self, params, tensors, no_grad=False):
        """(GraphedTrainStep.)  Use `tensors` -- fp32, contiguous, zero now, e.g. views of the data-parallel gradient buckets -- as the
        accumulators of `params`.  no_grad=True: whoever binds them adds EVERY micro-batch's gradient into them itself (and all-reduces
        them), so step() passes no gradient tensors and steps on acc * (1 / k); p.grad only says which parameters are stepped."""
        for p, t in zip(params, tensors):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != p.numel() or t.device != p.device:
                raise ValueError("HybridAdamW: an accumulator must be a contiguous fp32 tensor of its parameter's size, on its device")
            self._acc[p] = t
        self._acc_only = bool(no_grad)
        self._tables.clear()
        self._acc_tables.clear()

    def _accumulate_into(self, key, params, accs, keep=True):
        """accs[i] += params[i].grad in one hyb_grad_accumulate call, its table cached under `key` (keep=False: built for this call only)."""
        u = self._unit(self._acc_tables if keep else None, key, None, params, p=params, acc=accs)
        lib.call("hyb_grad_accumulate", u.n, u.acc, self._float_grads(params), u.numel, _stream())

    @torch.no_grad()
    def accumulate(self):
        """End one of the micro-batches 1 .. k - 1: acc += grad for every parameter with a gradient, one hyb_grad_accumulate launch per
        group, or one for all groups where step() merges them.  The gradients are only read (zero_grad() as usual before the next backward)."""
        if self._accum_k < 2:
            raise RuntimeError("HybridAdamW.accumulate() needs accumulation_steps > 1 (with 1, step() does not read the accumulators)")
        if self._acc_only:
            raise RuntimeError("HybridAdamW.accumulate(): the accumulators are bound to external buffers whose owner adds the gradients itself")
        for key, unit in self._plan(lambda p: p.grad is not None)[1]:
            ps = [p for gi in unit for p in self.param_groups[gi]["params"] if p.grad is not None]
            self._accumulate_into(key, ps, self._accumulators(ps))

    @staticmethod
    def _float_grads(ps):
        grads = []
        for p in ps:
            g = p.grad
            if g.dtype != torch.float32 or not g.is_contiguous():
                g = g.float().contiguous()
            grads.append(g)
        return grads

    # ---- the step -----------------------------------------------------------------------------------------------------------------------
    def _prepare(self, key, unit, merged):
        """One launch unit of step(): create what its parameters lack (accumulators, averages, moments), count the step, and return
        (its _Unit, its gradients or None, the step number the call takes, whether it keeps averages)."""
        ps, layout, ema = [], [], None
        for gi in unit:
            group = self.param_groups[gi]
            gps = [p for p in group["params"] if p.grad is not None]
            ema = self._group_ema(group)            # (merged: every group of the unit has one, or none has)
            ps += gps
            layout += [gi] * len(gps)
        accs = self._accumulators(ps) if self._accum_k > 1 else None     # (first: a refusal under capture leaves the step counts untouched)
        for p in ps:
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                raise RuntimeError("HybridAdamW: contiguous fp32 CUDA parameters only (no CPU fallback)")
            st = self.state[p]
            if ema is not None and "ema" not in st:
                st["ema"] = self._new_ema(p)         # the value before this step
            if self._STATE[0] not in st:             # (ema_init() may have left a state that holds the average only)
                st["step"] = 0
                for name in self._STATE:
                    st[name] = torch.zeros_like(p, memory_format=torch.preserve_format)
            if self._step_counter is None:
                st["step"] += 1
        # with a device counter the Python-side step stays put and the kernel uses (step + 1) + counter
        steps = {int(self.state[p]["step"]) + (1 if self._step_counter is not None else 0) for p in ps}
        if len(steps) != 1:
            raise RuntimeError("HybridAdamW: parameters of one group must share the step count")
        states = [self.state[p] for p in ps]
        m, v = ([st[name] for st in states] for name in self._STATE) if len(self._STATE) == 2 else ([st[self._STATE[0]] for st in states], None)
        u = self._unit(self._tables, key, unit[0], ps, layout, merged, p=ps, m=m, v=v,
                       ema=None if ema is None else [st["ema"] for st in states], acc=accs)
        return u, None if accs is not None and self._acc_only else self._float_grads(ps), steps.pop(), ema is not None

    def _norm(self, work, hyper, guard):
        """ONE norm over the gradients of all units, as clip_grad_norm_(model.parameters()) -- in an accumulated step over the mean of the k
        micro-batches' gradients; the guard takes its decision from it, so it runs without clipping too (hyper[5] == 0: coefficient 1)."""
        accum = self._accum_k > 1
        grads = None if accum and self._acc_only else [g for _, gs, _ in work for g in gs]
        numels = tuple(n for u, _, _ in work for n in u.numel)
        if self._partials is None or self._partials[0] != numels:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("HybridAdamW: the gradient-norm workspace cannot be created under stream capture -- take one eager "
                                   "step() with the same gradients first")
            arr = (ctypes.c_longlong * len(numels))(*numels)
            chunks = lib.query("hyb_grad_norm_workspace", len(numels), arr)
            self._partials = (numels, torch.zeros(chunks, dtype=torch.float32, device=hyper.device), arr)
        _, partials, numel = self._partials
        args = (ptr_array([a[-1] for u, _, _ in work for a in u.addrs]), grads, numel, self._accum_k) if accum else (grads, numel)
        lib.call(_norm_symbol(guard is not None, accum), len(numels), *args, partials, hyper[work[0][0].first], self._norm_out,
                 *(() if guard is None else (guard,)), _stream())
        return self._norm_out

    def _step_values(self, u, grads, step, hyper, clip, guard):
        """Every argument a device-path step call of the unit can take, by the names of _STEP_ARGS.  A merged call takes the blocks' bases,
        any other its group's rows."""
        ema_hyper = None if u.ema is None else self._ema_hyper
        vals = u._asdict()
        vals.update(grads=grads, groups=len(self.param_groups), k=self._accum_k, step=step, counter=self._step_counter,
                    ticket=self._ticket if self._advance else None, clip=clip, guard=guard, hyper=hyper if u.group is not None else hyper[u.first],
                    ema_hyper=ema_hyper if u.group is not None or ema_hyper is None else ema_hyper[u.first])
        return vals

    def _launch(self, u, grads, step, hyper, clip, guard):
        """The one AdamW call of a unit on the device path."""
        name = _step_symbol(u.group is not None, guard is not None, self._accum_k > 1, u.ema is not None)
        vals = self._step_values(u, grads, step, hyper, clip, guard)
        lib.call(name, *[vals[f] for f in _STEP_ARGS[name]], _stream())

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        # merged: one call ends the step, so the counter may advance with several groups
        merged, units = self._plan(lambda p: p.grad is not None)
        if self._advance and len(units) != 1:
            raise RuntimeError("HybridAdamW: an advancing step counter needs exactly one parameter group with gradients")
        guard = self._guard_block() if self._skip_nonfinite else None     # (first: a refusal under capture leaves the step counts untouched)
        work, ema_groups = [], []
        for key, unit in units:
            u, grads, step, ema = self._prepare(key, unit, merged)
            work.append((u, grads, step))
            ema_groups += unit if ema else []
        if not self.uses_device_hyper():
            for u, grads, step in work:
                lr, b1, b2, eps, wd, _ = self._group_hyper(self.param_groups[u.first])
                lib.call("hyb_adamw_step", u.n, u.p, grads, u.m, u.v, u.numel, lr, b1, b2, eps, wd, step, self._step_counter,
                         self._ticket if self._advance else None, _stream())
            return loss
        # ---- device path: hyper-parameters (and the clip coefficient) are read from device memory by the launches themselves ----
        clip = self._clip_value()
        hyper = self._device_buffers()
        if torch.cuda.is_current_stream_capturing():
            # only the norm and the AdamW calls are recorded; the upload is the replaying caller's (GraphedTrainStep.step)
            if len(self._hyper_sent) != len(self.param_groups) or any(gi not in self._ema_sent for gi in ema_groups):
                raise RuntimeError("HybridAdamW: hyper-parameters were never uploaded -- call sync_hyper() before capturing step()")
        else:
            self.sync_hyper()
        if not work:
            return loss
        clip_coef = self._norm(work, hyper, guard) if clip is not None or guard is not None else None
        for u, grads, step in work:
            self._launch(u, grads, step, hyper, clip_coef, guard)
        return loss


class HybridLAMB(HybridAdamW):
    """LAMB (You et al., 2020; timm's Lamb, apex's FusedLAMB without nvlamb) on HybridAdamW's device path: per tensor the Adam update
    u = m_hat / (sqrt(v_hat) + eps) + weight_decay * p is scaled by the trust ratio r = |p| / |u| (1 where either norm is zero, and for a
    tensor whose group has weight_decay == 0 unless always_adapt), p <- p - lr * r * u.  That is the AdamW step of the tensor at the rate
    r * lr, so a step is the existing norm call (when clipping or guarding), ONE read-only launch pair that forms every tensor's ratio on
    the device (hyb_lamb_trust: the moments as the step will form them, bit-reproducible sums) and the AdamW launch reading the ratios
    (hyb_lamb_step_dev) -- per launch unit, whatever the number of tensors, with no host read: it works under GraphedTrainStep with
    everything HybridAdamW offers there (clipping, schedules, the average, accumulation, the guard, merged groups, data parallelism).

    Defaults as timm: eps 1e-6, weight_decay 1e-2, max_grad_norm 1.0 (None: no clipping).  State-dict keys are HybridAdamW's, so
    checkpoints interchange with it and with torch.optim.AdamW.  always_adapt is an attribute fixed at construction (it travels by value
    in the captured launch).  `trust_ratios()` gives the last step's {|p|, |u|, r} per parameter as device tensors.  weight_decay is read
    on the device: setting a group's weight_decay to 0 between replays stops adapting its tensors without a recapture."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=1e-2, always_adapt=False, max_grad_norm=1.0, ema_decay=None,
                 ema_warmup=False, accumulation_steps=1, skip_nonfinite=False, merge_groups=True):
        if not isinstance(always_adapt, bool):
            raise ValueError("always_adapt must be a bool")
        self._always_adapt = always_adapt
        self._trust = {}             # unit key -> (numels, device fp32 [2 * chunks], device fp32 [n, 3], the unit's parameters)
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm, ema_decay=ema_decay,
                         ema_warmup=ema_warmup, accumulation_steps=accumulation_steps, skip_nonfinite=skip_nonfinite, merge_groups=merge_groups)

    always_adapt = property(lambda self: self._always_adapt)
    _TRUST_WORKSPACE = "hyb_lamb_trust_workspace"

    def uses_device_hyper(self):
        """Always: the ratios are formed and read on the device (there is no by-value LAMB)."""
        return True

    def _trust_workspace(self, u):
        """The unit's partial sums and trust block, created eagerly (_no_capture) and kept while the unit serves the same tensor sizes."""
        numels = tuple(u.numel)
        w = self._trust.get(u.key)
        if w is None or w[0] != numels:
            _no_capture("the trust-ratio workspace", "take one eager step() with the same gradients first")
            dev = self._device()
            floats = lib.query(self._TRUST_WORKSPACE, u.n, u.numel)
            w = self._trust[u.key] = (numels, torch.zeros(floats, dtype=torch.float32, device=dev), torch.ones(u.n, 3, dtype=torch.float32, device=dev),
                                      u.params)
        elif w[3] is not u.params:                  # (the same sizes behind other tensors: the rows now speak of these)
            w = self._trust[u.key] = w[:3] + (u.params,)
        return w[1], w[2]

    def trust_ratios(self):
        """{parameter: device fp32 tensor [3] = (|p|, |u|, r)} of the last step, for every parameter that step served: views of the blocks
        the launches write, no host read.  After a step the guard skipped, the contents are unspecified."""
        return {p: block[i] for _, _, block, params in self._trust.values() for i, p in enumerate(params)}

    def _launch(self, u, grads, step, hyper, clip, guard):
        """The trust pass and the step that reads it: two calls per unit."""
        partials, trust = self._trust_workspace(u)
        vals = self._step_values(u, grads, step, hyper, clip, guard)
        vals.update(always_adapt=int(self._always_adapt), partials=partials, trust=trust)
        for name in ("hyb_lamb_trust", "hyb_lamb_step_dev"):
            lib.call(name, *[vals[f] for f in _STEP_ARGS[name]], _stream())


class HybridSGD(HybridAdamW):
    """SGD with momentum -- torch.optim.SGD's rule: coupled L2 weight decay, dampening, Nesterov; maximize off -- on HybridAdamW's device
    path (hyb_sgd_step_dev): per element d = g + weight_decay * p, buf <- d at the first step and momentum * buf + (1 - dampening) * d
    after it, p <- p - lr * (d + momentum * buf if nesterov else buf).  One launch per unit with one state tensor per parameter: 5 x 4
    bytes per parameter where the AdamW launch moves 7 x 4.  It always takes the device path (there is no by-value SGD launch), so it
    works under GraphedTrainStep with everything HybridAdamW offers there: clipping, schedules of lr / momentum / dampening / weight_decay
    between replays, the weight average, accumulation, the non-finite guard, merged groups, data parallelism.

    State keys are torch's `momentum_buffer` plus `step` (which says whether the buffer has been started), so checkpoints interchange with
    torch.optim.SGD: a loaded state with a buffer and no `step` gets step = 1, so that the buffer is used.  With momentum == 0 the buffer
    is still kept (torch keeps none): it is harmless -- it holds (1 - dampening) * d and never reaches p, the step is on d itself as
    in torch -- and the parameter values are torch's.  `nesterov` is a group key so that it travels in the state dict, and like max_grad_norm it must be equal in all groups: it
    travels by value in the captured launch, and GraphedTrainStep refuses a change after capture."""
    _STATE = ("momentum_buffer",)

    def __init__(self, params, lr, momentum=0.9, dampening=0.0, weight_decay=0.0, nesterov=False, max_grad_norm=None, ema_decay=None,
                 ema_warmup=False, accumulation_steps=1, skip_nonfinite=False, merge_groups=True):
        self._setup(params, self._sgd_rule(lr, momentum, dampening, weight_decay, nesterov), max_grad_norm, ema_decay, ema_warmup,
                    accumulation_steps, skip_nonfinite, merge_groups)

    @staticmethod
    def _sgd_rule(lr, momentum, dampening, weight_decay, nesterov):
        if lr < 0.0 or not 0.0 <= momentum < 1.0 or not 0.0 <= dampening < 1.0 or weight_decay < 0.0:
            raise ValueError("invalid SGD hyper-parameter")
        if not isinstance(nesterov, bool):
            raise ValueError("nesterov must be a bool")
        if nesterov and (momentum <= 0.0 or dampening != 0.0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        return dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov)

    def uses_device_hyper(self):
        """Always: there is no by-value SGD launch."""
        return True

    def _group_hyper(self, group):
        """The group's row of the device block: {lr, momentum, dampening, lars_eps, weight_decay, max_grad_norm}."""
        c = group.get("max_grad_norm")             # (groups loaded from a torch.optim.SGD state dict lack the key)
        return (float(group["lr"]), float(group["momentum"]), float(group["dampening"]), float(group.get("eps", 0.0)), float(group["weight_decay"]),
                0.0 if c is None else float(c))

    def _by_value(self, group):
        return (("nesterov", bool(group.get("nesterov", False))),)

    def _nesterov_value(self):
        vals = {bool(g.get("nesterov", False)) for g in self.param_groups}
        if len(vals) != 1:
            raise RuntimeError("HybridSGD: nesterov travels by value in the launch -- every param group must carry the same nesterov")
        nesterov = vals.pop()
        if nesterov and any(float(g["momentum"]) <= 0.0 or float(g["dampening"]) != 0.0 for g in self.param_groups):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        return nesterov

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for st in self.state.values():
            if st.get("momentum_buffer") is None:
                st.pop("momentum_buffer", None)     # (as after ema_init(): the buffer is created, and started, by the next step)
            elif "step" not in st:
                st["step"] = 1                       # torch.optim.SGD's state: the buffer has been started

    def _sgd_values(self, u, grads, step, hyper, clip, guard):
        vals = self._step_values(u, grads, step, hyper, clip, guard)
        vals.update(nesterov=int(self._nesterov_value()), trust=None)
        return vals

    def _launch(self, u, grads, step, hyper, clip, guard):
        """The one SGD call of a unit."""
        vals = self._sgd_values(u, grads, step, hyper, clip, guard)
        lib.call("hyb_sgd_step_dev", *[vals[f] for f in _STEP_ARGS["hyb_sgd_step_dev"]], _stream())


class HybridLARS(HybridSGD):
    """LARS (You et al., 2017; timm's Lars with trust_clip=False) on HybridSGD's launch: per tensor the decayed gradient d = g + weight_decay * p
    is scaled by the trust ratio r = trust_coeff * |p| / (|g| + weight_decay * |p| + eps) -- 1 where either norm is zero, and for a tensor
    whose group has weight_decay == 0 unless always_adapt -- and then takes HybridSGD's momentum step.  g is the effective gradient: the
    mean over an accumulated step, after clipping.  A step is the existing norm call (when clipping or guarding), ONE read-only launch pair
    that forms every tensor's ratio on the device (hyb_lars_trust, bit-reproducible sums) and the SGD launch reading the ratios, per launch
    unit, with no host read: everything HybridSGD offers under GraphedTrainStep holds.  weight_decay and eps are read on the device;
    trust_coeff and always_adapt are attributes fixed at construction (they travel by value in the captured launch).  `trust_ratios()`
    gives the last step's (|p|, |g|, r) per parameter as device tensors.  With weight_decay == 0 everywhere (and always_adapt off) every
    ratio is 1 and the step is HybridSGD's bit for bit."""
    _TRUST_WORKSPACE = "hyb_lars_trust_workspace"

    def __init__(self, params, lr, momentum=0.9, weight_decay=1e-4, nesterov=False, trust_coeff=1e-3, eps=1e-8, always_adapt=False, dampening=0.0,
                 max_grad_norm=None, ema_decay=None, ema_warmup=False, accumulation_steps=1, skip_nonfinite=False, merge_groups=True):
        if not isinstance(always_adapt, bool):
            raise ValueError("always_adapt must be a bool")
        if isinstance(trust_coeff, bool) or not 0.0 < float(trust_coeff) < float("inf") or eps < 0.0:
            raise ValueError("invalid LARS hyper-parameter")
        self._always_adapt, self._trust_coeff = always_adapt, float(trust_coeff)
        self._trust = {}             # unit key -> (numels, device fp32 [2 * chunks], device fp32 [n, 3], the unit's parameters)
        self._setup(params, dict(self._sgd_rule(lr, momentum, dampening, weight_decay, nesterov), eps=eps), max_grad_norm, ema_decay, ema_warmup,
                    accumulation_steps, skip_nonfinite, merge_groups)

    always_adapt = property(lambda self: self._always_adapt)
    trust_coeff = property(lambda self: self._trust_coeff)
    _trust_workspace = HybridLAMB._trust_workspace
    trust_ratios = HybridLAMB.trust_ratios

    def _launch(self, u, grads, step, hyper, clip, guard):
        """The trust pass and the step that reads it: two calls per unit."""
        partials, trust = self._trust_workspace(u)
        vals = self._sgd_values(u, grads, step, hyper, clip, guard)
        vals.update(trust_coeff=self._trust_coeff, always_adapt=int(self._always_adapt), partials=partials, trust=trust)
        for name in ("hyb_lars_trust", "hyb_sgd_step_dev"):
            lib.call(name, *[vals[f] for f in _STEP_ARGS[name]], _stream())
