"""One AdamW launch for all parameter groups (HybridAdamW(merge_groups=True), hyb_adamw_step_dev_groups): bit for bit the per-group launches
in every variant of the device path, torch.optim.AdamW's result within the device path's bounds, the launches a step / an upload / an
accumulate makes, the advancing step counter over several groups and more than one tensor table, the cases that keep the per-group
launches, and GraphedTrainStep replaying TransformerCNNHybrid.param_groups with and without merging.

Three groups whose hyper-parameters differ grossly (a tensor served with another group's row cannot hide), over the smallest tensor sizes
at which the kernel takes each of its paths: 1, 3, 4 (the 16-byte tail and below), 4095 / 4096 / 4097 (around one 4096-element chunk),
2 * 4096 + 5 (several chunks and a tail) and a 1025-element view at a 4-byte offset (the element-wise path); the first group ends with the
4096-element tensor, so a group boundary coincides with a chunk boundary."""
import ctypes
import warnings

import pytest
import torch

from test_gpu_clip_lr import _sched_step, _setup, _warmup_lambda

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 4095, 4096, 4097, 2 * 4096 + 5]
LAYOUT = [5, 2, 1]                                   # tensors per group: {1, 3, 4, 4095, 4096}, {4097, 8197}, {the misaligned view}
HYPER = [dict(lr=1e-3, weight_decay=0.0, betas=(0.9, 0.999), eps=1e-8),
         dict(lr=1e-1, weight_decay=0.5, betas=(0.8, 0.95), eps=1e-6),
         dict(lr=3e-2, weight_decay=1e-2, betas=(0.5, 0.9), eps=1e-3)]
PER_GROUP = ("hyb_adamw_step", "hyb_adamw_step_dev", "hyb_adamw_step_dev_ema", "hyb_adamw_step_dev_acc", "hyb_adamw_step_dev_guard")
VARIANTS = {"dynamic": {}, "clip": dict(max_grad_norm=1.0), "ema": dict(ema_decay=0.9, ema_warmup=True), "accum": dict(accumulation_steps=2),
            "guard": dict(skip_nonfinite=True),
            "all": dict(max_grad_norm=1.0, ema_decay=0.9, ema_warmup=True, accumulation_steps=2, skip_nonfinite=True)}


def P():
    import transformer_cnn_hybrid_network_for_video_processing_amd as pkg
    return pkg


def _lib():
    from transformer_cnn_hybrid_network_for_video_processing_amd._lib import lib
    return lib


def _init(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) for n in SIZES] + [torch.randn(1030, generator=g)]


def _params(init):
    """Fresh parameters holding `init`; the last one is a 1025-element view one element into its buffer: 4-byte aligned only."""
    ps = [torch.nn.Parameter(t.clone().cuda()) for t in init[:-1]]
    ps.append(torch.nn.Parameter(init[-1].clone().cuda()[1:1026]))
    assert ps[-1].data_ptr() % 16 == 4 and all(p.data_ptr() % 16 == 0 for p in ps[:-1])
    return ps


def _groups(ps, layout=LAYOUT, extra=()):
    groups, first = [], 0
    for i, n in enumerate(layout):
        groups.append(dict(params=ps[first:first + n], **HYPER[i], **(extra[i] if extra else {})))
        first += n
    assert first == len(ps)
    return groups


def _opt(ps, merge, layout=LAYOUT, **kw):
    opt = P().HybridAdamW(_groups(ps, layout), merge_groups=merge, **kw)
    opt.set_dynamic_hyper(True)
    return opt


def _grads(ps, gen, poison=False):
    gs = [torch.randn(p.shape, generator=gen).cuda() for p in ps]
    if poison:
        gs[5][10] = float("nan")                     # in the second group's first tensor
    return gs


def _bind(ps, gs):
    for p, g in zip(ps, gs):
        p.grad = g


def _state(ps, opt):
    out = []
    for p in ps:
        st = opt.state[p]
        out.append([p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()] + ([st["ema"].clone()] if "ema" in st else [])
                   + ([opt._acc[p].clone()] if p in opt._acc else []))
    return out


def _assert_same(a, b, tag):
    assert len(a) == len(b)
    for i, (ta, tb) in enumerate(zip(a, b)):
        assert len(ta) == len(tb), (tag, i)
        for j, (x, y) in enumerate(zip(ta, tb)):
            assert torch.equal(x, y), (tag, "tensor", i, "entry (p, exp_avg, exp_avg_sq, then ema / acc where kept)", j)


class Recorder:
    """Records the entry-point name of every lib.call (which it passes on)."""

    def __init__(self, monkeypatch):
        lib = _lib()
        self.names, real = [], lib.call

        def call(name, *args):
            self.names.append(name)
            return real(name, *args)
        monkeypatch.setattr(lib, "call", call)

    def take(self):
        names, self.names = self.names, []
        return names


# ---- 1. merged == per group, bit for bit ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_merged_step_equals_the_per_group_launches_bit_for_bit(variant, monkeypatch):
    kw = VARIANTS[variant]
    k = kw.get("accumulation_steps", 1)
    guarded = kw.get("skip_nonfinite", False)
    init = _init(1)
    a, b = _params(init), _params(init)
    oa, ob = _opt(a, True, **kw), _opt(b, False, **kw)
    assert oa.merges_groups() and not ob.merges_groups()
    rec = Recorder(monkeypatch)
    gen = torch.Generator().manual_seed(2)
    for s in range(4):
        poison = guarded and s == 2                  # one NaN step in the middle
        before = (_state(a, oa), _state(b, ob)) if poison else None
        for j in range(k):
            gs = _grads(a, gen, poison and j == k - 1)
            _bind(a, gs); _bind(b, gs)               # (shared: the launches only read them)
            if j < k - 1:
                oa.accumulate(); ob.accumulate()
                for i, (pa, pb) in enumerate(zip(a, b)):
                    assert torch.equal(oa._acc[pa], ob._acc[pb]) and bool(oa._acc[pa].any()), (variant, s, "accumulator", i)
            else:
                oa.step(); ob.step()
        _assert_same(_state(a, oa), _state(b, ob), (variant, "step", s))
        if poison:                                   # nothing moved (the accumulators were zero at the boundary before, and are zero again)
            assert int(oa.last_step_skipped.item()) == 1 and int(ob.last_step_skipped.item()) == 1
            _assert_same(before[0], _state(a, oa), (variant, "skipped step, merged"))
            _assert_same(before[1], _state(b, ob), (variant, "skipped step, per group"))
        if "max_grad_norm" in kw and not poison:
            assert torch.equal(oa._norm_out, ob._norm_out) and oa.clip_coef.item() < 1.0        # clipping was active
    names = rec.take()
    assert names.count("hyb_adamw_step_dev_groups") == 4 and "hyb_adamw_step_dev_groups" in names        # the merged optimizer did merge
    assert sum(names.count(n) for n in PER_GROUP) == 4 * len(LAYOUT)                                    # and the other one did not
    if guarded:
        assert int(oa.skipped_steps.item()) == 1 and int(ob.skipped_steps.item()) == 1
    if k > 1:
        assert all(not bool(oa._acc[p].any()) for p in a)                                               # zero at the step boundary
    if "ema_decay" in kw:
        assert all(not torch.equal(oa.state[p]["ema"], p) for p in a[3:])                              # the average is a thing of its own


# ---- 2. against torch.optim.AdamW ---------------------------------------------------------------------------------------------------------------
def test_merged_step_against_torch_adamw():
    """rtol 2e-6, atol 2e-7: the bounds tests/test_gpu_optim.py uses for the device-formed bias corrections over 3 steps."""
    init = _init(3)
    a, b = _params(init), _params(init)
    ot = torch.optim.AdamW(_groups(a))
    oh = _opt(b, True)
    assert oh.merges_groups()
    gen = torch.Generator().manual_seed(4)
    for s in range(3):
        gs = _grads(a, gen)
        _bind(a, gs); _bind(b, [g.clone() for g in gs])
        ot.step(); oh.step()
        for i, (pa, pb) in enumerate(zip(a, b)):
            err = (pb.data - pa.data).abs().max().item()
            print(f"step {s} tensor {i} ({pa.numel()} elements): max |hip - torch| {err:.3e}")
            torch.testing.assert_close(pb.data, pa.data, rtol=2e-6, atol=2e-7)
    # the three groups did get three different updates: the first tensors of the groups moved by about their own rates
    moved = [(b[i].data - init_i.cuda().view_as(b[i])).abs().mean().item() for i, init_i in ((3, init[3]), (5, init[5]))]
    assert moved[1] > 20 * moved[0], moved


# ---- 3. the launches ------------------------------------------------------------------------------------------------------------------------------
def test_launch_shape(monkeypatch):
    init = _init(5)
    gen = torch.Generator().manual_seed(6)
    for merge in (True, False):
        ps = _params(init)
        opt = _opt(ps, merge, accumulation_steps=2)
        rec = Recorder(monkeypatch)
        _bind(ps, _grads(ps, gen))
        opt.accumulate()
        names = rec.take()
        assert names.count("hyb_grad_accumulate") == (1 if merge else 3) and len(names) == names.count("hyb_grad_accumulate"), names
        _bind(ps, _grads(ps, gen))
        opt.step()                                   # the first step also uploads every group's hyper-parameters
        names = rec.take()
        if merge:
            assert names == ["hyb_adamw_hyper_set_groups", "hyb_adamw_step_dev_groups"], names
        else:
            assert names == ["hyb_adamw_hyper_set"] * 3 + ["hyb_adamw_step_dev_acc"] * 3, names
        opt.sync_hyper()
        assert rec.take() == []                      # nothing changed
        for g in opt.param_groups:
            g["lr"] *= 0.5
        opt.sync_hyper()
        names = rec.take()
        assert names == (["hyb_adamw_hyper_set_groups"] if merge else ["hyb_adamw_hyper_set"] * 3), names
        torch.cuda.synchronize()
        want = torch.tensor([[h["lr"] * 0.5, h["betas"][0], h["betas"][1], h["eps"], h["weight_decay"], 0.0] for h in HYPER], dtype=torch.float64)
        assert torch.equal(opt._hyper.cpu(), want)   # every row holds its own group's values
        opt.param_groups[1]["lr"] = 0.25             # a single changed group keeps the per-group call
        opt.sync_hyper()
        assert rec.take() == ["hyb_adamw_hyper_set"]
        assert opt._hyper[1, 0].item() == 0.25
        monkeypatch.undo()
    # the average's rows travel in the same upload
    ps = _params(init)
    opt = P().HybridAdamW(_groups(ps, extra=[dict(ema_decay=0.5), dict(ema_decay=0.9, ema_warmup=True), dict(ema_decay=0.0)]))
    rec = Recorder(monkeypatch)
    opt.sync_hyper()
    assert rec.take() == ["hyb_adamw_hyper_set_groups"]
    assert torch.equal(opt._ema_hyper.cpu(), torch.tensor([[0.5, 0.0], [0.9, 1.0], [0.0, 0.0]], dtype=torch.float64))


# ---- 4. the advancing counter -----------------------------------------------------------------------------------------------------------------------
def _hundred(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(int(n), generator=g) for n in torch.randint(1, 5000, (100,), generator=g)]


@pytest.mark.parametrize("which", ["sizes", "hundred"])
def test_advancing_counter_with_several_groups(which):
    """The merged call ends the step, so it may advance the counter.  "hundred": 100 tensors in groups of 30 / 55 / 15 are two tensor tables
    (80 + 20, the second group on both): both launches read the same step number, only the last one advances."""
    if which == "sizes":
        init, layout = _init(7), LAYOUT
        a, b = _params(init), _params(init)
    else:
        init, layout = _hundred(7), [30, 55, 15]
        a, b = ([torch.nn.Parameter(t.clone().cuda()) for t in init] for _ in range(2))
    oa, ob = _opt(a, True, layout), _opt(b, False, layout)
    ca, cb = (torch.zeros(1, dtype=torch.int64, device="cuda") for _ in range(2))
    oa.set_step_counter(ca, advance=True)
    ob.set_step_counter(cb)                          # per-group launches cannot advance it: the host adds
    gen = torch.Generator().manual_seed(8)
    for s in range(3):
        gs = [torch.randn(p.shape, generator=gen).cuda() for p in a]
        _bind(a, gs); _bind(b, gs)
        oa.step(); ob.step()
        cb.add_(1)
        assert int(ca.item()) == s + 1
        assert int(oa._ticket.item()) == 0           # the ticket word is back at rest
        _assert_same(_state(a, oa), _state(b, ob), (which, s))
    assert all(int(oa.state[p]["step"]) == 0 for p in a)      # the Python-side step stays put with a device counter


# ---- 5. what keeps the per-group launches -------------------------------------------------------------------------------------------------------------
def test_fallbacks(monkeypatch):
    init = _init(9)
    gen = torch.Generator().manual_seed(10)
    # groups that disagree on keeping an average: per-group launches, and no advancing counter
    ps = _params(init)
    opt = P().HybridAdamW(_groups(ps, extra=[dict(ema_decay=0.9), {}, {}]))
    assert opt.uses_device_hyper() and not opt.merges_groups()
    rec = Recorder(monkeypatch)
    _bind(ps, _grads(ps, gen))
    opt.step()
    names = rec.take()
    assert "hyb_adamw_step_dev_groups" not in names
    assert [n for n in names if n in PER_GROUP] == ["hyb_adamw_step_dev_ema", "hyb_adamw_step_dev", "hyb_adamw_step_dev"], names
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    opt.set_step_counter(counter, advance=True)
    with pytest.raises(RuntimeError, match="one parameter group"):
        opt.step()
    # the by-value path: untouched
    ps = _params(init)
    plain = P().HybridAdamW(_groups(ps))
    assert not plain.uses_device_hyper() and not plain.merges_groups()
    _bind(ps, _grads(ps, gen))
    plain.step()
    assert rec.take() == ["hyb_adamw_step"] * 3
    plain.set_step_counter(counter, advance=True)
    with pytest.raises(RuntimeError, match="one parameter group"):
        plain.step()
    # groups that do not share the step number (one of them joined later)
    ps = _params(init)
    late = _opt(ps, True)
    _bind(ps[:5], _grads(ps, gen)[:5])               # only the first group has gradients: one live group, today's launch
    late.step()
    assert [n for n in rec.take() if n in PER_GROUP + ("hyb_adamw_step_dev_groups",)] == ["hyb_adamw_step_dev"]
    _bind(ps, _grads(ps, gen))
    late.step()                                      # steps 2, 1, 1
    assert [n for n in rec.take() if n in PER_GROUP + ("hyb_adamw_step_dev_groups",)] == ["hyb_adamw_step_dev"] * 3
    assert int(counter.item()) == 0 and torch.isfinite(torch.cat([p.detach().flatten() for p in ps])).all()


def test_c_abi_argument_checks():
    lib = _lib()
    ps = [torch.zeros(8, device="cuda") for _ in range(2)]
    gs, ms, vs = ([torch.zeros(8, device="cuda") for _ in range(2)] for _ in range(3))
    numel = (ctypes.c_longlong * 2)(8, 8)
    hyper = torch.zeros(2, 6, dtype=torch.float64, device="cuda")
    ema_hyper = torch.zeros(2, 2, dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    row = [1e-3, 0.9, 0.999, 1e-8, 1e-2, 0.0]

    def step(group, groups, k=1, step_no=1, grads=gs, ema=None, ema_h=None, clip=None, guard=None):
        lib.call("hyb_adamw_step_dev_groups", 2, ps, grads, ms, vs, None, ema, numel, (ctypes.c_ubyte * 2)(*group), groups, hyper, ema_h, k, step_no, None,
                 None, clip, guard, stream)

    def upload(groups, idx, rows, ema_idx=(), ema_rows=()):
        lib.call("hyb_adamw_hyper_set_groups", hyper, ema_hyper, groups, len(idx), (ctypes.c_ubyte * len(idx))(*idx),
                 (ctypes.c_double * (6 * len(idx)))(*[v for r in rows for v in r]), len(ema_idx), (ctypes.c_ubyte * len(ema_idx))(*ema_idx),
                 (ctypes.c_double * (2 * len(ema_idx)))(*[v for r in ema_rows for v in r]), stream)
    upload(2, [0, 1], [row, row])
    step([0, 1], 2)                                  # a good call
    for bad in (lambda: step([0, 2], 2),             # a group index that is not below the group count
                lambda: step([0, 1], 256),           # more than 255 groups
                lambda: step([0, 1], 0),
                lambda: step([0, 1], 2, k=2),        # k > 1 without accumulators
                lambda: step([0, 1], 2, step_no=0),
                lambda: step([0, 1], 2, grads=None),
                lambda: step([0, 1], 2, ema=ms),     # the average without its hyper block
                lambda: step([0, 1], 2, guard=torch.zeros(2, dtype=torch.int64, device="cuda")),       # the guard without the norm's output
                lambda: upload(2, [0, 2], [row, row]),
                lambda: upload(2, [1, 1], [row, row]),           # a group listed twice
                lambda: upload(256, [0], [row]),
                lambda: upload(2, [], []),                        # nothing to write
                lambda: upload(2, [0], [[1e-3, 1.0, 0.999, 1e-8, 1e-2, 0.0]]),                           # beta1 = 1
                lambda: upload(2, [], [], [0], [[1.0, 0.0]])):                                           # decay = 1
        with pytest.raises(RuntimeError, match="argument check"):
            bad()
    torch.cuda.synchronize()
    assert torch.equal(hyper.cpu(), torch.tensor([row, row], dtype=torch.float64))


# ---- 6. under replay ------------------------------------------------------------------------------------------------------------------------------------
def test_replay_with_layerwise_groups_merged_equals_per_group():
    """TransformerCNNHybrid.param_groups(layer_decay=0.75) under GraphedTrainStep with a LambdaLR warm-up that moves every group's rate before
    every replay: the merged step (one AdamW launch, which also advances the counter) against the per-group one (a launch per group and a
    counter launch) -- the same losses as Python floats, every parameter bit for bit, the same counter."""
    runs = {}
    for merge in (True, False):
        m, x, y = _setup()
        groups = m.param_groups(lr=1e-3, layer_decay=0.75)
        assert len(groups) == 2 * (2 + 1 + 2 + 1)    # KW: two conv stages, the token projection, two encoder layers, the head
        opt = P().HybridAdamW(groups, merge_groups=merge)
        sched = torch.optim.lr_scheduler.LambdaLR(opt, _warmup_lambda)
        tr = P().GraphedTrainStep(m, P().HybridCrossEntropyLoss(), opt, x, y, warmup=2, dynamic_hyper=True)
        try:
            assert tr._advancing is merge and opt.merges_groups() is merge
            losses, rates = [], []
            for _ in range(4):
                losses.append(tr.step().item())
                rates.append([g["lr"] for g in opt.param_groups])
                _sched_step(sched)
            torch.cuda.synchronize()
            assert all(len({r[i] for r in rates}) == 4 for i in range(len(groups)))         # every group's rate moved on every step
            runs[merge] = (losses, [p.detach().clone() for p in m.parameters()], int(tr.counter.item()), [n for n, _ in m.named_parameters()])
            opt.set_merge_groups(not merge)
            with pytest.raises(RuntimeError, match="merge_groups was switched on or off after capture"):
                tr.step()
            opt.set_merge_groups(merge)
        finally:
            tr.close()
    (la, pa, ca, names), (lb, pb, cb, _) = runs[True], runs[False]
    assert la == lb, (la, lb)
    assert ca == cb == 2 + 4
    for n, a, b in zip(names, pa, pb):
        assert torch.equal(a, b), n
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert all(torch.isfinite(p).all() for p in pa)
