"""TransformerCNNHybrid.param_groups -- no weight decay on 1-d parameters, a learning rate that decays layer by layer towards the input --
and HybridAdamW's merge_groups attribute, as far as they go without a GPU."""
import pytest
import torch

import transformer_cnn_hybrid_network_for_video_processing_amd as P
from test_dp_gloo import KW


def _model():
    torch.manual_seed(0)
    return P.TransformerCNNHybrid(**KW)


def _depths(model):
    """parameter id -> depth, written out from the module names: conv stage i, then the token projection, then the encoder layers, then the head."""
    S, L = len(KW["cnn_channels"]), KW["num_layers"]
    depth = {}
    for name, p in model.named_parameters():
        part = name.split(".")
        if part[0].startswith("encoder") and part[0] != "encoder":
            d = int(part[0][len("encoder"):]) - 1
        elif part[0] == "token_proj":
            d = S
        elif part[0] == "encoder":
            assert part[1] in ("attention_layers", "feedforward_layers", "layer_norm"), name
            d = S + 1 + int(part[2])
        else:
            assert part[0] == "head", name
            d = S + 1 + L
        depth[id(p)] = d
    return depth, S + 1 + L


@pytest.mark.parametrize("layer_decay,no_decay_1d", [(0.75, True), (0.75, False), (1.0, True), (1.0, False), (0.5, True)])
def test_groups_partition_the_parameters(layer_decay, no_decay_1d):
    model = _model()
    groups = model.param_groups(lr=2e-3, weight_decay=0.05, layer_decay=layer_decay, no_decay_1d=no_decay_1d)
    listed = [p for g in groups for p in g["params"]]
    assert len(listed) == len({id(p) for p in listed})                                    # no parameter twice
    assert {id(p) for p in listed} == {id(p) for p in model.parameters()}                 # and every one of them
    assert all(g["params"] for g in groups)                                               # empty groups are dropped
    assert len({g["name"] for g in groups}) == len(groups)
    depth, D = _depths(model)
    for g in groups:
        for p in g["params"]:
            # weight decay: 0 for every parameter with ndim <= 1 (biases, BatchNorm, LayerNorm) when asked for, and for no other
            assert g["weight_decay"] == (0.0 if (no_decay_1d and p.ndim <= 1) else 0.05), g["name"]
            # the rate: lr * layer_decay ** (D - depth); the head trains at lr
            assert g["lr"] == pytest.approx(2e-3 * layer_decay ** (D - depth[id(p)]), rel=1e-12), g["name"]
            assert g["lr_scale"] == pytest.approx(layer_decay ** (D - depth[id(p)]), rel=1e-12)
    head = next(g for g in groups if any(p is model.head.weight for p in g["params"]))
    assert head["lr"] == 2e-3
    depths_used = len({depth[id(p)] for p in model.parameters()})
    assert depths_used == D + 1
    assert len(groups) == (depths_used if layer_decay != 1.0 else 1) * (2 if no_decay_1d else 1)


def test_defaults_and_one_dimensional_parameters():
    model = _model()
    groups = model.param_groups()
    assert len(groups) == 2 and {g["weight_decay"] for g in groups} == {0.0, 1e-2} and all(g["lr"] == 1e-3 for g in groups)
    assert len(model.param_groups(no_decay_1d=False)) == 1
    no_decay = next(g for g in groups if g["weight_decay"] == 0.0)
    one_d = [p for p in model.parameters() if p.ndim <= 1]
    assert one_d and {id(p) for p in no_decay["params"]} == {id(p) for p in one_d}
    # BatchNorm and LayerNorm weights are among them, not only biases
    assert any(p is model.encoder1[1].weight for p in no_decay["params"]) and any(p is model.encoder.layer_norm[0].weight for p in no_decay["params"])


def test_frozen_parameters_are_left_out():
    model = _model()
    for p in model.encoder1.parameters():
        p.requires_grad_(False)
    groups = model.param_groups(layer_decay=0.75)
    listed = {id(p) for g in groups for p in g["params"]}
    assert listed == {id(p) for p in model.parameters() if p.requires_grad}
    assert not any(g["name"].startswith("stage1") for g in groups)


def test_param_groups_rejects_bad_arguments():
    model = _model()
    for kw in (dict(lr=-1.0), dict(weight_decay=-0.1), dict(layer_decay=0.0), dict(layer_decay=1.5)):
        with pytest.raises(ValueError):
            model.param_groups(**kw)


def test_torch_adamw_and_a_scheduler_accept_the_groups():
    model = _model()
    groups = model.param_groups(lr=1e-3, layer_decay=0.75)
    want = [g["lr"] for g in groups]
    opt = torch.optim.AdamW(groups, lr=123.0)                       # the groups' own lr wins over the default
    assert [g["lr"] for g in opt.param_groups] == want and [g["name"] for g in opt.param_groups] == [g["name"] for g in groups]
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda e: 0.5)
    assert [g["initial_lr"] for g in opt.param_groups] == want
    assert [g["lr"] for g in opt.param_groups] == [0.5 * w for w in want]
    del sched
    for p in model.parameters():
        p.grad = torch.ones_like(p)
    opt.step()
    hyb = P.HybridAdamW(model.param_groups(layer_decay=0.75))
    assert [g["lr"] for g in hyb.param_groups] == want and hyb.param_groups[0]["name"] == "stage1.decay"


def test_merge_groups_is_an_attribute_not_a_group_key():
    ps = [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2, 2))]
    opt = P.HybridAdamW([{"params": ps[:1]}, {"params": ps[1:]}])
    assert opt.merge_groups is True                                 # the default
    off = P.HybridAdamW([{"params": ps[:1]}, {"params": ps[1:]}], merge_groups=False)
    assert off.merge_groups is False
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="merge_groups must be a bool"):
            P.HybridAdamW(ps, merge_groups=bad)
        with pytest.raises(ValueError, match="merge_groups must be a bool"):
            opt.set_merge_groups(bad)
    sd = opt.state_dict()
    assert all("merge_groups" not in g for g in sd["param_groups"]) and "merge_groups" not in sd["state"]
    assert all("merge_groups" not in g for g in opt.param_groups)
    off.load_state_dict(sd)                                         # neither saved nor loaded: the attribute stays
    assert off.merge_groups is False
    # the setter drops the cached pointer tables, which are laid out for one way of launching
    opt._tables["all"] = object(); opt._acc_tables["all"] = object()
    opt.set_merge_groups(True)                                      # no change: nothing dropped
    assert opt._tables and opt._acc_tables
    opt.set_merge_groups(False)
    assert opt.merge_groups is False and not opt._tables and not opt._acc_tables


def test_merges_groups_says_when_one_launch_serves_all_groups():
    def opt(**kw):
        ps = [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2, 2))]
        groups = kw.pop("groups", None) or [{"params": ps[:1]}, {"params": ps[1:]}]
        return P.HybridAdamW(groups, **kw), ps
    o, _ = opt()
    assert not o.merges_groups()                                    # the plain, by-value path is untouched
    o.set_dynamic_hyper(True)
    assert o.merges_groups()
    o.set_merge_groups(False)
    assert not o.merges_groups()
    assert opt(max_grad_norm=1.0)[0].merges_groups() and opt(ema_decay=0.9)[0].merges_groups() and opt(accumulation_steps=2)[0].merges_groups()
    assert opt(skip_nonfinite=True)[0].merges_groups()
    one = P.HybridAdamW([torch.nn.Parameter(torch.zeros(3))], max_grad_norm=1.0)
    assert not one.merges_groups()                                  # one group: today's launch
    ps = [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2, 2))]
    mixed = P.HybridAdamW([{"params": ps[:1], "ema_decay": 0.9}, {"params": ps[1:]}])
    assert mixed.uses_device_hyper() and not mixed.merges_groups()  # the groups disagree on keeping an average
    o, ps = opt(max_grad_norm=1.0)
    ps[1].requires_grad_(False)
    assert not o.merges_groups()                                    # one live group only
    o, ps = opt(max_grad_norm=1.0)
    o.state[ps[0]]["step"] = 3                                      # the groups do not share the step number
    assert not o.merges_groups()
