"""Child process of tests/test_gpu_pool_ext.py:  python tests/pool_ext_worker.py OUT.pt

HYB_POOL_EXT is read once per process, so the two sides of the comparison are two runs of this script under the two values of the switch.
Every case is built from its own seeded CPU generator: both runs see the same inputs.  Saves {case: {tensor name: CPU tensor}} to OUT.pt."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import transformer_cnn_hybrid_network_for_video_processing_amd as P                     # noqa: E402
from transformer_cnn_hybrid_network_for_video_processing_amd import ops                 # noqa: E402

# name: (N, H, W, Ci, Co)
STAGES = {
    "full_28_32to64": (2, 28, 28, 32, 64),
    "full_28_64to128": (2, 28, 28, 64, 128),
    "full_28_128to256": (2, 28, 28, 128, 256),
    "edge_30x44_32to64": (2, 30, 44, 32, 64),
    "odd_31x45_32to64": (2, 31, 45, 32, 64),
    "padded_24_16to24": (2, 24, 24, 16, 24),
    "tiles_in_a_row_56_32to64": (3, 56, 56, 32, 64),
    # runs of 4 tiles per workgroup, across images and through every order of full and edge tiles (tests/conv_run_shapes.py); the cases above
    # reach runs of 2.  Four-wave variants: the eight-wave ones with 64 channels per wave have no such epilogue.
    "runs_257x10x58_32to64": (257, 10, 58, 32, 64),
    "runs_257x10x58_64to128": (257, 10, 58, 64, 128),
}
SIGNS = "signs_28_32to64"
SMOKE_KW = dict(cnn_channels=(32, 64, 128, 256), d_model=512, num_heads=8, num_layers=2, hidden_dim=2048)      # __graft_entry__.smoke()


def mixed_sign_bn(Co, g):
    """tests/test_gpu_infer.py::_randomize_bn: a quarter of the channels get a negative gamma."""
    gamma = (torch.rand(Co, generator=g) * 1.5 + 0.25) * torch.where(torch.rand(Co, generator=g) < 0.25, -1.0, 1.0)
    beta = torch.randn(Co, generator=g) * 0.3
    return gamma, beta, torch.randn(Co, generator=g) * 0.2, torch.rand(Co, generator=g) * 1.5 + 0.25


def run_stage(N, H, W, Ci, Co, x, w, bn):
    dt = ops.dtype_code("bf16")
    Cip, Cop = ops.pad_channels(Ci), ops.pad_channels(Co)
    gamma, beta, rm, rv = (t.cuda() for t in bn)
    xh = ops.nchw_to_nhwc(x.cuda(), dt, Cip)
    pooled, y_raw, ss, mi, _, running = ops.convstage_op(xh, w.cuda(), gamma, beta, rm, rv, True, 0.1, 1e-5, dt, False)
    torch.cuda.synchronize()
    out = dict(pooled=pooled, y_raw=y_raw, scale_shift=ss, mean_invstd=mi, running=running)
    out = {k: v.cpu() for k, v in out.items()}
    out["route"] = torch.tensor(int(ops.conv3x3_pool_ext(dt, W, Cip, Cop)))
    return out


def stage_case(name):
    N, H, W, Ci, Co = STAGES[name]
    g = torch.Generator().manual_seed(2000 + H * W + Ci)
    x = torch.randn(N, Ci, H, W, generator=g)
    w = torch.randn(Co, Ci, 3, 3, generator=g) * (2.0 / (9 * Ci)) ** 0.5
    return run_stage(N, H, W, Ci, Co, x, w, mixed_sign_bn(Co, g))


def sign_case():
    """gamma exactly 0, -0.0 and negative next to positive ones; one image constant (its interior windows tie in every channel) and one
    output channel with zero weights (every window of it ties, in every image)."""
    N, H, W, Ci, Co = 2, 28, 28, 32, 64
    g = torch.Generator().manual_seed(77)
    x = torch.randn(N, Ci, H, W, generator=g)
    x[1] = 0.5
    w = torch.randn(Co, Ci, 3, 3, generator=g) * (2.0 / (9 * Ci)) ** 0.5
    w[5] = 0.0
    w[6] = 0.0
    gamma, beta, rm, rv = mixed_sign_bn(Co, g)
    gamma[0:4] = 0.0
    gamma[8:12] = -0.0
    gamma[16:24] = -gamma[16:24].abs()
    gamma[5], gamma[6] = 0.7, -0.7
    beta[2], beta[9] = 0.0, 0.0
    return run_stage(N, H, W, Ci, Co, x, w, (gamma, beta, rm, rv))


def model_case(mode):
    """One training step of the smoke configuration: loss, logits, every gradient, every updated parameter and buffer."""
    torch.manual_seed(0)
    m = P.TransformerCNNHybrid(compute_dtype=mode, dropout=0.0, **SMOKE_KW)
    for a in m.encoder.attention_layers:
        a.dropoutLayer.p = 0.0
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for s in m.modules():
            if isinstance(s, torch.nn.BatchNorm2d):
                gamma, beta, _, _ = mixed_sign_bn(s.num_features, g)
                s.weight.copy_(gamma)
                s.bias.copy_(beta)
    m = m.cuda().train()
    x = torch.rand(2, 4, 3, 64, 64, generator=g).cuda()
    y = torch.randint(0, 8, (2,), generator=g).cuda()
    opt = P.HybridAdamW(m.parameters(), lr=1e-3)
    logits = m(x)
    loss = P.HybridCrossEntropyLoss()(logits, y)
    loss.backward()
    out = {"loss": loss.detach(), "logits": logits.detach()}
    for n, p in m.named_parameters():
        out["grad." + n] = p.grad.detach().clone()
    opt.step()
    torch.cuda.synchronize()
    for n, p in m.named_parameters():
        out["param." + n] = p.detach()
    for n, b in m.named_buffers():
        out["buffer." + n] = b.detach()
    return {k: v.cpu() for k, v in out.items()}


if __name__ == "__main__":
    res = {name: stage_case(name) for name in STAGES}
    res[SIGNS] = sign_case()
    for mode in ("bf16", "mixed"):
        res["model_" + mode] = model_case(mode)
    torch.save(res, sys.argv[1])
