"""The training-time conv epilogue that stores every 2 x 2 window's raw extreme (HYB_POOL_EXT) against the
conv -> bn_relu_pool pair it replaces: the two routes must give the same tensors BIT FOR BIT (values compared with torch.equal, so
-0 == +0).  Per channel y -> y * scale + shift is monotone with the direction of sign(gamma), and rounding to bf16 is monotone, so the
maximum of the transformed window is the transform of the window's maximum (gamma >= 0) or minimum (gamma < 0): nothing to tolerate.

The switch is read once per process: tests/pool_ext_worker.py runs every case once under HYB_POOL_EXT=1 and once under =0 (two child
processes for the whole file) and the tests compare what they saved."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pool_ext_worker as worker      # noqa: E402  (the case tables; importing it starts nothing)

STAGE_TENSORS = ("pooled", "y_raw", "scale_shift", "mean_invstd", "running")
MAY_KEEP_THE_PAIR = {"full_28_64to128", "full_28_128to256"}       # stage-3/4 shapes: a conv variant that would spill with the epilogue is not built


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    d = tmp_path_factory.mktemp("pool_ext")
    out = {}
    for v in ("1", "0"):
        path = str(d / f"ext{v}.pt")
        env = dict(os.environ, HYB_POOL_EXT=v)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "pool_ext_worker.py"), path], env=env, cwd=ROOT,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-4000:]
        out[v] = torch.load(path)
    return out


def _same(on, off, names):
    for k in names:
        assert on[k].dtype == off[k].dtype and on[k].shape == off[k].shape, k
        assert torch.isfinite(on[k].float()).all(), k
        assert torch.equal(on[k], off[k]), f"{k}: {(on[k].float() != off[k].float()).sum().item()} of {on[k].numel()} values differ"


@pytest.mark.parametrize("name", list(worker.STAGES))
def test_stage_with_the_epilogue_extreme_equals_the_pair(both, name):
    on, off = both["1"][name], both["0"][name]
    assert int(off["route"]) == 0, "HYB_POOL_EXT=0 forces the pair"
    if not int(on["route"]):
        assert name in MAY_KEEP_THE_PAIR, "this shape must take the new route"
        pytest.skip(f"{name}: hyb_conv3x3_pool_ext reports the pair for this shape; the comparison would be vacuous")
    _same(on, off, STAGE_TENSORS)
    N, H, W, Ci, Co = worker.STAGES[name]
    assert tuple(on["pooled"].shape) == (N, H // 2, W // 2, (Co + 31) // 32 * 32)
    assert (on["pooled"].float() > 0).float().mean() > 0.2, "the ReLU passes a fair share: the comparison is not one of zeros"


def test_zero_and_negative_gamma_and_tied_windows(both):
    on, off = both["1"][worker.SIGNS], both["0"][worker.SIGNS]
    assert int(on["route"]) == 1 and int(off["route"]) == 0
    _same(on, off, STAGE_TENSORS)
    ss = on["scale_shift"]
    assert (ss[0, 0:4] == 0).all() and (ss[0, 8:12] == 0).all() and (ss[0, 16:24] < 0).all(), "the case holds the gammas it is about"
    y = on["y_raw"].float()
    assert (y[..., 5] == 0).all() and (y[..., 6] == 0).all() and (y[1, 4:-4, 4:-4, 0] == y[1, 8, 8, 0]).all(), "... and the tied windows"


@pytest.mark.parametrize("mode", ["bf16", "mixed"])
def test_one_training_step_of_the_smoke_model_is_the_same_on_both_routes(both, mode):
    on, off = both["1"]["model_" + mode], both["0"]["model_" + mode]
    assert set(on) == set(off) and any(k.startswith("grad.") for k in on)
    _same(on, off, sorted(on))


def test_graphed_steps_equal_eager_steps_with_the_route_on():
    """tests/test_gpu_graph.py's comparison on a clip whose second stage (32 x 32, 32 -> 64) has full and edge tiles: three replays of the
    captured step == three eager steps, bit for bit."""
    import transformer_cnn_hybrid_network_for_video_processing_amd as P
    from transformer_cnn_hybrid_network_for_video_processing_amd import ops
    assert ops.conv3x3_pool_ext(ops.dtype_code("bf16"), 32, 32, 64), "the default takes the new route for this stage"
    K, WARM = 3, 1
    kw = dict(cnn_channels=(32, 64), d_model=64, num_heads=4, num_layers=2, hidden_dim=128)

    def setup():
        torch.manual_seed(0)
        m = P.TransformerCNNHybrid(dropout=0.0, compute_dtype="bf16", **kw)
        with torch.no_grad():
            for s in m.modules():
                if isinstance(s, torch.nn.BatchNorm2d):
                    s.weight.copy_(worker.mixed_sign_bn(s.num_features, torch.Generator().manual_seed(9))[0])
        m = m.cuda().train()
        for a in m.encoder.attention_layers:
            a.dropoutLayer.p = 0.0
        g = torch.Generator().manual_seed(3)
        return m, torch.rand(3, 4, 3, 64, 64, generator=g).cuda(), torch.randint(0, 8, (3,), generator=g).cuda()

    m1, x, y = setup()
    m2, _, _ = setup()
    crit = P.HybridCrossEntropyLoss()
    o1, o2 = P.HybridAdamW(m1.parameters(), lr=1e-3), P.HybridAdamW(m2.parameters(), lr=1e-3)
    eager = []
    for _ in range(WARM + K):
        o1.zero_grad(set_to_none=True)
        loss = crit(m1(x), y)
        loss.backward()
        o1.step()
        eager.append(loss.item())
    tr = P.GraphedTrainStep(m2, crit, o2, x, y, warmup=WARM)
    try:
        graphed = [tr.step().item() for _ in range(K)]
        assert graphed == eager[WARM:], (graphed, eager)
        for (n, a), (_, b) in zip(m1.named_parameters(), m2.named_parameters()):
            assert torch.equal(a, b), n
        for (n, a), (_, b) in zip(m1.named_buffers(), m2.named_buffers()):
            assert torch.equal(a, b), n
    finally:
        tr.close()
