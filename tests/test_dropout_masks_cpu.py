"""CPU tests of the dropout-mask replica (oracle/dropout_masks.py) and the masked-dropout oracle (oracle/hybrid_ref_masked.py,
the mask arguments of oracle/hybrid_ref_bf16.py).  The GPU side -- the kernels draw exactly these masks -- is tests/test_gpu_dropout.py."""
import copy
import math

import numpy as np
import pytest
import torch

from oracle import dropout_masks as DM
from oracle import hybrid_ref as R
from oracle import hybrid_ref_bf16 as RB
from oracle import hybrid_ref_masked as RM

M64 = (1 << 64) - 1


def _hash_scalar(seed, idx):
    """hyb_hash (csrc/hyb_common.h) transcribed on Python integers."""
    z = (idx * 0x9E3779B97F4A7C15 + seed) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z = z ^ (z >> 31)
    return z >> 32


def _mult_scalar(seed, idx, p):
    p32 = float(np.float32(p))
    u = (_hash_scalar(seed, idx) >> 8) / 16777216.0
    return float(np.float32(1) / (np.float32(1) - np.float32(p))) if u >= p32 else 0.0


SEEDS = [0, 1, 2 ** 63, 2 ** 63 - 1, M64, 0x9E3779B97F4A7C15, 12345678901234567]
IDX = np.array([0, 1, 2, 255, 2 ** 31 - 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 7, 3 * 2 ** 40 + 5, 2 ** 63, M64 - 1, M64], dtype=np.uint64)


@pytest.mark.parametrize("seed", SEEDS)
def test_vectorised_hash_equals_big_int_transcription(seed):
    with np.errstate(all="raise"):                      # the replica silences its own wrap-around; nothing may leak out
        got = DM.hash(seed, IDX)
    assert got.dtype == np.uint32
    assert [int(g) for g in got] == [_hash_scalar(seed, int(i)) for i in IDX]
    for p in (0.1, 0.5, 0.9):
        assert [float(m) for m in DM.mult(seed, IDX, p)] == [_mult_scalar(seed, int(i), p) for i in IDX]


def test_seed_derivations_wrap_mod_2_64():
    for seed in SEEDS:
        for i in range(4):
            assert DM.attn_seed(seed, i) == (seed + 0x9E3779B97F4A7C15 * (2 * i + 1)) % 2 ** 64
            assert DM.drop_seed(seed, i) == (seed + 0x9E3779B97F4A7C15 * (2 * i + 2)) % 2 ** 64
    # the step counter: added only when p > 0 and a counter is given; an int64 counter is read as its two's-complement uint64
    assert DM.with_step(M64 - 3, 0.1, 10) == 6
    assert DM.with_step(5, 0.1, -7) == M64 - 1
    assert DM.with_step(5, 0.0, 10) == 5 and DM.with_step(5, 0.1, None) == 5
    s = 2 ** 64 - 100
    idx = np.arange(1000, dtype=np.uint64)
    assert np.array_equal(DM.mult(DM.with_step(s, 0.5, 300), idx, 0.5), DM.mult(200, idx, 0.5))


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_rate_within_binomial_bounds(p):
    n = 1 << 20
    for seed in (0, 7, 2 ** 63 + 11):
        k = DM.keep(seed, np.arange(n, dtype=np.uint64) + np.uint64(2 ** 33), p).sum()
        mean, sd = n * (1 - p), math.sqrt(n * p * (1 - p))
        assert abs(k - mean) < 6 * sd, (seed, k, mean)
    m = DM.mult(3, np.arange(n, dtype=np.uint64), p)
    assert set(np.unique(m).tolist()) == {0.0, float(np.float32(1) / (np.float32(1) - np.float32(p)))}
    assert DM.mult(3, np.arange(10, dtype=np.uint64), 0.0).tolist() == [1.0] * 10


def test_float32_p_boundary():
    """The kernels compare u = (h >> 8) * 2^-24 with float(p).  Every u is a float32 number, so p and float32(p) decide differently
    exactly when p rounds DOWN onto a u: p = t * 2^-24 + tiny keeps the elements with u = t * 2^-24 (a double comparison would drop them).
    The multiplier is float32(1) / float32(1 - p) as well."""
    n = 1 << 20
    idx = np.arange(n, dtype=np.uint64)
    u = (DM.hash(0, idx) >> np.uint32(8)).astype(np.int64)
    for target in (0.1, 0.3, 0.5):
        t = int(u[u >= target * 2 ** 24].min())         # a 24-bit value some element draws
        p = t * 2.0 ** -24 + 1e-13
        assert float(np.float32(p)) == t * 2.0 ** -24 < p
        k = DM.keep(0, idx, p)
        assert np.array_equal(k, u >= t) and k[u == t].all()     # u == float32(p) < p: kept
        assert (DM.mult(0, idx[u == t], p) == np.float32(1) / (np.float32(1) - np.float32(p))).all()
    assert DM.inv_keep(0.1) == np.float32(1) / (np.float32(1) - np.float32(0.1))


# ---------------------------------------------------------------------------------------------------------------------------
# masked oracle
# ---------------------------------------------------------------------------------------------------------------------------
def _encoder_pair(D=32, Hid=48, L=2, H=4, dropout=0.0, seed=0):
    torch.manual_seed(seed)
    ref = R.TransformerEncoder(D, Hid, L, H, dropout)
    with torch.no_grad():
        for ln in ref.layer_norm:
            ln.weight.copy_(torch.randn(D) * 0.3 + 1.0)
            ln.bias.copy_(torch.randn(D) * 0.1)
    return ref.double()


def test_masked_oracle_with_all_keep_masks_equals_oracle_exactly():
    B, S, D, H, L = 2, 5, 32, 4, 2
    enc = _encoder_pair(D=D, L=L, H=H)
    for a in enc.attention_layers:
        a.dropoutLayer.p = 0.0
    x = torch.randn(B, S, D, dtype=torch.float64)
    mask = (torch.rand(B, S, S) > 0.3).double()
    mask[:, :, 0] = 1
    am, lm = DM.encoder_masks(123, L, B, S, D, H, 0.0, 0.0)
    assert all((m == 1).all() for m in am + lm)
    enc.train()
    assert torch.equal(RM.encoder(enc, x, mask, am, lm), enc(x, mask))
    assert torch.equal(RM.encoder(enc, x, mask), enc(x, mask))
    att = enc.attention_layers[0]
    assert torch.equal(RM.mha(att, x, x, x, mask, am[0]), att(x, x, x, mask))
    torch.manual_seed(1)
    ref = R.TransformerCNNHybridRef(cnn_channels=(8, 16), d_model=32, num_heads=4, num_layers=2, hidden_dim=48).double()
    for a in ref.encoder.attention_layers:
        a.dropoutLayer.p = 0.0
    xc = torch.rand(2, 3, 3, 16, 16, dtype=torch.float64)
    ref2 = copy.deepcopy(ref)
    am, lm = DM.encoder_masks(5, 2, 2, 3, 32, 4, 0.0, 0.0)
    assert torch.equal(RM.forward(ref, xc, None, am, lm), ref2(xc))


def test_masked_oracle_places_the_masks_where_the_oracle_drops():
    """Replay the masks through the oracle's own nn.Dropout calls (in call order: attention of layer 0, layer 0, attention of layer 1, ...):
    the masked oracle must give the same output and gradients -- the masks multiply the softmax output (src L58) and the layer output after
    the x sqrt(0.5) (src L122-123)."""
    B, S, D, H, L = 2, 6, 32, 4, 2
    enc = _encoder_pair(D=D, L=L, H=H, dropout=0.5).train()
    am, lm = DM.encoder_masks(99, L, B, S, D, H, 0.1, 0.5)
    order = [m for pair in zip(am, lm) for m in pair]
    calls = []

    def fake_dropout(self, x):
        m = torch.from_numpy(order[len(calls)]).to(x.dtype)
        calls.append(self.p)
        return x * m
    x = torch.randn(B, S, D, dtype=torch.float64)
    xr, xm = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    r = torch.randn(B, S, D, dtype=torch.float64)
    orig = torch.nn.Dropout.forward
    torch.nn.Dropout.forward = fake_dropout
    try:
        want = enc(xr, None)
    finally:
        torch.nn.Dropout.forward = orig
    assert calls == [0.1, 0.5, 0.1, 0.5]
    (want * r).sum().backward()
    gw = [p.grad.clone() for p in enc.parameters()]
    enc.zero_grad()
    got = RM.encoder(enc, xm, None, am, lm)
    (got * r).sum().backward()
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)
    assert (got == 0).any() and torch.allclose(xm.grad, xr.grad, rtol=1e-12, atol=1e-12)
    for a, b in zip(gw, enc.parameters()):
        assert torch.allclose(b.grad, a, rtol=1e-12, atol=1e-12)


def test_bf16_oracle_masks_default_to_the_unmasked_functions():
    B, S, D, H, L = 2, 5, 32, 4, 2
    enc = _encoder_pair(D=D, L=L, H=H).eval()
    x = torch.randn(B, S, D, dtype=torch.float64)
    am, lm = DM.encoder_masks(7, L, B, S, D, H, 0.0, 0.0)
    base = RB.encoder(enc, x, None)
    assert torch.equal(RB.encoder(enc, x, None, am, lm), base)
    am, lm = DM.encoder_masks(7, L, B, S, D, H, 0.1, 0.5)
    got = RB.encoder(enc, x, None, am, lm)
    assert torch.equal(got == 0, torch.from_numpy(lm[-1] == 0))     # the last layer's dropped elements are exactly the output's zeros
    with pytest.raises(AssertionError):
        RB.encoder(_encoder_pair(D=D, L=L, H=H, dropout=0.5), x, None)
