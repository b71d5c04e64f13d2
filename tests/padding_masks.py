"""Attention masks with fully masked query rows, shared by tests/test_gpu_padding_mask.py, the padding cases of tests/test_gpu_temporal.py and
tests/test_gpu_dropout.py, and the CPU tests that pin the oracle's semantics for them (tests/test_oracle.py).  Not a test module.

A padding mask ``valid (x) valid`` for clips of different lengths zeroes the whole row of every padded frame, and so does a ``[B,S,1]`` query
mask.  The reference fills masked scores with -1e9 before the softmax (``masked_fill``): such a row attends uniformly (1/S per key) and passes
no gradient to any of its scores.  Every builder is a pure function of its arguments (a seeded generator where it draws anything).
"""
import torch


def valid_frames(B, S):
    """[B,S] 0/1: clip b keeps its first S - (1 + b % 3) frames; with B >= 2 clip 1 is full length (padded and unpadded clips in one batch)."""
    valid = torch.zeros(B, S)
    for b in range(B):
        valid[b, :S - (1 + b % 3)] = 1
    if B >= 2:
        valid[1] = 1
    return valid


def pad(B, S, seed=0):
    v = valid_frames(B, S)
    return v[:, :, None] * v[:, None, :]


def rows(B, S, seed=0):
    """[B,S,1]: about a quarter of the queries zero (query 0 of every clip kept, the last query of clip 0 dropped: both kinds always present)."""
    g = torch.Generator().manual_seed(1000 + seed)
    m = (torch.rand(B, S, 1, generator=g) > 0.25).float()
    m[:, 0] = 1
    m[0, S - 1] = 0
    return m


def keys(B, S, seed=0):
    """[B,1,S] with key 0 kept: no query row is fully masked (the control)."""
    g = torch.Generator().manual_seed(2000 + seed)
    m = (torch.rand(B, 1, S, generator=g) > 0.3).float()
    m[:, :, 0] = 1
    return m


def clip0(B, S, seed=0):
    assert B >= 2
    m = pad(B, S)
    m[0] = 0
    return m


def late(B, S, seed=0):
    """Keys 0..63 masked for every query, on top of pad: the first online-softmax block is fully masked and real keys follow."""
    assert S > 64
    m = pad(B, S)
    m[:, :, :64] = 0
    return m


def early(B, S, seed=0):
    """Only keys 0..2 visible, on top of pad: every later 64-key block is fully masked."""
    assert S > 64
    m = pad(B, S)
    m[:, :, 3:] = 0
    return m


def values(B, S, seed=0):
    """pad with its non-zero entries drawn from {0.5, -1, 2, 1} and its zero entries from {0.0, -0.0}: only ``mask == 0`` may matter."""
    g = torch.Generator().manual_seed(3000 + seed)
    m = pad(B, S)
    nz = torch.tensor([0.5, -1.0, 2.0, 1.0])[torch.randint(0, 4, m.shape, generator=g)]
    z = torch.tensor([0.0, -0.0])[torch.randint(0, 2, m.shape, generator=g)]
    return torch.where(m != 0, nz, z)


BUILDERS = {"pad": pad, "rows": rows, "keys": keys, "clip0": clip0, "late": late, "early": early, "values": values}


def build(name, B, S, seed=0):
    """name: a builder, or "values:bool" / "values:int64" (the values mask passed as ``mask != 0`` in that dtype)."""
    base, _, dt = name.partition(":")
    m = BUILDERS[base](B, S, seed)
    if dt:
        m = (m != 0).to({"bool": torch.bool, "int64": torch.int64}[dt])
    return m


def row_census(mask, B, S, H):
    """(fully masked, with a visible key): numbers of (problem, query) rows of each kind under the reference's head-replication rule --
    problem b * H + h reads mask[(b * H + h) % B] (``mask.repeat(H, 1, 1)``)."""
    full = problem_rows_fully_masked(mask, B, S, H)
    return int(full.sum()), int((~full).sum())


def problem_rows_fully_masked(mask, B, S, H):
    """bool [B*H, S]: query rows of each attention problem whose keys are all masked."""
    m = (mask != 0).expand(B, S, S)
    per_problem = m[torch.arange(B * H) % B]                 # [B*H, S, S]
    return ~per_problem.any(dim=2)


# ---- the module-level cases of tests/test_gpu_padding_mask.py (the CPU test measures the fp32 oracle's own error on the same list) ----
# (B, S, D, H, mask), grouped by the kernel the shape reaches
MHA_CASES = (
    # one token tile (SINGLE); (3,5,24,3) has B = H
    [(B, S, D, H, m) for (B, S, D, H) in ((2, 6, 16, 2), (3, 5, 24, 3), (2, 16, 64, 4))
     for m in ("pad", "rows", "keys", "clip0", "values", "values:bool", "values:int64")]
    # >= 2048 problems: four per workgroup, ragged last group
    + [(683, 7, 24, 3, "pad")]
    # several tiles (fp32, and the bf16 variant with V staged in LDS)
    + [(B, S, D, H, m) for (B, S, D, H) in ((2, 17, 32, 4), (3, 40, 96, 2), (2, 64, 256, 2)) for m in ("pad", "rows", "clip0")]
    # online softmax
    + [(B, S, D, H, m) for (B, S, D, H) in ((2, 70, 32, 4), (3, 128, 96, 2), (1, 200, 256, 2)) for m in ("pad", "rows", "late", "early")]
)
# (B, S, D, Hid, L, H): packed q|k|v variants of the attention kernels, relu_out stores
ENCODER_CASES = [(1, 7, 32, 40, 1, 2), (2, 16, 64, 128, 2, 4), (2, 96, 64, 128, 2, 4)]
