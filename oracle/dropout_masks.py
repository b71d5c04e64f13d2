"""Host replica of the HIP kernels' dropout masks -- TEST INFRASTRUCTURE, NOT PRODUCT CODE (same rules as oracle/hybrid_ref.py).

Dropout in the HIP library is a stateless counter hash of (seed, element index) (csrc/hyb_common.h: ``hyb_hash`` /
``dropout_mult``), so every mask bit can be reproduced here exactly and a reference can apply the SAME masks the kernels drew:
train mode becomes as testable as eval mode.

* ``hash(seed, idx)``: splitmix64's finaliser of ``idx * 0x9E3779B97F4A7C15 + seed``, upper 32 bits; all arithmetic mod 2^64.
* ``keep(seed, idx, p)``: ``u >= p`` with ``u = (hash >> 8) * 2^-24`` and p taken as float32 (the kernels receive ``float p_drop``;
  float32(0.1) != 0.1).  ``mult(seed, idx, p)``: the kernels' multiplier, 0 or float32(1) / float32(1 - p).
* seeds (mod 2^64): layer i of the temporal encoder draws its attention-weight mask with ``attn_seed(seed, i)`` and its per-layer
  mask with ``drop_seed(seed, i)`` (csrc/model.hip); every site adds the device step counter ``*seed_inc`` (graph replays) when
  p > 0 and the pointer is given (``with_step``; the long kernels' ``flash_seed``, attention.hip).
* element indices (read off the kernels):
    - attention weights, short (attention.hip, ``(pidx * S + query) * S + key``, pidx = b * H + h) and long kernels
      (``(blockIdx.y * S + query) * S + key``, blockIdx.y = b * H + h): ``attn_index`` -- the reference's [B*H, S, S] weights in order;
    - LayerNorm rows (ln_rows.h, layernorm.hip ``ln_fwd_row`` / ``ln_residual_bwd``): ``row * D + col``, row = b * S + s -- the [B, S, D]
      layer output in order;
    - ``dropout2d`` (bn2d.hip): one draw per (image, channel) plane, index ``n * C + c``;
    - FCT dropout (fct_bwd.hip ``dropout_kernel``): the flat element index.
"""
import numpy as np

MASK64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)


def _u64(x):
    return np.asarray(x, dtype=np.uint64) if not isinstance(x, int) else np.uint64(x & MASK64)


def hash(seed, idx):  # noqa: A001  (the kernels' name)
    """hyb_hash(seed, idx) for a scalar seed and an array of indices (uint64, wrap-around arithmetic) -> uint32 array."""
    s, i = _u64(seed), _u64(idx)
    with np.errstate(over="ignore"):
        z = i * np.uint64(GOLDEN) + s
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(32)).astype(np.uint32)


def keep(seed, idx, p):
    """Boolean keep decisions of dropout_mult (u >= float32(p))."""
    u = (hash(seed, idx) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24          # exact: 24-bit integer times a power of two
    return u >= np.float64(np.float32(p))


def inv_keep(p):
    """The kernels' multiplier of a kept element: float32(1) / (float32(1) - float32(p))."""
    p32 = np.float32(p)
    return np.float32(1.0) / (np.float32(1.0) - p32) if p32 > 0 else np.float32(1.0)


def mult(seed, idx, p):
    """dropout_mult as an fp32 array: 0 where dropped, inv_keep(p) where kept; all ones when p == 0 (the kernels skip the draw)."""
    idx = np.asarray(idx)
    if np.float32(p) <= 0:
        return np.ones(idx.shape, dtype=np.float32)
    return np.where(keep(seed, idx, p), inv_keep(p), np.float32(0.0)).astype(np.float32)


# ---- seeds ----------------------------------------------------------------------------------------------------------------
def attn_seed(seed, layer):
    return (seed + GOLDEN * (2 * layer + 1)) & MASK64


def drop_seed(seed, layer):
    return (seed + GOLDEN * (2 * layer + 2)) & MASK64


def with_step(seed, p, inc=None):
    """The seed a kernel draws with: seed + *seed_inc when p > 0 and a counter is given (inc: its int64 value, two's complement)."""
    if inc is None or not np.float32(p) > 0:
        return seed & MASK64
    return (seed + inc) & MASK64


# ---- element indices ------------------------------------------------------------------------------------------------------
def attn_index(B, H, S):
    """[B*H, S, S] indices of the attention weights (short and long kernels alike)."""
    return np.arange(B * H * S * S, dtype=np.uint64).reshape(B * H, S, S)


def row_index(B, S, D):
    """[B, S, D] indices of the per-layer dropout (LayerNorm rows, row = b * S + s)."""
    return np.arange(B * S * D, dtype=np.uint64).reshape(B, S, D)


def plane_index(N, C):
    """[N, C] indices of dropout2d's (image, channel) planes."""
    return np.arange(N * C, dtype=np.uint64).reshape(N, C)


# ---- the masks of the temporal encoder ------------------------------------------------------------------------------------
def attn_mask(seed, layer, B, H, S, p, inc=None):
    """Multipliers [B*H, S, S] that layer `layer`'s attention kernels apply to the softmax output (src L58)."""
    return mult(with_step(attn_seed(seed, layer), p, inc), attn_index(B, H, S), p)


def layer_mask(seed, layer, B, S, D, p, inc=None):
    """Multipliers [B, S, D] of layer `layer`'s per-layer dropout (after the x sqrt(0.5), src L122-123)."""
    return mult(with_step(drop_seed(seed, layer), p, inc), row_index(B, S, D), p)


def encoder_masks(seed, L, B, S, D, H, attn_p, layer_p, inc=None):
    """(attention masks, layer masks): one list entry per layer, as the encoder operator (seed = its `seed` argument) draws them."""
    return ([attn_mask(seed, i, B, H, S, attn_p, inc) for i in range(L)],
            [layer_mask(seed, i, B, S, D, layer_p, inc) for i in range(L)])
