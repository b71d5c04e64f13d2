"""Train-mode oracle with INJECTED dropout masks -- TEST INFRASTRUCTURE, NOT PRODUCT CODE (same rules as oracle/hybrid_ref.py).

oracle/hybrid_ref.py draws its dropout masks from torch's RNG, so a train-mode run cannot be compared with the HIP path.  These
functions are the same algorithm on the parameters of the oracle's modules (``MultiheadAttention``, ``TransformerEncoder``,
``TransformerCNNHybridRef``; run them on a ``.double()`` copy for an fp64 reference) with the dropout multipliers passed in --
typically the HIP kernels' own masks, replayed bit for bit by oracle/dropout_masks.py:

* attention weights (quirk Q5, src L58): ``weights = softmax(dot) * attn_mask``, attn_mask [B*H, S, S];
* per-layer dropout (quirk Q6, src L122-123): ``x = (LayerNorm(f) + skip2) * sqrt(0.5) * layer_mask``, layer_mask [B, S, D].

A mask of None means "no dropout" there.  With all-keep masks every function equals the oracle's own forward (tests/test_dropout_masks_cpu.py).
"""
import math

import torch


def _t(m, like):
    return None if m is None else torch.as_tensor(m).to(dtype=like.dtype, device=like.device)


def attention(att, q, k, v, mask, drop=None):
    """MultiheadAttention.attention (src L49-62) with the attention-weight dropout multipliers `drop` [B*H, S, S]."""
    dot = torch.matmul(q, k.transpose(-2, -1)) / math.sqrt(att.input_dim)
    if mask is not None:
        dot = dot.masked_fill(mask == 0, -1e9)
    weights = att.softmax(dot)
    if drop is not None:
        weights = weights * _t(drop, weights)
    return torch.matmul(weights, v)


def mha(att, q, k, v, mask=None, drop=None):
    """MultiheadAttention.forward (src L67-89) with injected attention dropout."""
    q, k, v = att.query_layer(q), att.key_layer(k), att.value_layer(v)
    q, k, v = att.activation(q), att.activation(k), att.activation(v)
    q = att.__reshape_to_batches__(q)
    k = att.__reshape_to_batches__(k)
    v = att.__reshape_to_batches__(v)
    if mask is not None:
        mask = mask.repeat(att.num_heads, 1, 1)
    a = attention(att, q, k, v, mask, drop)
    a = att.__reshape_from_batches__(a)
    return att.output_layer(a)


def encoder(enc, x, mask=None, attn_masks=None, layer_masks=None):
    """TransformerEncoder.forward (src L110-126); attn_masks / layer_masks: one entry (or None) per layer."""
    for i in range(enc.num_layers):
        ln = enc.layer_norm[i]
        skip1 = x
        x = mha(enc.attention_layers[i], x, x, x, mask, attn_masks[i] if attn_masks else None)
        x = ln(x) + skip1
        skip2 = x
        x = enc.feedforward_layers[i](x)
        x = (ln(x) + skip2) * math.sqrt(0.5)
        if layer_masks and layer_masks[i] is not None:
            x = x * _t(layer_masks[i], x)
    return x


def temporal(ref, feat, B, mask=None, attn_masks=None, layer_masks=None):
    """Frame features [B*T, C] -> logits: token projection, encoder, mean over the tokens, head (TransformerCNNHybridRef.forward's tail)."""
    tok = ref.token_proj(feat).reshape(B, feat.shape[0] // B, -1)
    return ref.head(encoder(ref.encoder, tok, mask, attn_masks, layer_masks).mean(dim=1))


def forward(ref, x, mask=None, attn_masks=None, layer_masks=None):
    """TransformerCNNHybridRef.forward with injected masks."""
    if x.dim() == 4:
        x = x.unsqueeze(1)
    B, T = x.shape[:2]
    f = x.reshape(B * T, *x.shape[2:])
    for i in range(ref.num_stages):
        f = getattr(ref, f"encoder{i + 1}")(f)
    return temporal(ref, f.mean(dim=(2, 3)), B, mask, attn_masks, layer_masks)
