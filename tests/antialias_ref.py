"""fp64 numpy restatement of hyb_clips_u8_transform_aa's rule (include/hybrid_hip.h), shared by tests/test_antialias_cpu.py (which pins it to
torch.nn.functional.interpolate(..., antialias=True)) and tests/test_gpu_antialias.py (which holds the kernel to it).

The weights are the rule's integers; the sums and the normalisation are float64, so the only roundings are fp64's.  ``mean_invstd`` is the fp32
[2,C] array the kernel reads (mean, then 1/std), widened exactly."""
import numpy as np

from clip_transform_ref import clamp_rows


def aa_weights(n, m, flip=False):
    """-> int64 [m, n]: W(i, k) = max(0, D - |(2k+1) m - (2i+1) n|), D = 2 max(n, m), for the m output positions of an axis that resamples n
    source positions; flip: output position i takes the weights of position m-1-i."""
    i = np.arange(m, dtype=np.int64)
    if flip:
        i = m - 1 - i
    k = np.arange(n, dtype=np.int64)
    D = 2 * max(n, m)
    return np.maximum(0, D - np.abs((2 * k[None, :] + 1) * m - (2 * i[:, None] + 1) * n))


def taps(n, m):
    """The largest number of non-zero weights of an output position."""
    return int((aa_weights(n, m) > 0).sum(axis=1).max())


def clip_transform_aa_ref(src, rows, mean_invstd, V, Tout, Ho, Wo):
    """src uint8 [B,Tin,Hin,Win,C], rows int [B*V,8], mean_invstd fp32 [2,C] or None -> float64 [B*V,Tout,C,Ho,Wo]."""
    src = np.asarray(src)
    B, Tin, Hin, Win, C = src.shape
    raw = np.array(rows, dtype=np.int64).reshape(B * V, 8)
    rows = clamp_rows(raw, Hin, Win)
    out = np.empty((B * V, Tout, C, Ho, Wo), dtype=np.float64)
    for r in range(B * V):
        y0, x0, ch, cw, flip = (int(v) for v in rows[r, :5])
        t0, ts_ = int(raw[r, 5]), int(raw[r, 6])
        wy, wx = aa_weights(ch, Ho).astype(np.float64), aa_weights(cw, Wo, bool(flip)).astype(np.float64)
        wy, wx = wy / wy.sum(axis=1, keepdims=True), wx / wx.sum(axis=1, keepdims=True)
        for t in range(Tout):
            ts = min(max(t0 + t * ts_, 0), Tin - 1)
            a = src[r // V, ts, y0:y0 + ch, x0:x0 + cw].astype(np.float64)          # [ch,cw,C]
            v = np.einsum("yk,xl,klc->cyx", wy, wx, a) / 255.0
            if mean_invstd is not None:
                mi = np.asarray(mean_invstd, dtype=np.float32).astype(np.float64)
                v = (v - mi[0][:, None, None]) * mi[1][:, None, None]
            out[r, t] = v
    return out
