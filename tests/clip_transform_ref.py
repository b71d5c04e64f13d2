"""fp64 numpy restatement of hyb_clips_u8_transform's sampling rule (include/hybrid_hip.h), shared by tests/test_clip_transform_cpu.py
(which pins it to torch.nn.functional.interpolate) and tests/test_gpu_clip_transform.py (which holds the kernel to it).

Source index and fraction come from integer arithmetic exactly as in the kernel; everything after that is float64, so the only roundings
are fp64's.  ``mean_invstd`` is the fp32 [2,C] array the kernel reads (mean, then 1/std), widened exactly."""
import numpy as np


def clamp_rows(rows, Hin, Win):
    """The kernel's clamps of {y0, x0, ch, cw, flip}: y0 into [0, Hin-1], ch into [1, Hin-y0], the same for x0 / cw, flip read as != 0."""
    rows = np.array(rows, dtype=np.int64).reshape(-1, 8)
    out = rows.copy()
    out[:, 0] = np.clip(rows[:, 0], 0, Hin - 1)
    out[:, 1] = np.clip(rows[:, 1], 0, Win - 1)
    out[:, 2] = np.clip(rows[:, 2], 1, Hin - out[:, 0])
    out[:, 3] = np.clip(rows[:, 3], 1, Win - out[:, 1])
    out[:, 4] = rows[:, 4] != 0
    return out


def axis_taps(n_out, crop, flip=False):
    """-> (i0, i1, frac) for the n_out output positions of an axis that resamples `crop` source positions."""
    o = np.arange(n_out, dtype=np.int64)
    if flip:
        o = n_out - 1 - o
    n = np.maximum((2 * o + 1) * crop - n_out, 0)
    i0, r = n // (2 * n_out), n % (2 * n_out)
    return i0, np.minimum(i0 + 1, crop - 1), r.astype(np.float64) / float(2 * n_out)


def clip_transform_ref(src, rows, mean_invstd, Tout, Ho, Wo):
    """src uint8 [B,Tin,Hin,Win,C], rows int [B,8], mean_invstd fp32 [2,C] or None -> float64 [B,Tout,C,Ho,Wo]."""
    src = np.asarray(src)
    B, Tin, Hin, Win, C = src.shape
    raw = np.array(rows, dtype=np.int64).reshape(B, 8)
    rows = clamp_rows(raw, Hin, Win)
    out = np.empty((B, Tout, C, Ho, Wo), dtype=np.float64)
    for b in range(B):
        y0, x0, ch, cw, flip = (int(v) for v in rows[b, :5])
        t0, ts_ = int(raw[b, 5]), int(raw[b, 6])
        iy0, iy1, fy = axis_taps(Ho, ch)
        ix0, ix1, fx = axis_taps(Wo, cw, bool(flip))
        fy, fx = fy[:, None, None], fx[None, :, None]
        for t in range(Tout):
            ts = min(max(t0 + t * ts_, 0), Tin - 1)
            fr = src[b, ts].astype(np.float64)                                  # [Hin,Win,C]
            a00, a01 = fr[y0 + iy0][:, x0 + ix0], fr[y0 + iy0][:, x0 + ix1]
            a10, a11 = fr[y0 + iy1][:, x0 + ix0], fr[y0 + iy1][:, x0 + ix1]
            top, bot = a00 + fx * (a01 - a00), a10 + fx * (a11 - a10)
            v = (top + fy * (bot - top)) / 255.0                                # [Ho,Wo,C]
            if mean_invstd is not None:
                mi = np.asarray(mean_invstd, dtype=np.float32).astype(np.float64)
                v = (v - mi[0]) * mi[1]
            out[b, t] = v.transpose(2, 0, 1)
    return out
