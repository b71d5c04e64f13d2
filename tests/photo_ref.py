"""fp64 restatement of hyb_clips_u8_transform_photo and hyb_clips_u8_luma_sums (include/hybrid_hip.h), shared by tests/test_photo_cpu.py and
tests/test_gpu_photo.py.  It stands on tests/clip_transform_ref.py (the resampled value / 255) and tests/mix_ref.py (the mix rows' clamps); the
hash is oracle/dropout_masks.py's replica of the library's counter hash.

The factors, sigma and the pivot mu enter as the fp32 values the kernel uses, widened exactly; everything after that is float64, so the
only roundings are fp64's.  The luma sums are Python ints: exact."""
import numpy as np

from oracle.dropout_masks import hash as hyb_hash

from clip_transform_ref import clamp_rows, clip_transform_ref
from mix_ref import clamp_mix_rows, mix_lam

ONE_BITS = 0x3f800000
ORDERS = ("BCS", "BSC", "CBS", "CSB", "SBC", "SCB")          # order 0..5: the lexicographic permutations
LUMA_W = (0.2989, 0.587, 0.114)
LUMA_INT = (2989, 5870, 1140)


def f32_bits(x):
    """The int32 a photo row carries for the fp32 value x."""
    return int(np.asarray(x, dtype=np.float32).view(np.int32))


def _f32(bits):
    return np.asarray(int(bits), dtype=np.int64).astype(np.int32).view(np.float32)


def photo_row(fb=1.0, fc=1.0, fs=1.0, order=0, gray=0, sigma=0.0, seed=0, box=(0, 0, 0, 0), mode=0):
    """One photo row from values (factors and sigma as floats, the seed as a 64-bit integer)."""
    seed &= (1 << 64) - 1
    lo, hi = (int(np.asarray(v, dtype=np.uint32).view(np.int32)) for v in (seed & 0xffffffff, seed >> 32))
    return [f32_bits(fb), f32_bits(fc), f32_bits(fs), order, gray, f32_bits(sigma), lo, hi, *box, mode, 0, 0, 0]


def clamp_photo_rows(photo, Ho, Wo):
    """The kernel's clamps as rows the kernel would read unchanged: a factor that is not >= 0 (NaN included) becomes 1, one above 16 becomes 16; an
    order outside 0..5 is 0; gray is 0 / 1; a sigma that is not > 0 becomes 0, one above 1 becomes 1; the box is clamped like the CutMix box;
    a mode outside 0..2 is 0.  The seed words and the reserved words stay."""
    photo = np.array(photo, dtype=np.int64).reshape(-1, 16)
    out = photo.copy()
    for b in range(len(photo)):
        for i in range(3):
            f = _f32(photo[b, i])
            out[b, i] = f32_bits(1.0 if not f >= 0 else min(f, np.float32(16)))
        s = _f32(photo[b, 5])
        out[b, 5] = f32_bits(0.0 if not s > 0 else min(s, np.float32(1)))
    out[:, 3] = np.where((photo[:, 3] >= 0) & (photo[:, 3] <= 5), photo[:, 3], 0)
    out[:, 4] = photo[:, 4] != 0
    out[:, 8] = np.clip(photo[:, 8], 0, Ho)
    out[:, 9] = np.clip(photo[:, 9], 0, Wo)
    out[:, 10] = np.clip(photo[:, 10], 0, Ho - out[:, 8])
    out[:, 11] = np.clip(photo[:, 11], 0, Wo - out[:, 9])
    out[:, 12] = np.where((photo[:, 12] >= 0) & (photo[:, 12] <= 2), photo[:, 12], 0)
    return out


def row_seed(row):
    return (int(row[6]) & 0xffffffff) | ((int(row[7]) & 0xffffffff) << 32)


def luma_sums_ref(src, rows, Tout):
    """-> [B][Tout] Python ints: the sum over the clamped crop of output frame t's source frame of 2989 R + 5870 G + 1140 B (C == 1: 10000 v)."""
    src = np.asarray(src)
    B, Tin, Hin, Win, C = src.shape
    raw = np.array(rows, dtype=np.int64).reshape(B, 8)
    cl = clamp_rows(raw, Hin, Win)
    out = []
    for b in range(B):
        y0, x0, ch, cw = (int(v) for v in cl[b, :4])
        per = []
        for t in range(Tout):
            ts = min(max(int(raw[b, 5]) + t * int(raw[b, 6]), 0), Tin - 1)
            crop = src[b, ts, y0:y0 + ch, x0:x0 + cw].astype(np.int64).reshape(-1, C).sum(0)
            per.append(10000 * int(crop[0]) if C == 1 else sum(w * int(v) for w, v in zip(LUMA_INT, crop)))
        out.append(per)
    return out


def noise_z(seed, idx):
    """The standard normal draws at element indices idx: Box-Muller on two 24-bit uniforms of hash(seed, 2 idx) and hash(seed, 2 idx + 1)."""
    idx = np.asarray(idx, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h1, h2 = hyb_hash(seed, idx * np.uint64(2)), hyb_hash(seed, idx * np.uint64(2) + np.uint64(1))
    u1 = ((h1 >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (h2 >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def _luma(v):
    return LUMA_W[0] * v[:, 0] + LUMA_W[1] * v[:, 1] + LUMA_W[2] * v[:, 2]


def _one_clip(unit, ph, sums, ch, cw, mi):
    """unit float64 [Tout,C,Ho,Wo] (the resampled value / 255) -> steps 2-6 under the CLAMPED photo row ph."""
    Tout, C, Ho, Wo = unit.shape
    v = unit.copy()
    fb, fc, fs = (float(_f32(ph[i])) for i in range(3))
    order = ORDERS[int(ph[3])]
    mu = float(np.float32(sum(sums) / (10000 * 255 * ch * cw * Tout)))          # int / int: correctly rounded to double, then to fp32 once
    if order.index("B") < order.index("C"):
        mu = min(fb * mu, 1.0)
    for op in order:
        if op == "B" and fb != 1.0:
            v = np.clip(fb * v, 0.0, 1.0)
        elif op == "C" and fc != 1.0:
            v = np.clip(fc * v + (1.0 - fc) * mu, 0.0, 1.0)
        elif op == "S" and fs != 1.0 and C == 3:
            v = np.clip(fs * v + (1.0 - fs) * _luma(v)[:, None], 0.0, 1.0)
    if ph[4] != 0 and C == 3:
        v = np.repeat(_luma(v)[:, None], 3, axis=1)
    sigma, seed = float(_f32(ph[5])), row_seed(ph)
    e = np.arange(Tout * C * Ho * Wo, dtype=np.uint64).reshape(Tout, C, Ho, Wo)
    if sigma != 0.0:
        v = np.clip(v + sigma * noise_z(seed, e), 0.0, 1.0)
    black = np.zeros(C)
    if mi is not None:
        m = np.asarray(mi, dtype=np.float32).astype(np.float64)
        v = (v - m[0][None, :, None, None]) * m[1][None, :, None, None]
        black = (0.0 - m[0]) * m[1]
    ey0, ex0, eh, ew, mode = (int(x) for x in ph[8:13])
    if eh * ew:
        box = (slice(None), slice(None), slice(ey0, ey0 + eh), slice(ex0, ex0 + ew))
        if mode == 0:
            v[box] = 0.0
        elif mode == 1:
            v[box] = np.broadcast_to(black[None, :, None, None], v[box].shape)
        else:
            v[box] = noise_z(seed, e + np.uint64(Tout * C * Ho * Wo))[box]
    return v


def clip_photo_ref(src, rows, mix, photo, mean_invstd, Tout, Ho, Wo):
    """src uint8 [B,Tin,Hin,Win,C], rows / mix int [B,8] (mix may be None), photo int [B,16] -> float64 [B,Tout,C,Ho,Wo]."""
    src = np.asarray(src)
    B, Tin, Hin, Win, C = src.shape
    unit = clip_transform_ref(src, rows, None, Tout, Ho, Wo)
    cl = clamp_rows(np.array(rows, dtype=np.int64).reshape(B, 8), Hin, Win)
    ph = clamp_photo_rows(photo, Ho, Wo)
    sums = luma_sums_ref(src, rows, Tout)
    own = np.stack([_one_clip(unit[b], ph[b], sums[b], int(cl[b, 2]), int(cl[b, 3]), mean_invstd) for b in range(B)])
    if mix is None:
        return own
    m = clamp_mix_rows(mix, B, Ho, Wo)
    out = own.copy()
    for b in range(B):
        p, kind, by0, bx0, bh, bw = (int(v) for v in m[b, :6])
        if kind == 1:
            lam = mix_lam(m[b, 6])
            out[b] = lam * own[b] + (1.0 - lam) * own[p]
        elif kind == 2:
            out[b, :, :, by0:by0 + bh, bx0:bx0 + bw] = own[p, :, :, by0:by0 + bh, bx0:bx0 + bw]
    return out
