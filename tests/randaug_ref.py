"""Restatement of hyb_clip_aug_u8_transform (include/hybrid_hip.h), shared by tests/test_randaug_cpu.py, tests/test_gpu_randaug.py and
scripts/randaug_errors.py.  It stands on tests/clip_transform_ref.py (the integer-tap resampling), tests/photo_ref.py (steps 2-6 of the photo
rule, the luma sums, the photo rows' clamps) and tests/mix_ref.py (the mix rows' clamps).

``clip_aug_ref`` is the float64 rule: M, fill, the factors and the hue shift enter as the fp32 values the kernel reads, widened exactly, and
everything after that is float64.  With ``fp32=True`` the geometry (coordinates, fractions, lerps, the division by 255) and the hue shift are
restated operation by operation in numpy float32, a fused multiply-add as the float64 result rounded once; the distance between the two is the
yardstick of the GPU test's gate for those two families -- it is measured against this file alone, never against the kernel.

Beside the values the reference returns ``near``: the pixels that lie within 2^-10 (in byte units) of a boundary on which a quantising step
decides (Posterize: a change of the kept bits; Solarize: the threshold; SolarizeAdd: 128), or whose geometry lies within 2^-10 px of the frame's
edge.  A comparison leaves them out, all channels of the pixel: a later Color or Hue step spreads a channel's decision over the pixel."""
import numpy as np

from clip_transform_ref import clamp_rows, clip_transform_ref
from mix_ref import clamp_mix_rows, mix_lam
from photo_ref import LUMA_W, _f32, _one_clip, clamp_photo_rows, f32_bits, luma_sums_ref, photo_row

OPS = ("Identity", "Invert", "Brightness", "Contrast", "Color", "Posterize", "Solarize", "SolarizeAdd", "Hue")
IDENTITY_M = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
BAND = 2.0 ** -10


def aug_row(prog=(), M=None, fill=(0.5, 0.5, 0.5), flags=None, n=None, tail=(0, 0, 0, 0, 0)):
    """One aug row from values.  prog: up to 8 (op, arg) with op a name of OPS or a code; the arg of Brightness / Contrast / Color / Hue is a float
    (stored as fp32 bits), of the others an int.  M: six floats (flags defaults to "geometry on" when M is given); n defaults to len(prog)."""
    row = [0] * 32
    row[0] = (0 if M is None else 1) if flags is None else flags
    row[1] = len(prog) if n is None else n
    for i, (op, arg) in enumerate(prog):
        code = OPS.index(op) if isinstance(op, str) else int(op)
        row[2 + 2 * i] = code
        row[3 + 2 * i] = f32_bits(arg) if isinstance(arg, float) else int(arg)
    row[18:24] = [f32_bits(v) for v in (IDENTITY_M if M is None else M)]
    row[24:27] = [f32_bits(v) for v in fill]
    row[27:32] = list(tail)
    return row


def clamp_aug_rows(aug):
    """The kernel's clamps as rows the kernel would read unchanged: n into 0..8; the steps behind n zeroed (they are not read); an op outside 0..8 is
    Identity with arg 0; a factor that is not >= 0 becomes 1, one above 16 becomes 16; bits into 0..8, the threshold into 0..256, the addend into
    0..255; a hue that is NaN becomes 0, else it is clamped into [-1/2, 1/2]; a non-finite M clears the geometry flag, and without the flag M is the
    identity; flags keep bit 0 only; a fill that is not >= 0 becomes 0, one above 1 becomes 1; the reserved words are zeroed."""
    aug = np.array(aug, dtype=np.int64).reshape(-1, 32)
    out = np.zeros_like(aug)
    for b in range(len(aug)):
        n = int(np.clip(aug[b, 1], 0, 8))
        out[b, 1] = n
        for s in range(n):
            op, arg = int(aug[b, 2 + 2 * s]), int(aug[b, 3 + 2 * s])
            if op < 0 or op > 8 or op == 0:
                op, arg = 0, 0
            elif op == 1:
                arg = 0
            elif op in (2, 3, 4):
                f = _f32(arg)
                arg = f32_bits(1.0 if not f >= 0 else min(f, np.float32(16)))
            elif op == 5:
                arg = int(np.clip(arg, 0, 8))
            elif op == 6:
                arg = int(np.clip(arg, 0, 256))
            elif op == 7:
                arg = int(np.clip(arg, 0, 255))
            else:
                h = _f32(arg)
                arg = f32_bits(0.0 if np.isnan(h) else min(max(h, np.float32(-0.5)), np.float32(0.5)))
            out[b, 2 + 2 * s], out[b, 3 + 2 * s] = op, arg
        M = np.array([_f32(v) for v in aug[b, 18:24]])
        geo = bool(aug[b, 0] & 1) and bool(np.all(np.isfinite(M)))
        out[b, 0] = int(geo)
        out[b, 18:24] = [f32_bits(v) for v in (M if geo else IDENTITY_M)]
        for i in range(3):
            f = _f32(aug[b, 24 + i])
            out[b, 24 + i] = f32_bits(0.0 if not f >= 0 else min(f, np.float32(1)))
    return out


def _fma(a, b, c, dt):
    """a * b + c: float64 arithmetic; for float32 operands the fused result (the product of two fp32 is exact in float64) rounded once."""
    r = np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)
    return r.astype(dt)


def geometry_unit(frame, crop, M, fill, Ho, Wo, dt=np.float64):
    """Step 1 with the geometry for one source frame.  frame uint8 [Hin,Win,C]; crop = the CLAMPED (y0, x0, ch, cw, flip); M, fill: fp32 values.
    -> (unit dt [C,Ho,Wo], edge float64 [Ho,Wo]: the distance in px of the mapped point from the nearest edge of [0, Wo) x [0, Ho))."""
    y0, x0, ch, cw, flip = (int(v) for v in crop)
    C = frame.shape[2]
    M = np.asarray(M, dtype=np.float32).astype(dt)
    xc = (np.arange(Wo, dtype=dt) + dt(0.5))[None, :]
    yc = (np.arange(Ho, dtype=dt) + dt(0.5))[:, None]
    with np.errstate(all="ignore"):
        x = _fma(M[0], xc, _fma(M[1], yc, M[2], dt), dt)
        y = _fma(M[3], xc, _fma(M[4], yc, M[5], dt), dt)
        inside = (x >= 0) & (x < Wo) & (y >= 0) & (y < Ho)
        edge = np.minimum(np.minimum(np.abs(x), np.abs(x - Wo)), np.minimum(np.abs(y), np.abs(y - Ho))).astype(np.float64)
    xs = np.where(inside, x, dt(0))
    ys = np.where(inside, y, dt(0))
    if flip:
        xs = dt(Wo) - xs
    sx = (xs * dt(cw)) / dt(Wo) - dt(0.5)
    sy = (ys * dt(ch)) / dt(Ho) - dt(0.5)
    flx, fly = np.floor(sx), np.floor(sy)
    fx, fy = (sx - flx)[..., None], (sy - fly)[..., None]
    ix, iy = np.clip(flx.astype(np.int64), -1, cw), np.clip(fly.astype(np.int64), -1, ch)
    ix0, ix1 = np.clip(ix, 0, cw - 1), np.clip(ix + 1, 0, cw - 1)
    iy0, iy1 = np.clip(iy, 0, ch - 1), np.clip(iy + 1, 0, ch - 1)
    fr = frame.astype(dt)
    a00, a01 = fr[y0 + iy0, x0 + ix0], fr[y0 + iy0, x0 + ix1]                   # [Ho,Wo,C]
    a10, a11 = fr[y0 + iy1, x0 + ix0], fr[y0 + iy1, x0 + ix1]
    top, bot = _fma(fx, a01 - a00, a00, dt), _fma(fx, a11 - a10, a10, dt)
    v = _fma(fy, bot - top, top, dt) / dt(255)
    v = np.where(inside[..., None], v, np.asarray(fill, dtype=np.float32)[:C].astype(dt)[None, None, :])
    return v.transpose(2, 0, 1), edge


def hue_shift(v, h, dt=np.float64):
    """torchvision's adjust_hue on floats, v dt [..., 3 (the channel axis is axis 1 of [T,C,H,W]) ...] given as (r, g, b) arrays -> (r, g, b)."""
    r, g, b = (np.asarray(c, dtype=dt) for c in v)
    one, h = dt(1), dt(np.float32(h))
    mx, mn = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
    cr = mx - mn
    eq = mx == mn
    s = cr / np.where(eq, one, mx)
    d = np.where(eq, one, cr)
    rc, gc, bc = (mx - r) / d, (mx - g) / d, (mx - b) / d
    hh = np.where(mx == r, bc - gc, np.where(mx == g, dt(2) + rc - bc, dt(4) + gc - rc))
    hh = hh / dt(6) + one
    hh = hh - np.floor(hh)
    hh = hh + h
    hh = hh - np.floor(hh)
    h6 = hh * dt(6)
    fl = np.floor(h6)
    f = h6 - fl
    i = fl.astype(np.int64) % 6
    p = np.clip(mx * (one - s), 0, 1)
    q = np.clip(mx * (one - s * f), 0, 1)
    t = np.clip(mx * (one - s * (one - f)), 0, 1)
    pick = lambda table: np.choose(i, table)                                    # noqa: E731
    return pick([mx, q, p, p, t, mx]), pick([t, mx, mx, q, p, p]), pick([p, p, t, mx, mx, q])


def byte_of(v):
    return np.floor(255.0 * v + 0.5)


def _luma(v):
    return LUMA_W[0] * v[:, 0] + LUMA_W[1] * v[:, 1] + LUMA_W[2] * v[:, 2]


def run_program(unit, row, mu0, hue_dt=np.float64):
    """Step 1a on unit float64 [Tout,C,Ho,Wo] under the CLAMPED aug row; mu0: the clip's mean luma as the fp32 the kernel forms, or None without
    luma sums (every Contrast factor then counts as 1).  -> (values, near bool [Tout,Ho,Wo])."""
    v = unit.copy()
    C = v.shape[1]
    near = np.zeros((v.shape[0],) + v.shape[2:], dtype=bool)
    mu = 0.0 if mu0 is None else float(mu0)
    for s in range(int(row[1])):
        op, arg = int(row[2 + 2 * s]), int(row[3 + 2 * s])
        if op == 1:
            v, mu = 1.0 - v, 1.0 - mu
        elif op == 2:
            f = float(_f32(arg))
            if f != 1.0:
                v = np.clip(f * v, 0.0, 1.0)
            mu = min(f * mu, 1.0)
        elif op == 3:
            f = float(_f32(arg)) if mu0 is not None else 1.0
            if f != 1.0:
                v = np.clip(f * v + (1.0 - f) * mu, 0.0, 1.0)
        elif op == 4:
            f = float(_f32(arg))
            if f != 1.0 and C == 3:
                v = np.clip(f * v + (1.0 - f) * _luma(v)[:, None], 0.0, 1.0)
        elif op in (5, 6, 7):
            z = 255.0 * v + 0.5
            q = np.floor(z)
            if op == 5:
                step = 1 << (8 - arg)
                # the kept bits change where q passes a multiple of step
                k = np.round(z / step) * step
                near |= (np.abs(z - k) < BAND).any(1)
                v = (q.astype(np.int64) & ~(step - 1)).astype(np.float64) / 255.0
            elif op == 6:
                near |= (np.abs(z - arg) < BAND).any(1)
                v = np.where(q >= arg, 1.0 - v, v)
            else:
                near |= (np.abs(z - 128.0) < BAND).any(1)
                v = np.where(q < 128, np.minimum(1.0, v + arg / 255.0), v)
        elif op == 8:
            h = float(_f32(arg))
            if h != 0.0 and C == 3:
                r, g, b = hue_shift((v[:, 0].astype(hue_dt), v[:, 1].astype(hue_dt), v[:, 2].astype(hue_dt)), h, hue_dt)
                v = np.stack([r, g, b], axis=1).astype(np.float64)
    return v, near


def clip_aug_ref(src, rows, mix, photo, aug, mean_invstd, Tout, Ho, Wo, luma=True, fp32=False):
    """src uint8 [B,Tin,Hin,Win,C], rows / mix int [B,8] (mix may be None), photo int [B,16] or None, aug int [B,32]
    -> (float64 [B,Tout,C,Ho,Wo], near bool [B,Tout,C,Ho,Wo]).  luma=False: no luma sums, every contrast factor counts as 1."""
    src = np.asarray(src)
    B, Tin, Hin, Win, C = src.shape
    raw = np.array(rows, dtype=np.int64).reshape(B, 8)
    cl = clamp_rows(raw, Hin, Win)
    ag = clamp_aug_rows(aug)
    ph = clamp_photo_rows([photo_row()] * B if photo is None else photo, Ho, Wo)
    if not luma:
        ph[:, 1] = f32_bits(1.0)
    sums = luma_sums_ref(src, rows, Tout)
    plain = clip_transform_ref(src, rows, None, Tout, Ho, Wo)
    dt = np.float32 if fp32 else np.float64
    own, near = [], []
    for b in range(B):
        ch, cw = int(cl[b, 2]), int(cl[b, 3])
        unit, nb = plain[b], np.zeros((Tout, Ho, Wo), dtype=bool)
        if ag[b, 0]:
            M = [_f32(x) for x in ag[b, 18:24]]
            fill = [_f32(x) for x in ag[b, 24:27]]
            frames = []
            for t in range(Tout):
                ts = min(max(int(raw[b, 5]) + t * int(raw[b, 6]), 0), Tin - 1)
                u, edge = geometry_unit(src[b, ts], cl[b, :5], M, fill, Ho, Wo, dt)
                frames.append(u.astype(np.float64))
                nb[t] = edge < BAND
            unit = np.stack(frames)
        mu0 = float(np.float32(sum(sums[b]) / (10000 * 255 * ch * cw * Tout))) if luma else None
        v, nq = run_program(unit, ag[b], mu0, dt)
        own.append(_one_clip(v, ph[b], sums[b], ch, cw, mean_invstd))
        near.append(np.repeat((nb | nq)[:, None], C, axis=1))
    own, near = np.stack(own), np.stack(near)
    if mix is None:
        return own, near
    m = clamp_mix_rows(mix, B, Ho, Wo)
    out, nout = own.copy(), near.copy()
    for b in range(B):
        p, kind, by0, bx0, bh, bw = (int(x) for x in m[b, :6])
        if kind == 1:
            lam = mix_lam(m[b, 6])
            out[b] = lam * own[b] + (1.0 - lam) * own[p]
            nout[b] = near[b] | near[p]
        elif kind == 2:
            out[b, :, :, by0:by0 + bh, bx0:bx0 + bw] = own[p, :, :, by0:by0 + bh, bx0:bx0 + bw]
            nout[b, :, :, by0:by0 + bh, bx0:bx0 + bw] = near[p, :, :, by0:by0 + bh, bx0:bx0 + bw]
    return out, nout
