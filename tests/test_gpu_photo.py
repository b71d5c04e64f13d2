"""GPU: colour jitter, grayscale, Gaussian noise and random erasing inside the clip augmentation kernel (hyb_clips_u8_transform_photo and
hyb_clips_u8_luma_sums through hybrid::clip_transform_photo / hybrid::clip_luma_sums, and ClipPipeline with a photometric ClipTransform).

The source, the parameter rows and the output sizes are those of tests/test_gpu_clip_transform.py: 3 clips of 5 frames 37 x 53 whose rows
differ in crop, flip and temporal window, Tout = 3; 24 x 24 takes the 16-byte stores, 9 x 13 the scalar tail, 64 x 64 more than one block per
frame, 8 x 8 has the 1 x 1 crops.  Everything that does no arithmetic is compared with torch.equal; the arithmetic against tests/photo_ref.py
(float64).  With T = max(1, max_c invstd_c) the gates are derived, not measured:

    jitter   2^-16 * T.  The existing gate 2^-20 * T bounds the resampled value.  Each op with a factor in [0.5, 1.5] amplifies an error by at
             most f + |1 - f| <= 2: three ops give 8 * 2^-20 = 2^-17.  The ops' own roundings, about four each on values <= 1.5 and amplified
             at most 4x, add less than 2^-18.  Clamps and the luma, whose weights sum to below 1, are 1-Lipschitz.
    noise    the jitter gate + 2^-16 * sigma * T.  |z| <= 5.77; the radius is good to a few ulp, the angle carries at most two roundings at
             magnitude up to 8, about 2^-21 absolute, plus the cosine's own few ulp: |dz| < 2^-17, and one factor 2 is kept in hand.
    pixel    2^-17 on an erased value in "pixel" mode, which is z itself.
    mixup    the operands' gate + 2^-20 * T for the blend's own roundings."""
import functools
import itertools

import numpy as np
import pytest
import torch

import transformer_cnn_hybrid_network_for_video_processing_amd as P
from transformer_cnn_hybrid_network_for_video_processing_amd._lib import lib

from mix_ref import lam_bits
from photo_ref import clamp_photo_rows, clip_photo_ref, f32_bits, luma_sums_ref, noise_z, photo_row
from test_gpu_clip_transform import CLAMP_CASES, IMAGENET, ROWS, _mean_invstd, _source
from test_gpu_mix_transform import _boxes, _mix_rows

pytestmark = pytest.mark.gpu

SIZES = [(24, 24), (9, 13), (64, 64), (8, 8)]
VARIANTS = [(3, True), (3, False), (1, False)]
VIDS = ["rgb-imagenet", "rgb-plain", "grey"]
OPCHECK_TESTS = ("test_schema", "test_autograd_registration", "test_faketensor", "test_aot_dispatch_static")
NAN_BITS = 0x7fc00000
T_OUT = 3
SEEDS = (0x0123456789abcdef, (7 << 32) | 5, 2 ** 64 - 1)
size_ids = dict(ids=lambda s: f"{s[0]}x{s[1]}")


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _scale(norm, C):
    mi = _mean_invstd(norm, C)
    return max(1.0, float(mi[1].max())) if mi is not None else 1.0


def _mi(norm, C):
    mi = _mean_invstd(norm, C)
    return None if mi is None else mi[:, :C]


@functools.lru_cache(maxsize=None)
def _luma(size, C):
    """hybrid::clip_luma_sums of the shared source and rows, computed once and kept (test_luma_sums_are_exact holds it to the reference)."""
    return P.clip_luma_sums(_dev(_source(C)), _dev(np.asarray(ROWS[size], dtype=np.int32)), T_OUT)


def _photo(size, C, norm, photo, mix=None, luma=True, src=None, rows=None):
    mi = _mi(norm, C)
    rows = ROWS[size] if rows is None else rows
    srcd = _dev(_source(C) if src is None else src)
    rowsd = _dev(np.asarray(rows, dtype=np.int32))
    sums = None if not luma else (_luma(size, C) if src is None and rows is ROWS[size] else P.clip_luma_sums(srcd, rowsd, T_OUT))
    out = P.clip_transform_photo(srcd, rowsd, None if mix is None else _dev(np.asarray(mix, dtype=np.int32)),
                                 _dev(np.asarray(photo, dtype=np.int64).astype(np.int32)), sums, None if mi is None else _dev(mi), T_OUT, *size)
    assert out.shape == (3, T_OUT, C, *size) and out.dtype == torch.float32
    return out


@functools.lru_cache(maxsize=None)
def _plain(size, C, norm):
    mi = _mi(norm, C)
    return P.clip_transform(_dev(_source(C)), _dev(np.asarray(ROWS[size], dtype=np.int32)), None if mi is None else _dev(mi), T_OUT, *size)


def _ref(size, C, norm, photo, mix=None):
    return clip_photo_ref(_source(C), ROWS[size], mix, photo, _mi(norm, C), T_OUT, *size)


def _err(got, want):
    return float(np.abs(got.double().cpu().numpy() - want).max())


# an identity row whose seed, order, mode and (zero-area) box would matter if they were read
IDENTITY = [photo_row(order=3, seed=SEEDS[1], box=(3, 5, 0, 7), mode=2), photo_row(order=5, seed=SEEDS[0], box=(0, 0, 9, 0), mode=1),
            photo_row(order=9, gray=0, sigma=-1.0, seed=SEEDS[2], box=(2, 2, 0, 0), mode=7)]


# ---- 1. identity rows are the plain kernels, bit for bit -----------------------------------------------------------------------------------
@pytest.mark.parametrize("C,norm", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("size", SIZES, **size_ids)
def test_identity_rows_are_the_plain_kernels_bit_for_bit(size, C, norm):
    mi = _mi(norm, C)
    for luma in (False, True):
        assert torch.equal(_photo(size, C, norm, IDENTITY, luma=luma), _plain(size, C, norm))
    mixes = {"kind0": _mix_rows((0, 0, 0), boxes=[(1, 1, 5, 5)] * 3, lams=[lam_bits(0.3)] * 3),
             "cutmix": _mix_rows((2, 2, 2), boxes=_boxes(*size)["inside-quad"], lams=[NAN_BITS] * 3),
             "mixup": _mix_rows((1, 1, 1), lams=(NAN_BITS, lam_bits(0.3), lam_bits(0.85)))}
    for name, mix in mixes.items():
        want = P.clip_transform_mix(_dev(_source(C)), _dev(np.asarray(ROWS[size], dtype=np.int32)), _dev(mix), None if mi is None else _dev(mi),
                                    T_OUT, *size)
        assert torch.equal(_photo(size, C, norm, IDENTITY, mix=mix), want), name


# ---- 2. luma sums are exact ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("size", SIZES, **size_ids)
def test_luma_sums_are_exact(size, C):
    got = _luma(size, C)
    assert got.shape == (3, T_OUT) and got.dtype == torch.int64
    assert torch.equal(got.cpu(), torch.tensor(luma_sums_ref(_source(C), ROWS[size], T_OUT), dtype=torch.int64))


def test_luma_sums_of_a_wide_frame_use_every_load_path():
    # rows of 3 * 701 bytes from odd offsets: 16-byte chunks in every phase mod 3, heads and tails of every length, several rows per workgroup
    src = np.random.default_rng(9).integers(0, 256, (2, 2, 70, 701, 3), dtype=np.uint8)
    rows = [(1, 0, 69, 701, 0, 0, 1, 0), (0, 7, 70, 689, 1, 1, 1, 0)]
    for C in (3, 1):
        s = np.ascontiguousarray(src[..., :C])
        got = P.clip_luma_sums(_dev(s), _dev(np.asarray(rows, dtype=np.int32)), 2)
        assert torch.equal(got.cpu(), torch.tensor(luma_sums_ref(s, rows, 2), dtype=torch.int64)), C


@pytest.mark.parametrize("rows,clamped", CLAMP_CASES, ids=["overshoot", "far"])
def test_luma_sums_clamp_their_rows(rows, clamped):
    B, T, H, W, C = 2, 2, 16, 16, 3
    n = B * T * H * W * C
    big = _dev(np.random.default_rng(7).integers(0, 256, (3 * n,), dtype=np.uint8))
    src = big[n:2 * n].view(B, T, H, W, C)
    got = [P.clip_luma_sums(src, _dev(np.asarray(r, dtype=np.int32)), 2) for r in (rows, clamped)]
    assert torch.equal(got[0], got[1])
    assert torch.equal(got[0].cpu(), torch.tensor(luma_sums_ref(src.cpu().numpy(), rows, 2), dtype=torch.int64))


# ---- 3. jitter -----------------------------------------------------------------------------------------------------------------------------
def _jitter_cases():
    cases = {}
    for i, op in enumerate("bcs"):
        for f in (0.5, 1.5):
            fac = [1.0, 1.0, 1.0]
            fac[i] = f
            cases[f"{op}{f}"] = [photo_row(*fac, order=b) for b in range(3)]
    for o in range(6):
        # every clip in order o, the three factors rotated from clip to clip
        cases[f"order{o}"] = [photo_row(*np.roll((0.6, 1.4, 0.5), b), order=o) for b in range(3)]
    cases["gray"] = [photo_row(0.6, 1.4, 0.5, order=(2, 4, 1)[b], gray=(1, 7, -1)[b]) for b in range(3)]
    cases["gray-alone"] = [photo_row(gray=1)] * 3
    return cases


JITTER = _jitter_cases()


@pytest.mark.parametrize("C,norm", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("size", SIZES, **size_ids)
def test_jitter_against_the_fp64_reference(size, C, norm):
    tol = 2.0 ** -16 * _scale(norm, C)
    plain = _plain(size, C, norm)
    for name, photo in JITTER.items():
        got = _photo(size, C, norm, photo)
        err = _err(got, _ref(size, C, norm, photo))
        print(f"clip_transform_photo jitter {name} {size} C={C} norm={norm}: max abs err {err:.3e} (tol {tol:.3e})")
        assert err <= tol, name
        if C == 1 and (name[0] == "s" or name == "gray-alone"):      # saturation and gray do nothing to a grey clip
            assert torch.equal(got, plain), name
        else:
            assert not torch.equal(got, plain), name


# ---- 4. noise ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [0.1, 0.25])
@pytest.mark.parametrize("C,norm", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("size", SIZES, **size_ids)
def test_noise_against_the_fp64_reference(size, C, norm, sigma):
    T = _scale(norm, C)
    tol = 2.0 ** -16 * T + 2.0 ** -16 * sigma * T
    for name, jit in (("alone", (1.0, 1.0, 1.0)), ("jittered", (0.6, 1.4, 0.5))):
        photo = [photo_row(*jit, order=3, sigma=sigma, seed=SEEDS[b]) for b in range(3)]
        got = _photo(size, C, norm, photo)
        err = _err(got, _ref(size, C, norm, photo))
        print(f"clip_transform_photo noise {name} sigma={sigma} {size} C={C} norm={norm}: max abs err {err:.3e} (tol {tol:.3e})")
        assert err <= tol, name
        assert not torch.equal(got, _plain(size, C, norm))


@pytest.mark.parametrize("size", [(24, 24), (9, 13)], **size_ids)
def test_noise_is_a_function_of_the_seed(size):
    src = _source(3).copy()
    src[1] = src[0]
    rows = [ROWS[size][0], ROWS[size][0], ROWS[size][2]]
    same = [photo_row(sigma=0.2, seed=SEEDS[0])] * 3
    other = [same[0], photo_row(sigma=0.2, seed=SEEDS[0] + 1), same[0]]
    a, b = _photo(size, 3, True, same, src=src, rows=rows), _photo(size, 3, True, other, src=src, rows=rows)
    assert torch.equal(a[0], a[1]) and torch.equal(a[0], b[0]) and not torch.equal(b[0], b[1])


# ---- 5. erase ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2], ids=["zero", "black", "pixel"])
@pytest.mark.parametrize("which", ["inside-quad", "last-row-col", "odd"])
@pytest.mark.parametrize("C,norm", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("size", SIZES[:3], **size_ids)
def test_erase_writes_the_box_and_nothing_else(size, C, norm, which, mode):
    Ho, Wo = size
    boxes = _boxes(Ho, Wo)[which]
    base = dict(fb=1.2, sigma=0.1)
    photo = [photo_row(seed=SEEDS[b], box=boxes[b], mode=mode, **base) for b in range(3)]
    got = _photo(size, C, norm, photo, luma=False)
    without = _photo(size, C, norm, [photo_row(seed=SEEDS[b], mode=mode, **base) for b in range(3)], luma=False)
    mi = _mi(norm, C)
    inside = torch.zeros(3, T_OUT, C, Ho, Wo, dtype=torch.bool)
    for b, (ey0, ex0, eh, ew) in enumerate(boxes):
        inside[b, :, :, ey0:ey0 + eh, ex0:ex0 + ew] = True
    got, without = got.cpu(), without.cpu()
    assert torch.equal(got[~inside], without[~inside])
    if mode == 0:
        want = torch.zeros_like(got)
    elif mode == 1:
        want = torch.zeros_like(got)
        if mi is not None:
            m = torch.from_numpy(mi)
            want += ((torch.zeros(C) - m[0]) * m[1]).view(1, 1, C, 1, 1)      # fp32 arithmetic, as the kernel does it
    else:
        n = T_OUT * C * Ho * Wo
        e = np.arange(n, dtype=np.uint64).reshape(T_OUT, C, Ho, Wo) + np.uint64(n)
        z = torch.from_numpy(np.stack([noise_z(SEEDS[b], e) for b in range(3)]))
        err = float((got.double() - z)[inside].abs().max()) if inside.any() else 0.0
        print(f"clip_transform_photo erase pixel {which} {size} C={C} norm={norm}: max abs err {err:.3e} (tol {2.0 ** -17:.3e})")
        assert err <= 2.0 ** -17
        return
    assert torch.equal(got[inside], want[inside])
    assert inside.any() and not torch.equal(got, without)


# ---- 6. composition with mixing ------------------------------------------------------------------------------------------------------------
def _all_on(size):
    Ho, Wo = size
    boxes = [(1, 2, Ho // 2, Wo // 3), (Ho - 3, 0, 3, Wo), (0, Wo - 2, Ho, 2)]
    return [photo_row(*np.roll((0.7, 1.3, 0.6), b), order=(1, 3, 4)[b], gray=(0, 0, 1)[b], sigma=(0.1, 0.05, 0.2)[b], seed=SEEDS[b], box=boxes[b],
                      mode=(2, 1, 0)[b]) for b in range(3)]


@pytest.mark.parametrize("which", ["inside-quad", "last-row-col", "odd"])
@pytest.mark.parametrize("C,norm", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("size", SIZES[:3], **size_ids)
def test_cutmix_is_a_composition_of_the_photo_outputs(size, C, norm, which):
    boxes = _boxes(*size)[which]
    photo = _all_on(size)
    own = _photo(size, C, norm, photo)
    got = _photo(size, C, norm, photo, mix=_mix_rows((2, 2, 2), boxes=boxes, lams=[NAN_BITS] * 3))
    want = own.clone()
    for b, (by0, bx0, bh, bw) in enumerate(boxes):
        want[b, :, :, by0:by0 + bh, bx0:bx0 + bw] = own[(b + 1) % 3, :, :, by0:by0 + bh, bx0:bx0 + bw]
    assert torch.equal(got, want)
    assert torch.equal(_photo(size, C, norm, photo, mix=_mix_rows((0, 0, 0), boxes=boxes)), own)
    assert not torch.equal(own, _plain(size, C, norm))


@pytest.mark.parametrize("C,norm", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("size", SIZES, **size_ids)
def test_mixup_blends_the_photo_outputs(size, C, norm):
    T = _scale(norm, C)
    photo = _all_on(size)
    mix = _mix_rows((1, 1, 1), lams=(lam_bits(0.3), NAN_BITS, lam_bits(0.85)))
    tol = 2.0 ** -16 * T + 2.0 ** -16 * 0.2 * T + 2.0 ** -20 * T
    got = _photo(size, C, norm, photo, mix=mix)
    err = _err(got, _ref(size, C, norm, photo, mix))
    err_own = _err(_photo(size, C, norm, photo), _ref(size, C, norm, photo))
    print(f"clip_transform_photo mixup {size} C={C} norm={norm}: max abs err {err:.3e}, un-mixed {err_own:.3e} (tol {tol:.3e})")
    assert err <= tol and err_own <= tol
    assert torch.equal(got[1], _photo(size, C, norm, photo)[1])           # a NaN lam counts as 1


# ---- 7. clamping: photo rows that overshoot behave exactly like their clamped twins.  The source sits in the middle of a larger allocation, so
# that a clamping bug shows as wrong values and never as a fault. ---------------------------------------------------------------------------
CLAMP_PHOTO = {
    "factors": [photo_row(fb=float("nan"), fc=-0.5, fs=1e9, order=2), photo_row(fb=-1e9, fc=1e9, fs=float("nan"), order=1)],
    "order": [photo_row(0.6, 1.4, 0.5, order=9), photo_row(0.6, 1.4, 0.5, order=-1)],
    "box-beyond": [photo_row(seed=5, box=(5, 6, 40, 50), mode=2), photo_row(seed=6, box=(30, 3, 2, 2), mode=1)],
    "box-before": [photo_row(seed=5, box=(-3, -2, 6, 7), mode=2), photo_row(seed=6, box=(2, 2, -4, -1), mode=1)],
    "mode": [photo_row(seed=5, box=(1, 1, 3, 3), mode=7), photo_row(seed=6, box=(1, 1, 3, 3), mode=-1)],
    "sigma": [photo_row(sigma=float("nan"), seed=5), photo_row(sigma=5.0, seed=6)],
    "sigma-negative": [photo_row(sigma=-1.0, seed=5), photo_row(sigma=0.1, seed=6, gray=-3)],
}


@pytest.mark.parametrize("size", [(8, 8), (5, 7)], ids=["vec", "tail"])
@pytest.mark.parametrize("which", list(CLAMP_PHOTO))
def test_out_of_range_photo_rows_equal_their_clamped_twins(which, size):
    B, T, H, W, C = 2, 2, 16, 16, 3
    n = B * T * H * W * C
    big = _dev(np.random.default_rng(7).integers(0, 256, (10 * n,), dtype=np.uint8))
    src = big[4 * n:5 * n].view(B, T, H, W, C)
    rows = _dev(np.asarray([(1, 2, 9, 11, 1, 0, 1, 0), (0, 0, 16, 16, 0, 1, 0, 0)], dtype=np.int32))
    mi = _dev(_mean_invstd(True, C))
    sums = P.clip_luma_sums(src, rows, 2)
    photo = np.asarray(CLAMP_PHOTO[which], dtype=np.int64)
    twin = clamp_photo_rows(photo, *size)
    assert not np.array_equal(twin, photo)
    out = [P.clip_transform_photo(src, rows, None, _dev(p.astype(np.int32)), sums, mi, 2, *size) for p in (photo, twin)]
    assert torch.equal(out[0], out[1])
    want = clip_photo_ref(src.cpu().numpy(), rows.cpu().numpy(), None, twin, mi.cpu().numpy(), 2, *size)
    err = _err(out[0], want)
    tol = (2.0 ** -16 + 2.0 ** -16 * 1.0) * float(mi[1].max())       # the jitter gate + the noise gate at the largest sigma, 1
    if which != "factors":                                   # (factors of 16 are outside the gate's derivation: equality with the twin is the test)
        assert err <= tol, err


# ---- 8. replay -----------------------------------------------------------------------------------------------------------------------------
def test_captured_launches_replay_with_new_rows():
    size = (24, 24)
    src, mi = _dev(_source(3)), _dev(_mean_invstd(True, 3))
    first_p, second_p = (torch.tensor(ROWS[k], dtype=torch.int32) for k in ((24, 24), (64, 64)))
    first_h, second_h = (torch.from_numpy(np.asarray(p, dtype=np.int64).astype(np.int32)) for p in (_all_on(size), JITTER["order2"]))
    params, photo = first_p.cuda(), first_h.cuda()

    def run(p, h):
        return P.clip_transform_photo(src, p, None, h, P.clip_luma_sums(src, p, T_OUT), mi, T_OUT, *size)
    eager_first = run(params, photo)                                 # also loads the kernels before the capture
    eager_second = run(second_p.cuda(), second_h.cuda())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                        # memset, luma sums, transform: one chain, no parallel branches
        out = run(params, photo)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager_first)
    params.copy_(second_p)                                           # the rows are device memory: nothing of them was baked into the nodes
    photo.copy_(second_h)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager_second) and not torch.equal(out, eager_first)


# ---- 9. the pipeline -----------------------------------------------------------------------------------------------------------------------
ALL_ON = dict(brightness=0.4, contrast=0.4, saturation=0.4, jitter_prob=0.8, grayscale=0.2, noise_std=(0.05, 0.2), noise_prob=0.7, erase_prob=0.7,
              erase_mode="pixel")


@pytest.mark.parametrize("mixing", [False, True], ids=["plain", "mixing"])
def test_pipeline_runs_the_photo_kernel_on_its_rows(mixing):
    src = P.SyntheticClipSource(4, 5, 24, distinct=5)
    kw = dict(frames=3, frame_stride=(1, 2), seed=5, **IMAGENET, **ALL_ON)
    if mixing:
        kw.update(mixup_alpha=0.8, cutmix_alpha=1.0, mix_mode="clip", mix_prob=0.9)
    pipe = P.ClipPipeline(itertools.islice(iter(src), 9), depth=2, transform=P.ClipTransform(16, **kw))
    twin = P.ClipTransform(16, **kw)
    mi = _dev(twin.mean_invstd(3))
    seen, jittered = 0, 0
    for i, (x, y) in enumerate(pipe):                       # 9 batches over 3 slots: every slot's rows and luma buffer are reused
        fr, lab = src.batches[i % 5]
        rows = _dev(twin.sample(4, 5, 24, 24))
        mix = lam = partner = None
        if mixing:
            mix, lam, partner = twin.sample_mix(4, 16, 16)
        photo = twin.sample_photo(4, 3, 16, 16)
        jittered += int((photo[:, :3] != f32_bits(1.0)).any(1).sum())
        want = P.clip_transform_photo(_dev(fr), rows, None if mix is None else _dev(mix), _dev(photo), P.clip_luma_sums(_dev(fr), rows, 3), mi, 3, 16, 16)
        assert x.shape == (4, 3, 3, 16, 16) and torch.equal(x, want), f"batch {i}"
        if mixing:
            assert isinstance(y, P.MixTarget)
            assert torch.equal(y.y_a.cpu(), torch.from_numpy(lab)) and torch.equal(y.y_b.cpu(), torch.from_numpy(lab[partner]))
            assert y.lam.dtype == torch.float32 and torch.equal(y.lam.cpu(), torch.from_numpy(lam))
        else:
            assert isinstance(y, torch.Tensor) and torch.equal(y.cpu(), torch.from_numpy(lab))
        seen += 1
    assert seen == 9 and jittered > 18
    torch.cuda.synchronize()


@pytest.mark.parametrize("mixing", [False, True], ids=["plain", "mixing"])
def test_pipeline_with_default_options_calls_only_the_existing_kernels(mixing, monkeypatch):
    names = []
    call = lib.call

    def recording(name, *args):
        names.append(name)
        return call(name, *args)
    monkeypatch.setattr(lib, "call", recording)
    src = P.SyntheticClipSource(2, 3, 24, seed=3, distinct=2)
    kw = dict(seed=1, **IMAGENET)
    if mixing:
        kw.update(mixup_alpha=0.8, cutmix_alpha=1.0)
    outs = [(x.clone(), y) for x, y in P.ClipPipeline(itertools.islice(iter(src), 2), transform=P.ClipTransform(16, **kw))]
    torch.cuda.synchronize()
    assert set(names) == {"hyb_clips_u8_transform_mix" if mixing else "hyb_clips_u8_transform"}, names
    twin = P.ClipTransform(16, **kw)
    mi = _dev(twin.mean_invstd(3))
    for i, (x, _) in enumerate(outs):
        rows = _dev(twin.sample(2, 3, 24, 24))
        fr = _dev(src.batches[i][0])
        want = P.clip_transform_mix(fr, rows, _dev(twin.sample_mix(2, 16, 16)[0]), mi, 3, 16, 16) if mixing else P.clip_transform(fr, rows, mi, 3, 16, 16)
        assert torch.equal(x, want)
    # and an evaluation transform with every option set is not photometric either
    names.clear()
    next(iter(P.ClipPipeline(itertools.islice(iter(src), 1), transform=P.ClipTransform(16, train=False, **ALL_ON))))
    torch.cuda.synchronize()
    assert names == ["hyb_clips_u8_transform"]


# ---- 10. the operators -----------------------------------------------------------------------------------------------------------------------
def test_opcheck_both_operators_and_their_argument_checks():
    size = (24, 24)
    srcd, rows = _dev(_source(3)), _dev(np.asarray(ROWS[size], dtype=np.int32))
    mi = _dev(_mean_invstd(True, 3))
    mix = _dev(_mix_rows((1, 2, 0), boxes=[(0, 0, 0, 0), (2, 3, 5, 6), (0, 0, 0, 0)], lams=[lam_bits(0.3)] * 3))
    photo = _dev(np.asarray(_all_on(size), dtype=np.int64).astype(np.int32))
    torch.library.opcheck(torch.ops.hybrid.clip_luma_sums.default, (srcd, rows, 3), test_utils=OPCHECK_TESTS)
    sums = P.clip_luma_sums(srcd, rows, 3)
    for m, x, s in ((mi, mix, sums), (None, None, sums), (mi, mix, None)):
        torch.library.opcheck(torch.ops.hybrid.clip_transform_photo.default, (srcd, rows, x, photo, s, m, 3, 24, 24), test_utils=OPCHECK_TESTS)
    with pytest.raises(TypeError, match="photo must be int32"):
        P.clip_transform_photo(srcd, rows, mix, photo.long(), sums, mi, 3, 24, 24)
    with pytest.raises(TypeError, match="photo must be int32"):
        P.clip_transform_photo(srcd, rows, mix, photo[:, :8].contiguous(), sums, mi, 3, 24, 24)
    with pytest.raises(TypeError, match="photo must be int32"):
        P.clip_transform_photo(srcd, rows, mix, photo[:2], sums, mi, 3, 24, 24)
    with pytest.raises(TypeError, match="luma_sums must be int64"):
        P.clip_transform_photo(srcd, rows, mix, photo, sums.int(), mi, 3, 24, 24)
    with pytest.raises(TypeError, match="mix must be int32"):
        P.clip_transform_photo(srcd, rows, mix.long(), photo, sums, mi, 3, 24, 24)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.clip_transform_photo(srcd, rows, mix, photo.cpu(), sums, mi, 3, 24, 24)
    with pytest.raises(TypeError, match="uint8"):
        P.clip_luma_sums(srcd.float(), rows, 3)
    with pytest.raises(TypeError, match="int32"):
        P.clip_luma_sums(srcd, rows.long(), 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.clip_luma_sums(srcd.cpu(), rows, 3)
    with pytest.raises(ValueError, match="C == 1 or C == 3"):
        P.clip_transform_photo(srcd[..., :2].contiguous(), rows, None, photo, None, None, 3, 24, 24)
