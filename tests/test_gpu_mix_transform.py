"""GPU: Mixup / CutMix inside the clip augmentation kernel (hyb_clips_u8_transform_mix through hybrid::clip_transform_mix and
ClipPipeline with a mixing ClipTransform).

The source, the parameter rows and the output sizes are those of tests/test_gpu_clip_transform.py: 3 clips of 5 frames 37 x 53 whose rows
differ in crop, flip and temporal window, Tout = 3; 24 x 24 takes the 16-byte stores, 9 x 13 the scalar tail, 64 x 64 more than one
block per frame.  Clip b's partner is clip (b + 1) % 3, so every partner differs from its clip in all three.

kind 0 and CutMix do no arithmetic on the values: they are compared with torch.equal against hybrid::clip_transform's own output and
compositions of it.  Mixup is compared against tests/mix_ref.py (float64) with

    tol = 2^-19 * max(1, max_c invstd_c)        absolute

which is derived, not measured: the existing gate 2^-20 * max(1, max invstd) bounds each operand's error, a convex combination keeps
that bound, and the three further fp32 roundings (1 - lam, the two products' sum as the kernel forms it) on a value of that magnitude
add less than the same again."""
import functools
import itertools

import numpy as np
import pytest
import torch

import transformer_cnn_hybrid_network_for_video_processing_amd as P

from mix_ref import clamp_mix_rows, clip_mix_ref, lam_bits
from test_gpu_clip_transform import IMAGENET, ROWS, _mean_invstd, _source

pytestmark = pytest.mark.gpu

SIZES = [(24, 24), (9, 13), (64, 64)]
VARIANTS = [(3, True), (3, False), (1, False)]
VIDS = ["rgb-imagenet", "rgb-plain", "grey"]
OPCHECK_TESTS = ("test_schema", "test_autograd_registration", "test_faketensor", "test_aot_dispatch_static")
NAN_BITS = 0x7fc00000
T_OUT = 3


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _mix_rows(kinds, boxes=None, lams=None, partners=(1, 2, 0)):
    rows = np.zeros((3, 8), dtype=np.int32)
    for b in range(3):
        box = boxes[b] if boxes is not None else (0, 0, 0, 0)
        rows[b, :6] = (partners[b], kinds[b], *box)
        rows[b, 6] = lams[b] if lams is not None else 0
    return rows


@functools.lru_cache(maxsize=None)
def _own(size, C, norm):
    """hybrid::clip_transform's output for the shared source and rows: what every clip contributes, computed once (on the device, kept)."""
    mi = _mean_invstd(norm, C)
    return P.clip_transform(_dev(_source(C)), _dev(np.asarray(ROWS[size], dtype=np.int32)), None if mi is None else _dev(mi), T_OUT, *size)


def _mix(size, C, norm, mix):
    mi = _mean_invstd(norm, C)
    out = P.clip_transform_mix(_dev(_source(C)), _dev(np.asarray(ROWS[size], dtype=np.int32)), _dev(np.asarray(mix, dtype=np.int32)),
                               None if mi is None else _dev(mi), T_OUT, *size)
    assert out.shape == (3, T_OUT, C, *size) and out.dtype == torch.float32
    return out


@pytest.mark.parametrize("C,norm", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kind_zero_rows_are_the_plain_kernel_bit_for_bit(size, C, norm):
    # partners, boxes and lam bits that would matter under another kind: kind 0 reads none of them
    mix = _mix_rows((0, 0, 0), boxes=[(1, 1, 5, 5)] * 3, lams=[lam_bits(0.3)] * 3)
    assert torch.equal(_mix(size, C, norm, mix), _own(size, C, norm))


def _boxes(Ho, Wo):
    return {
        # starts and ends inside a quad of four pixels | empty | the whole frame
        "inside-quad": [(2, 3, 5, 6), (4, 4, 0, 7), (0, 0, Ho, Wo)],
        # the last row | the last column | the bottom-right pixel
        "last-row-col": [(Ho - 1, 0, 1, Wo), (0, Wo - 1, Ho, 1), (Ho - 1, Wo - 1, 1, 1)],
        # one pixel in the middle of a quad | empty by width | everything but the first row and column
        "odd": [(3, 5, 1, 1), (0, 0, Ho, 0), (1, 1, Ho - 1, Wo - 1)],
    }


@pytest.mark.parametrize("which", ["inside-quad", "last-row-col", "odd"])
@pytest.mark.parametrize("C,norm", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_cutmix_is_a_composition_of_the_plain_kernels_outputs(size, C, norm, which):
    boxes = _boxes(*size)[which]
    got = _mix(size, C, norm, _mix_rows((2, 2, 2), boxes=boxes, lams=[NAN_BITS] * 3))       # (lam_bits is not read)
    own = _own(size, C, norm)
    want = own.clone()
    for b, (by0, bx0, bh, bw) in enumerate(boxes):
        p = (b + 1) % 3
        want[b, :, :, by0:by0 + bh, bx0:bx0 + bw] = own[p, :, :, by0:by0 + bh, bx0:bx0 + bw]
    assert torch.equal(got, want)
    if which == "inside-quad":
        assert torch.equal(got[1], own[1]) and torch.equal(got[2], own[0]) and not torch.equal(got[0], own[0])


LAMS = {"0.3-0-1": (lam_bits(0.3), lam_bits(0.0), lam_bits(1.0)), "nan-0.3-0.85": (NAN_BITS, lam_bits(0.3), lam_bits(0.85))}


@functools.lru_cache(maxsize=None)
def _mix_reference(size, C, norm, which):
    return clip_mix_ref(_source(C), ROWS[size], _mix_rows((1, 1, 1), lams=LAMS[which]), _mean_invstd(norm, C), T_OUT, *size)


@pytest.mark.parametrize("which", list(LAMS))
@pytest.mark.parametrize("C,norm", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_mixup_against_the_fp64_reference(size, C, norm, which):
    mi = _mean_invstd(norm, C)
    got = _mix(size, C, norm, _mix_rows((1, 1, 1), lams=LAMS[which]))
    want = _mix_reference(size, C, norm, which)
    tol = 2.0 ** -19 * max(1.0, float(mi[1].max()) if mi is not None else 1.0)
    err = np.abs(got.double().cpu().numpy() - want).max()
    print(f"clip_transform_mix mixup {size} C={C} norm={norm} lam={which}: max abs err {err:.3e} (tol {tol:.3e})")
    assert err <= tol
    own = _own(size, C, norm)
    assert not torch.equal(got[1], own[1])                         # clip 1 really blends in both lam sets
    if which == "nan-0.3-0.85":
        assert torch.equal(got[0], own[0])                         # a NaN lam counts as 1: 1 * own + 0 * partner


# ---- clamping: mix rows that overshoot behave exactly like their clamped twins.  The source sits in the middle of a larger allocation and
# every unclamped address of these rows (partner -1 .. B + 5) would still fall inside it: a clamping bug shows as wrong values, never as a fault.
CLAMP_MIX = {
    "partner": [(2 + 5, 1, 0, 0, 0, 0, lam_bits(0.25), 0), (-1, 2, 1, 1, 4, 5, 0, 0)],      # B + 5 -> clip 1, -1 -> clip 0: each the OTHER clip
    "box-beyond": [(1, 2, 5, 6, 40, 50, 0, 0), (0, 2, 30, 3, 2, 2, 0, 0)],
    "negative": [(1, 2, -3, -2, 6, 7, 0, 0), (0, 2, 2, 2, -4, -1, 0, 0)],
    "kind": [(1, 9, 0, 0, 8, 8, lam_bits(0.5), 0), (0, -1, 0, 0, 8, 8, lam_bits(0.5), 0)],
}


@pytest.mark.parametrize("size", [(8, 8), (5, 7)], ids=["vec", "tail"])
@pytest.mark.parametrize("which", list(CLAMP_MIX))
def test_out_of_range_mix_rows_equal_their_clamped_twins(which, size):
    B, T, H, W, C = 2, 2, 16, 16, 3
    n = B * T * H * W * C
    big = _dev(np.random.default_rng(7).integers(0, 256, (10 * n,), dtype=np.uint8))
    src = big[4 * n:5 * n].view(B, T, H, W, C)
    rows = _dev(np.asarray([(1, 2, 9, 11, 1, 0, 1, 0), (0, 0, 16, 16, 0, 1, 0, 0)], dtype=np.int32))
    mi = _dev(_mean_invstd(True, C))
    mix = np.asarray(CLAMP_MIX[which], dtype=np.int64)
    twin = clamp_mix_rows(mix, B, *size)
    assert not np.array_equal(twin, mix)
    out = [P.clip_transform_mix(src, rows, _dev(m.astype(np.int32)), mi, 2, *size) for m in (mix, twin)]
    assert torch.equal(out[0], out[1])
    want = clip_mix_ref(src.cpu().numpy(), rows.cpu().numpy(), twin, mi.cpu().numpy(), 2, *size)
    assert np.abs(out[0].double().cpu().numpy() - want).max() <= 2.0 ** -19 * float(mi[1].max())
    if which == "kind":
        assert torch.equal(out[0], P.clip_transform(src, rows, mi, 2, *size))


@pytest.mark.parametrize("mode", ["batch", "clip"])
def test_pipeline_mixes_on_the_device_and_yields_mix_targets(mode):
    src = P.SyntheticClipSource(4, 5, 24, distinct=5)
    kw = dict(frames=3, frame_stride=(1, 2), seed=5, mixup_alpha=0.8, cutmix_alpha=1.0, mix_mode=mode, mix_prob=0.9, **IMAGENET)
    pipe = P.ClipPipeline(itertools.islice(iter(src), 9), depth=2, transform=P.ClipTransform(16, **kw))
    twin = P.ClipTransform(16, **kw)
    mi = _dev(twin.mean_invstd(3))
    kinds, seen = set(), 0
    for i, (x, y) in enumerate(pipe):                       # 9 batches over 3 slots: every slot's rows, lam and label buffers are reused
        fr, lab = src.batches[i % 5]
        rows = twin.sample(4, 5, 24, 24)
        mix, lam, partner = twin.sample_mix(4, 16, 16)
        kinds.update(mix[:, 1].tolist())
        assert isinstance(y, P.MixTarget) and x.shape == (4, 3, 3, 16, 16)
        want = P.clip_transform_mix(_dev(fr), _dev(rows), _dev(mix), mi, 3, 16, 16)
        assert torch.equal(x, want), f"batch {i}"
        assert torch.equal(y.y_a.cpu(), torch.from_numpy(lab)) and torch.equal(y.y_b.cpu(), torch.from_numpy(lab[partner]))
        assert y.lam.dtype == torch.float32 and torch.equal(y.lam.cpu(), torch.from_numpy(lam))
        assert np.array_equal(mix[:, 6], lam.view(np.int32))
        seen += 1
    assert seen == 9 and {1, 2} <= kinds
    torch.cuda.synchronize()


def test_pipeline_without_mixing_yields_what_it_always_yielded():
    src = P.SyntheticClipSource(2, 3, 24, seed=3, distinct=2)
    for tr in (P.ClipTransform(16, seed=1), P.ClipTransform(16, seed=1, mixup_alpha=0.8, train=False)):
        x, y = next(iter(P.ClipPipeline(itertools.islice(iter(src), 1), transform=tr)))
        assert isinstance(y, torch.Tensor) and torch.equal(y.cpu(), torch.from_numpy(src.batches[0][1]))
    torch.cuda.synchronize()


def test_opcheck_clip_transform_mix_and_its_argument_checks():
    srcd, rows = _dev(_source(3)), _dev(np.asarray(ROWS[(24, 24)], dtype=np.int32))
    mi = _dev(_mean_invstd(True, 3))
    mix = _dev(_mix_rows((1, 2, 0), boxes=[(0, 0, 0, 0), (2, 3, 5, 6), (0, 0, 0, 0)], lams=[lam_bits(0.3)] * 3))
    for m in (mi, None):
        torch.library.opcheck(torch.ops.hybrid.clip_transform_mix.default, (srcd, rows, mix, m, 3, 24, 24), test_utils=OPCHECK_TESTS)
    with pytest.raises(TypeError, match="mix must be int32"):
        P.clip_transform_mix(srcd, rows, mix.long(), mi, 3, 24, 24)
    with pytest.raises(TypeError, match="mix must be int32"):
        P.clip_transform_mix(srcd, rows, mix[:2], mi, 3, 24, 24)
    with pytest.raises(RuntimeError):
        P.clip_transform_mix(srcd, rows, mix.cpu(), mi, 3, 24, 24)
