"""GPU: clip augmentation on the device (hyb_clips_u8_transform through hybrid::clip_transform and ClipPipeline(transform=...)).

The kernel is held to tests/clip_transform_ref.py, the fp64 restatement of the sampling rule that tests/test_clip_transform_cpu.py pins
to torch's bilinear interpolate.  Three cases are exact by construction and compared with torch.equal (identity = ToTensor, 2x
down-scale, 2x up-scale); everything else is compared element by element against the reference with

    tol = 2^-20 * max(1, max_c invstd_c)        absolute

from the rule's own arithmetic: about nine fp32 roundings (three lerps on values <= 255 with one correctly rounded fraction each, the
division by 255, the subtraction, the multiplication), each at most 2^-24 relative, so ~12 * 2^-24 * invstd; the gate is 16 * 2^-24.
Nothing is summed, so no re-ordering has to be allowed for.  Shapes are the smallest at which the kernel's paths differ: Wo % 4 == 0
(16-byte stores) and not (scalar tail), more than one block per frame, up- and down-scale, a 1x1 crop, flip, C = 1 and 3."""
import functools
import itertools

import numpy as np
import pytest
import torch

import transformer_cnn_hybrid_network_for_video_processing_amd as P

from clip_transform_ref import clamp_rows, clip_transform_ref

pytestmark = pytest.mark.gpu

IMAGENET = dict(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))


def _run(src, rows, mi, Tout, Ho, Wo):
    out = P.clip_transform(torch.from_numpy(src).cuda(), torch.from_numpy(np.asarray(rows, dtype=np.int32).reshape(-1, 8)).cuda(),
                           None if mi is None else torch.from_numpy(mi).cuda(), Tout, Ho, Wo)
    assert out.shape == (src.shape[0], Tout, src.shape[4], Ho, Wo) and out.dtype == torch.float32 and out.is_cuda
    return out.cpu()


def _to_tensor_kernel(src):
    from transformer_cnn_hybrid_network_for_video_processing_amd._lib import lib
    B, T, H, W, C = src.shape
    d = torch.from_numpy(src).cuda()
    out = torch.empty(B, T, C, H, W, device="cuda")
    lib.call("hyb_frames_u8hwc_to_f32chw", d, out, B * T, H, W, C, torch.cuda.current_stream().cuda_stream)
    return out.cpu()


def test_identity_rows_are_the_totensor_kernel_bit_for_bit():
    src = np.ascontiguousarray(np.broadcast_to(np.arange(256, dtype=np.uint8).reshape(1, 1, 16, 16, 1), (1, 2, 16, 16, 3)))      # every byte value
    got = _run(src, [(0, 0, 16, 16, 0, 0, 1, 0)], None, 2, 16, 16)
    assert torch.equal(got, _to_tensor_kernel(src))
    assert torch.equal(got, torch.from_numpy(src).permute(0, 1, 4, 2, 3).to(torch.float32).div(255))


def test_2x_downscale_is_the_rounded_mean_of_four_bytes():
    src = np.random.default_rng(0).integers(0, 256, (2, 2, 36, 52, 3), dtype=np.uint8)
    got = _run(src, [(0, 0, 36, 52, 0, 0, 1, 0)] * 2, None, 2, 18, 26)                    # Wo = 26: the scalar tail path
    s = torch.from_numpy(src).to(torch.float32).reshape(2, 2, 18, 2, 26, 2, 3).sum(dim=(3, 5)).permute(0, 1, 4, 2, 3)
    assert torch.equal(got, (s / 4) / 255)


def test_2x_upscale_is_the_fp64_result_rounded_once():
    src = np.random.default_rng(1).integers(0, 256, (1, 1, 10, 10, 3), dtype=np.uint8)
    row = [(0, 0, 10, 10, 0, 0, 1, 0)]
    got = _run(src, row, None, 1, 20, 20)                                                  # fractions 1/4 and 3/4: every lerp is exact
    assert torch.equal(got, torch.from_numpy(clip_transform_ref(src, row, None, 1, 20, 20)).to(torch.float32))


# ---- general cases: B = 3 clips of 5 frames 37 x 53, a different row per clip; Tout = 3 (stride 2 from t0 = 0; stride 1 from t0 = 2) -------
ROWS = {
    # full frame (down-scale) | a 7 x 9 crop (up-scale), flipped | a 20 x 33 crop, flipped
    (24, 24): [(0, 0, 37, 53, 0, 0, 2, 0), (30, 44, 7, 9, 1, 2, 1, 0), (3, 11, 20, 33, 1, 0, 1, 0)],
    (9, 13): [(0, 0, 37, 53, 1, 0, 2, 0), (30, 44, 7, 9, 0, 2, 1, 0), (3, 11, 20, 33, 1, 0, 1, 0)],
    # 1 x 1 crops (flipped, and the frame's last pixel) | full frame, beyond 2x down
    (8, 8): [(17, 29, 1, 1, 1, 0, 2, 0), (36, 52, 1, 1, 0, 2, 1, 0), (0, 0, 37, 53, 1, 0, 1, 0)],
    # a frame wider than one block of quads (64 x 64 / 4 = 1024 positions = 4 blocks), up-scale with flip
    (64, 64): [(0, 0, 37, 53, 1, 0, 2, 0), (30, 44, 7, 9, 1, 2, 1, 0), (3, 11, 20, 33, 0, 0, 1, 0)],
}


@functools.lru_cache(maxsize=None)
def _source(C):
    return np.random.default_rng(40 + C).integers(0, 256, (3, 5, 37, 53, C), dtype=np.uint8)


def _mean_invstd(norm, C):
    return P.ClipTransform(8, **IMAGENET).mean_invstd(3) if norm else None


@functools.lru_cache(maxsize=None)
def _reference(size, C, norm):
    return clip_transform_ref(_source(C), ROWS[size], _mean_invstd(norm, C), 3, *size)


@pytest.mark.parametrize("C,norm", [(3, True), (3, False), (1, False)], ids=["rgb-imagenet", "rgb-plain", "grey"])
@pytest.mark.parametrize("size", list(ROWS), ids=lambda s: f"{s[0]}x{s[1]}")
def test_general_cases_against_the_fp64_reference(size, C, norm):
    mi = _mean_invstd(norm, C)
    got = _run(_source(C), ROWS[size], mi, 3, *size).double().numpy()
    want = _reference(size, C, norm)
    tol = 2.0 ** -20 * max(1.0, float(mi[1].max()) if mi is not None else 1.0)
    err = np.abs(got - want).max()
    print(f"clip_transform {size} C={C} norm={norm}: max abs err {err:.3e} (tol {tol:.3e})")
    assert err <= tol


# ---- clamping: rows that overshoot must behave exactly like their clamped twins.  The source sits in the middle of a larger allocation and
# every unclamped address of these rows would still fall inside it: a clamping bug shows as wrong values, never as a fault. ---------------
CLAMP_CASES = [
    # clip 0: rectangle 2 rows / 2 columns past the frame, flip = 7, t0 + t*tstride past Tin-1 | clip 1: negative offsets, ch = 0, negative t0
    ([(10, 9, 8, 9, 7, 1, 1, 0), (-2, -1, 0, 18, 0, -1, 1, 0)], [(10, 9, 6, 7, 1, 1, 0, 0), (0, 0, 1, 16, 0, 0, 0, 0)]),
    # clip 0: offsets past the frame, stride 5 | clip 1: negative extents, a negative stride from past the end
    ([(17, 18, 4, 4, 0, 0, 5, 0), (3, 3, -5, -5, 1, 3, -1, 0)], [(15, 15, 1, 1, 0, 0, 1, 0), (3, 3, 1, 1, 1, 1, 0, 0)]),
]


@pytest.mark.parametrize("size", [(8, 8), (5, 7)], ids=["vec", "tail"])
@pytest.mark.parametrize("rows,clamped", CLAMP_CASES, ids=["overshoot", "far"])
def test_out_of_range_rows_equal_their_clamped_twins(rows, clamped, size):
    B, T, H, W, C = 2, 2, 16, 16, 3
    n = B * T * H * W * C
    big = torch.from_numpy(np.random.default_rng(7).integers(0, 256, (3 * n,), dtype=np.uint8)).cuda()
    src = big[n:2 * n].view(B, T, H, W, C)
    assert np.array_equal(clamp_rows(rows, H, W)[:, :5], np.asarray(clamped)[:, :5])
    mi = torch.from_numpy(_mean_invstd(True, C)).cuda()
    out = [P.clip_transform(src, torch.tensor(r, dtype=torch.int32).cuda(), mi, 2, *size).cpu() for r in (rows, clamped)]
    assert torch.equal(out[0], out[1])
    want = clip_transform_ref(src.cpu().numpy(), clamped, mi.cpu().numpy(), 2, *size)
    assert np.abs(out[0].double().numpy() - want).max() <= 2.0 ** -20 * float(mi[1].max())


# ---- the pipeline ------------------------------------------------------------------------------------------------------------------------
def _to_tensor(frames_u8):
    return torch.from_numpy(frames_u8).permute(0, 1, 4, 2, 3).contiguous().to(torch.float32).div(255)


def test_pipeline_applies_one_row_per_clip_and_recycles_its_slots():
    src = P.SyntheticClipSource(3, 5, 24, distinct=7)
    kw = dict(frames=3, frame_stride=(1, 2), seed=5, **IMAGENET)
    pipe = P.ClipPipeline(itertools.islice(iter(src), 11), depth=2, transform=P.ClipTransform(16, **kw))
    twin = P.ClipTransform(16, **kw)
    mi = torch.from_numpy(twin.mean_invstd(3)).cuda()
    seen, all_rows = 0, []
    for i, (x, y) in enumerate(pipe):                       # 11 batches over 3 slots: every slot's byte and parameter buffers are reused
        fr, lab = src.batches[i % 7]
        rows = twin.sample(3, 5, 24, 24)
        all_rows.append(rows)
        assert x.shape == (3, 3, 3, 16, 16) and x.dtype == torch.float32 and x.is_cuda
        want = P.clip_transform(torch.from_numpy(fr).cuda(), torch.from_numpy(rows).cuda(), mi, 3, 16, 16)
        assert torch.equal(x, want), f"batch {i}"
        assert torch.equal(y.cpu(), torch.from_numpy(lab))
        seen += 1
    assert seen == 11
    assert len({tuple(r) for rows in all_rows for r in rows.tolist()}) > 11       # the batches really were augmented differently
    torch.cuda.synchronize()


def test_pipeline_without_a_transform_is_still_totensor():
    src = P.SyntheticClipSource(2, 3, 24, seed=3, distinct=2)
    n = 0
    for i, (x, y) in enumerate(P.ClipPipeline(itertools.islice(iter(src), 4), depth=2, transform=None)):
        assert torch.equal(x.cpu(), _to_tensor(src.batches[i % 2][0])) and torch.equal(y.cpu(), torch.from_numpy(src.batches[i % 2][1]))
        n += 1
    assert n == 4


def test_pipeline_checks_the_channel_count_at_the_first_batch():
    pipe = P.ClipPipeline(itertools.islice(iter(P.SyntheticClipSource(1, 2, 8)), 1), transform=P.ClipTransform(4, mean=(0.5,), std=(0.5,)))
    with pytest.raises(ValueError, match="channels"):
        next(iter(pipe))


def test_captured_launch_replays_with_new_parameter_rows():
    src = torch.from_numpy(_source(3)).cuda()
    mi = torch.from_numpy(_mean_invstd(True, 3)).cuda()
    first, second = (torch.tensor(ROWS[k], dtype=torch.int32) for k in ((24, 24), (64, 64)))
    params = first.cuda()
    eager_first = P.clip_transform(src, params, mi, 3, 24, 24)       # also loads the kernel before the capture
    eager_second = P.clip_transform(src, second.cuda(), mi, 3, 24, 24)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                        # one kernel node, no parallel branches
        out = P.clip_transform(src, params, mi, 3, 24, 24)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager_first)
    params.copy_(second)                                             # the rows are device memory: nothing of them was baked into the node
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager_second) and not torch.equal(out, eager_first)


def test_pipeline_feeds_the_model():
    torch.manual_seed(0)
    m = P.TransformerCNNHybrid(cnn_channels=(32, 64), d_model=64, num_heads=4, num_layers=1, hidden_dim=128).cuda().eval()
    src = P.SyntheticClipSource(2, 6, 40, seed=2, distinct=3)
    kw = dict(frames=4, frame_stride=(1, 1), seed=8, **IMAGENET)
    twin = P.ClipTransform(32, **kw)
    mi = torch.from_numpy(twin.mean_invstd(3)).cuda()
    outs = []
    with torch.no_grad():
        for x, y in P.ClipPipeline(itertools.islice(iter(src), 4), depth=2, transform=P.ClipTransform(32, **kw)):
            outs.append(m(x).clone())
        for i, o in enumerate(outs):
            rows = torch.from_numpy(twin.sample(2, 6, 40, 40)).cuda()
            direct = P.clip_transform(torch.from_numpy(src.batches[i % 3][0]).cuda(), rows, mi, 4, 32, 32)
            assert torch.isfinite(o).all() and torch.equal(o, m(direct))


def test_operator_checks_its_arguments():
    src = torch.from_numpy(_source(3)).cuda()
    rows = torch.tensor(ROWS[(8, 8)], dtype=torch.int32).cuda()
    with pytest.raises(TypeError, match="int32"):
        P.clip_transform(src, rows.long(), None, 3, 8, 8)
    with pytest.raises(TypeError, match="mean_invstd"):
        P.clip_transform(src, rows, torch.zeros(3, 2, device="cuda"), 3, 8, 8)
    with pytest.raises(TypeError, match="uint8"):
        P.clip_transform(src.float(), rows, None, 3, 8, 8)
