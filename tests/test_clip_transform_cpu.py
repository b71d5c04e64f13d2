"""CPU: device-side clip augmentation (hyb_clips_u8_transform / hybrid::clip_transform / ClipTransform) as far as it goes without a
device: the C ABI declares and both builds export the entry point, its argument checks fail cleanly, the fp64 reference of the sampling
rule (tests/clip_transform_ref.py) IS torch's bilinear interpolate, and ClipTransform.sample draws what it documents."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import transformer_cnn_hybrid_network_for_video_processing_amd as P
from transformer_cnn_hybrid_network_for_video_processing_amd import _lib

from clip_transform_ref import clip_transform_ref

NAME = "hyb_clips_u8_transform"


@pytest.fixture(scope="module")
def built():
    from transformer_cnn_hybrid_network_for_video_processing_amd import build
    build.build()
    return _lib.lib


def test_header_declares_the_entry_point_with_13_parameters():
    protos = _lib.parse_header()
    assert NAME in protos
    ret, args = protos[NAME]
    assert ret == "int" and len(args) == 13
    assert args == ["ptr"] * 4 + ["int"] * 8 + ["ptr"]
    assert NAME not in _lib.DTYPE_FIRST                     # no dtype argument: always the main build


def test_both_libraries_export_it_and_the_abi_version_stays(built):
    for path in (_lib.LIB_PATH, _lib.LIB_X3_PATH):
        assert hasattr(ctypes.CDLL(path), NAME), f"{NAME} not exported by {os.path.basename(path)}"
    assert built.query("hyb_abi_version") == 9 and built.x3.query("hyb_abi_version") == 9


def test_argument_checks_fail_without_a_device(built):
    ok = dict(B=2, Tin=4, Hin=32, Win=32, C=3, Tout=4, Ho=16, Wo=16)
    bad = [dict(B=0), dict(Tin=0), dict(Hin=0), dict(Win=0), dict(C=0), dict(Tout=0), dict(Ho=0), dict(Wo=0), dict(C=5), dict(Hin=16385),
           dict(Win=16385), dict(Ho=16385), dict(Wo=16385)]
    p = 4096                                                # a made-up non-null address
    for lib in (built, built.x3):
        fn = lib.raw(NAME)
        for ptrs in ((None, None, None, None), (None, p, p, p), (p, None, p, p), (p, p, p, None), (p, None, None, p)):
            assert fn(*ptrs, *ok.values(), None) == -1     # a null pointer among them: refused whatever the checks of the extents do
        if not torch.cuda.is_available():
            # the extent checks need non-null pointers to be reached.  Without a device a check that failed to refuse would end in a failed
            # launch and a failed assertion; with one it would launch on the made-up address, so these cases run on device-less machines only
            for b in bad:
                assert fn(p, p, None, p, *{**ok, **b}.values(), None) == -1, b
    with pytest.raises(RuntimeError, match="argument check"):
        built.call(NAME, None, None, None, None, *ok.values(), None)


def _interp_ref(src, row, Tout, Ho, Wo):
    """The same clip through torch's own operator, in fp64: crop -> F.interpolate(bilinear, align_corners=False, antialias=False) / 255 -> flip."""
    y0, x0, ch, cw, flip, t0, ts = (int(v) for v in row[:7])
    frames = [src[min(max(t0 + t * ts, 0), src.shape[0] - 1)] for t in range(Tout)]
    crop = torch.from_numpy(np.stack(frames)[:, y0:y0 + ch, x0:x0 + cw]).permute(0, 3, 1, 2).to(torch.float64)
    out = F.interpolate(crop, (Ho, Wo), mode="bilinear", align_corners=False, antialias=False) / 255
    return (out.flip(-1) if flip else out).numpy()


# (Hin, Win, C, row, Ho, Wo): up-scale, down-scale (mild and beyond 2x), non-square, a 1x1 crop, a one-column crop, flip, temporal windows
CASES = [
    (37, 53, 3, (0, 0, 37, 53, 0, 0, 1, 0), 24, 24),
    (37, 53, 3, (5, 7, 30, 41, 1, 0, 1, 0), 24, 24),
    (37, 53, 3, (3, 11, 20, 33, 1, 1, 2, 0), 9, 13),
    (37, 53, 3, (30, 44, 7, 9, 0, 2, 1, 0), 24, 24),
    (37, 53, 3, (30, 44, 7, 9, 1, 0, 2, 0), 24, 20),
    (37, 53, 1, (17, 29, 1, 1, 1, 0, 1, 0), 8, 8),
    (37, 53, 3, (2, 50, 33, 1, 1, 0, 1, 0), 8, 12),
    (16, 16, 3, (0, 0, 16, 16, 0, 0, 1, 0), 16, 16),
    (36, 52, 3, (0, 0, 36, 52, 1, 0, 1, 0), 18, 26),
    (10, 10, 3, (0, 0, 10, 10, 0, 0, 1, 0), 20, 20),
    (64, 64, 4, (1, 2, 60, 61, 1, 0, 1, 0), 7, 5),
]


@pytest.mark.parametrize("Hin,Win,C,row,Ho,Wo", CASES)
def test_reference_is_torch_bilinear_interpolate(Hin, Win, C, row, Ho, Wo):
    rng = np.random.default_rng(Hin * 131 + Wo)
    Tin, Tout = 5, 3
    src = rng.integers(0, 256, (1, Tin, Hin, Win, C), dtype=np.uint8)
    got = clip_transform_ref(src, [row], None, Tout, Ho, Wo)[0]
    want = _interp_ref(src[0], row, Tout, Ho, Wo)
    assert got.shape == want.shape == (Tout, C, Ho, Wo)
    err = np.abs(got - want).max()
    assert err <= 1e-12, err


def test_reference_exact_cases():
    rng = np.random.default_rng(3)
    src = rng.integers(0, 256, (1, 1, 36, 52, 3), dtype=np.uint8)
    ident = clip_transform_ref(src, [(0, 0, 36, 52, 0, 0, 1, 0)], None, 1, 36, 52)
    assert np.array_equal(ident, src.transpose(0, 1, 4, 2, 3).astype(np.float64) / 255.0)
    half = clip_transform_ref(src, [(0, 0, 36, 52, 0, 0, 1, 0)], None, 1, 18, 26)
    s = src.astype(np.float64).reshape(1, 1, 18, 2, 26, 2, 3).sum(axis=(3, 5)).transpose(0, 1, 4, 2, 3)
    assert np.array_equal(half, s / 4 / 255.0)
    mi = np.array([[0.485, 0.456, 0.406], [1 / 0.229, 1 / 0.224, 1 / 0.225]], dtype=np.float32)
    norm = clip_transform_ref(src, [(0, 0, 36, 52, 0, 0, 1, 0)], mi, 1, 36, 52)
    assert np.array_equal(norm, (ident - mi[0].astype(np.float64)[:, None, None]) * mi[1].astype(np.float64)[:, None, None])


def test_sample_rows_lie_inside_the_clip_and_follow_scale_and_ratio():
    B, Tin, Hin, Win = 64, 16, 96, 128
    tr = P.ClipTransform(32, scale=(0.35, 1.0), ratio=(3 / 4, 4 / 3), frames=5, frame_stride=(1, 3), seed=11)
    rows = tr.sample(B, Tin, Hin, Win)
    assert rows.shape == (B, 8) and rows.dtype == np.int32
    y0, x0, ch, cw, flip, t0, ts, pad = rows.T.astype(np.int64)
    assert (y0 >= 0).all() and (x0 >= 0).all() and (ch >= 1).all() and (cw >= 1).all()
    assert (y0 + ch <= Hin).all() and (x0 + cw <= Win).all()
    assert set(flip.tolist()) <= {0, 1} and (pad == 0).all()
    assert (ts >= 1).all() and (ts <= 3).all() and (t0 >= 0).all() and (t0 + 4 * ts <= Tin - 1).all()
    # sides are rounded to integers: each moves by at most 1/2, so area and ratio sit within that of the drawn values
    lo_a, hi_a = 0.35 * Hin * Win, 1.0 * Hin * Win
    assert ((ch + 0.5) * (cw + 0.5) >= lo_a).all() and ((ch - 0.5) * (cw - 0.5) <= hi_a).all()
    assert ((cw + 0.5) / (ch - 0.5) >= 3 / 4).all() and ((cw - 0.5) / (ch + 0.5) <= 4 / 3).all()
    assert len({tuple(r) for r in rows.tolist()}) > 1                   # one row per clip, not one per batch
    assert len(set(ts.tolist())) > 1 and len(set(t0.tolist())) > 1


def test_sample_is_a_seeded_stream():
    a, b, c = (P.ClipTransform(24, frames=3, frame_stride=(1, 2), seed=s) for s in (5, 5, 6))
    ra = [a.sample(4, 8, 40, 48) for _ in range(3)]
    rb = [b.sample(4, 8, 40, 48) for _ in range(3)]
    rc = [c.sample(4, 8, 40, 48) for _ in range(3)]
    assert all(np.array_equal(x, y) for x, y in zip(ra, rb))
    assert not np.array_equal(ra[0], ra[1])                             # the stream advances
    assert not all(np.array_equal(x, y) for x, y in zip(ra, rc))        # another seed (seed + rank), other rows


def test_flip_frequency():
    rows = P.ClipTransform(8, seed=1).sample(4000, 1, 16, 16)
    assert abs(rows[:, 4].mean() - 0.5) <= 0.04                         # 5 sigma of Binomial(4000, 0.5) / 4000 = 0.0395
    assert P.ClipTransform(8, hflip=0.0, seed=1).sample(50, 1, 16, 16)[:, 4].sum() == 0
    assert P.ClipTransform(8, hflip=1.0, seed=1).sample(50, 1, 16, 16)[:, 4].sum() == 50


def test_frames_none_keeps_every_frame():
    tr = P.ClipTransform(8, seed=2)
    rows = tr.sample(6, 7, 20, 20)
    assert tr.out_frames(7) == 7 and (rows[:, 5] == 0).all() and (rows[:, 6] == 1).all()


def test_eval_transform_is_deterministic_and_centred():
    tr = P.ClipTransform((16, 32), frames=4, frame_stride=(2, 3), seed=9, train=False)
    r1, r2 = tr.sample(3, 12, 60, 100), tr.sample(3, 12, 60, 100)
    assert np.array_equal(r1, r2) and (r1 == r1[0]).all()
    # 60 x 100 source, 1:2 output: the largest 1:2 crop is 50 x 100, centred; window of (4-1)*2+1 = 7 frames centred in 12
    assert r1[0].tolist() == [5, 0, 50, 100, 0, 2, 2, 0]
    tall = P.ClipTransform((16, 32), train=False).sample(1, 3, 100, 60)
    assert tall[0].tolist() == [35, 0, 30, 60, 0, 0, 1, 0]
    assert P.ClipTransform(24, train=False, seed=1).sample(2, 2, 24, 24)[1].tolist() == [0, 0, 24, 24, 0, 0, 1, 0]


def test_fallback_crop_when_no_try_fits():
    # a 10 x 200 strip: no crop with ratio in [3/4, 4/3] and >= 35% of the area fits, so the centred fallback with the ratio clamped to 4/3
    rows = P.ClipTransform(8, seed=0).sample(5, 1, 10, 200)
    assert (rows[:, :4] == np.array([0, 93, 10, 13])).all()


def test_value_errors():
    with pytest.raises(ValueError, match="zero"):
        P.ClipTransform(8, mean=(0.5, 0.5, 0.5), std=(0.2, 0.0, 0.2))
    with pytest.raises(ValueError, match="both or neither"):
        P.ClipTransform(8, mean=(0.5, 0.5, 0.5))
    with pytest.raises(ValueError, match="both or neither"):
        P.ClipTransform(8, std=(0.5, 0.5, 0.5))
    with pytest.raises(ValueError, match="channels"):
        P.ClipTransform(8, mean=(0.5, 0.5), std=(0.2, 0.2)).mean_invstd(3)
    with pytest.raises(ValueError, match="exceeds the clip length"):
        P.ClipTransform(8, frames=9).sample(2, 8, 16, 16)
    mi = P.ClipTransform(8, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)).mean_invstd(3)
    assert mi.dtype == np.float32 and mi.shape == (2, 3)
    assert np.array_equal(mi[0], np.array([0.485, 0.456, 0.406], dtype=np.float32))
    assert np.array_equal(mi[1], np.float32(1) / np.array([0.229, 0.224, 0.225], dtype=np.float32))


def test_cpu_tensors_and_cpu_pipeline_are_refused():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.ClipPipeline(P.SyntheticClipSource(1, 2, 8), device="cpu", transform=P.ClipTransform(8))
    src = torch.zeros(1, 2, 8, 8, 3, dtype=torch.uint8)
    rows = torch.from_numpy(P.ClipTransform(4).sample(1, 2, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.clip_transform(src, rows, None, 2, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        torch.ops.hybrid.clip_transform(src, rows, None, 2, 4, 4)


def test_operator_has_a_fake_kernel_and_checks_its_arguments():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        src = torch.empty(2, 5, 20, 24, 3, dtype=torch.uint8)
        rows = torch.empty(2, 8, dtype=torch.int32)
        mi = torch.empty(2, 3)
        out = torch.ops.hybrid.clip_transform(src, rows, mi, 3, 12, 16)
        assert out.shape == (2, 3, 3, 12, 16) and out.dtype == torch.float32
        with pytest.raises(TypeError, match="int32"):
            torch.ops.hybrid.clip_transform(src, rows.long(), mi, 3, 12, 16)
        with pytest.raises(TypeError, match="uint8"):
            torch.ops.hybrid.clip_transform(src.float(), rows, mi, 3, 12, 16)
        with pytest.raises(TypeError, match="mean_invstd"):
            torch.ops.hybrid.clip_transform(src, rows, torch.empty(2, 4), 3, 12, 16)
