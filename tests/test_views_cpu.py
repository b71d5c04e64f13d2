"""CPU: multi-view evaluation clips (ClipTransform(train=False, eval_views=(K, S), eval_crop=..., eval_flip=...), hyb_clips_u8_transform_views) as
far as they go without a device: the sampler's rule -- pinned on the "resize 256, crop 224, 3 windows x 3 crops" layout, landscape and portrait --,
that no row it makes needs the kernel's clamps, that the training draws did not move, and the new entry point's declaration, export and argument
checks in both builds."""
import ctypes

import numpy as np
import pytest
import torch

import transformer_cnn_hybrid_network_for_video_processing_amd as P
from transformer_cnn_hybrid_network_for_video_processing_amd import _lib

NAME = "hyb_clips_u8_transform_views"
HYB_E_ARG = -1


@pytest.fixture(scope="module")
def built():
    from transformer_cnn_hybrid_network_for_video_processing_amd import build
    build.build()
    return _lib.lib


# ---- the sampler ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Tin,Hin,Win,size,frames", [(8, 32, 32, 16, None), (12, 256, 340, 224, 4), (9, 340, 256, (224, 112), 5), (5, 37, 53, (9, 13), 5),
                                                     (16, 24, 40, (40, 24), 3)])
def test_default_views_are_the_rows_of_sample(Tin, Hin, Win, size, frames):
    kw = dict(train=False, frames=frames, frame_stride=(2, 3) if frames == 3 else (1, 1))
    a, b = P.ClipTransform(size, **kw), P.ClipTransform(size, **kw)
    assert a.views == 1
    rows = a.sample_views(3, Tin, Hin, Win)
    assert rows.dtype == np.int32 and rows.shape == (3, 8)
    assert np.array_equal(rows, b.sample(3, Tin, Hin, Win))


def test_three_windows_by_three_crops_on_a_landscape_source():
    tr = P.ClipTransform(224, train=False, frames=4, eval_views=(3, 3), eval_crop=224 / 256)
    assert tr.views == 9
    rows = tr.sample_views(2, 12, 256, 340)
    assert rows.dtype == np.int32 and rows.shape == (18, 8)
    want = [(16, x0, 224, 224, 0, t0, 1, 0) for t0 in (0, 4, 8) for x0 in (0, 58, 116)]          # window k, then crop s: left, centre, right
    assert rows.tolist() == [list(r) for r in want] * 2                                             # clip-major: every clip the same nine rows


def test_a_portrait_source_spreads_the_crops_along_y():
    tr = P.ClipTransform(224, train=False, frames=4, eval_views=(3, 3), eval_crop=224 / 256)
    rows = tr.sample_views(1, 12, 340, 256)
    want = [(y0, 16, 224, 224, 0, t0, 1, 0) for t0 in (0, 4, 8) for y0 in (0, 58, 116)]
    assert rows.tolist() == [list(r) for r in want]


def test_flipped_twins_follow_their_views():
    plain = P.ClipTransform(224, train=False, frames=4, eval_views=(3, 3), eval_crop=224 / 256)
    tr = P.ClipTransform(224, train=False, frames=4, eval_views=(3, 3), eval_crop=224 / 256, eval_flip=True)
    assert tr.views == 18
    rows, base = tr.sample_views(2, 12, 256, 340), plain.sample_views(2, 12, 256, 340)
    assert rows.shape == (36, 8)
    assert np.array_equal(rows[0::2], base)                           # flip is the fastest index: rows 2i are the unflipped layout ...
    twin = rows[1::2].copy()
    assert np.all(twin[:, 4] == 1) and np.all(rows[0::2, 4] == 0)
    twin[:, 4] = 0
    assert np.array_equal(twin, base)                                 # ... and rows 2i + 1 differ from them in the flip field only


def test_views_that_coincide_without_slack_are_allowed():
    rows = P.ClipTransform(16, train=False, frames=6, eval_views=(2, 3)).sample_views(1, 6, 32, 32)      # square source, full crop, Tout == Tin
    assert rows.shape == (6, 8) and len({tuple(r) for r in rows.tolist()}) == 1
    assert rows[0].tolist() == [0, 0, 32, 32, 0, 0, 1, 0]


@pytest.mark.parametrize("eval_flip", [False, True])
@pytest.mark.parametrize("K,S", [(1, 1), (1, 3), (2, 1), (3, 3), (4, 5), (10, 3)])
def test_no_row_needs_a_clamp(K, S, eval_flip):
    seen = 0
    for (Hin, Win), size, crop, (Tin, frames, fs) in [((256, 340), 224, 224 / 256, (32, 16, (1, 1))), ((340, 256), 224, 224 / 256, (32, 16, (2, 2))),
                                                      ((37, 53), (9, 13), 0.5, (7, 3, (1, 3))), ((53, 37), (24, 24), 1.0, (5, 5, (1, 1))),
                                                      ((16, 16), 16, 1.0, (12, 4, (3, 3))), ((8, 9), (3, 7), 0.01, (4, 1, (1, 1))),
                                                      ((31, 31), (4, 30), 0.9, (11, 10, (1, 1)))]:
        tr = P.ClipTransform(size, train=False, frames=frames, frame_stride=fs, eval_views=(K, S), eval_crop=crop, eval_flip=eval_flip)
        rows = tr.sample_views(2, Tin, Hin, Win).astype(np.int64)
        V = K * S * (2 if eval_flip else 1)
        assert tr.views == V and rows.shape == (2 * V, 8)
        y0, x0, ch, cw, flip, t0, ts = rows[:, :7].T
        assert np.all(y0 >= 0) and np.all(x0 >= 0) and np.all(ch >= 1) and np.all(cw >= 1) and np.all(t0 >= 0) and np.all(ts >= 1)
        assert np.all(y0 + ch <= Hin) and np.all(x0 + cw <= Win)
        assert np.all(t0 + (tr.out_frames(Tin) - 1) * ts <= Tin - 1)
        assert np.all((flip == 0) | (flip == 1)) and np.all(rows[:, 7] == 0)
        if S > 1:                                                     # the first and last crops touch the two borders of the spread axis
            first, last = rows[0], rows[(S - 1) * (2 if eval_flip else 1)]
            if Win - cw[0] >= Hin - ch[0]:
                assert first[1] == 0 and last[1] + last[3] == Win
            else:
                assert first[0] == 0 and last[0] + last[2] == Hin
        if K > 1:                                                     # and the first and last windows the two ends of the clip
            assert rows[0, 5] == 0 and rows[V - 1, 5] + (tr.out_frames(Tin) - 1) * rows[V - 1, 6] == Tin - 1
        seen += 1
    assert seen == 7


def test_sample_views_draws_nothing():
    tr = P.ClipTransform(16, train=False, frames=3, eval_views=(2, 3), eval_flip=True, seed=11)
    states = [g.bit_generator.state for g in (tr.rng, tr.mix_rng, tr.photo_rng)]
    a = tr.sample_views(3, 9, 24, 40)
    b = tr.sample_views(3, 9, 24, 40)
    assert np.array_equal(a, b)
    assert states == [g.bit_generator.state for g in (tr.rng, tr.mix_rng, tr.photo_rng)]


def test_views_is_one_when_training():
    assert P.ClipTransform(16).views == 1
    assert P.ClipTransform(16, train=True, mixup_alpha=0.8).views == 1
    assert P.ClipTransform(16, train=False).views == 1
    assert P.ClipTransform(16, train=False, frames=2, eval_views=(2, 3), eval_flip=True).views == 12


def test_constructor_refuses_what_the_rule_cannot_serve():
    for kw in (dict(eval_views=(1, 3)), dict(eval_views=(2, 1), frames=4), dict(eval_crop=0.875), dict(eval_flip=True)):
        with pytest.raises(ValueError, match="train=False"):
            P.ClipTransform(16, train=True, **kw)
    with pytest.raises(ValueError, match="frames"):
        P.ClipTransform(16, train=False, eval_views=(2, 1))                   # K > 1 without frames: every window would be the whole clip
    for crop in (0.0, -0.5, 1.0001, 2.0, float("nan")):
        with pytest.raises(ValueError, match="eval_crop"):
            P.ClipTransform(16, train=False, eval_crop=crop)
    for views in ((0, 1), (1, 0), (-1, 3)):
        with pytest.raises(ValueError, match="eval_views"):
            P.ClipTransform(16, train=False, frames=2, eval_views=views)
    with pytest.raises(ValueError, match="train=False"):
        P.ClipTransform(16).sample_views(1, 4, 32, 32)


def test_the_training_draws_did_not_move():
    """The same calls on a transform constructed WITHOUT the new arguments and on one that names their defaults: the rows of sample / sample_mix /
    sample_photo are equal (tests/test_clip_transform_cpu.py, test_mix_cpu.py and test_photo_cpu.py pin the draws themselves)."""
    kw = dict(frames=3, frame_stride=(1, 2), seed=5, mixup_alpha=0.8, cutmix_alpha=1.0, mix_mode="clip", brightness=0.4, contrast=0.4, saturation=0.4,
              noise_std=(0.05, 0.2), erase_prob=0.7)
    old, new = P.ClipTransform(16, **kw), P.ClipTransform(16, eval_views=(1, 1), eval_crop=1.0, eval_flip=False, **kw)
    for _ in range(3):
        assert np.array_equal(old.sample(4, 7, 24, 40), new.sample(4, 7, 24, 40))
        for a, b in zip(old.sample_mix(4, 16, 16), new.sample_mix(4, 16, 16)):
            assert np.array_equal(a, b)
        assert np.array_equal(old.sample_photo(4, 3, 16, 16), new.sample_photo(4, 3, 16, 16))
    # and the evaluation transform's one row is what it was
    assert P.ClipTransform((16, 32), train=False, frames=3).sample(1, 8, 24, 40).tolist() == [[2, 0, 20, 40, 0, 2, 1, 0]]


# ---- the entry point --------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_point():
    protos = _lib.parse_header()
    # src, params, mean_invstd, dst | B, V, Tin, Hin, Win, C, Tout, Ho, Wo | stream
    assert protos[NAME] == ("int", ["ptr"] * 4 + ["int"] * 9 + ["ptr"])
    assert len(protos[NAME][1]) == len(protos["hyb_clips_u8_transform"][1]) + 1
    assert NAME not in _lib.DTYPE_FIRST


def test_both_libraries_export_it_under_abi_9(built):
    for path in (_lib.LIB_PATH, _lib.LIB_X3_PATH):
        assert hasattr(ctypes.CDLL(path), NAME), f"{NAME} is not exported by {path}"
    assert NAME in built.protos
    assert built.query("hyb_abi_version") == 9 and built.x3.query("hyb_abi_version") == 9


@pytest.mark.parametrize("which", ["main", "x3"])
def test_argument_checks_come_before_any_device_call(built, which):
    lib = built if which == "main" else built.x3
    fn = lib.raw(NAME)
    assert fn(*[None if a == "ptr" else 0 for a in lib.protos[NAME][1]]) == HYB_E_ARG
    ok = dict(B=2, V=3, Tin=4, Hin=32, Win=32, C=3, Tout=4, Ho=16, Wo=16)
    buf = (ctypes.c_longlong * 64)()                                # never read: the argument checks come before any HIP call
    p = ctypes.addressof(buf)
    for ptrs in ((None, p, None, p), (p, None, None, p), (p, p, None, None), (None, None, None, None)):
        assert fn(*ptrs, *ok.values(), None) == HYB_E_ARG, ptrs
    assert fn(None, None, None, None, *{**ok, "V": 0}.values(), None) == HYB_E_ARG
    with pytest.raises(RuntimeError, match="argument check"):
        lib.call(NAME, None, None, None, None, *ok.values(), None)
    if torch.cuda.is_available():
        # the extent checks need non-null pointers to be reached; on a machine with a device a check that failed to refuse would launch on this
        # host buffer, so those cases run on device-less machines only (as in tests/test_clip_transform_cpu.py)
        return
    bad = [dict(V=0), dict(V=-1), dict(B=65536, V=65536), dict(B=2 ** 31 - 1, V=2), dict(B=2, V=2 ** 30), dict(B=0), dict(Tin=0), dict(Hin=0),
           dict(Win=0), dict(C=0), dict(Tout=0), dict(Ho=0), dict(Wo=0), dict(C=5), dict(Hin=16385), dict(Win=16385), dict(Ho=16385), dict(Wo=16385)]
    for b in bad:
        assert fn(p, p, None, p, *{**ok, **b}.values(), None) == HYB_E_ARG, b
