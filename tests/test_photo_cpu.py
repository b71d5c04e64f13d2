"""Colour jitter, Gaussian noise and random erasing as far as they go without a GPU: the two new entry points of both libraries, the fp64
reference (tests/photo_ref.py) against its own building blocks, the noise generator's moments, and ClipTransform's photo draws."""
import ctypes

import numpy as np
import pytest

import transformer_cnn_hybrid_network_for_video_processing_amd as P
from transformer_cnn_hybrid_network_for_video_processing_amd import _lib

from clip_transform_ref import clamp_rows, clip_transform_ref
from photo_ref import LUMA_W, ONE_BITS, clamp_photo_rows, clip_photo_ref, f32_bits, luma_sums_ref, noise_z, photo_row

NEW = ("hyb_clips_u8_transform_photo", "hyb_clips_u8_luma_sums")
HYB_E_ARG = -1
IMAGENET = dict(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
ALL_ON = dict(brightness=0.4, contrast=0.4, saturation=0.4, jitter_prob=0.8, grayscale=0.2, noise_std=(0.05, 0.2), noise_prob=0.5, erase_prob=0.7,
              erase_mode="pixel")


@pytest.fixture(scope="module")
def built():
    from transformer_cnn_hybrid_network_for_video_processing_amd import build
    build.build()
    return _lib.lib


def test_header_declares_both_entry_points_with_their_parameter_lists():
    protos = _lib.parse_header()
    # src, params, mix, photo, luma_sums, mean_invstd, dst | B, Tin, Hin, Win, C, Tout, Ho, Wo | stream
    assert protos["hyb_clips_u8_transform_photo"] == ("int", ["ptr"] * 7 + ["int"] * 8 + ["ptr"])
    # src, params, sums | B, Tin, Hin, Win, C, Tout | stream
    assert protos["hyb_clips_u8_luma_sums"] == ("int", ["ptr"] * 3 + ["int"] * 6 + ["ptr"])
    assert len(protos["hyb_clips_u8_transform_photo"][1]) == len(protos["hyb_clips_u8_transform_mix"][1]) + 2


def test_both_libraries_export_the_new_symbols_under_abi_9(built):
    for path in (_lib.LIB_PATH, _lib.LIB_X3_PATH):
        dll = ctypes.CDLL(path)
        for name in NEW:
            assert name in built.protos, name
            assert hasattr(dll, name), f"{name} is not exported by {path}"
    assert built.query("hyb_abi_version") == 9 and built.x3.query("hyb_abi_version") == 9
    assert not set(NEW) & _lib.DTYPE_FIRST


@pytest.mark.parametrize("which", ["main", "x3"])
def test_null_pointers_and_channel_counts_are_refused_without_a_device(built, which):
    lib = built if which == "main" else built.x3
    for name in NEW:
        args = [None if a == "ptr" else 0 for a in lib.protos[name][1]]
        assert lib.raw(name)(*args) == HYB_E_ARG, name
    buf = (ctypes.c_longlong * 64)()                                # never read: the argument checks come before any HIP call
    p = ctypes.addressof(buf)
    photo, luma = lib.raw("hyb_clips_u8_transform_photo"), lib.raw("hyb_clips_u8_luma_sums")
    for C in (2, 4, 0, 5):
        assert photo(p, p, None, p, None, None, p, 1, 1, 4, 4, C, 1, 4, 4, None) == HYB_E_ARG, C
        assert luma(p, p, p, 1, 1, 4, 4, C, 1, None) == HYB_E_ARG, C
    # each required pointer alone (mix, luma_sums and mean_invstd may be NULL)
    for missing in (0, 1, 3, 6):
        a = [p, p, None, p, None, None, p]
        a[missing] = None
        assert photo(*a, 1, 1, 4, 4, 3, 1, 4, 4, None) == HYB_E_ARG, missing
    for missing in range(3):
        a = [p, p, p]
        a[missing] = None
        assert luma(*a, 1, 1, 4, 4, 3, 1, None) == HYB_E_ARG, missing
    assert photo(p, p, None, p, None, None, p, 1, 1, 4, 16385, 3, 1, 4, 4, None) == HYB_E_ARG
    assert luma(p, p, p, 1, 1, 16385, 4, 3, 1, None) == HYB_E_ARG


SRC = np.random.default_rng(43).integers(0, 256, (3, 5, 37, 53, 3), dtype=np.uint8)
ROWS = [(0, 0, 37, 53, 0, 0, 2, 0), (30, 44, 7, 9, 1, 2, 1, 0), (3, 11, 20, 33, 1, 0, 1, 0)]


@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("norm", [False, True])
def test_identity_photo_rows_give_the_plain_reference_exactly(C, norm):
    src = np.ascontiguousarray(SRC[..., :C])
    mi = P.ClipTransform(8, **IMAGENET).mean_invstd(3)[:, :C] if norm else None
    # seed, order, mode and a box of zero area that would matter if they were used
    ident = [photo_row(order=3, seed=(7 << 32) | 5, box=(3, 5, 0, 7), mode=2)] * 3
    for size in ((24, 24), (9, 13)):
        assert np.array_equal(clip_photo_ref(src, ROWS, None, ident, mi, 3, *size), clip_transform_ref(src, ROWS, mi, 3, *size))


def test_clamp_photo_rows_follows_the_header():
    nan = 0x7fc00000
    rows = [[f32_bits(-0.5), nan, f32_bits(1e9), 9, 7, f32_bits(5.0), 1, 2, 30, -4, 5, 100, 7, 11, 12, 13],
            [f32_bits(0.0), f32_bits(16.0), f32_bits(0.25), -1, 0, nan, 3, 4, 3, 3, -2, 6, -1, 0, 0, 0],
            [f32_bits(2.0), f32_bits(1.0), f32_bits(1.0), 5, 0, f32_bits(-1.0), 0, 0, 2, 3, 40, 50, 2, 0, 0, 0]]
    got = clamp_photo_rows(rows, 24, 16).tolist()
    assert got[0] == [ONE_BITS, ONE_BITS, f32_bits(16.0), 0, 1, ONE_BITS, 1, 2, 24, 0, 0, 16, 0, 11, 12, 13]
    assert got[1] == [0, f32_bits(16.0), f32_bits(0.25), 0, 0, 0, 3, 4, 3, 3, 0, 6, 0, 0, 0, 0]
    assert got[2] == [f32_bits(2.0), ONE_BITS, ONE_BITS, 5, 0, 0, 0, 0, 2, 3, 22, 13, 2, 0, 0, 0]


@pytest.mark.parametrize("C", [3, 1])
def test_luma_sums_are_the_weighted_mean_of_the_crop(C):
    src = np.ascontiguousarray(SRC[..., :C])
    rows = ROWS + []
    sums = luma_sums_ref(src, rows, 3)
    cl = clamp_rows(rows, 37, 53)
    for b in range(3):
        y0, x0, ch, cw = (int(v) for v in cl[b, :4])
        for t in range(3):
            ts = min(max(rows[b][5] + t * rows[b][6], 0), 4)
            crop = src[b, ts, y0:y0 + ch, x0:x0 + cw].astype(np.float64) / 255.0
            want = float(crop.mean()) if C == 1 else float((crop * np.asarray(LUMA_W)).sum(-1).mean())
            assert isinstance(sums[b][t], int)
            assert abs(sums[b][t] / (10000 * 255 * ch * cw) - want) <= 1e-12


@pytest.mark.parametrize("seed", [0, 1, 0x0123456789abcdef, (7 << 32) | 5, 2 ** 64 - 1], ids=hex)
def test_noise_z_is_standard_normal_by_its_moments(seed):
    N = 36864
    z = noise_z(seed, np.arange(N))
    mean, var, top = abs(z.mean()) * np.sqrt(N), abs(z.var() - 1.0) / np.sqrt(2.0 / N), np.abs(z).max()
    print(f"noise_z seed {seed:#x}: |mean| sqrt(N) {mean:.2f}, |var - 1| / sqrt(2/N) {var:.2f}, max |z| {top:.2f}")
    assert mean < 4 and var < 4 and top < 5.8


def test_sample_photo_is_reproducible_and_well_formed():
    Ho, Wo, B = 24, 40, 5
    kw = dict(seed=11, **ALL_ON)
    a, b = P.ClipTransform((Ho, Wo), **kw), P.ClipTransform((Ho, Wo), **kw)
    orders, boxes, noisy, gray, plain = set(), 0, 0, 0, 0
    for _ in range(40):                                             # 200 clips
        rows = a.sample_photo(B, 3, Ho, Wo)
        assert np.array_equal(rows, b.sample_photo(B, 3, Ho, Wo))
        assert rows.dtype == np.int32 and rows.shape == (B, 16) and not rows[:, 13:].any()
        assert np.array_equal(clamp_photo_rows(rows, Ho, Wo), rows)          # nothing for the kernel to clamp
        f = rows[:, :3].view(np.float32)
        assert ((f >= np.float32(0.6)) & (f <= np.float32(1.4))).all()
        sig = rows[:, 5].view(np.float32)
        assert (((sig >= np.float32(0.05)) & (sig <= np.float32(0.2))) | (rows[:, 5] == 0)).all()
        assert (rows[:, 12] == 2).all() and set(rows[:, 4].tolist()) <= {0, 1}
        for r, fr in zip(rows.tolist(), f):
            if (fr != 1).any():
                orders.add(r[3])
            else:
                plain += 1
                assert r[3] == 0
            noisy += r[5] != 0
            gray += r[4]
            ey0, ex0, eh, ew = r[8:12]
            if eh * ew:
                boxes += 1
                assert 0 < eh < Ho and 0 < ew < Wo and 0 <= ey0 <= Ho - eh and 0 <= ex0 <= Wo - ew
                # the sides are rounded to integers: each moves by at most 1/2, so the area by at most (eh + ew) / 2 + 1/4
                slack = (eh + ew) / 2 + 0.25
                assert 0.02 * Ho * Wo - slack <= eh * ew <= Ho * Wo / 3 + slack
            else:
                assert not any(r[8:12])
    assert orders == set(range(6))
    assert 100 < boxes < 180 and 60 < noisy < 140 and 15 < gray < 70 and 15 < plain < 70       # probabilities 0.7, 0.5, 0.2 and 1 - 0.8 of 200
    seeds = {(r[6], r[7]) for r in rows.tolist()}
    assert len(seeds) == B


def test_strength_draws_the_factor_from_torchvisions_range():
    t = P.ClipTransform(16, seed=2, brightness=2.5, saturation=0.1)
    f = np.concatenate([t.sample_photo(8, 3, 16, 16)[:, :3].view(np.float32) for _ in range(25)])
    assert f[:, 0].min() >= 0 and f[:, 0].max() <= np.float32(3.5) and f[:, 0].min() < 0.2 and f[:, 0].max() > 3.2      # U[max(0, 1 - s), 1 + s]
    assert (f[:, 1] == 1).all() and f[:, 2].min() >= np.float32(0.9) and f[:, 2].max() <= np.float32(1.1)
    assert t.photometric() and not t.needs_luma()
    fixed = P.ClipTransform(16, noise_std=0.1).sample_photo(4, 3, 16, 16)
    assert (fixed[:, 5] == f32_bits(0.1)).all() and (fixed[:, :3] == ONE_BITS).all()


def test_crop_and_mix_rows_do_not_move_when_the_photometric_options_are_switched_on():
    for seed in (0, 7):
        kw = dict(frames=3, frame_stride=(1, 2), seed=seed, mixup_alpha=0.8, cutmix_alpha=1.0, mix_mode="clip")
        a, b = P.ClipTransform(24, **kw), P.ClipTransform(24, **kw, **ALL_ON)
        for _ in range(4):
            assert np.array_equal(a.sample(5, 6, 37, 53), b.sample(5, 6, 37, 53))
            b.sample_photo(5, 3, 24, 24)                            # the photo draws come from their own Generator
            for x, y in zip(a.sample_mix(5, 24, 24), b.sample_mix(5, 24, 24)):
                assert np.array_equal(x, y)
        assert not a.photometric() and b.photometric() and b.needs_luma()


def test_defaults_and_eval_transforms_are_not_photometric():
    ident = np.zeros((3, 16), dtype=np.int32)
    ident[:, :3] = ONE_BITS
    for t in (P.ClipTransform(16), P.ClipTransform(16, train=False, **ALL_ON), P.ClipTransform(16, mixup_alpha=0.8)):
        assert not t.photometric() and not t.needs_luma()
        r = t.sample_photo(3, 2, 16, 16)
        assert np.array_equal(r[:, :12], ident[:, :12]) and not r[:, 13:].any()
    for name in ("brightness", "contrast", "saturation", "grayscale", "noise_std", "erase_prob"):
        t = P.ClipTransform(16, **{name: 0.3})
        assert t.photometric() and t.needs_luma() == (name == "contrast"), name


@pytest.mark.parametrize("kw,match", [(dict(brightness=-0.1), "strengths"), (dict(contrast=float("nan")), "strengths"), (dict(saturation=20), "<= 15"),
                                      (dict(jitter_prob=1.5), "probabilities"), (dict(erase_prob=-0.1), "probabilities"),
                                      (dict(noise_std=(0.3, 0.1)), "noise_std"), (dict(noise_std=1.5), "noise_std"),
                                      (dict(erase_scale=(0.5, 0.2)), "erase_scale"), (dict(erase_ratio=(0.0, 1.0)), "erase_scale"),
                                      (dict(erase_mode="random"), "erase_mode")])
def test_invalid_arguments_raise_in_the_constructor(kw, match):
    with pytest.raises(ValueError, match=match):
        P.ClipTransform(16, **kw)
