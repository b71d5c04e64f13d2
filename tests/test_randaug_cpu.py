"""CPU: RandAugment and hue jitter in the device clip transform (ClipTransform(randaugment=..., hue=...), hyb_clip_aug_u8_transform,
hybrid::clip_transform_aug) as far as they go without a device.

  - the reference (tests/randaug_ref.py) is PIL's: on byte-exact rows Posterize, Solarize, SolarizeAdd and Invert give the bytes of ImageOps.posterize /
    solarize / invert and of timm's solarize_add (a point table); its geometry is Image.transform(AFFINE, BILINEAR, fillcolor) in mode "F"
  - the hue shift: h then -h is the input, h = +-1/2 coincide
  - ClipTransform.sample_aug: the levels at m = 0, 5 and 10, rows that repeat, the other rows of a seed unmoved, kernel() and the refusals
  - the entry point's argument check in both libraries, the operator's fake kernel and its refusals on meta tensors"""
import ctypes
import math

import numpy as np
import pytest
import torch

import transformer_cnn_hybrid_network_for_video_processing_amd as P
from transformer_cnn_hybrid_network_for_video_processing_amd import _lib, ops

from photo_ref import _f32, f32_bits, photo_row
from randaug_ref import BAND, IDENTITY_M, aug_row, byte_of, clamp_aug_rows, clip_aug_ref, geometry_unit, hue_shift

NAME = "hyb_clip_aug_u8_transform"
HYB_E_ARG = -1
IMAGENET = dict(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
SRC = np.random.default_rng(43).integers(0, 256, (3, 5, 37, 53, 3), dtype=np.uint8)
# byte-exact rows: ch == Ho, cw == Wo, no flip -- every fraction is 0 and a value is its byte / 255
EXACT = [(0, 0, 24, 24, 0, 0, 1, 0), (13, 29, 24, 24, 0, 2, 1, 0), (5, 7, 24, 24, 0, 0, 2, 0)]


@pytest.fixture(scope="module")
def built():
    from transformer_cnn_hybrid_network_for_video_processing_amd import build
    build.build()
    return _lib.lib


# ---- the entry point ---------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_point_outside_the_closed_family():
    protos = _lib.parse_header()
    # src, params, mix, photo, aug, luma_sums, mean_invstd, dst | B, Tin, Hin, Win, C, Tout, Ho, Wo | stream
    assert protos[NAME] == ("int", ["ptr"] * 8 + ["int"] * 8 + ["ptr"])
    assert len(protos[NAME][1]) == len(protos["hyb_clips_u8_transform_photo"][1]) + 1
    assert NAME not in _lib.DTYPE_FIRST


@pytest.mark.parametrize("which", ["main", "x3"])
def test_the_argument_check_comes_before_any_device_call(built, which):
    lib = built if which == "main" else built.x3
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH if which == "main" else _lib.LIB_X3_PATH), NAME)
    assert lib.query("hyb_abi_version") == 9
    fn = lib.raw(NAME)
    if torch.cuda.is_available():
        return              # (the pointers below are a host buffer: on a machine with a device an accepted call would launch on it)
    buf = (ctypes.c_longlong * 64)()
    p = ctypes.addressof(buf)
    ok = dict(B=2, Tin=4, Hin=32, Win=32, C=3, Tout=4, Ho=16, Wo=16)

    def call(ptrs, **change):
        return fn(*ptrs, *{**ok, **change}.values(), None)
    full = [p] * 8
    for required in (0, 1, 4, 7):                                    # src, params, aug, dst
        a = list(full)
        a[required] = None
        assert call(a) == HYB_E_ARG, required
    for k in ok:
        for v in ((0, -1) if k != "C" else (0, 2, 4, 5, -1)):
            assert call(full, **{k: v}) == HYB_E_ARG, (k, v)
    for k in ("Hin", "Win", "Ho", "Wo"):
        assert call(full, **{k: 16385}) == HYB_E_ARG, k
    # what the check lets through reaches the first HIP call, which fails for want of a device: mix, photo, luma_sums, mean_invstd NULL; C = 1
    assert call([p, p, None, None, p, None, None, p]) not in (0, HYB_E_ARG)
    assert call(full, C=1) not in (0, HYB_E_ARG) and call(full, Ho=16384) not in (0, HYB_E_ARG)


# ---- the reference is PIL's --------------------------------------------------------------------------------------------------------------------
def _exact_bytes(prog, C=3):
    """The reference on the byte-exact rows under one program -> (bytes uint8 [B,Tout,C,24,24], the crops' bytes alike)."""
    src = np.ascontiguousarray(SRC[..., :C])
    out, near = clip_aug_ref(src, EXACT, None, None, [aug_row(prog)] * 3, None, 3, 24, 24)
    crops = np.stack([np.stack([src[b, t0 + t * ts, y0:y0 + 24, x0:x0 + 24] for t in range(3)]) for b, (y0, x0, _, _, _, t0, ts, _) in enumerate(EXACT)])
    scaled = 255.0 * out
    assert np.abs(scaled - np.round(scaled)).max() < 1e-9            # byte-exact rows stay byte-exact under these ops
    assert not near.any()                                            # a byte is half a unit away from every boundary
    return np.round(scaled).astype(np.uint8), crops.transpose(0, 1, 4, 2, 3)


def _pil(op, crops):
    from PIL import Image
    out = np.empty_like(crops)
    for idx in np.ndindex(crops.shape[:2]):
        im = Image.fromarray(np.ascontiguousarray(crops[idx].transpose(1, 2, 0)))
        out[idx] = np.asarray(op(im)).transpose(2, 0, 1)
    return out


@pytest.mark.parametrize("bits", range(9))
def test_posterize_is_pils(bits):
    from PIL import ImageOps
    got, crops = _exact_bytes([("Posterize", bits)])
    # ImageOps.posterize's table, i & ~(2 ** (8 - bits) - 1), written out for bits = 0, which the function itself does not take everywhere
    want = _pil(lambda im: ImageOps.posterize(im, bits), crops) if bits >= 1 else crops & np.uint8(0)
    assert np.array_equal(got, want)
    assert np.array_equal(got, crops & np.uint8(~((1 << (8 - bits)) - 1) & 0xff))


@pytest.mark.parametrize("thr", [0, 1, 128, 255, 256])
def test_solarize_is_pils(thr):
    from PIL import ImageOps
    got, crops = _exact_bytes([("Solarize", thr)])
    assert np.array_equal(got, _pil(lambda im: ImageOps.solarize(im, thr), crops))


@pytest.mark.parametrize("add", [0, 1, 55, 110, 255])
def test_solarize_add_is_timms_point_table(add):
    got, crops = _exact_bytes([("SolarizeAdd", add)])
    lut = [min(255, i + add) if i < 128 else i for i in range(256)]      # timm's solarize_add(img, add, thresh=128)
    want = _pil(lambda im: im.point(lut * 3), crops)
    assert np.array_equal(got, want)


def test_invert_is_pils_and_an_involution():
    from PIL import ImageOps
    got, crops = _exact_bytes([("Invert", 0)])
    assert np.array_equal(got, _pil(ImageOps.invert, crops))
    twice, _ = _exact_bytes([("Invert", 0), ("Invert", 0)])
    assert np.array_equal(twice, crops)


def test_nothing_happens_to_a_grey_clip_under_color_and_hue():
    got, crops = _exact_bytes([("Color", 1.7), ("Hue", 0.3)], C=1)
    assert np.array_equal(got, crops)


def _matrices(W, H):
    t = P.ClipTransform
    return {"rotate17": t._affine("Rotate", 17.0, H, W), "shearx": t._affine("ShearX", 0.3, H, W), "sheary": t._affine("ShearY", -0.21, H, W),
            "translate-fractional": t._affine("TranslateX", 0.2, H, W) @ t._affine("TranslateY", -0.13, H, W),
            "translate-integer": t._affine("TranslateX", 3 / W, H, W) @ t._affine("TranslateY", -2 / H, H, W)}


@pytest.mark.parametrize("which", ["rotate17", "shearx", "sheary", "translate-fractional", "translate-integer"])
def test_the_geometry_is_pils_affine_bilinear_in_float_mode(which):
    from PIL import Image
    H, W = 11, 17
    img = np.random.default_rng(3).integers(0, 256, (H, W, 1), dtype=np.uint8)
    M = _matrices(W, H)[which][:2].reshape(6).astype(np.float32)
    fill = np.float32(0.25)
    got, _ = geometry_unit(img, (0, 0, H, W, 0), M, [fill] * 3, H, W)
    pil = Image.fromarray(img[..., 0].astype(np.float32), mode="F").transform((W, H), Image.AFFINE, tuple(float(v) for v in M), resample=Image.BILINEAR,
                                                                              fillcolor=float(fill) * 255.0)
    want = np.asarray(pil, dtype=np.float64) / 255.0
    err = np.abs(got[0] - want).max()
    print(f"geometry vs PIL mode F, {which}: max abs err {err:.3e}")
    assert err <= 2.0 ** -20
    if which == "translate-integer":                                 # the shifted image, fill elsewhere
        shifted = np.full((H, W), float(fill))
        shifted[2:, :W - 3] = img[:H - 2, 3:, 0] / 255.0
        assert np.array_equal(got[0], shifted)
    # rotation by PIL's own Image.rotate: the same matrix
    if which == "rotate17":
        rot = Image.fromarray(img[..., 0].astype(np.float32), mode="F").rotate(17.0, resample=Image.BILINEAR, fillcolor=float(fill) * 255.0)
        assert np.abs(got[0] - np.asarray(rot, dtype=np.float64) / 255.0).max() <= 2.0 ** -20


def test_the_fp32_restatement_of_the_geometry_is_close_and_flips():
    src = SRC[0, 0]
    M = _matrices(24, 24)["rotate17"][:2].reshape(6).astype(np.float32)
    for flip in (0, 1):
        crop = (3, 11, 20, 33, flip)
        a, edge = geometry_unit(src, crop, M, [0.5] * 3, 24, 24)
        b, _ = geometry_unit(src, crop, M, [0.5] * 3, 24, 24, np.float32)
        keep = edge >= BAND
        assert keep.mean() > 0.98 and np.abs(a - b)[:, keep].max() < 2.0 ** -14
    # the flip mirrors the un-augmented frame: with the identity map it is the integer rule's flip, up to the rounding of the coordinates
    ident = np.asarray(IDENTITY_M, dtype=np.float32)
    from clip_transform_ref import clip_transform_ref
    plain = clip_transform_ref(SRC[:1], [(3, 11, 20, 33, 1, 0, 1, 0)], None, 1, 24, 24)[0, 0]
    got, _ = geometry_unit(src, (3, 11, 20, 33, 1), ident, [0.5] * 3, 24, 24)
    assert np.abs(got - plain).max() < 1e-12


# ---- hue -------------------------------------------------------------------------------------------------------------------------------------
def test_hue_there_and_back_and_the_half_turns():
    v = np.random.default_rng(5).random((3, 4000))
    v[:, :10] = v[0, :10]                                            # greys
    v[:, 10:20] = np.round(v[:, 10:20])                              # corners of the cube
    for h in (0.07, 0.25, 0.5):
        there = hue_shift(v, h)
        back = np.stack(hue_shift(there, -h))
        assert np.abs(back - v).max() < 1e-12, h
        assert np.abs(np.stack(there) - v).max() > 0.1
        # the fp32 restatement: within 4 x its own distance from fp64 of one shift, plus the resample gate
        t32 = np.stack(hue_shift(v.astype(np.float32), h, np.float32)).astype(np.float64)
        one = np.abs(t32 - np.stack(hue_shift(v.astype(np.float32).astype(np.float64), h))).max()
        b32 = np.stack(hue_shift(hue_shift(v.astype(np.float32), h, np.float32), -h, np.float32)).astype(np.float64)
        print(f"hue {h}: fp32 restatement {one:.3e} from fp64, there and back {np.abs(b32 - v.astype(np.float32)).max():.3e}")
        assert np.abs(b32 - v.astype(np.float32)).max() <= 4 * 2 * one + 2.0 ** -20
    plus, minus = np.stack(hue_shift(v, 0.5)), np.stack(hue_shift(v, -0.5))
    assert np.abs(plus - minus).max() < 1e-12
    assert np.abs(np.stack(hue_shift(v, 0.0)) - v).max() < 1e-12
    # a grey pixel has no hue: it stays
    assert np.abs(np.stack(hue_shift(v[:, :10], 0.3)) - v[:, :10]).max() < 1e-15


# ---- ClipTransform ---------------------------------------------------------------------------------------------------------------------------
def _one_op(name, m, seed=0, size=(16, 24)):
    """The rows of ClipTransform drawing exactly `name` at magnitude m, always applied."""
    t = P.ClipTransform(size, randaugment=(1, m), ra_ops=(name,), ra_prob=1.0, seed=seed)
    return t.sample_aug(64, *size)


@pytest.mark.parametrize("m", [0, 5, 10])
def test_levels_are_the_tables(m):
    L = m / 10.0
    Ho, Wo = 16, 24
    for name, code in (("Brightness", 2), ("Contrast", 3), ("Color", 4)):
        rows = _one_op(name, m)
        assert (rows[:, 0] == 0).all() and (rows[:, 1] == 1).all() and (rows[:, 2] == code).all()
        want = {f32_bits(max(0.1, 1.0 + 0.9 * L)), f32_bits(max(0.1, 1.0 - 0.9 * L))}
        assert set(rows[:, 3].tolist()) == want
    for name, code, arg in (("Posterize", 5, 4 - int(4 * L)), ("Solarize", 6, 256 - int(256 * L)), ("SolarizeAdd", 7, int(110 * L)), ("Invert", 1, 0)):
        rows = _one_op(name, m)
        assert (rows[:, 1] == 1).all() and (rows[:, 2] == code).all() and (rows[:, 3] == arg).all(), name
        assert (rows[:, 18:24] == np.asarray(IDENTITY_M, dtype=np.float32).view(np.int32)).all()
    ident = np.asarray(IDENTITY_M)
    for name, index, level in (("ShearX", 1, 0.3 * L), ("ShearY", 3, 0.3 * L), ("TranslateX", 2, 0.45 * L * Wo), ("TranslateY", 5, 0.45 * L * Ho)):
        rows = _one_op(name, m)
        M = rows[:, 18:24].copy().view(np.float32)
        assert (rows[:, 0] == 1).all() and (rows[:, 1] == 0).all()
        assert set(M[:, index].tolist()) == {np.float32(level), np.float32(-level)}, name
        rest = [i for i in range(6) if i != index]
        assert (M[:, rest] == ident[rest].astype(np.float32)).all(), name
    rows = _one_op("Rotate", m)
    M = rows[:, 18:24].copy().view(np.float32).astype(np.float64)
    assert np.allclose(np.abs(np.degrees(np.arctan2(M[:, 1], M[:, 0]))), 30.0 * L, atol=1e-4)
    assert m == 0 or {-1.0, 1.0} == set(np.sign(M[:, 1]).tolist())
    # about the centre: the centre maps to itself
    cx, cy = Wo / 2, Ho / 2
    assert np.allclose(M[:, 0] * cx + M[:, 1] * cy + M[:, 2], cx, atol=1e-4) and np.allclose(M[:, 3] * cx + M[:, 4] * cy + M[:, 5], cy, atol=1e-4)


def test_geometric_ops_compose_as_m1_after_m2_and_fill_defaults():
    t = P.ClipTransform((16, 24), randaugment=(2, 10), ra_ops=("ShearX", "TranslateY"), ra_prob=1.0, seed=4)
    rows = t.sample_aug(200, 16, 24)
    Ms = rows[:, 18:24].copy().view(np.float32)
    # ShearX then TranslateY: (1, s, 0, 0, 1, p);  TranslateY then ShearX: (1, s, s p, 0, 1, p)
    both = [M for M in Ms if M[1] != 0 and M[5] != 0]
    assert {bool(M[2] != 0) for M in both} == {False, True}
    for M in both:
        assert M[2] == 0 or M[2] == np.float32(float(M[1]) * float(M[5])) or abs(M[2] - M[1] * M[5]) < 1e-5
    assert (rows[:, 24:27].copy().view(np.float32) == 0.5).all()
    t = P.ClipTransform(16, randaugment=(1, 5), **IMAGENET)
    assert (t.sample_aug(2, 16, 16)[:, 24:27].copy().view(np.float32) == np.asarray(IMAGENET["mean"], dtype=np.float32)).all()
    t = P.ClipTransform(16, randaugment=(1, 5), fill=(0.1, 0.2, 0.3), **IMAGENET)
    assert (t.sample_aug(2, 16, 16)[:, 24:27].copy().view(np.float32) == np.asarray((0.1, 0.2, 0.3), dtype=np.float32)).all()


def test_the_default_fill_never_refuses_a_transform_that_was_accepted():
    # four channels, one channel, statistics outside [0, 1] (clips that are not on the ToTensor scale): constructed as before the option existed
    for mean, std, want in (((0.5, 0.4, 0.3, 0.2), (1, 1, 1, 1), (0.5, 0.4, 0.3)), ((0.45,), (0.2,), (0.45, 0.45, 0.45)),
                            ((-3.0, 120.0, 0.5), (1, 1, 1), (0.0, 1.0, 0.5))):
        t = P.ClipTransform(16, mean=mean, std=std)
        assert t.kernel() == "plain" and t.fill.tolist() == [float(np.float32(v)) for v in want]
    assert P.ClipTransform(16).fill.tolist() == [0.5, 0.5, 0.5]


def test_the_string_form_is_timms():
    assert P.ClipTransform(16, randaugment="rand-m7-n4-mstd0.5").randaugment == (4, 7.0, 0.5)
    assert P.ClipTransform(16, randaugment="rand-m9-mstd0.5-inc1").randaugment == (2, 9.0, 0.5)
    assert P.ClipTransform(16, randaugment="rand").randaugment == (2, 10.0, 0.0)
    assert P.ClipTransform(16, randaugment=(3, 4)).randaugment == (3, 4.0, 0.0)
    for bad, named in (("rand-m7-w0", "'w0'"), ("rand-m7-inc0", "'inc0'"), ("rand-m7-p0.3", "'p0.3'"), ("rand-mmax20", "'mmax20'"), ("rand-n", "'n'"),
                       ("augmix-m5", "'augmix-m5'")):
        with pytest.raises(ValueError, match=named):
            P.ClipTransform(16, randaugment=bad)
    for kw in (dict(randaugment=(9, 5)), dict(randaugment=(2, 11)), dict(randaugment=(8, 5), hue=0.1), dict(hue=0.6), dict(hue=-0.1),
               dict(ra_ops=("Sharpness",)), dict(ra_ops=()), dict(ra_prob=1.5), dict(fill=1.5), dict(fill=(0.1, 0.2, 0.3, 0.4))):
        with pytest.raises(ValueError):
            P.ClipTransform(16, **kw)
    assert P.ClipTransform.RA_OPS == ("Invert", "Rotate", "Posterize", "Solarize", "SolarizeAdd", "Color", "Contrast", "Brightness", "ShearX", "ShearY",
                                      "TranslateX", "TranslateY")


def test_magnitudes_are_clipped_normals_and_ops_are_drawn_with_replacement():
    t = P.ClipTransform(16, randaugment="rand-m7-n4-mstd0.5", ra_ops=("SolarizeAdd",), ra_prob=1.0, seed=2)
    rows = t.sample_aug(500, 16, 16)
    assert (rows[:, 1] == 4).all() and (rows[:, 2:10:2] == 7).all()             # the same op four times: with replacement
    adds = rows[:, 3:11:2].ravel()
    assert adds.min() >= 0 and adds.max() <= 110 and 70 < adds.mean() < 84 and adds.std() > 3          # int(110 * N(7, 0.5) / 10)
    t = P.ClipTransform(16, randaugment="rand-m10-n1-mstd5", ra_ops=("SolarizeAdd",), ra_prob=1.0, seed=2)
    adds = t.sample_aug(500, 16, 16)[:, 3]
    assert adds.max() == 110 and (adds == 110).mean() > 0.4                       # clipped at 10
    # ra_prob: about half of the drawn ops are applied
    t = P.ClipTransform(16, randaugment=(4, 5), ra_ops=("Invert",), seed=2)
    n = t.sample_aug(500, 16, 16)[:, 1]
    assert 1.8 < n.mean() < 2.2 and set(n.tolist()) == {0, 1, 2, 3, 4}
    # every op of the default set is drawn
    t = P.ClipTransform(16, randaugment=(4, 5), ra_prob=1.0, seed=2)
    rows = t.sample_aug(300, 16, 16)
    assert set(rows[:, 2:10:2].ravel().tolist()) >= {1, 2, 3, 4, 5, 6, 7} and rows[:, 0].any()


def test_hue_is_the_last_step_and_under_jitter_prob():
    t = P.ClipTransform(16, randaugment=(2, 5), ra_ops=("Invert",), ra_prob=1.0, hue=0.2, jitter_prob=0.5, seed=6)
    rows = t.sample_aug(400, 16, 16)
    with_hue = rows[:, 1] == 3
    assert 0.4 < with_hue.mean() < 0.6 and set(rows[:, 1].tolist()) == {2, 3}
    assert (rows[with_hue, 6] == 8).all() and (rows[~with_hue, 6] == 0).all()
    h = rows[with_hue, 7].copy().view(np.float32)
    assert h.min() >= -0.2 and h.max() <= 0.2 and h.min() < -0.15 and h.max() > 0.15
    alone = P.ClipTransform(16, hue=0.5)
    assert alone.augmenting() and alone.kernel() == "aug" and not alone.needs_luma() and not alone.photometric()
    rows = alone.sample_aug(50, 16, 16)
    assert (rows[:, 0] == 0).all() and (rows[:, 1] == 1).all() and (rows[:, 2] == 8).all()


ALL_ON = dict(mixup_alpha=0.8, cutmix_alpha=1.0, mix_mode="clip", brightness=0.4, contrast=0.4, saturation=0.4, noise_std=(0.05, 0.2), erase_prob=0.7,
              frames=3, frame_stride=(1, 2), **IMAGENET)


def test_rows_of_a_seed_repeat_and_the_other_rows_do_not_move():
    new = dict(randaugment="rand-m7-n4-mstd0.5", hue=0.1)
    a, b = (P.ClipTransform(16, seed=11, **ALL_ON, **new) for _ in range(2))
    plain = P.ClipTransform(16, seed=11, **ALL_ON)
    other = P.ClipTransform(16, seed=12, **ALL_ON, **new)
    for _ in range(3):
        ra = a.sample_aug(6, 16, 16)
        assert np.array_equal(ra, b.sample_aug(6, 16, 16)) and not np.array_equal(ra, other.sample_aug(6, 16, 16))
        assert ra.shape == (6, 32) and ra.dtype == np.int32 and (ra[:, 27:] == 0).all()
        assert np.array_equal(clamp_aug_rows(ra), ra)               # no drawn row needs the kernel's clamps
        assert np.array_equal(a.sample(6, 5, 24, 24), plain.sample(6, 5, 24, 24))
        for x, y in zip(a.sample_mix(6, 16, 16), plain.sample_mix(6, 16, 16)):
            assert np.array_equal(x, y)
        assert np.array_equal(a.sample_photo(6, 3, 16, 16), plain.sample_photo(6, 3, 16, 16))
    # without the options (or with train=False) the rows are the identity and nothing is drawn
    for t in (plain, P.ClipTransform(16, train=False, **new)):
        state = t.aug_rng.bit_generator.state
        rows = t.sample_aug(4, 16, 16)
        assert (rows[:, :18] == 0).all() and t.aug_rng.bit_generator.state == state
        assert np.array_equal(clamp_aug_rows(rows), rows)


@pytest.mark.parametrize("new", [dict(randaugment=(2, 9)), dict(randaugment="rand-m7-n4-mstd0.5"), dict(hue=0.1), dict(randaugment=(0, 0), hue=0.0)])
def test_kernel_is_aug_exactly_when_a_new_option_is_on(new):
    for base, was in ((dict(), "plain"), (dict(mixup_alpha=0.8), "mix"), (dict(brightness=0.4), "photo"), (dict(mixup_alpha=0.8, erase_prob=0.5), "photo")):
        assert P.ClipTransform(16, **base).kernel() == was
        t = P.ClipTransform(16, **base, **new)
        assert t.augmenting() and t.kernel() == "aug" and "aug" in ops.CLIP_OPS_EXT and "aug" not in ops.CLIP_OPS
        assert t.mixing() == ("mixup_alpha" in base) and t.photometric() == (was == "photo")
        assert not P.ClipTransform(16, train=False, **base, **new).augmenting()
        assert P.ClipTransform(16, train=False, **base, **new).kernel() == "plain"
    assert ops.CLIP_OPS_EXT["aug"].name == "clip_transform_aug" and ops.CLIP_OPS_EXT["aug"].symbol == NAME
    assert "clip_transform_aug" in P.__all__ and callable(P.clip_transform_aug)


def test_needs_luma_when_contrast_can_be_drawn():
    assert P.ClipTransform(16, randaugment=(2, 9)).needs_luma()
    assert not P.ClipTransform(16, randaugment=(2, 9), ra_ops=("Invert", "Rotate")).needs_luma()
    assert P.ClipTransform(16, randaugment=(2, 9), ra_ops=("Invert", "Rotate"), contrast=0.3).needs_luma()
    assert not P.ClipTransform(16, randaugment=(2, 9), train=False).needs_luma() and not P.ClipTransform(16, hue=0.2).needs_luma()


def test_antialias_with_a_new_option_raises():
    for new in (dict(randaugment=(2, 9)), dict(hue=0.1)):
        with pytest.raises(ValueError, match="antialias=True together with randaugment= or hue="):
            P.ClipTransform(16, antialias=True, **new)
    assert P.ClipTransform(16, antialias=True, train=False, hue=0.1).kernel() == "aa"      # an evaluation transform ignores the new options


# ---- the operator on meta tensors -----------------------------------------------------------------------------------------------------------
B_, TIN, HIN, WIN, C_, TOUT, HO, WO = 2, 5, 20, 24, 3, 4, 12, 16


def _meta(*shape, dtype=torch.float32):
    return torch.empty(*shape, dtype=dtype, device="meta")


def _args(**change):
    a = dict(src=_meta(B_, TIN, HIN, WIN, C_, dtype=torch.uint8), params=_meta(B_, 8, dtype=torch.int32), mix=_meta(B_, 8, dtype=torch.int32),
             photo=_meta(B_, 16, dtype=torch.int32), aug=_meta(B_, 32, dtype=torch.int32), luma_sums=_meta(B_, TOUT, dtype=torch.int64),
             mean_invstd=_meta(2, C_), Tout=TOUT, Ho=HO, Wo=WO)
    a.update(change)
    return [a[k] for k in "src params mix photo aug luma_sums mean_invstd Tout Ho Wo".split()]


def test_the_schema_and_the_fake_kernel():
    op = torch.ops.hybrid.clip_transform_aug
    assert str(op.default._schema) == ("hybrid::clip_transform_aug(Tensor src, Tensor params, Tensor? mix, Tensor? photo, Tensor aug, Tensor? luma_sums, "
                                       "Tensor? mean_invstd, int Tout, int Ho, int Wo) -> Tensor")
    for change in ({}, dict(mean_invstd=None), dict(mix=None, photo=None, luma_sums=None), dict(photo=None),
                   dict(src=_meta(B_, TIN, HIN, WIN, 1, dtype=torch.uint8), mean_invstd=_meta(2, 1))):
        out = op(*_args(**change))
        C = 1 if "src" in change else C_
        assert out.shape == (B_, TOUT, C, HO, WO) and out.dtype == torch.float32 and out.device.type == "meta"
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        out = op(*[torch.empty(a.shape, dtype=a.dtype) if isinstance(a, torch.Tensor) else a for a in _args()])
        assert out.shape == (B_, TOUT, C_, HO, WO) and out.dtype == torch.float32


_AUG = f"aug must be int32 [{B_},32]: one row {{flags, n, (op, arg) x 8, M[6] bits, fill[3] bits, 0 x 5}} per clip"
REFUSALS = [
    (dict(aug=_meta(B_, 32, dtype=torch.int64)), TypeError, _AUG), (dict(aug=_meta(B_, 16, dtype=torch.int32)), TypeError, _AUG),
    (dict(aug=_meta(B_ + 1, 32, dtype=torch.int32)), TypeError, _AUG), (dict(aug=None), TypeError, _AUG),
    (dict(photo=_meta(B_, 8, dtype=torch.int32)), TypeError, "photo must be int32"), (dict(mix=_meta(B_, 8)), TypeError, "mix must be int32"),
    (dict(luma_sums=_meta(B_, TOUT + 1, dtype=torch.int64)), TypeError, "luma_sums must be int64"),
    (dict(params=_meta(B_, 8, dtype=torch.int64)), TypeError, "params must be int32"),
    (dict(src=_meta(B_, TIN, HIN, WIN, 2, dtype=torch.uint8), mean_invstd=None), ValueError, "hybrid::clip_transform_aug needs C == 1 or C == 3"),
    (dict(src=_meta(B_, TIN, HIN, WIN, 4, dtype=torch.uint8), mean_invstd=None), ValueError, "hybrid::clip_transform_aug needs C == 1 or C == 3"),
    (dict(src=_meta(B_, TIN, HIN, WIN, 5, dtype=torch.uint8), mean_invstd=None), ValueError, "needs C <= 4"),
    (dict(Wo=16385), ValueError, "Hin, Win, Ho, Wo <= 16384"), (dict(src=_meta(B_, TIN, HIN, WIN, C_)), TypeError, "reads uint8 clips"),
]


@pytest.mark.parametrize("change,exc,message", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_refusals_of_the_operator(change, exc, message):
    with pytest.raises(exc) as info:
        torch.ops.hybrid.clip_transform_aug(*_args(**change))
    assert str(info.value).startswith(message) or message in str(info.value)


def test_cpu_tensors_are_refused():
    args = [torch.zeros(a.shape, dtype=a.dtype) if isinstance(a, torch.Tensor) else a for a in _args()]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        torch.ops.hybrid.clip_transform_aug(*args)


# ---- the reference against itself ------------------------------------------------------------------------------------------------------------
def test_identity_aug_rows_give_the_photo_reference_exactly():
    from photo_ref import clip_photo_ref
    rows = [(0, 0, 37, 53, 0, 0, 2, 0), (30, 44, 7, 9, 1, 2, 1, 0), (3, 11, 20, 33, 1, 0, 1, 0)]
    photo = [photo_row(0.6, 1.4, 0.5, order=b, sigma=0.1, seed=b + 1, box=(1, 2, 3, 4), mode=b) for b in range(3)]
    mi = P.ClipTransform(8, **IMAGENET).mean_invstd(3)
    want = clip_photo_ref(SRC, rows, None, photo, mi, 3, 24, 24)
    junk = aug_row([("Hue", 0.3)] * 8, n=0, M=(float("nan"), 2.0, 3.0, 4.0, 5.0, 6.0), tail=(1, 2, 3, 4, 5))
    for aug in ([aug_row()] * 3, [junk] * 3, [aug_row([("Identity", 7), (77, 5), (-1, 0)], flags=2)] * 3):
        got, near = clip_aug_ref(SRC, rows, None, photo, aug, mi, 3, 24, 24)
        assert np.array_equal(got, want) and not near.any()


def test_contrast_pivot_moves_with_brightness_and_invert():
    from photo_ref import luma_sums_ref
    rows = [EXACT[0]]
    src = SRC[:1]
    mu0 = float(np.float32(sum(luma_sums_ref(src, rows, 3)[0]) / (10000 * 255 * 24 * 24 * 3)))
    unit, _ = clip_aug_ref(src, rows, None, None, [aug_row()], None, 3, 24, 24)
    for prog, mu, pre in (([("Contrast", 0.5)], mu0, lambda v: v), ([("Brightness", 1.5), ("Contrast", 0.5)], min(1.5 * mu0, 1.0), lambda v: np.clip(1.5 * v, 0, 1)),
                          ([("Invert", 0), ("Contrast", 0.5)], 1.0 - mu0, lambda v: 1.0 - v),
                          ([("Color", 0.5), ("Posterize", 3), ("Contrast", 0.5)], mu0, None)):
        got, _ = clip_aug_ref(src, rows, None, None, [aug_row(prog)], None, 3, 24, 24)
        if pre is not None:
            assert np.allclose(got, np.clip(0.5 * pre(unit) + 0.5 * mu, 0, 1), atol=1e-15)
        without, _ = clip_aug_ref(src, rows, None, None, [aug_row(prog)], None, 3, 24, 24, luma=False)
        head, _ = clip_aug_ref(src, rows, None, None, [aug_row(prog[:-1])], None, 3, 24, 24)
        assert np.array_equal(without, head)                        # without luma sums the factor counts as 1
        if pre is None:
            assert np.allclose(got, np.clip(0.5 * head + 0.5 * mu0, 0, 1), atol=1e-15)      # nothing else moves the pivot


def test_clamped_twins_of_the_reference():
    nan, inf = float("nan"), float("inf")
    raw = [aug_row([("Brightness", nan), ("Posterize", 12), ("Solarize", -5), ("Hue", 3.0), ("Hue", nan), (77, 9), (-1, 3), ("Color", 1e9)], n=99,
                   M=(1.0, 0.0, inf, 0.0, 1.0, 0.0), fill=(nan, 7.0, -1.0), tail=(5, 4, 3, 2, 1)),
           aug_row([("SolarizeAdd", 999), ("Contrast", -2.0)], n=-3, M=(1.0, 0.1, 0.0, 0.0, 1.0, 0.0), flags=3)]
    twin = clamp_aug_rows(raw)
    assert twin[0, 1] == 8 and twin[0, 0] == 0 and twin[1, 1] == 0 and twin[1, 0] == 1
    want = [2, f32_bits(1.0), 5, 8, 6, 0, 8, f32_bits(0.5), 8, f32_bits(0.0), 0, 0, 0, 0, 4, f32_bits(16.0)]
    assert twin[0, 2:18].tolist() == want and (twin[1, 2:18] == 0).all()
    assert [float(_f32(v)) for v in twin[0, 24:27]] == [0.0, 1.0, 0.0]
    assert [float(_f32(v)) for v in twin[0, 18:24]] == list(IDENTITY_M) and math.isclose(float(_f32(twin[1, 19])), 0.1, rel_tol=1e-6)
    assert np.array_equal(clamp_aug_rows(twin), twin)
    assert byte_of(np.float64(0.5)) == 128.0
