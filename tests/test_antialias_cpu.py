"""CPU: the antialiased resize (ClipTransform(antialias=True), hyb_clips_u8_transform_aa, hybrid::clip_transform_aa) as far as it goes without a
device: the entry point's declaration, export and argument checks in both builds; the integer rule of include/hybrid_hip.h (tests/antialias_ref.py)
IS F.interpolate(bilinear, align_corners=False, antialias=True), to fp64 rounding; the two weight patterns the kernel's exact cases rest on; and the
new keyword leaves every draw alone."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import transformer_cnn_hybrid_network_for_video_processing_amd as P
from transformer_cnn_hybrid_network_for_video_processing_amd import _lib

from antialias_ref import aa_weights, clip_transform_aa_ref, taps

NAME = "hyb_clips_u8_transform_aa"
HYB_E_ARG = -1


@pytest.fixture(scope="module")
def built():
    from transformer_cnn_hybrid_network_for_video_processing_amd import build
    build.build()
    return _lib.lib


# ---- the entry point --------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_point():
    protos = _lib.parse_header()
    # src, params, mean_invstd, dst | B, V, Tin, Hin, Win, C, Tout, Ho, Wo | stream
    assert protos[NAME] == ("int", ["ptr"] * 4 + ["int"] * 9 + ["ptr"])
    assert protos[NAME] == protos["hyb_clips_u8_transform_views"]
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
    # with a null pointer among them the call is refused whatever the other checks do; V = 0, C = 5 and a zero extent beside it
    for b in (dict(V=0), dict(C=5), dict(Ho=0)):
        assert fn(None, None, None, None, *{**ok, **b}.values(), None) == HYB_E_ARG, b
    with pytest.raises(RuntimeError, match="argument check"):
        lib.call(NAME, None, None, None, None, *ok.values(), None)
    if torch.cuda.is_available():
        # the extent checks need non-null pointers to be reached; on a machine with a device a check that failed to refuse would launch on this
        # host buffer, so those cases run on device-less machines only (as in tests/test_views_cpu.py)
        return
    bad = [dict(V=0), dict(V=-1), dict(B=65536, V=65536), dict(B=2 ** 31 - 1, V=2), dict(B=0), dict(Tin=0), dict(Hin=0), dict(Win=0), dict(C=0),
           dict(Tout=0), dict(Ho=0), dict(Wo=0), dict(C=5), dict(Hin=16385), dict(Win=16385), dict(Ho=16385), dict(Wo=16385)]
    for b in bad:
        assert fn(p, p, None, p, *{**ok, **b}.values(), None) == HYB_E_ARG, b


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------
PAIRS = [(5, 4), (7, 3), (23, 4), (17, 16), (16, 16), (33, 8), (3, 1), (2, 1), (7, 12), (300, 224), (1, 5), (12, 6), (9, 40)]
SECOND = [(7, 12), (40, 9), (11, 11)]                               # the other axis: up-scaled, down-scaled, untouched


def _interp(a, m_y, m_x):
    """torch's operator in fp64, one axis per call and always the LAST axis (the filter is separable: the columns, then -- transposed -- the rows).
    torch 2.10 goes wrong when it resamples the rows of a tensor that is one column wide, as its own intermediate is in a single call with a
    one-column output: (3,5) -> (6,1) gives six times the first row's value, while (3,5) -> (6,5) -> (6,1) gives the six different ones.  So pairs
    like (7,12) x (3,1) cannot be checked in one call.  Where no extent is 1 the single call is checked too."""
    def f(t, size):
        return F.interpolate(t, size, mode="bilinear", align_corners=False, antialias=True)
    t = torch.from_numpy(a)[None, None]
    cols = f(t, (a.shape[0], m_x))
    both = f(cols.transpose(-1, -2).contiguous(), (m_x, m_y)).transpose(-1, -2)[0, 0].numpy()
    if min(a.shape[0], a.shape[1], m_y, m_x) > 1:
        assert np.abs(f(t, (m_y, m_x))[0, 0].numpy() - both).max() <= 1e-11
    return both


@pytest.mark.parametrize("n,m", PAIRS, ids=lambda v: str(v))
def test_weights_are_torch_antialias_interpolate(n, m):
    rng = np.random.default_rng(1000 * n + m)
    worst = 0.0
    for n2, m2 in SECOND:                                           # (n, m) on the rows with (n2, m2) on the columns, and the other way round
        for (ny, my), (nx, mx) in (((n, m), (n2, m2)), ((n2, m2), (n, m))):
            a = rng.integers(0, 256, (ny, nx)).astype(np.float64)
            wy, wx = aa_weights(ny, my).astype(np.float64), aa_weights(nx, mx).astype(np.float64)
            got = (wy / wy.sum(1, keepdims=True)) @ a @ (wx / wx.sum(1, keepdims=True)).T
            worst = max(worst, float(np.abs(got - _interp(a, my, mx)).max()))
    print(f"aa_weights ({n},{m}): max abs difference to F.interpolate(antialias=True) {worst:.3e} on the 0..255 scale")
    assert worst <= 1e-9


def test_reference_is_torch_on_a_cropped_flipped_clip():
    rng = np.random.default_rng(5)
    src = rng.integers(0, 256, (2, 4, 23, 40, 3), dtype=np.uint8)
    rows = [(2, 3, 20, 33, 1, 1, 2, 0), (0, 0, 23, 40, 0, 0, 1, 0), (5, 9, 3, 30, 0, 3, -1, 0), (22, 39, 9, 9, 1, 0, 0, 0)]      # the last one is clamped to 1 x 1
    mi = P.ClipTransform(8, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)).mean_invstd(3)
    got = clip_transform_aa_ref(src, rows, mi, 2, 2, 5, 7)
    assert got.shape == (4, 2, 3, 5, 7)
    for r, (y0, x0, ch, cw, flip, t0, ts, _) in enumerate(rows):
        ch, cw = min(ch, 23 - y0), min(cw, 40 - x0)
        for t in range(2):
            fr = src[r // 2, min(max(t0 + t * ts, 0), 3), y0:y0 + ch, x0:x0 + cw].astype(np.float64)
            for c in range(3):
                want = _interp(np.ascontiguousarray(fr[:, :, c]), 5, 7) / 255.0
                want = (want[:, ::-1] if flip else want)
                want = (want - np.float64(mi[0, c])) * np.float64(mi[1, c])
                assert np.abs(got[r, t, c] - want).max() <= 1e-11


@pytest.mark.parametrize("n", [1, 2, 16, 37])
def test_an_identity_axis_has_one_tap_per_row(n):
    for flip in (False, True):
        w = aa_weights(n, n, flip)
        assert ((w > 0).sum(axis=1) == 1).all() and taps(n, n) == 1
        want = np.eye(n, dtype=np.int64)[::-1] if flip else np.eye(n, dtype=np.int64)
        assert np.array_equal(w, 2 * n * want)                      # W == S == 2n: the normalised weight is exactly 1


@pytest.mark.parametrize("m", [2, 8, 12, 100])
def test_a_2x_downscale_has_interior_rows_1_3_3_1(m):
    w = aa_weights(2 * m, m)
    for i in range(1, m - 1):
        row = np.zeros(2 * m, dtype=np.int64)
        row[2 * i - 1:2 * i + 3] = np.array([1, 3, 3, 1]) * m
        assert np.array_equal(w[i], row)
    assert np.array_equal(w[0, :3], np.array([3, 3, 1]) * m) and not w[0, 3:].any()          # the border rows lose the clipped tap and are renormalised
    assert taps(2 * m, m) == (4 if m > 2 else 3)


def test_tap_counts():
    assert taps(23, 4) == 11 and taps(40, 12) == 7 and taps(3, 12) == 2 and taps(1, 5) == 1
    for n, m in PAIRS:
        assert taps(n, m) <= (2 * -(-n // m) + 1 if n > m else 2)


# ---- the transform ----------------------------------------------------------------------------------------------------------------------
def test_antialias_is_off_by_default():
    assert P.ClipTransform(16).antialias is False
    assert P.ClipTransform(16, antialias=True).antialias is True
    assert P.ClipTransform(16, train=False, antialias=1).antialias is True


def test_the_rows_do_not_depend_on_antialias():
    kw = dict(frames=3, frame_stride=(1, 2), seed=5)
    off, on = P.ClipTransform(16, **kw), P.ClipTransform(16, antialias=True, **kw)
    for _ in range(3):
        assert np.array_equal(off.sample(4, 7, 24, 40), on.sample(4, 7, 24, 40))
    kw = dict(train=False, frames=2, eval_views=(2, 3), eval_crop=0.75, eval_flip=True)
    off, on = P.ClipTransform((16, 12), **kw), P.ClipTransform((16, 12), antialias=True, **kw)
    assert on.views == off.views == 12
    assert np.array_equal(off.sample_views(3, 6, 24, 40), on.sample_views(3, 6, 24, 40))
    assert np.array_equal(off.sample(3, 6, 24, 40), on.sample(3, 6, 24, 40))


def test_antialias_with_mixing_or_photometrics_is_refused():
    for kw in (dict(mixup_alpha=0.8), dict(cutmix_alpha=1.0), dict(brightness=0.4), dict(noise_std=0.1), dict(erase_prob=0.5), dict(grayscale=0.2)):
        with pytest.raises(ValueError, match="not provided"):
            P.ClipTransform(16, antialias=True, **kw)
        assert P.ClipTransform(16, antialias=False, **kw).antialias is False
    # the evaluation transform never mixes or jitters, whatever the training options say
    assert P.ClipTransform(16, train=False, antialias=True, mixup_alpha=0.8, brightness=0.4).antialias is True


# ---- the operator -----------------------------------------------------------------------------------------------------------------------
def test_it_is_exported():
    assert "clip_transform_aa" in P.__all__ and callable(P.clip_transform_aa)


def test_cpu_tensors_are_refused():
    src = torch.zeros(1, 2, 8, 8, 3, dtype=torch.uint8)
    rows = torch.from_numpy(P.ClipTransform(4, antialias=True).sample(1, 2, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.clip_transform_aa(src, rows, None, 1, 2, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        torch.ops.hybrid.clip_transform_aa(src, rows, None, 1, 2, 4, 4)


def test_operator_has_a_fake_kernel_and_checks_its_arguments():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        src = torch.empty(2, 5, 20, 24, 3, dtype=torch.uint8)
        rows = torch.empty(6, 8, dtype=torch.int32)
        mi = torch.empty(2, 3)
        out = torch.ops.hybrid.clip_transform_aa(src, rows, mi, 3, 3, 12, 16)
        assert out.shape == (6, 3, 3, 12, 16) and out.dtype == torch.float32
        with pytest.raises(TypeError, match="params"):
            torch.ops.hybrid.clip_transform_aa(src, rows, mi, 2, 3, 12, 16)
        with pytest.raises(TypeError, match="int32"):
            torch.ops.hybrid.clip_transform_aa(src, rows.long(), mi, 3, 3, 12, 16)
        with pytest.raises(TypeError, match="uint8"):
            torch.ops.hybrid.clip_transform_aa(src.float(), rows, mi, 3, 3, 12, 16)
        with pytest.raises(ValueError, match="V >= 1"):
            torch.ops.hybrid.clip_transform_aa(src, rows, mi, 0, 3, 12, 16)
        with pytest.raises(ValueError, match="C <= 4"):
            torch.ops.hybrid.clip_transform_aa(torch.empty(2, 5, 20, 24, 5, dtype=torch.uint8), rows, None, 3, 3, 12, 16)
