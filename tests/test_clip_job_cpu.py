"""CPU: the clip transforms' one job, one check and one choice rule, as far as they go without a device.

  - the six hyb_clips_u8_* entry points refuse, with HYB_E_ARG and before any HIP call, exactly what include/hybrid_hip.h says they refuse -- the
    table below is written from the header's limits, in both builds of the library -- and an optional pointer left NULL is no reason to refuse
  - ClipTransform.kernel() over the grid of options, the expected answers written out from the class docstring
  - the fake kernels of the five transform operators and of clip_luma_sums on meta tensors
  - the operators' refusals, message for message as they were before the operators were built from one table"""
import ctypes

import pytest
import torch

import transformer_cnn_hybrid_network_for_video_processing_amd as P
from transformer_cnn_hybrid_network_for_video_processing_amd import _lib

HYB_E_ARG = -1
INT_MAX = 2 ** 31 - 1

# ---- the entry points, from include/hybrid_hip.h: parameter names in order, the pointers that may be NULL, and the limits that differ -------
_EXT = ["B", "Tin", "Hin", "Win", "C", "Tout", "Ho", "Wo"]
_EXT_V = ["B", "V", "Tin", "Hin", "Win", "C", "Tout", "Ho", "Wo"]
ENTRY = {
    "hyb_clips_u8_transform": dict(ptrs=["src", "params", "mean_invstd", "dst"], optional={"mean_invstd"}, ints=_EXT),
    "hyb_clips_u8_transform_mix": dict(ptrs=["src", "params", "mix", "mean_invstd", "dst"], optional={"mean_invstd"}, ints=_EXT),
    "hyb_clips_u8_transform_views": dict(ptrs=["src", "params", "mean_invstd", "dst"], optional={"mean_invstd"}, ints=_EXT_V),
    "hyb_clips_u8_transform_aa": dict(ptrs=["src", "params", "mean_invstd", "dst"], optional={"mean_invstd"}, ints=_EXT_V),
    "hyb_clips_u8_transform_photo": dict(ptrs=["src", "params", "mix", "photo", "luma_sums", "mean_invstd", "dst"],
                                         optional={"mix", "luma_sums", "mean_invstd"}, ints=_EXT, gray_rgb=True),
    "hyb_clips_u8_luma_sums": dict(ptrs=["src", "params", "sums"], optional=set(), ints=["B", "Tin", "Hin", "Win", "C", "Tout"], gray_rgb=True),
}
OK = dict(B=2, V=3, Tin=4, Hin=32, Win=32, C=3, Tout=4, Ho=16, Wo=16)


def refused(name):
    """[(what, pointer names left NULL, extents changed)]: every call here is refused; each case departs from a valid call in ONE thing."""
    e = ENTRY[name]
    cases = [(f"{p} NULL", {p}, {}) for p in e["ptrs"] if p not in e["optional"]]
    for k in e["ints"]:
        cases += [(f"{k} = {v}", set(), {k: v}) for v in ((0, -1) if k != "C" else ())]
    cases += [(f"C = {c}", set(), dict(C=c)) for c in ((0, 2, 4, 5, -1) if e.get("gray_rgb") else (0, 5, -1))]
    cases += [(f"{k} = 16385", set(), {k: 16385}) for k in ("Hin", "Win", "Ho", "Wo") if k in e["ints"]]
    if "V" in e["ints"]:
        cases += [("B * V = 2^31", set(), dict(B=65536, V=32768))]
    return cases


def accepted(name):
    """Calls that the argument check must let through: every optional pointer NULL, and each limit itself."""
    e = ENTRY[name]
    cases = [("optional pointers NULL", set(e["optional"]), {})]
    cases += [(f"{p} alone NULL", {p}, {}) for p in sorted(e["optional"])]
    cases += [(f"{k} = 16384", set(), {k: 16384}) for k in ("Hin", "Win", "Ho", "Wo") if k in e["ints"]]
    cases += [(f"C = {c}", set(), dict(C=c)) for c in ((1, 3) if e.get("gray_rgb") else (1, 2, 3, 4))]
    if "V" in e["ints"]:
        cases += [("V = 1", set(), dict(V=1)), ("B * V = 2^31 - 1", set(), dict(B=INT_MAX, V=1))]
    return cases


@pytest.fixture(scope="module")
def built():
    from transformer_cnn_hybrid_network_for_video_processing_amd import build
    build.build()
    return _lib.lib


def test_the_table_is_the_headers():
    protos = _lib.parse_header()
    for name, e in ENTRY.items():
        assert protos[name] == ("int", ["ptr"] * len(e["ptrs"]) + ["int"] * len(e["ints"]) + ["ptr"]), name
    assert sorted(n for n in protos if n.startswith("hyb_clips_u8_")) == sorted(ENTRY)


def test_both_libraries_export_the_six_symbols_under_abi_9(built):
    for path in (_lib.LIB_PATH, _lib.LIB_X3_PATH):
        dll = ctypes.CDLL(path)
        for name in ENTRY:
            assert hasattr(dll, name), f"{name} is not exported by {path}"
    assert built.query("hyb_abi_version") == 9 and built.x3.query("hyb_abi_version") == 9


def _call(fn, name, buf, null, change):
    e = ENTRY[name]
    ints = {**OK, **change}
    return fn(*[None if p in null else buf for p in e["ptrs"]], *[ints[k] for k in e["ints"]], None)


@pytest.mark.parametrize("which", ["main", "x3"])
@pytest.mark.parametrize("name", sorted(ENTRY))
def test_refusals_are_the_headers_and_come_before_any_device_call(built, which, name):
    if torch.cuda.is_available():
        # the pointers below are a host buffer that a refused call never reads; on a machine with a device a check that failed to refuse would
        # launch on it, so the table runs on device-less machines only (as in tests/test_views_cpu.py and tests/test_antialias_cpu.py)
        return
    lib = built if which == "main" else built.x3
    fn = lib.raw(name)
    buf = ctypes.addressof((ctypes.c_longlong * 64)())
    for what, null, change in refused(name):
        assert _call(fn, name, buf, null, change) == HYB_E_ARG, (name, what)
    # a call the check lets through reaches the first HIP call, which fails for want of a device: any status but 0 and HYB_E_ARG
    for what, null, change in accepted(name):
        rc = _call(fn, name, buf, null, change)
        assert rc not in (0, HYB_E_ARG), (name, what, rc)


# ---- ClipTransform.kernel() -----------------------------------------------------------------------------------------------------------------
# (train, mixing, a photometric option, antialias, eval_views) -> kernel, from ClipTransform's docstring: the photometric options, mixing and
# eval_views do nothing outside their mode (train=True resp. train=False); photo carries the mix rows itself; antialias is for training rows and
# evaluation views alike.  Rows the constructor refuses (antialias with mixing / photo, eval_views with train=True) are in the grid too.
T, F = True, False
ONE, SIX = (1, 1), (2, 3)
CHOICE = [
    (T, F, F, F, ONE, "plain"), (T, F, F, F, SIX, "plain"), (T, F, F, T, ONE, "aa"), (T, F, F, T, SIX, "aa"),
    (T, F, T, F, ONE, "photo"), (T, F, T, F, SIX, "photo"), (T, F, T, T, ONE, "photo"), (T, F, T, T, SIX, "photo"),
    (T, T, F, F, ONE, "mix"), (T, T, F, F, SIX, "mix"), (T, T, F, T, ONE, "aa"), (T, T, F, T, SIX, "aa"),
    (T, T, T, F, ONE, "photo"), (T, T, T, F, SIX, "photo"), (T, T, T, T, ONE, "photo"), (T, T, T, T, SIX, "photo"),
    (F, F, F, F, ONE, "plain"), (F, F, F, F, SIX, "views"), (F, F, F, T, ONE, "aa"), (F, F, F, T, SIX, "aa"),
    (F, F, T, F, ONE, "plain"), (F, F, T, F, SIX, "views"), (F, F, T, T, ONE, "aa"), (F, F, T, T, SIX, "aa"),
    (F, T, F, F, ONE, "plain"), (F, T, F, F, SIX, "views"), (F, T, F, T, ONE, "aa"), (F, T, F, T, SIX, "aa"),
    (F, T, T, F, ONE, "plain"), (F, T, T, F, SIX, "views"), (F, T, T, T, ONE, "aa"), (F, T, T, T, SIX, "aa"),
]


def _transform(train, mixing, photo, antialias, eval_views):
    """The transform with these options; what the constructor would refuse is set behind it, the way a later variant would lift the refusal."""
    t = P.ClipTransform(16, frames=2, train=train, mixup_alpha=0.8 if mixing else 0.0, brightness=0.4 if photo else 0.0)
    t.antialias, t.eval_views = antialias, eval_views
    return t


def test_the_choice_table_covers_the_grid():
    assert len(CHOICE) == 32 and len({c[:5] for c in CHOICE}) == 32
    assert {c[5] for c in CHOICE} == {"plain", "mix", "views", "photo", "aa"}


@pytest.mark.parametrize("train,mixing,photo,antialias,eval_views,want", CHOICE)
def test_kernel_choice(train, mixing, photo, antialias, eval_views, want):
    t = _transform(train, mixing, photo, antialias, eval_views)
    assert t.kernel() == want
    if not train:
        assert t.kernel() in ("plain", "views", "aa") and (antialias or t.kernel() == ("views" if eval_views == SIX else "plain"))
    if train and photo:
        assert t.kernel() == "photo"                                   # photo wins over mix (its kernel takes the mix rows) and over antialias
    if antialias and not (train and photo):
        assert t.kernel() == "aa" and t.views == (6 if not train and eval_views == SIX else 1)      # V = 1 and V = 6 alike


def test_kernel_names_an_operator_row():
    from transformer_cnn_hybrid_network_for_video_processing_amd import ops
    assert set(ops.CLIP_OPS) == {c[5] for c in CHOICE}
    assert {k: (r.name, r.symbol) for k, r in ops.CLIP_OPS.items()} == {
        "plain": ("clip_transform", "hyb_clips_u8_transform"), "mix": ("clip_transform_mix", "hyb_clips_u8_transform_mix"),
        "views": ("clip_transform_views", "hyb_clips_u8_transform_views"), "photo": ("clip_transform_photo", "hyb_clips_u8_transform_photo"),
        "aa": ("clip_transform_aa", "hyb_clips_u8_transform_aa")}
    # what the constructor accepts chooses as before: the defaults, and every option alone
    assert P.ClipTransform(16).kernel() == "plain" and P.ClipTransform(16, cutmix_alpha=1.0).kernel() == "mix"
    assert P.ClipTransform(16, erase_prob=0.5, mixup_alpha=0.2).kernel() == "photo" and P.ClipTransform(16, antialias=True).kernel() == "aa"
    assert P.ClipTransform(16, train=False, eval_flip=True).kernel() == "views" and P.ClipTransform(16, train=False, eval_crop=0.5).kernel() == "plain"


# ---- the operators: fake kernels and refusals -----------------------------------------------------------------------------------------------
B_, V_, TIN, HIN, WIN, C_, TOUT, HO, WO = 2, 3, 5, 20, 24, 3, 4, 12, 16
ROW = "{y0, x0, ch, cw, flip, t0, tstride, 0}"


def _meta(*shape, dtype=torch.float32):
    return torch.empty(*shape, dtype=dtype, device="meta")


def _args(op, **change):
    """The operator's argument list on meta tensors, valid unless `change` says otherwise."""
    V = V_ if op in ("clip_transform_views", "clip_transform_aa") else 1
    a = dict(src=_meta(B_, TIN, HIN, WIN, C_, dtype=torch.uint8), params=_meta(B_ * V, 8, dtype=torch.int32), mix=_meta(B_, 8, dtype=torch.int32),
             photo=_meta(B_, 16, dtype=torch.int32), luma_sums=_meta(B_, TOUT, dtype=torch.int64), mean_invstd=_meta(2, C_), V=V, Tout=TOUT, Ho=HO,
             Wo=WO)
    a.update(change)
    order = {"clip_transform": "src params mean_invstd Tout Ho Wo", "clip_transform_mix": "src params mix mean_invstd Tout Ho Wo",
             "clip_transform_photo": "src params mix photo luma_sums mean_invstd Tout Ho Wo",
             "clip_transform_views": "src params mean_invstd V Tout Ho Wo", "clip_transform_aa": "src params mean_invstd V Tout Ho Wo",
             "clip_luma_sums": "src params Tout"}[op]
    return [a[k] for k in order.split()]


def _op(op):
    return getattr(torch.ops.hybrid, op)


TRANSFORM_OPS = ["clip_transform", "clip_transform_mix", "clip_transform_photo", "clip_transform_views", "clip_transform_aa"]


@pytest.mark.parametrize("op", TRANSFORM_OPS)
def test_fake_kernels_give_the_output_clips(op):
    V = V_ if op in ("clip_transform_views", "clip_transform_aa") else 1
    for change in ({}, dict(mean_invstd=None)) + ((dict(mix=None, luma_sums=None),) if op == "clip_transform_photo" else ()):
        out = _op(op)(*_args(op, **change))
        assert out.shape == (B_ * V, TOUT, C_, HO, WO) and out.dtype == torch.float32 and out.device.type == "meta"
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        out = _op(op)(*[torch.empty(a.shape, dtype=a.dtype) if isinstance(a, torch.Tensor) else a for a in _args(op)])
        assert out.shape == (B_ * V, TOUT, C_, HO, WO) and out.dtype == torch.float32


def test_fake_kernel_of_luma_sums():
    out = torch.ops.hybrid.clip_luma_sums(*_args("clip_luma_sums"))
    assert out.shape == (B_, TOUT) and out.dtype == torch.int64


def test_schemas_are_what_they_were():
    want = {"clip_transform": "hybrid::clip_transform(Tensor src, Tensor params, Tensor? mean_invstd, int Tout, int Ho, int Wo) -> Tensor",
            "clip_transform_mix": "hybrid::clip_transform_mix(Tensor src, Tensor params, Tensor mix, Tensor? mean_invstd, int Tout, int Ho, int Wo) -> Tensor",
            "clip_transform_photo": "hybrid::clip_transform_photo(Tensor src, Tensor params, Tensor? mix, Tensor photo, Tensor? luma_sums, "
                                    "Tensor? mean_invstd, int Tout, int Ho, int Wo) -> Tensor",
            "clip_transform_views": "hybrid::clip_transform_views(Tensor src, Tensor params, Tensor? mean_invstd, int V, int Tout, int Ho, int Wo) -> Tensor",
            "clip_transform_aa": "hybrid::clip_transform_aa(Tensor src, Tensor params, Tensor? mean_invstd, int V, int Tout, int Ho, int Wo) -> Tensor",
            "clip_luma_sums": "hybrid::clip_luma_sums(Tensor src, Tensor params, int Tout) -> Tensor"}
    for op, schema in want.items():
        assert str(_op(op).default._schema) == schema


# The messages, copied from the operators as they were written one by one.  hybrid::clip_transform_mix and _photo checked src, params,
# mean_invstd and the limits through clip_transform's function and so name clip_transform there.
def _says(op):
    return "clip_transform" if op in ("clip_transform_mix", "clip_transform_photo") else op


_ONE_ROW = f"params must be int32 [{B_},8]: one row {ROW} per clip"
_V_ROWS = f"params must be int32 [{B_ * V_},8]: V = {V_} adjacent rows {ROW} per source clip"
MESSAGES = []
for _o in TRANSFORM_OPS + ["clip_luma_sums"]:
    _views = _o in ("clip_transform_views", "clip_transform_aa")
    MESSAGES += [
        (_o, dict(src=_meta(B_, TIN, HIN, WIN, C_)), TypeError, f"hybrid::{_says(_o)} reads uint8 clips [B,Tin,Hin,Win,C]"),                    # wrong dtype
        (_o, dict(src=_meta(B_, TIN, HIN, WIN, dtype=torch.uint8)), TypeError, f"hybrid::{_says(_o)} reads uint8 clips [B,Tin,Hin,Win,C]"),     # wrong shape
        (_o, dict(params=_meta(B_ * (V_ if _views else 1), 8, dtype=torch.int64)), TypeError, _V_ROWS if _views else _ONE_ROW),
        (_o, dict(params=_meta(B_ * (V_ if _views else 1) + 1, 8, dtype=torch.int32)), TypeError, _V_ROWS if _views else _ONE_ROW),
    ]
    if _o != "clip_luma_sums":
        MESSAGES += [
            (_o, dict(mean_invstd=_meta(2, C_, dtype=torch.float64)), TypeError, f"mean_invstd must be float32 [2,{C_}]: mean, then 1/std"),
            (_o, dict(mean_invstd=_meta(C_, 2)), TypeError, f"mean_invstd must be float32 [2,{C_}]: mean, then 1/std"),
            (_o, dict(src=_meta(B_, TIN, HIN, WIN, 5, dtype=torch.uint8), mean_invstd=None), ValueError,
             f"hybrid::{_says(_o)} needs C <= 4, extents > 0 and Hin, Win, Ho, Wo <= 16384"),
            (_o, dict(Wo=16385), ValueError, f"hybrid::{_says(_o)} needs C <= 4, extents > 0 and Hin, Win, Ho, Wo <= 16384"),
            (_o, dict(Tout=0, luma_sums=None), ValueError, f"hybrid::{_says(_o)} needs C <= 4, extents > 0 and Hin, Win, Ho, Wo <= 16384"),
        ]
    if _views:
        MESSAGES += [(_o, dict(V=0), ValueError, f"hybrid::{_o} needs V >= 1 and B * V within int32, got V = 0 for {B_} clips"),
                     (_o, dict(V=2 ** 30), ValueError, f"hybrid::{_o} needs V >= 1 and B * V within int32, got V = {2 ** 30} for {B_} clips")]
_MIX = f"mix must be int32 [{B_},8]: one row {{partner, kind, by0, bx0, bh, bw, lam_bits, 0}} per clip"
_PHOTO = (f"photo must be int32 [{B_},16]: one row {{brightness, contrast, saturation bits, order, gray, sigma bits, seed lo, seed hi, "
          "ey0, ex0, eh, ew, mode, 0, 0, 0} per clip")
_LUMA = f"luma_sums must be int64 [{B_},{TOUT}]: hybrid::clip_luma_sums of the same src, params and Tout"
MESSAGES += [
    ("clip_transform_mix", dict(mix=_meta(B_, 8, dtype=torch.int64)), TypeError, _MIX),
    ("clip_transform_mix", dict(mix=_meta(B_, 16, dtype=torch.int32)), TypeError, _MIX),
    ("clip_transform_photo", dict(mix=_meta(B_, 8)), TypeError, _MIX),
    ("clip_transform_photo", dict(mix=_meta(B_ + 1, 8, dtype=torch.int32)), TypeError, _MIX),
    ("clip_transform_photo", dict(photo=_meta(B_, 16, dtype=torch.int64)), TypeError, _PHOTO),
    ("clip_transform_photo", dict(photo=_meta(B_, 8, dtype=torch.int32)), TypeError, _PHOTO),
    ("clip_transform_photo", dict(luma_sums=_meta(B_, TOUT, dtype=torch.int32)), TypeError, _LUMA),
    ("clip_transform_photo", dict(luma_sums=_meta(B_, TOUT + 1, dtype=torch.int64)), TypeError, _LUMA),
    ("clip_transform_photo", dict(src=_meta(B_, TIN, HIN, WIN, 2, dtype=torch.uint8), mean_invstd=None), ValueError,
     "hybrid::clip_transform_photo needs C == 1 or C == 3 (the luma is defined for grey and RGB clips)"),
    ("clip_transform_photo", dict(src=_meta(B_, TIN, HIN, WIN, 4, dtype=torch.uint8), mean_invstd=None), ValueError,
     "hybrid::clip_transform_photo needs C == 1 or C == 3 (the luma is defined for grey and RGB clips)"),
    ("clip_luma_sums", dict(src=_meta(B_, TIN, HIN, WIN, 2, dtype=torch.uint8)), ValueError,
     "hybrid::clip_luma_sums needs C == 1 or C == 3, extents > 0 and Hin, Win <= 16384"),
    ("clip_luma_sums", dict(src=_meta(B_, TIN, 16385, WIN, 3, dtype=torch.uint8)), ValueError,
     "hybrid::clip_luma_sums needs C == 1 or C == 3, extents > 0 and Hin, Win <= 16384"),
    ("clip_luma_sums", dict(Tout=0), ValueError, "hybrid::clip_luma_sums needs C == 1 or C == 3, extents > 0 and Hin, Win <= 16384"),
]


@pytest.mark.parametrize("op,change,exc,message", MESSAGES, ids=[f"{m[0]}-{i}" for i, m in enumerate(MESSAGES)])
def test_refusal_messages_are_what_they_were(op, change, exc, message):
    with pytest.raises(exc) as info:
        _op(op)(*_args(op, **change))
    assert str(info.value) == message


def test_the_order_of_the_checks_is_what_it_was():
    # photo: clip_transform's rule (C = 5 is its refusal, not the luma's), then the luma's channels, then mix, photo, luma_sums in that order
    bad = dict(mix=_meta(1, 8, dtype=torch.int32), photo=_meta(1, 16, dtype=torch.int32), luma_sums=_meta(1, TOUT, dtype=torch.int64))
    for change, exc, start in ((dict(src=_meta(B_, TIN, HIN, WIN, 5, dtype=torch.uint8), mean_invstd=None, **bad), ValueError, "hybrid::clip_transform needs"),
                               (dict(src=_meta(B_, TIN, HIN, WIN, 2, dtype=torch.uint8), mean_invstd=None, **bad), ValueError, "hybrid::clip_transform_photo needs"),
                               (bad, TypeError, "mix must be"), ({**bad, "mix": None}, TypeError, "photo must be"),
                               (dict(luma_sums=bad["luma_sums"]), TypeError, "luma_sums must be")):
        with pytest.raises(exc) as info:
            torch.ops.hybrid.clip_transform_photo(*_args("clip_transform_photo", **change))
        assert str(info.value).startswith(start), change
    # views: V before the rows
    with pytest.raises(ValueError, match="V >= 1"):
        torch.ops.hybrid.clip_transform_views(*_args("clip_transform_views", V=0, params=_meta(1, 8, dtype=torch.int64)))


def test_cpu_tensors_are_refused_before_anything_else():
    for op in TRANSFORM_OPS + ["clip_luma_sums"]:
        args = [torch.zeros(a.shape, dtype=a.dtype) if isinstance(a, torch.Tensor) else a for a in _args(op)]
        args[0] = args[0].float()                                      # wrong as well: the device comes first
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            _op(op)(*args)
