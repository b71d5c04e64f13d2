"""CPU-only tests (no GPU): the C-ABI library loads and exports every symbol include/hybrid_hip.h declares, argument
checks fail cleanly without touching a device, the drop-in modules keep the reference's constructor/state-dict contract,
and the product path refuses CPU tensors (no fallback)."""
import ctypes
import os
import re

import pytest
import torch

import transformer_cnn_hybrid_network_for_video_processing_amd as P
from transformer_cnn_hybrid_network_for_video_processing_amd import _lib, ops
from oracle import hybrid_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    from transformer_cnn_hybrid_network_for_video_processing_amd import build
    build.build()
    return _lib.lib


def test_header_declares_expected_entry_points():
    protos = _lib.parse_header()
    for name in ["hyb_conv3x3_fwd", "hyb_conv3x3_wgrad", "hyb_bn_stats_finalize", "hyb_profile_set", "hyb_convstage_fwd", "hyb_convstage_bwd", "hyb_bn_finalize",
                 "hyb_bn_relu_pool_fwd", "hyb_linear_fwd", "hyb_linear_bwd", "hyb_attention_fwd", "hyb_attention_bwd",
                 "hyb_ln_residual_fwd", "hyb_ln_residual_bwd", "hyb_encoder_fwd", "hyb_encoder_bwd", "hyb_head_fwd",
                 "hyb_head_bwd", "hyb_cross_entropy_fwd", "hyb_cross_entropy_bwd", "hyb_gap_fwd", "hyb_gap_bwd"]:
        assert name in protos, name
    # every declaration in the header was understood by the parser
    src = open(os.path.join(ROOT, "include", "hybrid_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    assert set(re.findall(r"\b(hyb_\w+)\s*\(", src)) == set(protos)


def test_library_exports_every_declared_symbol(built):
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in built.protos:
        assert hasattr(dll, name), f"{name} declared in include/hybrid_hip.h but not exported"
    assert built.query("hyb_abi_version") == 9
    assert built.query("hyb_dtype_size", 0) == 4 and built.query("hyb_dtype_size", 1) == 2 and built.query("hyb_dtype_size", 7) == -1
    assert built.query("hyb_pad_channels", 3) == 32 and built.query("hyb_pad_channels", 64) == 64 and built.query("hyb_pad_channels", 65) == 96


def test_no_torch_types_in_the_abi():
    src = open(os.path.join(ROOT, "include", "hybrid_hip.h")).read()
    assert "torch" not in re.sub(r"/\*.*?\*/", " ", src, flags=re.S).lower()
    assert "at::" not in src and "Tensor" not in src


def test_argument_checks_fail_without_a_device(built):
    """Bad arguments return HYB_E_ARG before any HIP call (so this runs on a GPU-less host)."""
    assert built.raw("hyb_conv3x3_fwd")(0, 0, None, None, None, None, None, 1, 8, 8, 3, 32, 32, None) == -1
    assert built.raw("hyb_linear_fwd")(1, None, 8, None, None, None, 4, 8, 8, 0, None) == -1
    assert built.raw("hyb_attention_fwd")(1, None, None, None, None, None, None, 1, 4, 8, 2, 0.0, 0, None) == -1
    assert built.raw("hyb_cross_entropy_fwd")(None, None, None, 1, 2, None) == -1
    assert built.raw("hyb_adamw_step")(0, None, None, None, None, None, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1, None, 0, None) == -1
    with pytest.raises(RuntimeError, match="argument check"):
        built.call("hyb_gap_fwd", 1, None, None, 1, 1, 32, None)
    # workspace / size queries are pure host functions
    assert built.query("hyb_conv_packed_elems", 1, 0, 32) == 32 * 32
    assert built.query("hyb_conv_packed_elems", 0, 64, 128) == 128 * 9 * 64
    assert built.query("hyb_conv_stats_workspace", 64) > 0
    assert built.query("hyb_conv3x3_wgrad_workspace", 0, 4, 16, 16, 32, 64) > 0
    assert built.query("hyb_encoder_saved_bytes", 1, 8, 16, 512, 2048, 2, 8) > 0
    assert built.query("hyb_encoder_workspace_bytes", 1, 8, 16, 512, 2048, 2, 8) > 0
    assert built.query("hyb_convstage_bwd_workspace", 1, 0, 128, 28, 28, 128, 256) > 0


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    fresh = _lib._Lib(str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="no CPU/eager fallback"):
        fresh.call("hyb_abi_version")


def test_split_bf16_build_serves_the_same_abi(built):
    """compute_dtype="bf16x3" = the second build of the library (-DHYB_F32_X3): every declared symbol is there, and a call whose first
    argument is the host-side dtype code HYB_F32X3 is routed to it with HYB_F32 in its place."""
    assert ops.dtype_code("bf16x3") == _lib.HYB_F32X3 and ops.torch_dtype(_lib.HYB_F32X3) is torch.float32
    for name in built.protos:
        built.x3.raw(name)
    assert built.x3.query("hyb_abi_version") == built.query("hyb_abi_version")
    assert "hyb_convstage_fwd" in _lib.DTYPE_FIRST and "hyb_abi_version" not in _lib.DTYPE_FIRST
    assert built.query("hyb_encoder_saved_bytes", _lib.HYB_F32X3, 8, 16, 512, 2048, 2, 8) == built.query("hyb_encoder_saved_bytes", _lib.HYB_F32, 8, 16, 512, 2048, 2, 8)
    with pytest.raises(RuntimeError, match="argument check"):                  # reaches the x3 library's own argument check
        built.call("hyb_gap_fwd", _lib.HYB_F32X3, None, None, 1, 1, 32, None)


def test_module_contract_matches_reference_and_oracle():
    m = P.TransformerCNNHybrid()                              # zero-argument constructible (Model.py:27 / FCT.py:302)
    ref = R.TransformerCNNHybridRef()
    assert sum(p.numel() for p in m.parameters()) == 6_827_304
    assert list(m.state_dict().keys()) == list(ref.state_dict().keys())
    m.load_state_dict(ref.state_dict())                       # oracle <-> product checkpoints interchange
    ref.load_state_dict(m.state_dict())
    for k in ("encoder1.enc1conv1.weight", "encoder1.enc1norm1.running_var", "encoder1.enc1norm1.num_batches_tracked",
              "encoder.attention_layers.0.query_layer.weight", "encoder.feedforward_layers.1.2.bias", "encoder.layer_norm.0.weight"):
        assert k in m.state_dict()
    assert all(p.dtype == torch.float32 for p in m.parameters())
    torch.optim.AdamW(m.parameters(), lr=1e-3)                # stock optimizer accepts them (Model.py:153)


def test_encoder_ctor_contract():
    with pytest.raises(ValueError, match="Input dimension must be divisible by number of heads. Here, Input dimension = 10"):
        P.TransformerEncoder(10, 16, 1, 3, 0.0)
    with pytest.raises(TypeError):
        P.TransformerEncoder(8, 16)                           # five required positionals, as in the reference
    enc = P.TransformerEncoder(8, 16, 2, 2, 0.1)
    assert enc.attention_layers[0].dropoutLayer.p == 0.1 and enc.dropout == 0.1
    assert enc.attention_layers[0]._attn_p() == 0.1
    enc.eval()
    assert enc.attention_layers[0]._attn_p() == 0.0           # quirk Q5: attention dropout follows train()/eval()
    with pytest.raises(ValueError):
        P.TransformerCNNHybrid(compute_dtype="fp16")
    with pytest.raises(ValueError, match="multiple of 8"):       # the token projection's 16-byte rows: said at construction, not as a C status later
        P.TransformerCNNHybrid(cnn_channels=(8, 12))


def test_product_path_refuses_cpu_tensors():
    m = P.TransformerCNNHybrid(cnn_channels=(32,), d_model=32, num_heads=2, num_layers=1, hidden_dim=32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.rand(1, 2, 3, 16, 16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.TransformerEncoder(8, 16, 1, 2, 0.0)(torch.rand(1, 4, 8), None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.HybridCrossEntropyLoss()(torch.rand(2, 3), torch.tensor([0, 1]))
    w = torch.nn.Parameter(torch.rand(4)); w.grad = torch.rand(4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.HybridAdamW([w]).step()
    with pytest.raises(ValueError):
        m(torch.rand(3, 16, 16))


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "transformer_cnn_hybrid_network_for_video_processing_amd")
    for f in os.listdir(pkg):
        if f.endswith(".py"):
            src = open(os.path.join(pkg, f)).read()
            assert "oracle" not in src, f
    for f in os.listdir(os.path.join(pkg, "csrc")):
        if f.endswith((".hip", ".h")):
            assert "oracle" not in open(os.path.join(pkg, "csrc", f)).read(), f


# ---- conv3x3 variant queries (csrc/conv_plan.h; include/hybrid_hip.h documents the codes) ----------------------------------------------------
F32, BF16 = 0, 1
# code = 100 * family + table row -> a shape (dtype, N, H, W, Cip, Cop) that takes it.  Asynchronous rows come in two tile orientations:
# 8 x 28 (N = 2, H = 8, W = 28) and 4 x 56, which wins the cost comparison only when 8 x 28 needs a second round of 256 workgroups
# (N = 130, H = 4, W = 56: 260 tiles against 130).
FWD_VARIANTS = {
    0: (F32, 1, 12, 20, 128, 256), 1: (F32, 2, 16, 16, 64, 128), 2: (F32, 2, 19, 37, 32, 64), 3: (F32, 2, 16, 32, 32, 32),
    100: (BF16, 2, 16, 32, 32, 32),
    101: (BF16, 2, 8, 28, 64, 64), 102: (BF16, 130, 4, 56, 64, 64),
    103: (BF16, 2, 8, 28, 64, 128), 104: (BF16, 130, 4, 56, 64, 128),
    105: (BF16, 2, 8, 28, 64, 256), 106: (BF16, 130, 4, 56, 64, 256),
    200: (BF16, 2, 8, 28, 32, 64), 201: (BF16, 130, 4, 56, 32, 64),
}
FWD_HAS_EXT = {100, 101, 102, 103, 104, 200, 201}          # 105 / 106 (eight waves, 64 channels per wave) have no EXT instantiation
FWD_HAS_POOL = set(range(100, 107)) | {200, 201}
CHANNELS = (32, 64, 96, 128, 192, 256)


def test_every_forward_variant_code_has_a_shape(built, monkeypatch):
    for k in [k for k in os.environ if k.startswith("HYB_")]:
        monkeypatch.delenv(k)
    q = lambda *a: built.query("hyb_conv3x3_fwd_variant", *a)
    for code, args in FWD_VARIANTS.items():
        assert q(*args) == code, (code, args)
    # the table has no other code: a sweep over channel counts, both orientations and both dtypes returns nothing else
    seen = {q(dt, n, h, w, ci, co) for dt in (F32, BF16) for (n, h, w) in ((2, 8, 28), (130, 4, 56), (1, 5, 5)) for ci in CHANNELS for co in CHANNELS}
    assert seen == set(FWD_VARIANTS)
    assert q(BF16, 32, 112, 112, 32, 64) == 200 and q(BF16, 32, 14, 14, 128, 256) in (105, 106)      # config-2 stages 2 and 4
    for bad in ((BF16, 0, 8, 8, 32, 32), (BF16, 1, 8, 8, 33, 32), (BF16, 1, 8, 8, 32, 40), (7, 1, 8, 8, 32, 32), (BF16, 1, 0, 8, 32, 32)):
        assert q(*bad) == -1, bad


def test_pool_queries_and_stats_rows_follow_the_forward_variant(built, monkeypatch):
    for k in [k for k in os.environ if k.startswith("HYB_")]:
        monkeypatch.delenv(k)
    for dt in (F32, BF16):
        for ci in CHANNELS:
            for co in CHANNELS:
                for (n, h, w) in ((2, 8, 28), (130, 4, 56), (3, 30, 58)):
                    code = built.query("hyb_conv3x3_fwd_variant", dt, n, h, w, ci, co)
                    assert built.query("hyb_conv3x3_pool_ext", dt, w, ci, co) == int(code in FWD_HAS_EXT), (dt, ci, co, code)
                    assert built.query("hyb_conv3x3_pool_fused", dt, w, ci, co) == int(code in FWD_HAS_POOL), (dt, ci, co, code)
                    # the promised partial-statistics rows: the first-generation tiling of Cop (8 x 16, 16 x 16 or 16 x 32 pixels), at most 512
                    th, tw = (8, 16) if co % 256 == 0 else (16, 16) if co % 128 == 0 else (16, 32)
                    rows = min(512, n * -(-h // th) * -(-w // tw))
                    assert built.query("hyb_conv_stats_rows", 0, n, h, w, co) == rows, (n, h, w, co)


def test_wgrad_variant_reproduces_the_benchmarks_third_generation_rule(built, monkeypatch):
    """bench.py names the weight-gradient kernel of stages 2-4 by its own copy of the rule (it may not ask the library while it is the yardstick);
    the plan must agree with it on the benchmark's own shapes, bf16 and fp32."""
    for k in [k for k in os.environ if k.startswith("HYB_")]:
        monkeypatch.delenv(k)
    chans = (3, 32, 64, 128, 256)
    for size in (224, 448, 112):                     # CONFIGS 2 / 4, 5, and the accuracy leg
        H = size // 2
        for li in range(1, 4):
            ci, co = chans[li], chans[li + 1]
            gen3 = ci % 64 == 0 and co % 64 == 0 and H % 28 == 0 and H % 4 == 0            # bench.py, kernel_specs of the conv stages
            want = 364 if gen3 else 200 + (64 if ci % 64 == 0 else 32)
            assert built.query("hyb_conv3x3_wgrad_variant", BF16, 1, 32, H, H, ci, co) == want, (size, li)
            assert built.query("hyb_conv3x3_wgrad_variant", F32, 1, 32, H, H, ci, co) == 100 + (64 if ci % 64 == 0 else 32)
            H //= 2
    q = lambda *a: built.query("hyb_conv3x3_wgrad_variant", *a)
    assert q(BF16, 0, 2, 8, 28, 64, 64) == 264 and q(BF16, 1, 2, 8, 28, 64, 64) == 364          # only the fused form has a third generation
    assert q(BF16, 1, 2, 8, 28, 64, 96) == 164 and q(BF16, 1, 2, 8, 28, 96, 64) == 232           # Cop % 64 != 0: first generation
    assert q(BF16, 1, 2, 8, 28, 33, 64) == -1 and q(BF16, 1, 0, 8, 28, 32, 64) == -1
