"""CPU-only tests of the inference path (predict): the C ABI declares and both builds of the library export the new entry points, their
argument checks fail cleanly without a device, the workspace / dispatch queries are pure host functions, and the Python entry points
refuse CPU tensors (no fallback)."""
import ctypes
import os

import pytest
import torch

import transformer_cnn_hybrid_network_for_video_processing_amd as P
from transformer_cnn_hybrid_network_for_video_processing_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["hyb_conv3x3_pool_fused", "hyb_convstage_infer_workspace", "hyb_convstage_infer", "hyb_backbone_infer_workspace", "hyb_backbone_infer"]
F32, BF16 = _lib.HYB_F32, _lib.HYB_BF16


@pytest.fixture(scope="module")
def built():
    from transformer_cnn_hybrid_network_for_video_processing_amd import build
    build.build()
    return _lib.lib


def test_header_declares_the_inference_entry_points():
    protos = _lib.parse_header()
    for name in NEW:
        assert name in protos, name
    # dtype-dependent ones keep `int dtype` first: _lib routes compute_dtype="bf16x3" to the second library by it
    for name in NEW:
        assert name in _lib.DTYPE_FIRST, name
    assert protos["hyb_convstage_infer"][0] == "int" and len(protos["hyb_convstage_infer"][1]) == 20
    assert protos["hyb_backbone_infer"][0] == "int" and len(protos["hyb_backbone_infer"][1]) == 13
    assert protos["hyb_backbone_infer_workspace"] == ("size_t", ["int", "int", "ptr", "int", "int", "int"])
    assert protos["hyb_conv3x3_pool_fused"] == ("int", ["int", "int", "int", "int"])


def test_both_libraries_export_them_and_the_abi_version_stays(built):
    for path in (_lib.LIB_PATH, _lib.LIB_X3_PATH):
        dll = ctypes.CDLL(path)
        for name in NEW:
            assert hasattr(dll, name), f"{name} not exported by {os.path.basename(path)}"
    assert built.query("hyb_abi_version") == 9 and built.x3.query("hyb_abi_version") == 9


def test_argument_checks_fail_without_a_device(built):
    for lib in (built, built.x3):
        assert lib.raw("hyb_convstage_infer")(BF16, 0, None, None, None, None, None, None, 1e-5, 2, 56, 56, 64, 64, 128, 128, None, None, 0, None) == -1
        assert lib.raw("hyb_convstage_infer")(F32, 1, None, None, None, None, None, None, 1e-5, 2, 56, 56, 3, 0, 32, 32, None, None, 0, None) == -1
        ch = (ctypes.c_int * 5)(3, 32, 64, 128, 256)
        assert lib.raw("hyb_backbone_infer")(BF16, 4, ch, None, None, 1e-5, 2, 64, 64, None, None, 0, None) == -1
        assert lib.raw("hyb_backbone_infer")(BF16, 4, None, None, None, 1e-5, 2, 64, 64, None, None, 0, None) == -1
    with pytest.raises(RuntimeError, match="argument check"):
        built.call("hyb_convstage_infer", BF16, 0, None, None, None, None, None, None, 1e-5, 2, 56, 56, 64, 64, 128, 128, None, None, 0, None)
    with pytest.raises(RuntimeError, match="argument check"):          # routed to the split-bf16 build by the dtype code
        built.call("hyb_convstage_infer", _lib.HYB_F32X3, 0, None, None, None, None, None, None, 1e-5, 2, 56, 56, 64, 64, 128, 128, None, None, 0, None)


def test_workspace_queries_are_positive_host_functions(built):
    ch = (ctypes.c_int * 5)(3, 32, 64, 128, 256)
    for dt in (F32, BF16, _lib.HYB_F32X3):
        assert built.query("hyb_convstage_infer_workspace", dt, 1, 2, 64, 64, 0, 32) > 0
        assert built.query("hyb_convstage_infer_workspace", dt, 0, 2, 56, 56, 64, 128) > 0
        assert built.query("hyb_backbone_infer_workspace", dt, 4, ch, 2, 64, 64) > 0
    # bad arguments: 0, like the other size queries
    assert built.query("hyb_backbone_infer_workspace", BF16, 0, ch, 2, 64, 64) == 0
    assert built.query("hyb_backbone_infer_workspace", BF16, 4, None, 2, 64, 64) == 0
    assert built.query("hyb_convstage_infer_workspace", BF16, 0, 2, 56, 56, 60, 128) == 0
    # the fused stage holds no full-resolution conv output, the fallback does: fp32 needs N*H*W*Cop*4 bytes more than weights + scale/shift
    n, h, w, cip, cop = 128, 56, 56, 64, 128
    fused = built.query("hyb_convstage_infer_workspace", BF16, 0, n, h, w, cip, cop)
    assert fused < n * h * w * cop * 2
    assert built.query("hyb_convstage_infer_workspace", F32, 0, n, h, w, cip, cop) >= n * h * w * cop * 4
    # config 2, bf16: the whole backbone's workspace is the two ping-pong pooled maps (102.8 + 51.4 MB) plus 0.8 MB of packed weights and rows
    # and the first stage's scratch (9.4 MB, sized for its training passes): nothing of the 359.7 MB of full-resolution conv outputs
    ws = built.query("hyb_backbone_infer_workspace", BF16, 4, ch, 128, 224, 224)
    pooled = 128 * 112 * 112 * 32 * 2 + 128 * 56 * 56 * 64 * 2
    assert pooled <= ws <= pooled + (12 << 20)


def test_pool_fused_dispatch_query(built):
    q = lambda *a: built.query("hyb_conv3x3_pool_fused", *a)
    for w, cip, cop in ((112, 32, 64), (56, 64, 128), (28, 128, 256), (24, 32, 32)):
        assert q(BF16, w, cip, cop) == 1, (w, cip, cop)
        assert q(F32, w, cip, cop) == 0, (w, cip, cop)
        assert q(_lib.HYB_F32X3, w, cip, cop) == 0, (w, cip, cop)
        assert ops.conv3x3_pool_fused(BF16, w, cip, cop) is True
    assert q(BF16, 1 << 20, 32, 64) == 0            # past the asynchronous kernels' 32-bit offset limit: the conv -> bn_relu_pool pair
    assert q(BF16, 112, 48, 64) == 0 and q(BF16, 112, 32, 48) == 0      # channel counts arrive padded to multiples of 32


def test_inference_entry_points_refuse_cpu_tensors():
    m = P.TransformerCNNHybrid(cnn_channels=(32,), d_model=32, num_heads=2, num_layers=1, hidden_dim=32)
    for training in (True, False):
        m.train(training)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.predict(torch.rand(1, 2, 3, 16, 16))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.forward_backbone_infer(torch.rand(2, 3, 16, 16))
        assert m.training is training                 # predict never changes the mode
    with pytest.raises(ValueError):
        m.predict(torch.rand(3, 16, 16))
    st = P.ConvBNReLUPool(3, 32, "enc1")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        st.infer(torch.rand(1, 3, 16, 16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.ConvBNReLUPool(32, 64, "enc2").infer(torch.rand(1, 32, 16, 16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.GraphedPredict(m, torch.rand(1, 2, 3, 16, 16))
    # a model the fused path rejects takes the existing forward -- which refuses CPU tensors too -- and gets its flags back
    m.train()
    m.fuse_model_ops = False
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.predict(torch.rand(1, 2, 3, 16, 16))
    assert m.training and all(s.training for s in m.modules())


def test_inference_operators_are_registered_with_fake_kernels():
    assert "GraphedPredict" in P.__all__
    x = torch.empty(2, 56, 56, 64, dtype=torch.bfloat16, device="meta")
    w = torch.empty(128, 64, 3, 3, device="meta")
    v = torch.empty(128, device="meta")
    out = torch.ops.hybrid.convstage_infer(x, w, v, v, v, v, 1e-5, BF16, False)
    assert out.shape == (2, 28, 28, 128) and out.dtype == torch.bfloat16
    f = torch.empty(4, 3, 64, 64, device="meta")
    ws = [torch.empty(8, 3, 3, 3, device="meta"), torch.empty(24, 8, 3, 3, device="meta")]
    vs = [torch.empty(8, device="meta"), torch.empty(24, device="meta")]
    out = torch.ops.hybrid.backbone_infer(f, ws, vs, vs, vs, vs, 1e-5, F32)
    assert out.shape == (4, 16, 16, 32) and out.dtype == torch.float32


def test_product_package_still_never_names_the_oracle():
    pkg = os.path.join(ROOT, "transformer_cnn_hybrid_network_for_video_processing_amd")
    for f in os.listdir(pkg):
        if f.endswith(".py"):
            assert "oracle" not in open(os.path.join(pkg, f)).read(), f
    for f in os.listdir(os.path.join(pkg, "csrc")):
        if f.endswith((".hip", ".h")):
            assert "oracle" not in open(os.path.join(pkg, "csrc", f)).read(), f
    assert "oracle" not in open(os.path.join(ROOT, "include", "hybrid_hip.h")).read()
