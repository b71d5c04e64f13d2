"""The GPU side of tests/test_gpu_convstage_bwd_exact.py: hyb_convstage_bwd (and its public pieces) on the integer data of
tests/convstage_bwd_ref.py, through the ctypes binding with caller-owned buffers.  Importing it starts nothing.

As a child process:  python tests/convstage_bwd_worker.py OUT.pt
The HYB_* switches are read once per process, so each side of a switch is a run of this script under its value: the eval-mode table in bf16
(the storage type the switches act on), every row compared with the fp64 reference by the assertions of the default run.  Saves
{row id: {"fails": [...], "paths": (wgrad code, dgrad code), "dW", "dgamma", "dbeta", "dx_sum"}} to OUT.pt."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import convstage_bwd_ref as R                                                           # noqa: E402

# mode -> (dtype code of the binding, torch storage type, storage of the dense gradient in the reference)
DT = {"fp32": (0, torch.float32, "fp32"), "bf16": (1, torch.bfloat16, "bf16"), "bf16x3": (2, torch.float32, "fp32")}
SENTINEL = 7.0


def L():
    from transformer_cnn_hybrid_network_for_video_processing_amd._lib import lib
    return lib


def st():
    return torch.cuda.current_stream().cuda_stream


def to_nhwc(x, code, tdt, cp):
    """fp64 CPU NCHW -> T NHWC on the device, channels padded with zeros to cp"""
    N, C, H, W = x.shape
    out = torch.empty(N, H, W, cp, dtype=tdt, device="cuda")
    L().call("hyb_nchw_to_nhwc", code, x.float().cuda().contiguous(), out, N, C, H, W, cp, st())
    return out


def to_nchw(x, code, C):
    """T NHWC on the device -> fp64 CPU NCHW of the first C channels"""
    N, H, W, cp = x.shape
    out = torch.empty(N, C, H, W, dtype=torch.float32, device="cuda")
    L().call("hyb_nhwc_to_nchw", code, x, out, N, C, H, W, cp, st())
    return out.cpu().double()


def padded_rows(a, b, cop):
    """two [Co] fp64 rows -> fp32 [2][Cop] on the device, padded channels zero"""
    out = torch.zeros(2, cop, dtype=torch.float32)
    out[0, :a.numel()] = a.float()
    out[1, :b.numel()] = b.float()
    return out.cuda()


def stage_inputs(c, mode):
    code, tdt, _ = DT[mode]
    ci, co, n, h, w = c["shape"]
    cip, cop = R.pad32(ci), R.pad32(co)
    return dict(code=code, tdt=tdt, cip=cip, cop=cop, x=to_nhwc(c["x"], code, tdt, cip), y=to_nhwc(c["y"], code, tdt, cop),
                dp=to_nhwc(c["dp"], code, tdt, cop), pooled=to_nhwc(c["pooled"], code, tdt, cop), w=c["w"].float().cuda().contiguous(),
                gamma=c["gamma"].float().cuda(), ss=padded_rows(c["scale"], c["shift"], cop), mi=padded_rows(c["mean"], c["invstd"], cop))


def run_bwd(c, mode, training, use_pooled=True, use_packed=True):
    """hyb_convstage_bwd (first = 0) -> dict of fp64 CPU tensors: dW, dx (true channels), dgamma, dbeta, and dx_pad_zero"""
    ci, co, n, h, w = c["shape"]
    a = stage_inputs(c, mode)
    code, tdt, cip, cop = a["code"], a["tdt"], a["cip"], a["cop"]
    packed = None
    if use_packed:
        packed = torch.empty(L().query("hyb_convstage_packed_bwd_elems", 0, cip, cop), dtype=tdt, device="cuda")
        L().call("hyb_conv_pack_weight", code, 1, a["w"], packed, co, ci, cop, cip, st())
    dx = torch.full((n, h, w, cip), SENTINEL, dtype=tdt, device="cuda")
    dw = torch.full((co, ci, 3, 3), SENTINEL, device="cuda")
    dgamma, dbeta = torch.full((co,), SENTINEL, device="cuda"), torch.full((co,), SENTINEL, device="cuda")
    nb = L().query("hyb_convstage_bwd_workspace", code, 0, n, h, w, cip, cop)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    L().call("hyb_convstage_bwd", code, 0, a["dp"], a["x"], a["y"], a["pooled"] if use_pooled else None, a["w"], a["gamma"], a["ss"], a["mi"],
             int(training), n, h, w, ci, cip, co, cop, dx, dw, dgamma, dbeta, packed, ws, nb, st())
    torch.cuda.synchronize()
    return dict(dW=dw.cpu().double(), dx=to_nchw(dx, code, ci), dgamma=dgamma.cpu().double(), dbeta=dbeta.cpu().double(),
                dx_pad_zero=bool((dx[..., ci:] == 0).all()))


def run_reduce_dx(c, mode, training, use_pooled):
    """the public two-pass form, hyb_bn_relu_pool_bwd_reduce + hyb_bn_relu_pool_bwd_dx -> dyraw (fp64 CPU NCHW), dgamma, dbeta"""
    ci, co, n, h, w = c["shape"]
    a = stage_inputs(c, mode)
    code, tdt, cop = a["code"], a["tdt"], a["cop"]
    sums = torch.full((2, cop), SENTINEL, device="cuda")
    part = torch.empty(L().query("hyb_bn_bwd_reduce_workspace", cop), dtype=torch.uint8, device="cuda")
    dgamma, dbeta = torch.full((co,), SENTINEL, device="cuda"), torch.full((co,), SENTINEL, device="cuda")
    L().call("hyb_bn_relu_pool_bwd_reduce", code, a["dp"], a["y"], a["pooled"] if use_pooled else None, a["ss"], a["mi"], sums, part, dgamma, dbeta,
             n, h, w, co, cop, st())
    dyraw = torch.full((n, h, w, cop), SENTINEL, dtype=tdt, device="cuda")
    L().call("hyb_bn_relu_pool_bwd_dx", code, a["dp"], a["y"], a["ss"], a["mi"], a["gamma"], sums, int(training), n * h * w, dyraw, None, None,
             n, h, w, co, cop, st())
    torch.cuda.synchronize()
    return dict(dyraw=to_nchw(dyraw, code, co), dgamma=dgamma.cpu().double(), dbeta=dbeta.cpu().double(), pad_zero=bool((dyraw[..., co:] == 0).all()))


def describe_mismatch(c, r, name, got, ref):
    """Where an exact comparison failed, in the kernels' terms: tile (8 x 28 of the later generations, 8 x 16 of the first), 32-channel block,
    position inside the 2 x 2 window, and whether the windows involved tie or hold a zero pre-activation."""
    bad = (got != ref).nonzero()
    lines = [f"{name}: {bad.shape[0]} of {ref.numel()} differ"]
    for idx in bad[:6].tolist():
        if name == "dx":
            nn, ch, yy, xx = idx
            lines.append(f"  n {nn} ci {ch} (block {ch // 32}) y {yy} x {xx}: tile28 ({yy // 8},{xx // 28}) tile16 ({yy // 8},{xx // 16}) window pos ({yy % 2},{xx % 2}) "
                         f"got {got[tuple(idx)].item()} want {ref[tuple(idx)].item()}")
        else:
            co_, ci_, ky, kx = idx
            z = c["z"][:, co_]
            lines.append(f"  co {co_} (block {co_ // 32}, octet {co_ // 8}) ci {ci_} (block {ci_ // 32}) tap ({ky},{kx}): got {got[tuple(idx)].item()} want "
                         f"{ref[tuple(idx)].item()}; channel has gamma {c['gamma'][co_].item()} zero pre-activations {int((z == 0).sum())}")
    return "\n".join(lines)


def check_eval(c, r, got, mode):
    """-> list of failures of the eval-mode assertions: dweight, dgamma, dbeta equal, dx the one correct rounding, padded dx channels zero"""
    fails, _ = R.compare(r, got, False, DT[mode][2])
    if not got["dx_pad_zero"]:
        fails.append("padded input channels of dx are not exact zeros")
    if fails:
        dx_ref = R.bf16_rne(r["dx"]) if mode == "bf16" else r["dx"]
        for name, ref in (("dW", r["dW"]), ("dx", dx_ref)):
            if not torch.equal(got[name], ref):
                fails.append(describe_mismatch(c, r, name, got[name], ref))
    return fails


def query_paths(mode, shape):
    ci, co, n, h, w = shape
    code = DT[mode][0]
    cip, cop = R.pad32(ci), R.pad32(co)
    return (L().query("hyb_conv3x3_wgrad_variant", code, 1, n, h, w, cip, cop), L().query("hyb_conv3x3_fwd_variant", code, n, h, w, cop, cip))


if __name__ == "__main__":
    res = {}
    for shape, rid in zip(R.SHAPES, R.IDS):
        c = R.case(*shape)
        r = R.reference_for(shape, False)
        got = run_bwd(c, "bf16", False)
        res[rid] = dict(fails=check_eval(c, r, got, "bf16"), paths=query_paths("bf16", shape), dW=got["dW"].float(), dgamma=got["dgamma"].float(),
                        dbeta=got["dbeta"].float(), dx_sum=got["dx"].sum(dim=(0, 2, 3)))
        print(rid, res[rid]["paths"], "ok" if not res[rid]["fails"] else res[rid]["fails"], flush=True)
    torch.save(res, sys.argv[1])
