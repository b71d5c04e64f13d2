"""hyb_convstage_bwd -- the backward of a conv stage as training runs it: the BatchNorm sums (from the raw conv output or from `pooled`), the
weight gradient with the BatchNorm / ReLU / MaxPool backward fused into its tile staging, the dense gradient handed NHWC or block-planar to
the dgrad conv -- pinned BIT FOR BIT on the integer data of tests/convstage_bwd_ref.py, on every kernel path the dispatch rules hold
(tests/test_convstage_bwd_ref_cpu.py asserts the table reaches them and that the recipe's conditions hold).

  eval mode      every product and sum is exactly representable: dweight, dgamma, dbeta equal the fp64 reference, dx is its one correct rounding
  training mode  power-of-two counts: the batch means are exact as well, the dense gradient equals bf16_rne(pre) element for element and
                 dgamma / dbeta stay exact; dweight and dx within the accumulation bounds below.  Other counts: the same bounds plus the slack
                 of the elements whose rounding the evaluation order can flip (`unsafe`, at most 2 % of them).
  bounds         |dW - ref| <= (count + 8) 2^-24 sum |x| |dyraw|  (count fp32 additions and the slab sums on exact products),
                 |dx - ref| <= 2^-8 |ref| + (9 Cop + 8) 2^-23 dgrad(|dyraw|, |w|)  (the form of tests/test_gpu_infer.py: one storage rounding, fp32
                 accumulation over 9 Cop products) -- derived from the reference, none fitted to a kernel.

Measured ratios: profiles/convstage_bwd_exact.txt."""
import os
import subprocess
import sys
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convstage_bwd_ref as R          # noqa: E402
import convstage_bwd_worker as G       # noqa: E402  (importing it starts nothing)

POW2 = [c[:5] for c in R.CASES if c[8]]
POW2_IDS = [i for c, i in zip(R.CASES, R.IDS) if c[8]]
OTHER = [c[:5] for c in R.CASES if not c[8]]
OTHER_IDS = [i for c, i in zip(R.CASES, R.IDS) if not c[8]]


# ---- eval mode: equal ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "bf16", "bf16x3"])
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.IDS)
def test_eval_backward_equals_the_reference(shape, mode):
    c, r = R.case(*shape), R.reference_for(shape, False)
    t0 = time.time()
    got = G.run_bwd(c, mode, False)
    fails = G.check_eval(c, r, got, mode)
    print(f"eval {mode} {shape}: paths {G.query_paths(mode, shape)} {time.time() - t0:.2f} s")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("mode", ["fp32", "bf16", "bf16x3"])
@pytest.mark.parametrize("shape", R.COMBO_SHAPES, ids=["%dto%d_%dx%dx%d" % s for s in R.COMBO_SHAPES])
def test_eval_backward_with_and_without_pooled_and_packed_weights(shape, mode):
    """`pooled` given (the sums come from it, octet by octet where |beta / gamma| <= 4 and no gamma is zero) or NULL (from the raw conv output);
    packed_bwd from hyb_conv_pack_weight mode 1 or NULL (repacked into the workspace): the same bits all four ways."""
    c, r = R.case(*shape), R.reference_for(shape, False)
    outs = []
    for use_pooled in (True, False):
        for use_packed in (True, False):
            got = G.run_bwd(c, mode, False, use_pooled, use_packed)
            fails = G.check_eval(c, r, got, mode)
            assert not fails, f"pooled {use_pooled} packed {use_packed}:\n" + "\n".join(fails)
            outs.append(got)
    for o in outs[1:]:
        for k in ("dW", "dx", "dgamma", "dbeta"):
            assert torch.equal(o[k], outs[0][k]), k


# ---- training mode ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", POW2, ids=POW2_IDS)
def test_training_dense_gradient_is_exact_on_power_of_two_counts(shape, mode):
    """Through the public two-pass form: the sums from `pooled` and from the raw output, then hyb_bn_relu_pool_bwd_dx."""
    c, r = R.case(*shape), R.reference_for(shape, True, G.DT[mode][2])
    for use_pooled in (True, False):
        got = G.run_reduce_dx(c, mode, True, use_pooled)
        assert torch.equal(got["dgamma"], r["dgamma"]) and torch.equal(got["dbeta"], r["dbeta"]), use_pooled
        bad = (got["dyraw"] != r["dyraw"]).nonzero()
        assert bad.shape[0] == 0, f"pooled {use_pooled}: {bad.shape[0]} of {r['dyraw'].numel()} elements of the dense gradient differ, first (n, co, y, x) {bad[:6].tolist()}"
        assert got["pad_zero"]


def _training_case(shape, mode):
    c, r = R.case(*shape), R.reference_for(shape, True, G.DT[mode][2])
    t0 = time.time()
    got = G.run_bwd(c, mode, True)
    fails, ratios = R.compare(r, got, True, G.DT[mode][2], cop=R.pad32(shape[1]))
    print(f"training {mode} {shape}: error / bound dW {ratios.get('dW', 0):.3g} dx {ratios.get('dx', 0):.3g}, unsafe share {float(r['unsafe'].double().mean()):.5f}, "
          f"{time.time() - t0:.2f} s")
    assert got["dx_pad_zero"]
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", POW2, ids=POW2_IDS)
def test_training_backward_on_power_of_two_counts(shape, mode):
    _training_case(shape, mode)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", OTHER, ids=OTHER_IDS)
def test_training_backward_on_other_counts(shape, mode):
    _training_case(shape, mode)


# ---- the switches: one child process per value ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("switch", ["HYB_DYRAW_PLANAR", "HYB_WGRAD_V3", "HYB_WGRAD_V2", "HYB_CONV_V2"])
def test_eval_table_with_a_kernel_generation_switched_off(tmp_path, switch):
    path = str(tmp_path / "out.pt")
    env = dict(os.environ)
    env[switch] = "0"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "convstage_bwd_worker.py"), path], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:]
    res = torch.load(path)
    assert set(res) == set(R.IDS)
    wg = {v["paths"][0] for v in res.values()}
    dg = {v["paths"][1] for v in res.values()}
    if switch == "HYB_WGRAD_V3":
        assert wg == {132, 164, 232, 264}
    elif switch == "HYB_WGRAD_V2":
        assert wg == {132, 164}
    elif switch == "HYB_CONV_V2":
        assert dg == R.DGRAD_F32
    else:
        assert wg == R.WGRAD_BF16 and dg == R.DGRAD_BF16
    for rid, v in res.items():
        assert not v["fails"], rid + "\n" + "\n".join(v["fails"])
    # equal to the reference on both sides of the switch, hence to the default run bit for bit; two rows said out loud
    for shape, rid in list(zip(R.SHAPES, R.IDS))[6:8]:
        got = G.run_bwd(R.case(*shape), "bf16", False)
        assert torch.equal(got["dW"].float(), res[rid]["dW"]) and torch.equal(got["dx"].sum(dim=(0, 2, 3)), res[rid]["dx_sum"])


# ---- first stage (first = 1), eval mode ---------------------------------------------------------------------------------------------------------
def _run_first(c, mode, route=None, offset=False):
    code, tdt, _ = G.DT[mode]
    ci, co, n, h, w = c["shape"]
    cop = R.pad32(co)
    L = G.L()
    if offset:                       # a view 4 bytes into a larger buffer: not 16-byte aligned, the block-level kernels
        buf = torch.zeros(n * ci * h * w + 1, device="cuda")
        x = buf[1:].view(n, ci, h, w)
        x.copy_(c["x"].float())
        assert x.data_ptr() % 16 == 4 and x.is_contiguous()
    else:
        x = c["x"].float().cuda().contiguous()
    dp = G.to_nhwc(c["dp"], code, tdt, cop)
    wt, gamma = c["w"].float().cuda().contiguous(), c["gamma"].float().cuda()
    ss, mi = G.padded_rows(c["scale"], c["shift"], cop), G.padded_rows(c["mean"], c["invstd"], cop)
    dw = torch.full((co, ci, 3, 3), G.SENTINEL, device="cuda")
    dgamma, dbeta = torch.full((co,), G.SENTINEL, device="cuda"), torch.full((co,), G.SENTINEL, device="cuda")
    nb = L.query("hyb_convstage_bwd_workspace", code, 1, n, h, w, 0, cop)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    L.call("hyb_convstage_bwd", code, 1, dp, x, route, None, wt, gamma, ss, mi, 0, n, h, w, ci, 0, co, cop, None, dw, dgamma, dbeta, None, ws, nb, G.st())
    torch.cuda.synchronize()
    return dict(dW=dw.cpu().double(), dgamma=dgamma.cpu().double(), dbeta=dbeta.cpu().double())


def _first_forward_codes(c, mode):
    """hyb_convstage_fwd in eval mode with eps = 0 and running_var = 1 / invstd^2 (1 or 4): fills the routing codes; its scale_shift must be the
    hand-made one exactly and its pooled output the reference's"""
    code, tdt, _ = G.DT[mode]
    ci, co, n, h, w = c["shape"]
    cop = R.pad32(co)
    L = G.L()
    elems = L.query("hyb_convstage_route_elems", code, n, h, w, cop)
    if elems <= 0:
        return None
    route = torch.zeros(elems, dtype=tdt, device="cuda")
    x = c["x"].float().cuda().contiguous()
    pooled = torch.full((n, h // 2, w // 2, cop), G.SENTINEL, dtype=tdt, device="cuda")
    ss, mi = torch.full((2, cop), G.SENTINEL, device="cuda"), torch.full((2, cop), G.SENTINEL, device="cuda")
    nb = L.query("hyb_convstage_fwd_workspace", code, 1, 0, cop)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    rmean, rvar = c["mean"].float().cuda(), (1.0 / (c["invstd"] * c["invstd"])).float().cuda()
    L.call("hyb_convstage_fwd", code, 1, x, c["w"].float().cuda().contiguous(), c["gamma"].float().cuda(), c["beta"].float().cuda(), rmean, rvar, None, 0, 0.1, 0.0,
           n, h, w, ci, 0, co, cop, route, pooled, ss, mi, None, None, ws, nb, G.st())
    torch.cuda.synchronize()
    assert torch.equal(ss, G.padded_rows(c["scale"], c["shift"], cop)), "the forward's scale_shift is not the hand-made one"
    assert torch.equal(mi, G.padded_rows(c["mean"], c["invstd"], cop))
    assert torch.equal(G.to_nchw(pooled, code, co), c["pooled"])
    return route


@pytest.mark.parametrize("mode", ["fp32", "bf16", "bf16x3"])
@pytest.mark.parametrize("shape", R.FIRST_SHAPES, ids=["%dto%d_%dx%dx%d" % s for s in R.FIRST_SHAPES])
def test_first_stage_eval_backward_equals_the_reference(shape, mode):
    c = R.make_case(*shape, first=True)
    r = R.reference(c, False, with_bounds=False)
    got = _run_first(c, mode)
    for k in ("dW", "dgamma", "dbeta"):
        assert torch.equal(got[k], r[k]), (k, (got[k] != r[k]).nonzero()[:6].tolist())
    route = _first_forward_codes(c, mode)
    if route is not None:
        assert route.view(torch.int16).any(), "the forward wrote its routing codes"
        with_codes = _run_first(c, mode, route=route)
        for k in ("dW", "dgamma", "dbeta"):
            assert torch.equal(with_codes[k], got[k]), k


def test_first_stage_shapes_keep_routing_codes_where_expected():
    q = lambda mode, s: G.L().query("hyb_convstage_route_elems", G.DT[mode][0], s[2], s[3], s[4], R.pad32(s[1]))
    assert [q("bf16", s) > 0 for s in R.FIRST_SHAPES] == [True, True, True, True, False, True]          # 16 x 20: ragged blocks, no codes
    assert not any(q("fp32", s) for s in R.FIRST_SHAPES)


@pytest.mark.parametrize("mode", ["fp32", "bf16", "bf16x3"])
def test_first_stage_eval_backward_on_frames_that_are_not_16_byte_aligned(mode):
    shape = R.FIRST_SHAPES[0]
    c = R.make_case(*shape, first=True)
    r = R.reference(c, False, with_bounds=False)
    got = _run_first(c, mode, offset=True)
    for k in ("dW", "dgamma", "dbeta"):
        assert torch.equal(got[k], r[k]), (k, (got[k] != r[k]).nonzero()[:6].tolist())
