"""The GPU side of tests/test_gpu_stage1_runs.py: the first conv stage through the C ABI (hyb_convstage_fwd / hyb_convstage_bwd, first = 1) on the
rows of tests/stage1_run_shapes.py, compared with tests/stage1_ref.py.  Importing it starts nothing.

As a child process (the HYB_S1_*_WGS switches are read once per process, so every environment of the table is a run of this script under it):
  python tests/stage1_run_worker.py runs ENV OUT.json     no GPU: hyb_stage1_run of every row of ENV, {row id: {mode: [training 4, eval 4]}}
  python tests/stage1_run_worker.py check ENV OUT.json [MODE ...]   the eval and training assertions on every row of ENV in the modes named (all three):
                                                          {row id: {mode: {"runs": ..., "eval": {...}, "train": {...}}}}, fails lists inside"""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import stage1_run_shapes as S                                                           # noqa: E402

CODE = {"fp32": 0, "bf16": 1, "bf16x3": 2}


def L():
    from transformer_cnn_hybrid_network_for_video_processing_amd._lib import lib
    return lib


def pad32(c):
    return (c + 31) // 32 * 32


def query_runs(mode, shape):
    """-> [training: 4 passes, eval: 4 passes] of hyb_stage1_run"""
    ci, co, n, h, w = shape
    return [[L().query("hyb_stage1_run", CODE[mode], p, t, n, h, w, ci, pad32(co)) for p in range(4)] for t in (1, 0)]


# ---- everything below needs torch and a GPU ---------------------------------------------------------------------------------------------------------
def _mods():
    import torch
    import convstage_bwd_worker as G
    import stage1_ref as X
    return torch, G, X


def _ff(t):
    """a device buffer filled with 0xFF bytes (bf16 / fp32: NaNs)"""
    t.view(-1).view(_mods()[0].uint8).fill_(255)
    return t


def forward(d, mode, training, keep_pack=True):
    """hyb_convstage_fwd(first = 1).  d: dict with shape, x, w, gamma, beta, mean, invstd (fp64 CPU; eval mode runs on the hand-made mean / invstd
    with eps = 0, training mode starts the running statistics from them).  Outputs are filled with the sentinel, the workspace, the saved pack
    and the code buffer with 0xFF bytes.  -> dict of device tensors and CPU copies."""
    torch, G, X = _mods()
    code, tdt, _ = G.DT[mode]
    ci, co, n, h, w = d["shape"]
    cop = pad32(co)
    lib = L()
    elems = lib.query("hyb_convstage_route_elems", code, n, h, w, cop)
    route = _ff(torch.empty(elems, dtype=tdt, device="cuda")) if elems > 0 else None
    x = d["x"].float().cuda().contiguous()
    pooled = torch.full((n, h // 2, w // 2, cop), X.SENTINEL, dtype=tdt, device="cuda")
    ss, mi = torch.full((2, cop), X.SENTINEL, device="cuda"), torch.full((2, cop), X.SENTINEL, device="cuda")
    nb = lib.query("hyb_convstage_fwd_workspace", code, 1, 0, cop)
    ws = _ff(torch.empty(nb, dtype=torch.uint8, device="cuda"))
    pack = _ff(torch.empty(lib.query("hyb_convstage_packed_bwd_elems", 1, 0, cop), dtype=tdt, device="cuda")) if keep_pack else None
    rmean, rvar = d["mean"].float().cuda(), (1.0 / (d["invstd"] * d["invstd"])).float().cuda()
    nbt = torch.zeros(1, dtype=torch.int64, device="cuda")
    lib.call("hyb_convstage_fwd", code, 1, x, d["w"].float().cuda().contiguous(), d["gamma"].float().cuda(), d["beta"].float().cuda(), rmean, rvar, nbt,
             int(training), X.MOMENTUM, X.EPS if training else 0.0, n, h, w, ci, 0, co, cop, route, pooled, ss, mi, pack, None, ws, nb, G.st())
    torch.cuda.synchronize()
    out = dict(x=x, route=route, pack=pack, ss=ss, mi=mi, pooled_dev=pooled, pooled=G.to_nchw(pooled, code, co), pad_zero=bool((pooled[..., co:] == 0).all()),
               run_mean=rmean.cpu().double(), run_var=rvar.cpu().double(), nbt=int(nbt.item()), codes=None)
    if route is not None:
        out["codes"] = X.words_to_codes(route.view(torch.int32).cpu(), n, co, h // 2, w // 2, cop)
        out["codes_pad_zero"] = bool((X.words_to_codes(route.view(torch.int32).cpu(), n, cop, h // 2, w // 2, cop)[:, co:] == 0).all())
    return out


def backward(d, mode, training, fw, use_route, use_pack):
    """hyb_convstage_bwd(first = 1) on the forward's scale_shift / mean_invstd (and, when asked, its codes and saved pack) -> fp64 CPU dW, dgamma, dbeta"""
    torch, G, X = _mods()
    code, tdt, _ = G.DT[mode]
    ci, co, n, h, w = d["shape"]
    cop = pad32(co)
    lib = L()
    dp = G.to_nhwc(d["dp"], code, tdt, cop)
    dw = torch.full((co, ci, 3, 3), X.SENTINEL, device="cuda")
    dgamma, dbeta = torch.full((co,), X.SENTINEL, device="cuda"), torch.full((co,), X.SENTINEL, device="cuda")
    nb = lib.query("hyb_convstage_bwd_workspace", code, 1, n, h, w, 0, cop)
    ws = _ff(torch.empty(nb, dtype=torch.uint8, device="cuda"))
    lib.call("hyb_convstage_bwd", code, 1, dp, fw["x"], fw["route"] if use_route else None, None, d["w"].float().cuda().contiguous(), d["gamma"].float().cuda(),
             fw["ss"], fw["mi"], int(training), n, h, w, ci, 0, co, cop, None, dw, dgamma, dbeta, fw["pack"] if use_pack else None, ws, nb, G.st())
    torch.cuda.synchronize()
    return dict(dW=dw.cpu().double(), dgamma=dgamma.cpu().double(), dbeta=dbeta.cpu().double())


def _same_bits(a, b, keys):
    torch = _mods()[0]
    bad = []
    for k in keys:
        if a[k] is None and b[k] is None:
            continue
        x, y = a[k], b[k]
        if x.is_floating_point():       # bits, not values: NaNs of an unwritten buffer must compare too
            x, y = x.contiguous().view(-1).view(torch.uint8), y.contiguous().view(-1).view(torch.uint8)
        if not torch.equal(x, y):
            bad.append(k)
    return bad


def _backwards(d, mode, training, fw):
    """every form of the backward, each twice: with / without the codes, with / without the saved pack.  -> (first result, failures)"""
    fails, first = [], None
    for use_route in ((True, False) if fw["route"] is not None else (False,)):
        for use_pack in (True, False):
            a = backward(d, mode, training, fw, use_route, use_pack)
            b = backward(d, mode, training, fw, use_route, use_pack)
            if _same_bits(a, b, ("dW", "dgamma", "dbeta")):
                fails.append(f"backward (codes {use_route}, pack {use_pack}) gives other bits the second time")
            if first is None:
                first = a
            elif _same_bits(first, a, ("dW", "dgamma", "dbeta")):
                fails.append(f"backward (codes {use_route}, pack {use_pack}) differs from the first form in {_same_bits(first, a, ('dW', 'dgamma', 'dbeta'))}")
    return first, fails


def check_eval(shape, mode, forward_only=False):
    """-> (fails, info)"""
    torch, G, X = _mods()
    t0 = time.time()
    ev = X.eval_reference(shape, forward_only)
    co = shape[1]
    cop = pad32(co)
    fw = forward(ev, mode, False)
    fw2 = forward(ev, mode, False)
    fails = X.compare_eval_forward(ev, fw)
    if _same_bits(fw, fw2, ("pooled_dev", "ss", "mi", "route", "pack")):
        fails.append("the forward gives other bits the second time: " + ", ".join(_same_bits(fw, fw2, ("pooled_dev", "ss", "mi", "route", "pack"))))
    if not torch.equal(fw["ss"], G.padded_rows(ev["scale"], ev["shift"], cop)) or not torch.equal(fw["mi"], G.padded_rows(ev["mean"], ev["invstd"], cop)):
        fails.append("scale_shift / mean_invstd are not the hand-made rows")
    if fw["codes"] is not None and not fw["codes_pad_zero"]:
        fails.append("codes of padded channels are not zero")
    info = dict(codes=fw["codes"] is not None)
    if not forward_only:
        c = X.case(shape)
        first, bf = _backwards(c, mode, False, fw)
        fails += bf
        r = X.eval_backward(c)
        for k in ("dW", "dgamma", "dbeta"):
            fails += X.compare_exact(k, first[k], r[k])
    info["seconds"] = round(time.time() - t0, 2)
    return fails, info




def check_train(shape, mode, forward_only=False, rows=1024):
    """-> (fails, info).  forward_only (the 181-image row): the reference is formed in slices of images and the backward is left out."""
    torch, G, X = _mods()
    t0 = time.time()
    c = X.sliced_case(shape) if forward_only else X.case(shape)
    n, co = shape[2], shape[1]
    cop = pad32(co)
    runs = query_runs(mode, shape)[0]
    path = "gram" if runs[2] > 0 else "stats"
    s = X.train_stats(c)
    fw = forward(c, mode, True)
    fw2 = forward(c, mode, True)
    fails = []
    if _same_bits(fw, fw2, ("pooled_dev", "ss", "mi", "route", "pack", "run_mean", "run_var")):
        fails.append("the forward gives other bits the second time: " + ", ".join(_same_bits(fw, fw2, ("pooled_dev", "ss", "mi", "route", "pack", "run_mean", "run_var"))))
    ss, mi = fw["ss"].cpu().double(), fw["mi"].cpu().double()
    got = dict(mean=mi[0, :co], invstd=mi[1, :co], scale=ss[0, :co], shift=ss[1, :co], run_mean=fw["run_mean"], run_var=fw["run_var"], nbt=fw["nbt"],
               pad_zero=bool((ss[:, co:] == 0).all() and (mi[:, co:] == 0).all()))
    sf, ratios = X.compare_stats(s, c, got, path, rows)
    fails += sf
    storage = "bf16" if mode == "bf16" else "fp32"
    step = 16 if forward_only else n
    ratios["pooled"], unsafe, windows = 0.0, 0, 0
    for i in range(0, n, step):
        cs = dict(y=torch.nn.functional.conv2d(c["x"][i:i + step], c["w"], padding=1)) if forward_only else c
        f = X.train_forward(cs, got["scale"], got["shift"])
        pf, rp = X.compare_train_pooled(f, fw["pooled"][i:i + step], storage)
        fails += [f"images {i}..: " + m for m in pf]
        ratios["pooled"] = max(ratios["pooled"], rp)
        unsafe, windows = unsafe + int((~f["safe"]).sum()), windows + f["safe"].numel()
        if fw["codes"] is not None:
            fails += [f"images {i}..: " + m for m in X.compare_train_codes(f, fw["codes"][i:i + step])]
    if not fw["pad_zero"]:
        fails.append("padded channels of pooled are not exact zeros")
    if fw["codes"] is not None and not fw["codes_pad_zero"]:
        fails.append("codes of padded channels are not zero")
    if not forward_only:
        first, bf = _backwards(c, mode, True, fw)
        fails += bf
        r = X.train_backward(c, f, got["mean"], got["invstd"])
        cf, br = X.compare_backward(r, first)
        fails += cf
        ratios.update(br)
    info = dict(path=path, codes=fw["codes"] is not None, ratios={k: float("%.3g" % v) for k, v in ratios.items()}, unsafe=unsafe / windows,
                seconds=round(time.time() - t0, 2))
    return fails, info


def check_row(row, modes=S.MODES):
    env, shape, forward_only, _ = row
    out = {}
    for mode in modes:
        res = dict(runs=query_runs(mode, shape))
        fails, info = check_eval(shape, mode, forward_only)
        res["eval"] = dict(fails=fails, **info)
        fails, info = check_train(shape, mode, forward_only)
        res["train"] = dict(fails=fails, **info)
        out[mode] = res
        print(env, shape, mode, json.dumps(res), flush=True)
    return out


if __name__ == "__main__":
    what, env, path = sys.argv[1:4]
    modes = tuple(sys.argv[4:]) or S.MODES
    for k, v in S.ENVS[env].items():
        assert os.environ.get(k) == v, f"{k} is not {v}: start this script under the environment of tests/stage1_run_shapes.py ENVS[{env!r}]"
    res = {}
    for row, rid in zip(S.TABLE, S.ROW_IDS):
        if row[0] != env:
            continue
        res[rid] = {m: query_runs(m, row[1]) for m in S.MODES} if what == "runs" else check_row(row, modes)
    with open(path, "w") as fh:
        json.dump(res, fh)
