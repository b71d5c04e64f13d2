"""The first conv stage where a WAVE walks a run of blocks (csrc/conv_first_wave.hip, csrc/conv_first.hip): the halo double buffer, the single
image of the Gram pass and the backward, the prefetched frame rows, dpooled and routing codes, the block coordinates across row and image ends,
idle waves and idle workgroups' zero partial rows -- on the rows of tests/stage1_run_shapes.py (tests/test_stage1_run_cpu.py asserts that the
rows reach each of these), through hyb_convstage_fwd / hyb_convstage_bwd with first = 1, compared with tests/stage1_ref.py.

Before every call the outputs hold a sentinel and the workspace, the saved pack and the code buffer 0xFF bytes; every call runs twice and must
give the same bits.
  eval mode      pooled, scale_shift, mean_invstd, every routing-code word, dweight, dgamma, dbeta EQUAL the reference; padded channels are
                 zeros; the backward gives the same bits with and without the codes, with and without the saved pack
  training mode  the bounds of tests/stage1_ref.py's docstring, every one derived from the fp64 reference; the backward with the forward's saved
                 Gram matrix, without it, with the codes and recomputing must agree bit for bit
The small rows run in child processes under shrunk grids (the switches are read once per process): the workload's own run lengths -- 7 blocks in
the apply pass, 25 in the Gram pass and the backward -- and one workgroup per pass; hyb_stage1_run, asked inside the child, must say what the
table says.  Measured ratios: profiles/stage1_runs_exact.txt."""
import json
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stage1_run_shapes as S          # noqa: E402
import stage1_run_worker as Wk         # noqa: E402  (importing it starts nothing)
from convstage_bwd_ref import FIRST_SHAPES          # noqa: E402

DEFAULT = [(r[1], r[2]) for r in S.rows("default")] + [(s, False) for s in FIRST_SHAPES]      # ... and the one-block baseline
DEFAULT_IDS = ["%dto%d_%dx%dx%d" % s for s, _ in DEFAULT]


def _report(kind, shape, mode, info, t0):
    print(f"{kind} {mode} {shape}: runs {Wk.query_runs(mode, shape)} {json.dumps(info)} test {time.time() - t0:.2f} s")


def test_default_grids_walk_the_runs_the_table_says():
    for _, shape, _, want in S.rows("default"):
        for mode in S.MODES:
            training, ev = Wk.query_runs(mode, shape)
            assert tuple(training) == want[mode] and tuple(ev) == (0, want[mode][1], 0, want[mode][3]), (shape, mode, training, ev)


@pytest.mark.parametrize("mode", S.MODES)
@pytest.mark.parametrize("shape,forward_only", DEFAULT, ids=DEFAULT_IDS)
def test_eval_mode_equals_the_reference(shape, forward_only, mode):
    t0 = time.time()
    fails, info = Wk.check_eval(shape, mode, forward_only)
    _report("eval", shape, mode, info, t0)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("mode", S.MODES)
@pytest.mark.parametrize("shape,forward_only", DEFAULT, ids=DEFAULT_IDS)
def test_training_mode_within_the_reference_bounds(shape, forward_only, mode):
    t0 = time.time()
    fails, info = Wk.check_train(shape, mode, forward_only)
    _report("training", shape, mode, info, t0)
    assert not fails, "\n".join(fails)
    assert all(v < 1 for v in info["ratios"].values()) and info["unsafe"] <= 1e-3


@pytest.mark.parametrize("mode", S.MODES)
@pytest.mark.parametrize("env", ["workload", "single"])
def test_shrunk_grids_in_a_child_process(tmp_path, env, mode):
    """One fresh process per environment and mode: the small rows under the shrunk grids, the same eval and training assertions."""
    t0 = time.time()
    path = str(tmp_path / "out.json")
    e = {k: v for k, v in os.environ.items() if not k.startswith("HYB_S1_")}
    e.update(S.ENVS[env])
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "stage1_run_worker.py"), "check", env, path, mode], env=e, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-4000:]
    res = json.load(open(path))
    rows = S.rows(env)
    assert set(res) == {"%s_%dto%d_%dx%dx%d" % ((env,) + r[1]) for r in rows}
    for _, shape, _, want in rows:
        v = res["%s_%dto%d_%dx%dx%d" % ((env,) + shape)][mode]
        print(f"{env} {mode} {shape}: {json.dumps(v)}")
        training, ev = v["runs"]
        assert tuple(training) == want[mode] and tuple(ev) == (0, want[mode][1], 0, want[mode][3]), (shape, training, ev)
        assert not v["eval"]["fails"], "\n".join(v["eval"]["fails"])
        assert not v["train"]["fails"], "\n".join(v["train"]["fails"])
        assert all(x < 1 for x in v["train"]["ratios"].values()) and v["train"]["unsafe"] <= 1e-3
    print(f"{env} {mode}: child and checks {time.time() - t0:.2f} s")
