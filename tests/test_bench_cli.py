"""bench.py's command line without a GPU: a plain run measures the headline only, --full restores every other measurement,
and --dump-outputs stays within its size bound with the same sample in every run."""
import numpy as np
import torch

import bench


def test_plain_run_turns_off_everything_beside_the_headline():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert not a.full and a.steps == 7 and a.warmup == 2 and a.dump_outputs is None
    assert a.no_cpu_baseline and a.no_roofline and a.no_fwd_bwd_only and a.no_pipeline and a.no_live_traffic and a.no_extra_legs


def test_full_run_keeps_every_leg_unless_trimmed():
    a = bench.parse(["--full"])
    assert a.full and not (a.no_cpu_baseline or a.no_roofline or a.no_fwd_bwd_only or a.no_pipeline or a.no_live_traffic or a.no_extra_legs)
    a = bench.parse(["--full", "--no-cpu-baseline", "--dump-outputs", "out"])
    assert a.no_cpu_baseline and not a.no_roofline and a.dump_outputs == "out"


def test_dump_outputs_writes_float32_whole_when_small(tmp_path):
    bench._import_torch()
    g = torch.Generator().manual_seed(3)
    arrays = {"loss": torch.tensor(1.25, dtype=torch.float64), "w": torch.randn(64, 32, generator=g)}
    d = bench.dump_outputs(str(tmp_path), arrays)
    assert d["arrays"] == 2 and not d["sampled"]
    loss, w = np.load(tmp_path / "loss.npy"), np.load(tmp_path / "w.npy")
    assert loss.dtype == np.float32 and loss.shape == () and loss == np.float32(1.25)
    assert w.dtype == np.float32 and np.array_equal(w, arrays["w"].numpy())


def test_dump_outputs_samples_large_arrays_the_same_way_every_time(tmp_path):
    bench._import_torch()
    big = torch.arange(20_000_000, dtype=torch.float32)
    arrays = {"big": big, "small": torch.ones(10)}
    d1 = bench.dump_outputs(str(tmp_path / "a"), arrays)
    d2 = bench.dump_outputs(str(tmp_path / "b"), arrays)
    assert d1["sampled"] and d1["bytes"] <= bench.DUMP_LIMIT_BYTES and d1["bytes"] == d2["bytes"]
    total = sum(f.stat().st_size for f in (tmp_path / "a").iterdir())
    assert total <= 64 * 1000 * 1000
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert np.array_equal(a, b) and np.all(np.diff(a) >= 0)             # the same positions, in index order
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), np.ones(10, np.float32))
