"""bench.py --full: a plain run sets up, warms up, times its steps, writes --dump-outputs and prints the line; every other leg (the
sustained loop under the clock probe, the oracle check, the CPU baseline, the secondary configurations, the dense bank, the reference's
published benchmark) runs with --full alone, where the --no-* switches still take single legs out."""
import os

import pytest

from tests.test_bench_dump import _bench

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus")
EXTRA = ("cpu_baseline", "secondary", "dense_bank", "legacy")


def _dry_env():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["AFX_BENCH_DRYRUN"] = "1"
    return env


def test_no_leg_runs_without_full():
    import bench
    assert set(bench.LEGS) == {"sustained", "check", "cpu_baseline", "secondary", "legacy"}
    a = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert a.full is False and a.legs == dict.fromkeys(bench.LEGS, False)
    # the switches of single legs mean nothing on their own
    a = bench.parse_args(["--no-check", "--no-legacy"])
    assert a.legs == dict.fromkeys(bench.LEGS, False)


def test_full_runs_every_leg_but_those_switched_off():
    import bench
    a = bench.parse_args(["--full"])
    assert a.full is True and a.legs == dict.fromkeys(bench.LEGS, True)
    for leg in bench.LEGS:
        a = bench.parse_args(["--full", "--no-" + leg.replace("_", "-")])
        assert a.legs == {k: k != leg for k in bench.LEGS}
    # what the timed steps are does not depend on it
    plain, full = bench.parse_args(["--steps", "7", "--warmup", "2"]), bench.parse_args(["--steps", "7", "--warmup", "2", "--full"])
    for k in ("gpus", "steps", "warmup", "config", "clips", "total_clips", "clock_warmup", "dump_outputs"):
        assert getattr(plain, k) == getattr(full, k)


def test_plain_measure_ends_with_the_timed_steps():
    """measure() with no sustained loop and no clock probe calls the workload's step W + K times, all before it returns the K steps' time"""
    import torch

    import bench

    class Counted(bench.DryRun):
        calls = 0

        def step(self, i):
            Counted.calls += 1
            super().step(i)

    w = Counted(torch, None, torch.device("cpu"), 0, 4)
    m = bench.measure(w, torch, None, torch.device("cpu"), 1, 5, 2, 0.5, 0.0, dry=True, clock_probe=False)
    assert Counted.calls == 7 and m["last"] == 4 and m["sustained_ms"] is None and m["clock"] is None and m["elapsed"] > 0


@pytest.mark.timeout(300)
def test_dry_line_says_which_run_it_was():
    plain = _bench(["--gpus", "1", "--steps", "3", "--warmup", "1"], _dry_env())
    full = _bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--full"], _dry_env())
    assert plain["full"] is False and full["full"] is True
    for d in (plain, full):
        assert all(k in d for k in HEADLINE) and d["value"] > 0 and d["ms_per_step"] > 0 and d["higher_is_better"] is True
        assert d["steps"] == 3 and d["warmup"] == 1
        assert d["config"]["units_per_step_per_gpu"] * 3 / (d["ms_per_step"] * 3e-3) == pytest.approx(d["value"], rel=1e-6)
    assert not any(k in plain for k in EXTRA) and plain["oracle_check"]["clip0_max_rel_err"] is None
    assert "cpu_baseline" in full  # (the stand-in has no reference to time: the leg ran and found none)
    assert {k: plain[k] for k in ("metric", "unit", "dtype", "higher_is_better")} == {k: full[k] for k in ("metric", "unit", "dtype", "higher_is_better")}


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_plain_run_measures_the_headline_alone_and_full_adds_its_legs(tmp_path):
    """--config 2 at 6 clips: the plain line carries the headline figure, the timed steps' own roofline figures and no other leg; --full
    (its minutes-long legs switched off) adds the sustained loop, the clock probe and the oracle check, and both dump the same bits"""
    import numpy as np
    args = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--clips", "6"]
    plain = _bench(args + ["--dump-outputs", str(tmp_path / "plain")])
    assert plain["full"] is False and all(k in plain for k in HEADLINE) and not any(k in plain for k in EXTRA)
    r = plain["roofline"]
    assert plain["value"] > 0 and r["kernel_ms"] > 0 and r["frac"] > 0
    assert r["sustained_ms"] is None and r["clock_probe"] is None and plain["oracle_check"]["clip0_max_rel_err"] is None
    assert plain["config"]["device"]["compute_units"] > 0 and "power_cap_w" not in plain["config"]["device"]
    full = _bench(args + ["--full", "--no-secondary", "--no-legacy", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "full")])
    assert full["full"] is True and not any(k in full for k in EXTRA)
    r = full["roofline"]
    assert r["sustained_ms"] > 0 and r["sustained_value"] > 0
    from oracle import ref
    err = full["oracle_check"]["clip0_max_rel_err"]  # (no compiled reference: the check has nothing to compare with and says so)
    assert (err is not None and err <= 1e-5) if ref.available() else err is None
    for k in ("metric", "unit", "dtype", "higher_is_better", "steps", "warmup"):
        assert plain[k] == full[k]
    assert plain["dumped_outputs"]["arrays"] == full["dumped_outputs"]["arrays"]
    for name in ("mel", "mfcc"):
        assert np.array_equal(np.load(tmp_path / "plain" / (name + ".npy")), np.load(tmp_path / "full" / (name + ".npy")))
