"""bench.py --dump-outputs DIR: what the last timed step left for the caller, as DIR/<name>.npy -- whole when the arrays fit the
64 MB the flag promises, a fixed seeded choice of rows otherwise; the same files from every run of the same command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, env=None, timeout=280):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    return json.loads(lines[0])


def _load(path):
    out = {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}
    assert all(f.endswith(".npy") for f in os.listdir(path))
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    return out


def test_arrays_under_the_cap_are_written_whole(tmp_path):
    import torch

    import bench
    arrays = {"wide": torch.arange(24.0).reshape(2, 3, 4), "narrow": torch.arange(6.0).reshape(2, 3, 1)}
    rec = bench.dump_outputs(torch, str(tmp_path / "d"), arrays)
    got = _load(str(tmp_path / "d"))
    assert sorted(got) == ["narrow", "wide"]
    for name, t in arrays.items():
        assert got[name].dtype == np.float32 and np.array_equal(got[name], t.numpy())
        assert rec[name] == {"shape": list(t.shape), "rows_of": 6}


def test_arrays_over_the_cap_keep_the_same_seeded_rows(tmp_path, monkeypatch):
    import torch

    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", 4000)
    arrays = {"wide": torch.arange(8000.0).reshape(10, 100, 8), "narrow": torch.arange(2000.0).reshape(10, 100, 2)}  # 32 000 + 8 000 bytes
    bench.dump_outputs(torch, str(tmp_path / "a"), arrays)
    got = _load(str(tmp_path / "a"))
    assert 2000 < got["wide"].nbytes + got["narrow"].nbytes <= 4000
    # every kept row is a row of the source; the rows ascend and are the same ones in both arrays (a frame's mel and MFCC rows)
    rows = (got["wide"][:, 0] / 8).astype(int)
    assert np.all(np.diff(rows) > 0) and 0 < len(rows) < 1000 and rows[-1] - rows[0] > 500
    assert np.array_equal(got["wide"], arrays["wide"].reshape(1000, 8).numpy()[rows])
    assert np.array_equal(got["narrow"], arrays["narrow"].reshape(1000, 2).numpy()[rows])
    bench.dump_outputs(torch, str(tmp_path / "b"), arrays)
    again = _load(str(tmp_path / "b"))
    assert all(np.array_equal(got[k], again[k]) for k in got)


@pytest.mark.timeout(300)
def test_dump_is_the_last_of_exactly_k_timed_steps(tmp_path):
    """the CPU stand-in of the kernels (AFX_BENCH_DRYRUN=1) stamps every clip's features with clip id x 1000 + step: the dump carries
    step K - 1 of --steps K (warm-up steps count from 0 again), two runs of one command line write the same files"""
    env = dict(os.environ, AFX_BENCH_DRYRUN="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    dumps = {}
    for tag, steps in (("a", 3), ("b", 3), ("c", 5)):
        d = _bench(["--gpus", "1", "--steps", str(steps), "--warmup", "2", "--dump-outputs", str(tmp_path / tag)], env)
        assert d["steps"] == steps and d["dumped_outputs"]["of_step"] == steps - 1
        dumps[tag] = _load(str(tmp_path / tag))
        assert {k: list(v.shape) for k, v in dumps[tag].items()} == {k: v["shape"] for k, v in d["dumped_outputs"]["arrays"].items()}
        clip = np.arange(d["config"]["clips_per_gpu"], dtype=np.float32)[:, None, None]
        assert np.array_equal(dumps[tag]["small"], np.broadcast_to(clip * 1000 + (steps - 1), dumps[tag]["small"].shape))
        assert np.array_equal(dumps[tag]["wide"], np.broadcast_to(clip, dumps[tag]["wide"].shape))
    assert all(np.array_equal(dumps["a"][k], dumps["b"][k]) for k in dumps["a"])
    # without the flag nothing is written and the line says nothing about a dump
    d = _bench(["--gpus", "1", "--steps", "2", "--warmup", "1"], env)
    assert "dumped_outputs" not in d and sorted(os.listdir(tmp_path)) == ["a", "b", "c"]


def test_zero_timed_steps_are_refused():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "0"], cwd=ROOT,
                         env=dict(os.environ, AFX_BENCH_DRYRUN="1"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert res.returncode != 0 and "--steps" in res.stderr and not res.stdout.strip()


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_dump_equals_what_a_caller_of_the_timed_call_receives(tmp_path):
    """bench.py --config 2 at 6 clips (3.2 MB of results: written whole) against the same call on the same seeded clips, made here:
    bitwise, mel and MFCC; and a second run of the command line writes the same bits"""
    import torch

    import audioflux_amd as af
    args = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--clips", "6", "--clock-warmup", "0", "--no-sustained", "--no-secondary",
            "--no-legacy", "--no-cpu-baseline"]
    d = _bench(args + ["--dump-outputs", str(tmp_path / "a")])
    got = _load(str(tmp_path / "a"))
    assert d["steps"] == 3 and d["dumped_outputs"]["of_step"] == 2 and sorted(got) == ["mel", "mfcc"]
    gen = torch.Generator(device="cuda:0").manual_seed(1)  # rank 0's clips of Cfg2
    x = 0.1 * torch.randn((6, 16000 * 30), generator=gen, device="cuda:0", dtype=torch.float32)
    bft = af.BFT(128, radix2_exp=11, samplate=16000, low_fre=0.0, high_fre=8000.0, slide_length=512,
                 scale_type=af.SpectralFilterBankScaleType.MEL, data_type=af.SpectralDataType.POWER)
    bft.set_result_type(1)
    mel, cc = af.mel_mfcc_device(bft, af.XXCC(128), x, 13)
    torch.cuda.synchronize()
    assert got["mel"].shape == tuple(mel.shape) and got["mfcc"].shape == tuple(cc.shape) == (6, d["config"]["units_per_step_per_gpu"] // 6, 13)
    assert np.array_equal(got["mel"], mel.cpu().numpy()) and np.array_equal(got["mfcc"], cc.cpu().numpy())
    assert np.abs(got["mel"]).max() > 0 and np.all(np.isfinite(got["mel"])) and np.all(np.isfinite(got["mfcc"]))
    _bench(args + ["--dump-outputs", str(tmp_path / "b")])
    again = _load(str(tmp_path / "b"))
    assert all(np.array_equal(got[k], again[k]) for k in got)
