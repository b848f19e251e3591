"""bench.py --dump-outputs: what the last timed step computed, written for comparing two builds output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def test_dump_outputs_keeps_small_arrays_whole_and_samples_large_ones(tmp_path):
    import bench
    film = np.random.default_rng(1).random((700, 700, 4), dtype=np.float32)
    bench.dump_outputs(str(tmp_path / "small"), {"film": film})
    assert os.listdir(str(tmp_path / "small")) == ["film.npy"]
    got = np.load(str(tmp_path / "small" / "film.npy"))
    assert got.dtype == np.float32 and np.array_equal(got, film)
    big = np.random.default_rng(2).random((2400, 3000, 4), dtype=np.float32)      # 115 MB: over the budget
    for d in ("big0", "big1"):
        bench.dump_outputs(str(tmp_path / d), {"film": big})
    files = sorted(os.listdir(str(tmp_path / "big0")))
    assert files == ["film.npy", "film_index.npy"]
    assert sum(os.path.getsize(str(tmp_path / "big0" / f)) for f in files) <= bench.DUMP_BYTES
    idx = np.load(str(tmp_path / "big0" / "film_index.npy"))
    sample = np.load(str(tmp_path / "big0" / "film.npy"))
    assert idx.dtype == np.float64 and sample.dtype == np.float32 and len(idx) == len(sample) > 0
    assert np.all(np.diff(idx) > 0) and np.array_equal(sample, big.reshape(-1, 4)[idx.astype(np.int64)])
    for f in files:      # the sample is fixed: the same pixels every run
        assert np.array_equal(np.load(str(tmp_path / "big0" / f)), np.load(str(tmp_path / "big1" / f)))


@pytest.mark.gpu
def test_bench_dumps_the_film_of_its_last_timed_step(tmp_path, killeroo_oracle):
    """Two timed steps of a small frame: the line reports them, and film.npy is the film the oracle renders bit for bit."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "killeroo-simple", "--spp", "4", "--steps", "2",
           "--warmup", "1", "--no-secondary", "--no-cpu-baseline", "--no-trace-all", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 2 and line["ms_per_step"] > 0
    assert os.listdir(str(out)) == ["film.npy"]
    got = np.load(str(out / "film.npy"))
    assert got.dtype == np.float32 and got.shape == (700, 700, 4)
    killeroo_oracle.set_film(crop=(0, 1, 0, 1), spp=4)
    _, film0, _, _, _ = killeroo_oracle.render(spp=4, threads=16)
    killeroo_oracle.set_film(crop=(0, 1, 0, 1), spp=8)
    assert np.array_equal(got.view(np.uint32), film0.view(np.uint32))


def test_full_is_off_by_default(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1"])
    assert bench.parse_args().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--full", "--no-secondary"])
    a = bench.parse_args()
    assert a.full is True and a.no_secondary is True


@pytest.mark.gpu
def test_plain_bench_run_measures_the_headline_only():
    """Without --full the line carries the headline figures and none of the extras: no roofline, secondary workloads, CPU
    baseline, trace-all frames or reference ray count (that one comes from a counting render)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "killeroo-simple", "--spp", "4", "--steps", "1",
           "--warmup", "1"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["metric"] == "Mrays/s" and line["unit"] == "Mrays/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["steps"] == 1 and line["warmup"] == 1 and line["rays_per_step"] > 0
    assert line["full"] is False and line["secondary"] == []
    for k in ("roofline", "cpu_baseline", "with_every_reference_ray_traced", "reference_rays_per_step"):
        assert line[k] is None, k
