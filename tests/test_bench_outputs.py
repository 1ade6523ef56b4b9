"""`bench.py --dump-outputs DIR`: what the timed path computed in its last step, as DIR/<name>.npy within 64 MB; and a plain run
(no --full) that carries the headline fields and nothing of the secondary measurements."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import bench


def _sizes(d):
    return {f: os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_keeps_arrays_whole_within_the_budget(tmp_path):
    arrays = {"a": np.arange(1000, dtype=np.float32), "b": np.linspace(0, 1, 77, dtype=np.float64).reshape(7, 11)}
    bench.dump_outputs(str(tmp_path), arrays)
    for k, v in arrays.items():
        got = np.load(tmp_path / (k + ".npy"))
        assert got.dtype == v.dtype and got.shape == v.shape and np.array_equal(got, v)


def test_dump_samples_the_large_arrays_the_same_way_every_time(tmp_path):
    rng = np.random.default_rng(3)
    arrays = {"big": rng.standard_normal(200_000).astype(np.float32), "mid": rng.standard_normal((300, 200)),
              "small": np.arange(10, dtype=np.float64)}
    budget = 400_000
    d1, d2 = tmp_path / "one", tmp_path / "two"
    bench.dump_outputs(str(d1), arrays, budget=budget)
    bench.dump_outputs(str(d2), arrays, budget=budget)
    assert sum(_sizes(str(d1)).values()) <= budget
    for k, v in arrays.items():
        a, b = np.load(d1 / (k + ".npy")), np.load(d2 / (k + ".npy"))
        assert a.dtype == v.dtype and np.array_equal(a, b)
        assert np.isin(a, v.ravel()).all()  # a sample of the array's own entries
    assert np.array_equal(np.load(d1 / "small.npy"), arrays["small"])
    assert np.load(d1 / "big.npy").size < arrays["big"].size


def _run_bench(args, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
@pytest.mark.timeout(600)
@pytest.mark.parametrize("workload,dtype", [("journal-1pct", np.float32), ("er-5pct-2k", np.float64)])
def test_plain_run_and_its_outputs(tmp_path, workload, dtype):
    out = tmp_path / "out"
    d = _run_bench(["--gpus", "1", "--workload", workload, "--steps", "6", "--warmup", "2", "--dump-outputs", str(out)])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup"):
        assert k in d, k
    assert d["steps"] == 6 and d["warmup"] == 2 and d["timed_regions"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0
    for k in ("roofline", "device_us_per_step", "coloring", "cpu_baseline", "fp32_operands"):
        assert k not in d, k
    c = d["config"]
    expect = {"x_avg": c["nnzL"], "x": c["nnzL"], "y_avg": c["C"], "y": c["C"], "x_half": c["K"] * c["D"], "e_max": 1}
    assert sorted(_sizes(str(out))) == sorted(k + ".npy" for k in expect)
    assert sum(_sizes(str(out)).values()) <= bench.DUMP_BYTES
    for k, n in expect.items():
        a = np.load(out / (k + ".npy"))
        assert a.dtype == dtype and a.size == n and np.isfinite(a).all(), k
    e = float(np.load(out / "e_max.npy")[0])
    assert abs(e - d["objectives"]["max_violation_per_instance"][0]) <= 1e-6 + 1e-6 * abs(e)
