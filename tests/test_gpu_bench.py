"""bench.py keeps the driver's contract on the GPU: one JSON line with the metric / config of BASELINE.json, a
roofline object for the dominant kernel and (N = 1, --full) a cpu_baseline object; a plain run leaves the --full leg
out and --dump-outputs writes the last timed step's outputs, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *args],
                       capture_output=True, text=True, timeout=600, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_bench_json_line():
    d = _bench("--full", "--steps", "10", "--warmup", "3", "--time-every", "2", "--cpu-seconds", "1",
               "--cpu-envs", "16")
    base = json.load(open(os.path.join(REPO, "BASELINE.json")))
    assert d["metric"] == base["metric"] and d["unit"] == "env-steps/s" and d["higher_is_better"] is True
    assert d["n_gpus"] == 1 and d["steps"] == 10 and d["warmup"] == 3 and d["scaling"] == "weak"
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["config"]["num_envs_per_gpu"] == 8192
    rf = d["roofline"]
    # bound: the roofline the kernel sits closest to (bench.py derives it: HBM, or the dynamics waves' VALU issue);
    # achieved / peak / frac are the HBM roofline's in either case
    assert rf["bound"] in ("hbm", "valu_issue") and rf["unit"] == "GB/s" and rf["peak"] == 8000.0
    if rf["bound"] == "valu_issue":
        assert rf["issue"]["frac"] > rf["frac"]
    assert 0 < rf["frac"] < 1 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3
    assert rf["kernels"][rf["kernel"]]["timed_launches"] > 0
    cb = d["cpu_baseline"]
    assert cb["value"] > 0 and cb["cores"] >= 1 and cb["kind"] in ("port", "reference")


def test_bench_plain_run_dumps_outputs(tmp_path):
    """A plain run has no --full leg (cpu_baseline), --steps sets the timed steps, and --dump-outputs writes the last
    timed step's 5-tuple as float32 .npy files under 64 MB: at 8192 envs (obs alone 97 MiB) a sample of the envs."""
    out = str(tmp_path / "dump")
    d = _bench("--steps", "7", "--warmup", "2", "--dump-outputs", out)
    assert "cpu_baseline" not in d and d["steps"] == 7 and d["warmup"] == 2
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(8192 * 1e3 / d["ms_per_step"], rel=1e-3)
    a = _load(out)
    assert {"obs", "privileged_obs", "rew", "reset", "time_outs", "root_states", "extras_episode", "env_rows"} <= set(a)
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out)) <= 64e6
    rows = a["env_rows"]
    assert 0 < rows.size < 8192 and np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < 8192
    assert a["obs"].shape == (rows.size, 47 * 66) and a["privileged_obs"].shape == (rows.size, 73 * 3)
    assert a["rew"].shape == a["reset"].shape == (rows.size,) and a["root_states"].shape == (rows.size, 13)
    assert all(np.isfinite(a[k]).all() for k in ("obs", "privileged_obs", "rew", "root_states"))
    assert np.abs(a["obs"]).max() > 0 and set(np.unique(a["reset"])) <= {0.0, 1.0}


def test_bench_dump_repeats_run_to_run(tmp_path):
    """Same arguments, same inputs: two runs dump the same arrays (every env kept at this size)."""
    runs = []
    for name in ("a", "b"):
        out = str(tmp_path / name)
        _bench("--steps", "9", "--warmup", "2", "--num-envs", "500", "--mesh", "plane", "--dump-outputs", out)
        runs.append(_load(out))
    a, b = runs
    assert set(a) == set(b) and a["obs"].shape == (500, 47 * 66) and a["env_rows"].tolist() == list(range(500))
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
