"""bench.py's plain run, --full and --dump-outputs: what a plain run prints, what moved behind --full, and the arrays
written after the timed steps (float32 / float64 .npy files, a fixed sample of the envs for the images, size-capped)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = {"roofline", "fresh_outputs", "cpu_baseline", "cpu_baseline_all_cores"}


def _bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench

    return bench


def test_full_and_dump_are_opt_in():
    b = _bench()
    a = b.parse_args([])
    assert a.full is False and a.dump_outputs is None
    a = b.parse_args(["--full", "--dump-outputs", "out", "--steps", "7"])
    assert a.full is True and a.dump_outputs == "out" and a.steps == 7
    with pytest.raises(SystemExit):
        b.parse_args(["--steps", "0"])


def test_dump_writes_float_arrays_and_samples_images(tmp_path):
    b = _bench()
    n, s = 100, 48
    g = torch.Generator().manual_seed(0)
    arrays = {"obs": torch.rand(n, 4, s, s, generator=g), "full_state": torch.rand(n, s, s, 4, generator=g),
              "rewards": torch.rand(n, generator=g), "dones": torch.rand(n, generator=g) > 0.5,
              "position": torch.rand(n, 3, generator=g, dtype=torch.float64), "actions": np.arange(2 * n).reshape(n, 2)}
    budget = 4 << 20  # 72 KB of images per env: room for ~56 of the 100 envs
    shapes = b.dump_outputs(str(tmp_path / "a"), arrays, budget=budget)
    files = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert set(files) == set(arrays) | {"env_index"}
    assert {k: v.shape for k, v in files.items()} == shapes
    assert all(v.dtype in (np.float32, np.float64) for v in files.values())
    assert files["position"].dtype == np.float64 and files["dones"].dtype == np.float32
    idx = files["env_index"].astype(np.int64)
    assert 1 <= len(idx) < n and np.all(np.diff(idx) > 0) and idx[-1] < n
    assert sum(v.nbytes for v in files.values()) <= budget
    assert np.array_equal(files["obs"], arrays["obs"].numpy()[idx])
    assert np.array_equal(files["full_state"], arrays["full_state"].numpy()[idx])
    assert np.array_equal(files["rewards"], arrays["rewards"].numpy())  # small per env: written whole
    assert np.array_equal(files["dones"], arrays["dones"].numpy().astype(np.float32))
    assert np.array_equal(files["actions"], np.arange(2 * n, dtype=np.float32).reshape(n, 2))
    b.dump_outputs(str(tmp_path / "b"), arrays, budget=budget)  # the same sample every time
    assert np.array_equal(np.load(tmp_path / "b" / "env_index.npy"), files["env_index"])
    shapes = b.dump_outputs(str(tmp_path / "c"), arrays)  # the default budget holds everything
    assert shapes["obs"] == (n, 4, s, s) and shapes["env_index"] == (n,)
    with pytest.raises(ValueError):
        b.dump_outputs(str(tmp_path / "d"), {"a": np.zeros(3), "b": np.zeros(4)})


def _run_bench(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([line for line in r.stdout.splitlines() if line.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_run_dumps_and_full_run_adds_the_rest(tmp_path):
    n, s, steps = 32, 64, 3
    small = ["--workload", "teapot", "--envs", str(n), "--img", str(s), "--steps", str(steps), "--warmup", "1"]
    j = _run_bench(small + ["--dump-outputs", str(tmp_path / "plain")])
    assert j["steps"] == steps and j["unit"] == "env-steps/s" and j["higher_is_better"] is True and j["dtype"] == "f32"
    assert j["value"] == pytest.approx(n * steps / (j["ms_per_step"] * steps * 1e-3), rel=1e-9)
    assert not FULL_ONLY & set(j)
    d = {f[:-4]: np.load(tmp_path / "plain" / f) for f in os.listdir(tmp_path / "plain")}
    want = {"obs": (n, 4, s, s), "full_state": (n, s, s, 4), "rewards": (n,), "dones": (n,), "actions": (n, 2),
            "action_grad": (n, 2), "position": (n, 3), "full_reward": (n,), "env_index": (n,)}
    assert {k: v.shape for k, v in d.items()} == want
    assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in d.values())
    # --full: the same timed steps on the same inputs, plus the kernel-time / roofline figures and the fresh_outputs leg
    jf = _run_bench(small + ["--full", "--no-cpu-baseline", "--fresh-steps", "2", "--dump-outputs", str(tmp_path / "full")])
    assert jf["steps"] == steps and jf["roofline"]["launches"] >= 1 and jf["roofline"]["avg_launch_ms"] > 0
    assert jf["fresh_outputs"]["steps"] == 2
    assert np.array_equal(np.load(tmp_path / "full" / "actions.npy"), d["actions"])
