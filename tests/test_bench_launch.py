"""bench.py's multi-rank launch path on CPU (gloo).

`python bench.py --gpus N` without a launcher must start N ranks itself (the
driver's scaling runs read n_gpus from the JSON line), and a rank whose
WORLD_SIZE disagrees with --gpus must refuse to run.  `--dist-selftest`
replaces the GPU solve by the step's one collective (the u0 all-gather in
rank order), so the whole launch path runs here without a GPU.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(args, env_extra=None):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True,
                          env=env, timeout=180)


@pytest.mark.parametrize("n", [1, 2])
def test_bench_gpus_n_launches_n_ranks(n):
    p = _run(["--gpus", str(n), "--dist-selftest"])
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    res = json.loads(lines[0])
    assert res["n_gpus"] == n
    assert res["requested"] == n
    assert res["allgather_ok"] is True


def test_bench_rejects_world_size_mismatch():
    p = _run(["--gpus", "4", "--dist-selftest"],
             {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert p.returncode == 2
    assert "WORLD_SIZE=2 but --gpus 4" in p.stderr


def test_dump_outputs_formats_and_budget(tmp_path):
    """--dump-outputs' writer: float32 / float64 .npy files, every array whole
    under the budget, a fixed sorted row sample above it."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    rng = np.random.default_rng(3)
    arrays = {"u0": rng.standard_normal((100, 12)).astype(np.float32),
              "iters": rng.integers(0, 4000, 100).astype(np.int32),
              "obj64": rng.standard_normal(100)}
    rows = bench.dump_outputs(str(tmp_path / "a"), arrays)
    assert rows == {"u0": 100, "iters": 100, "obj64": 100}
    got = {k: np.load(str(tmp_path / "a" / (k + ".npy"))) for k in arrays}
    assert got["u0"].dtype == np.float32 and got["iters"].dtype == np.float32
    assert got["obj64"].dtype == np.float64
    for k in arrays:
        assert np.array_equal(got[k], arrays[k])
    # 3 arrays, 2400 bytes: 800 each -> 16 rows of u0 (48 B), 100 of the others
    budget = 2400
    rows = bench.dump_outputs(str(tmp_path / "b"), arrays, max_bytes=budget)
    assert rows == {"u0": 16, "iters": 100, "obj64": 100}
    cut = np.load(str(tmp_path / "b" / "u0.npy"))
    assert cut.shape == (16, 12)
    idx = [int(np.flatnonzero((arrays["u0"] == r).all(axis=1))[0]) for r in cut]
    assert idx == sorted(set(idx))
    assert sum(np.load(str(tmp_path / "b" / (k + ".npy"))).nbytes for k in arrays) <= budget
    bench.dump_outputs(str(tmp_path / "c"), arrays, max_bytes=budget)
    assert np.array_equal(np.load(str(tmp_path / "c" / "u0.npy")), cut)


def test_usable_cores_and_cpu_model():
    sys.path.insert(0, ROOT)
    import bench
    n = bench.usable_cores()
    assert 1 <= n <= (os.cpu_count() or 1)
    assert isinstance(bench.cpu_model(), str) and bench.cpu_model()
