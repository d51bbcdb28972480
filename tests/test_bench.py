"""bench.py command-line contract: --steps sets the timed step count, the
result line carries ms_per_step, --dump-outputs stores the last step's
outputs reproducibly, and --full is accepted."""

import json
import os
import subprocess
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_bench(*extra):
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
         "--device", "cpu", "--size", "10", *extra],
        capture_output=True, text=True, timeout=300, cwd=REPO)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_dump_outputs_reproducible(tmp_path):
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    rec = _run_bench("--steps", "2", "--warmup", "1", "--dump-outputs", d1)
    _run_bench("--steps", "2", "--warmup", "1", "--dump-outputs", d2,
               "--full")
    assert rec["steps"] == 2 and rec["warmup"] == 1
    assert rec["ms_per_step"] > 0
    assert abs(rec["ms_per_step"] - rec["value"] * 1e3) < 1e-9
    assert rec["config"]["converged"]
    assert sorted(os.listdir(d1)) == ["residual_history.npy", "x.npy"]
    x1 = np.load(os.path.join(d1, "x.npy"))
    x2 = np.load(os.path.join(d2, "x.npy"))
    assert x1.dtype == np.float64 and x1.shape == (1000,)
    assert np.isfinite(x1).all() and np.abs(x1).max() > 0
    assert np.array_equal(x1, x2)
    r1 = np.load(os.path.join(d1, "residual_history.npy"))
    r2 = np.load(os.path.join(d2, "residual_history.npy"))
    assert r1.dtype == np.float64
    assert r1.shape[0] == rec["config"]["iterations"] + 1
    assert r1[-1] / r1[0] == rec["config"]["final_rel_residual"]
    assert np.array_equal(r1, r2)


def test_bench_dump_outputs_sample(tmp_path, monkeypatch):
    """A solution over the size budget is stored as the same seeded sample
    of its entries every time, in ascending index order."""
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_X_ELEMS", 64)
    x = torch.arange(1000, dtype=torch.float64)
    st = types.SimpleNamespace(residuals=[1.0, 0.5])
    bench.dump_outputs(str(tmp_path / "a"), x, st, 0, 1)
    bench.dump_outputs(str(tmp_path / "b"), x, st, 0, 1)
    xa = np.load(str(tmp_path / "a" / "x.npy"))
    xb = np.load(str(tmp_path / "b" / "x.npy"))
    assert xa.shape == (64,) and np.array_equal(xa, xb)
    assert (np.diff(xa) > 0).all() and xa.min() >= 0 and xa.max() < 1000
