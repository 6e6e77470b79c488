"""bench.py's output dump (`--dump-outputs DIR`) and its plain / `--full` split: the size cap and the seeded
sample on the CPU, and one small plain run on the GPU whose dumped logliks are the engine's own."""
from __future__ import annotations

import json
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def test_dump_outputs_writes_float64_whole_when_small(tmp_path):
    import bench
    a = np.array([1.5, -np.inf, np.nan, 3.0])
    n = bench.dump_outputs(str(tmp_path / "d"), {"loglik": a, "best_candidate": np.array([2.0, 7.0], dtype=np.float32)})
    assert n == {"loglik": 4, "best_candidate": 2}
    got, cls = np.load(tmp_path / "d" / "loglik.npy"), np.load(tmp_path / "d" / "loglik_class.npy")
    assert got.dtype == cls.dtype == np.float64
    np.testing.assert_array_equal(got, [1.5, 0.0, 0.0, 3.0])  # every file holds finite numbers only
    np.testing.assert_array_equal(cls, [0.0, 1.0, 3.0, 0.0])  # 1 = −Inf, 3 = NaN (2 = +Inf)
    assert np.load(tmp_path / "d" / "best_candidate.npy").dtype == np.float64
    np.testing.assert_array_equal(np.load(tmp_path / "d" / "best_candidate_class.npy"), [0.0, 0.0])


def test_dump_outputs_caps_size_with_a_fixed_sample(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 1 << 16)
    big = np.arange(100_000, dtype=np.float64)
    small = np.arange(5, dtype=np.float64)
    for d in ("a", "b"):
        n = bench.dump_outputs(str(tmp_path / d), {"loglik": big, "best_candidate": small})
    files = sorted((tmp_path / "a").iterdir())
    assert sum(f.stat().st_size for f in files) <= 1 << 16
    got = np.load(tmp_path / "a" / "loglik.npy")
    assert got.size == n["loglik"] < big.size and np.all(np.diff(got) > 0)  # a sorted subset, no repeats
    np.testing.assert_array_equal(got, np.load(tmp_path / "b" / "loglik.npy"))  # the same elements every run
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "best_candidate.npy"), small)


@pytest.mark.gpu
def test_plain_run_dumps_the_timed_logliks(engine, tmp_path):
    """A plain run (no --full) times its steps and nothing else — no CPU baseline, host rate or comparison leg in
    the line — and `--dump-outputs` holds the logliks of the timed path: bitwise the engine's own for the same
    seeded inputs (the same kernel on the same θ)."""
    from yfm_amd import KIND_DNS
    from yfm_amd import synthetic as S
    B, T = 512, 120
    out = tmp_path / "dump"
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--batch", str(B), "--T", str(T), "--steps", "3",
           "--warmup", "1", "--settle-seconds", "0", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    line = lines[0]
    assert line["steps"] == 3 and line["full"] is False and line["ms_per_step"] > 0
    assert abs(line["value"] - B / (line["ms_per_step"] * 1e-3)) <= 1e-9 * line["value"]
    assert line["cpu_baseline"] is None and line["host_pointer_rate"] is None
    assert "steady_state" not in line and "fp64_mode" not in line
    assert line["dumped_outputs"]["elements"] == {"loglik": B}
    got, cls = np.load(out / "loglik.npy"), np.load(out / "loglik_class.npy")
    assert got.dtype == np.float64 and got.shape == cls.shape == (B,) and np.isfinite(got).all()
    engine.set_panel(S.simulate_panel(KIND_DNS, T), S.maturities_30())
    ref = engine.loglik(KIND_DNS, S.theta_batch(KIND_DNS, B, seed=S.BATCH_SEED))
    fin = np.isfinite(ref)
    assert fin.any()
    np.testing.assert_array_equal(got, np.where(fin, ref, 0.0))
    np.testing.assert_array_equal(cls, np.where(fin, 0.0, np.where(np.isneginf(ref), 1.0, 3.0)))
