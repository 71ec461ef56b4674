"""bench.py's host side: --dump-outputs writes the timed path's output as float32 .npy within its size limit (a fixed subset of samples
beyond it), and --steps / --warmup refuse values that would not time what the result line claims."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_outputs_writes_float32_npy(tmp_path):
    y = torch.randn(3, 512, 32, dtype=torch.float64)
    files = bench.dump_outputs(str(tmp_path / "out"), {"denoised": y})
    a = np.load(tmp_path / "out" / "denoised.npy")
    assert a.dtype == np.float32 and a.shape == (3, 512, 32)
    assert np.array_equal(a, y.float().numpy())
    assert files["denoised"]["shape"] == [3, 512, 32] and files["denoised"]["rows_of"] == 3


def test_dump_outputs_keeps_a_fixed_subset_within_the_limit(tmp_path):
    y = torch.randn(100, 64, 32)                   # 8 KiB per sample
    limit = 40 * 8192 + 4096                       # room for 40 samples and the header
    bench.dump_outputs(str(tmp_path / "a"), {"denoised": y}, limit=limit)
    bench.dump_outputs(str(tmp_path / "b"), {"denoised": y}, limit=limit)
    a, b = np.load(tmp_path / "a" / "denoised.npy"), np.load(tmp_path / "b" / "denoised.npy")
    assert os.path.getsize(tmp_path / "a" / "denoised.npy") <= limit
    assert a.shape == (40, 64, 32) and np.array_equal(a, b)
    rows = [next(i for i in range(100) if np.array_equal(r, y[i].numpy())) for r in a]
    assert rows == sorted(set(rows)) and rows[0] == 0 and rows[-1] >= 95  # distinct samples, spread over the whole batch


@pytest.mark.parametrize("args", [["--steps", "0"], ["--warmup", "-1"]])
def test_bench_refuses_steps_it_cannot_time(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr and not r.stdout


def test_secondary_measurements_need_full():
    """A plain run measures the headline alone; --full turns the CPU baseline and the secondary legs on, each with its own off switch."""
    legs = lambda *argv: bench.secondary_legs(bench.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "1", *argv]))
    assert bench.parse_args([]).full is False
    assert legs() == (False, False)
    assert legs("--no-extras") == (False, False) and legs("--no-cpu-baseline") == (False, False)
    assert legs("--full") == (True, True)
    assert legs("--full", "--no-extras") == (True, False)
    assert legs("--full", "--no-cpu-baseline") == (False, True)


HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY_KEYS = ("config4", "ddp_step", "sampler18_B8_s", "extras_error")


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_nothing_that_takes_runs_of_its_own(tmp_path):
    """One plain run of the command line at a small batch: one JSON line with the headline fields, the dumped output, no CPU baseline and
    none of the secondary legs - and therefore little time outside its steps (bound: the 30 s a plain run may spend there)."""
    import json
    import time
    steps, warmup = 2, 1
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--batch", "8",
                        "--dump-outputs", str(tmp_path / "out")], capture_output=True, text=True, timeout=120)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert all(k in out for k in HEADLINE_KEYS)
    assert out["full"] is False and out["steps"] == steps and out["warmup"] == warmup and out["value"] > 0
    assert out["metric"] == "denoising steps/sec (whole node)" and out["unit"] == "sample*NFE/s" and out["dtype"] == "bf16" and out["higher_is_better"] is True
    assert out.get("cpu_baseline") is None and not any(k in out for k in FULL_ONLY_KEYS)
    assert "cpu baseline" not in r.stderr and "extras" not in r.stderr
    a = np.load(tmp_path / "out" / "denoised.npy")
    assert a.dtype == np.float32 and a.shape == (8, 512, 32) and np.isfinite(a).all()
    outside = wall - (steps + warmup) * out["ms_per_step"] * 1e-3
    print(f"plain run: {wall:.1f} s in all, {outside:.1f} s outside its steps")
    assert outside <= 30.0
