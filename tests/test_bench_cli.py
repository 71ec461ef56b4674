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
