#!/usr/bin/env python3
"""Times farthest-point sampling per call, for (n, k) in --shapes and B in --batches dense clouds of uniform
points, two ways in one process on the same clouds:

  (a) kernel       postprocess.farthest_point_sample: one launch, one workgroup per cloud (resident form up to 16384 points, the
                   streaming form above)
  (b) torch_loop   the yardstick: the same algorithm as k iterations of torch device ops over the whole batch (subtract, square-sum,
                   minimum, argmax, gather of the next centre, two index writes) - several launches per iteration

Device events around every call, a warm-up of both, then repetitions that alternate the two; median, minimum and maximum in ms, and the
kernel's time per iteration in us.  `same_indices` says whether both chose the same rows (torch's sum order and argmax tie rule are its
own, so this is information, not a check: tests/test_gpu_fps.py checks the kernel).  Prints one JSON line per case and writes them
all to --out (default profiles/fps.json).  Run it under `timeout`."""
import argparse
import json
import os
import platform
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from rald_amd import postprocess as PP  # noqa: E402


def event_ms(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop), out


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def torch_loop(points: torch.Tensor, k: int) -> torch.Tensor:
    """points [B,n,3] -> idx [B,k]: the greedy choice from row 0 with torch ops, nothing read back."""
    B, n, _ = points.shape
    rows = torch.arange(B, device=points.device)
    idx = torch.empty(B, k, dtype=torch.int64, device=points.device)
    mind = torch.full((B, n), float("inf"), device=points.device)
    cur = torch.zeros(B, dtype=torch.int64, device=points.device)
    idx[:, 0] = cur
    for j in range(1, k):
        d = points - points[rows, cur][:, None, :]
        mind = torch.minimum(mind, (d * d).sum(dim=2))
        cur = mind.argmax(dim=1)
        idx[:, j] = cur
    return idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=int, nargs="+", default=[2048, 512, 10000, 512, 16384, 10000, 60000, 10000], help="n k pairs")
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fps.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_fps needs a GPU"
    assert len(a.shapes) % 2 == 0, "--shapes takes n k pairs"
    rows = []
    for n, k in zip(a.shapes[0::2], a.shapes[1::2]):
        for B in a.batches:
            gen = torch.Generator("cuda").manual_seed(1000 + B)
            pts = (torch.rand(B, n, 3, device="cuda", generator=gen) - 0.5) * torch.tensor([15.8, 31.6, 10.8], device="cuda")
            calls = {"kernel": lambda: PP.farthest_point_sample(pts, k), "torch_loop": lambda: torch_loop(pts, k)}
            times = {name: [] for name in calls}
            out = {}
            for rep in range(a.warmup + a.reps):
                for name in (("kernel", "torch_loop") if rep % 2 == 0 else ("torch_loop", "kernel")):
                    ms, out[name] = event_ms(calls[name])
                    if rep >= a.warmup:
                        times[name].append(ms)
            med = {name: statistics.median(v) for name, v in times.items()}
            row = {"n": n, "k": k, "B": B, "reps": a.reps, "form": "resident" if n <= 16384 else "streaming",
                   **{name: stats(v) for name, v in times.items()}, "kernel_us_per_iteration": round(1e3 * med["kernel"] / k, 3),
                   "kernel_over_torch_loop": round(med["kernel"] / med["torch_loop"], 4),
                   "same_indices": bool(torch.equal(out["kernel"], out["torch_loop"])), "device": torch.cuda.get_device_name(0), "host": platform.node()}
            print(json.dumps(row), flush=True)
            rows.append(row)
            del pts
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
