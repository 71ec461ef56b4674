#!/usr/bin/env python3
"""Times the fixed-radius neighbour search and the radius outlier filter per call in the cartesian box of
section 14 ([0, 15.8] x [-15.8, 15.8] x [-5.4, 5.4] m), grid cell = radius, these calls in one process on the same clouds:

  filter         postprocess.remove_radius_outliers_ragged(min_neighbors = --min-neighbors): the sort, the capped count, the compaction
  count          postprocess.radius_neighbor_count_ragged without a cap
  count_nearest  the same with return_nearest
  voxel          yardstick (b): postprocess.voxel_downsample_ragged on the same cloud and grid - the sort's share of the call
  torch_ops      yardstick (a): the uncapped counts by torch device ops, float32 brute force in blocks of 2048 rows against the whole
                 cloud.  It runs where it finishes in reasonable time: clouds of up to --torch-max-rows rows in all (default 8 x 45 000);
                 the rows of the table without it say `torch_ops: null`

Clouds: uniform ones of --sizes rows x --batches clouds (480 000 rows only up to B = 8), one `clustered` cloud of 480 000 rows with half
its rows in 1 % of the box, and `one_cell` clouds with every row inside one cell of the finest grid - the limit: without a cap every
row meets every other (n * n distances), so that section runs --limit-reps repetitions only.
Device events around every call, --warmup warm-ups, then --reps repetitions in which the compared calls alternate in rotating order;
median, minimum and maximum in ms.  Prints one JSON line per case and writes them all to --out (default
profiles/radius_filter.json).  Run it under `timeout`."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from rald_amd import postprocess as PP  # noqa: E402

LO, HI = (0.0, -15.8, -5.4), (15.8, 15.8, 5.4)


def event_ms(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop), out


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def time_calls(calls, warmup, reps):
    names = list(calls)
    times, out = {k: [] for k in names}, {}
    for rep in range(warmup + reps):
        order = names[rep % len(names):] + names[:rep % len(names)]
        for name in order:
            ms, out[name] = event_ms(calls[name])
            if rep >= warmup:
                times[name].append(ms)
    return times, out


def torch_counts(points, n, B, radius, block=2048):
    """The uncapped counts of B dense clouds of n rows by elementwise float32 ops, one rounding each: the definition's d2."""
    r2 = torch.tensor(radius, device=points.device, dtype=torch.float32) ** 2
    out = torch.empty(B * n, device=points.device, dtype=torch.int32)
    for b in range(B):
        p = points[b * n:(b + 1) * n]
        x, y, z = p[:, 0].contiguous(), p[:, 1].contiguous(), p[:, 2].contiguous()
        for s in range(0, n, block):
            e = min(s + block, n)
            dx, dy, dz = x[None, :] - x[s:e, None], y[None, :] - y[s:e, None], z[None, :] - z[s:e, None]
            d2 = (dx * dx + dy * dy) + dz * dz
            out[b * n + s:b * n + e] = (d2 <= r2).sum(dim=1) - 1                    # the row itself: d2 = 0
    return out


def uniform(B, n, seed):
    gen = torch.Generator("cuda").manual_seed(seed)
    span = torch.tensor([h - l for l, h in zip(LO, HI)], device="cuda")
    return torch.rand(B * n, 3, device="cuda", generator=gen) * span + torch.tensor(LO, device="cuda")


def clustered(n, seed):
    """Half the rows uniform in the box, half in a sub-box of 1 % of its volume."""
    pts = uniform(1, n, seed)
    gen = torch.Generator("cuda").manual_seed(seed + 1)
    span = torch.tensor([h - l for l, h in zip(LO, HI)], device="cuda") * (0.01 ** (1.0 / 3.0))
    pts[n // 2:] = torch.rand(n - n // 2, 3, device="cuda", generator=gen) * span + torch.tensor([6.0, 2.0, -1.0], device="cuda")
    return pts


def one_cell(n, seed):
    gen = torch.Generator("cuda").manual_seed(seed)
    return torch.rand(n, 3, device="cuda", generator=gen) * 0.04 + torch.tensor([7.005, 0.005, 0.005], device="cuda")


def case(section, pts, n, B, radius, a, reps, with_torch):
    grid = PP.voxel_grid(LO, HI, radius)
    off = torch.arange(B + 1, device="cuda", dtype=torch.int64) * n
    k = a.min_neighbors
    calls = {"filter": lambda: PP.remove_radius_outliers_ragged(pts, off, radius, k, grid, n),
             "count": lambda: PP.radius_neighbor_count_ragged(pts, off, radius, grid, n),
             "count_nearest": lambda: PP.radius_neighbor_count_ragged(pts, off, radius, grid, n, return_nearest=True),
             "voxel": lambda: PP.voxel_downsample_ragged(pts, off, grid, n)}
    if with_torch:
        calls["torch_ops"] = lambda: torch_counts(pts, n, B, radius)
    times, out = time_calls(calls, a.warmup, reps)
    med = {name: statistics.median(v) for name, v in times.items()}
    cnt = out["count"]
    row = {"section": section, "n": n, "B": B, "radius_m": radius, "min_neighbors": k, "cells": grid[2][0] * grid[2][1] * grid[2][2],
           "kept": int(out["filter"][1][-1].item()), "mean_count": round(float(cnt.clamp(min=0).float().mean()), 3),
           "max_count": int(cnt.max()), "reps": reps, **{name: stats(v) for name, v in times.items()},
           "voxel_over_filter": round(med["voxel"] / med["filter"], 3),
           "same_counts_with_nearest": bool(torch.equal(cnt, out["count_nearest"][0]))}
    if with_torch:
        row["torch_ops_over_count"] = round(med["torch_ops"] / med["count"], 3)
        row["torch_same_counts"] = bool(torch.equal(out["torch_ops"], cnt))
    else:
        row["torch_ops"] = None
    row["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[45000, 480000])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--radii", type=float, nargs="+", default=[0.05, 0.1, 0.2])
    ap.add_argument("--min-neighbors", type=int, default=2)
    ap.add_argument("--torch-max-rows", type=int, default=8 * 45000)
    ap.add_argument("--limit-sizes", type=int, nargs="*", default=[45000, 480000])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--limit-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip", nargs="*", default=[], choices=["uniform", "clustered", "one_cell"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "radius_filter.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_radius_filter needs a GPU"
    rows = []
    if "uniform" not in a.skip:
        for n in a.sizes:
            for B in a.batches:
                if n > 100000 and B > 8:
                    continue
                pts = uniform(B, n, 1000 + B)
                for radius in a.radii:
                    rows.append(case("uniform", pts, n, B, radius, a, a.reps, B * n <= a.torch_max_rows))
    if "clustered" not in a.skip:
        pts = clustered(480000, 7)
        for radius in a.radii:
            rows.append(case("clustered", pts, 480000, 1, radius, a, a.reps, False))
    if "one_cell" not in a.skip:
        for n in a.limit_sizes:
            rows.append(case("one_cell", one_cell(n, 5), n, 1, 0.05, a, a.limit_reps, n <= a.torch_max_rows))
            assert rows[-1]["max_count"] <= n - 1
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
