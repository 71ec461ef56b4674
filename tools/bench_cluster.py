#!/usr/bin/env python3
"""Times the density clustering and the small-cluster filter per call against the radius outlier filter on the
same cloud, in the cartesian box of section 14 ([0, 15.8] x [-15.8, 15.8] x [-5.4, 5.4] m), grid cell = eps, these calls in one process:

  labels         postprocess.cluster_dbscan_ragged(min_points = --min-points): the sort, the capped count, the link walk with the
                 union-find, the flatten, the numbering scans, the labels and sizes
  labels_all     the same with min_points = 0 (no count launch; every inside row is core, so the link walk joins every pair in reach)
  filter         postprocess.remove_small_clusters_ragged(min_cluster_size = --min-cluster-size), with the kept rows' labels
  filter_largest the same with largest_only
  radius_filter  the yardstick: postprocess.remove_radius_outliers_ragged(min_neighbors = --min-points): the sort, ONE capped walk, the
                 compaction

Clouds, those of tools/bench_radius_filter.py: `frames` (8 uniform clouds of 45 000 rows), `uniform` (one of 480 000 rows) and
`clustered` (480 000 rows, half of them in 1 % of the box).  Device events around every call, --warmup warm-ups, then --reps
repetitions in which the compared calls alternate in rotating order; median, minimum and maximum in ms and each call's median over the
yardstick's.  Prints one JSON line per case and writes them all to --out (default profiles/cluster.json) beside the per-kernel
resources the compiler reports (--resources, a JSON file, is copied in when given).  Run it under `timeout`."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from bench_radius_filter import HI, LO, clustered, stats, time_calls, uniform  # noqa: E402
from rald_amd import postprocess as PP  # noqa: E402


def case(section, pts, n, B, eps, a):
    grid = PP.voxel_grid(LO, HI, eps)
    off = torch.arange(B + 1, device="cuda", dtype=torch.int64) * n
    mp, size = a.min_points, a.min_cluster_size
    calls = {"labels": lambda: PP.cluster_dbscan_ragged(pts, off, eps, mp, grid, n, return_sizes=True),
             "labels_all": lambda: PP.cluster_dbscan_ragged(pts, off, eps, 0, grid, n),
             "filter": lambda: PP.remove_small_clusters_ragged(pts, off, eps, mp, size, grid, n, return_index=True, return_labels=True),
             "filter_largest": lambda: PP.remove_small_clusters_ragged(pts, off, eps, mp, 1, grid, n, largest_only=True),
             "radius_filter": lambda: PP.remove_radius_outliers_ragged(pts, off, eps, max(mp, 1), grid, n)}
    times, out = time_calls(calls, a.warmup, a.reps)
    med = {name: statistics.median(v) for name, v in times.items()}
    labels, num, sizes = out["labels"]
    row = {"section": section, "n": n, "B": B, "eps_m": eps, "min_points": mp, "min_cluster_size": size,
           "cells": grid[2][0] * grid[2][1] * grid[2][2], "clusters": num.tolist(), "largest": int(sizes.max()),
           "clustered_rows": int((labels >= 0).sum()), "noise_rows": int((labels == -1).sum()),
           "kept": int(out["filter"][1][-1].item()), "kept_largest": int(out["filter_largest"][1][-1].item()),
           "kept_radius_filter": int(out["radius_filter"][1][-1].item()), "reps": a.reps,
           **{name: stats(v) for name, v in times.items()},
           **{name + "_over_radius_filter": round(med[name] / med["radius_filter"], 3) for name in calls if name != "radius_filter"},
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--eps", type=float, nargs="+", default=[0.1, 0.2])
    ap.add_argument("--min-points", type=int, default=4)
    ap.add_argument("--min-cluster-size", type=int, default=50)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip", nargs="*", default=[], choices=["frames", "uniform", "clustered"])
    ap.add_argument("--resources", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_cluster needs a GPU"
    clouds = {"frames": lambda: (uniform(8, 45000, 1008), 45000, 8), "uniform": lambda: (uniform(1, 480000, 1001), 480000, 1),
              "clustered": lambda: (clustered(480000, 7), 480000, 1)}
    rows = []
    for section, make in clouds.items():
        if section in a.skip:
            continue
        pts, n, B = make()
        for eps in a.eps:
            rows.append(case(section, pts, n, B, eps, a))
    doc = {"cases": rows}
    if a.resources:
        with open(a.resources) as fh:
            doc["kernels"] = json.load(fh)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(doc, fh, indent=1)


if __name__ == "__main__":
    main()
