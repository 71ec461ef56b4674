#!/usr/bin/env python3
"""Times the PCA normals and the normal consistency per call, on the clouds and the box of tools/bench_knn.py,
these calls in one process on the same clouds:

  normals      postprocess.estimate_normals_ragged with a view, curvature and eigenvalues: the sort, the search, the gather of the
               neighbours into six moments per row, the Jacobi sweeps
  knn          the yardstick: postprocess.knn_ragged with the distances on the same cloud and grid - the same search, ending in the
               [T,k] tables instead of the gather
  consistency  postprocess.normal_consistency_ragged of the cloud with its normals against a second cloud of the same shape with its own
  nn_twice     its yardstick: postprocess.nearest_neighbors_ragged in both directions

Clouds: `uniform`, `clustered` and `scattered` as in bench_knn, --sizes rows x --batches clouds, k = --k, the cell edge half the edge
that holds k rows per cell.  The consistency cases run for clouds of up to --consistency-max-rows rows each (the exact search is
quadratic in the cloud).  Device events around every call, --warmup warm-ups, then --reps repetitions in which the compared calls
alternate in rotating order; median, minimum and maximum in ms.  Prints one JSON line per case and rewrites --out (default
profiles/normals.json) after each.  Run it under `timeout`."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import bench_knn as BK  # noqa: E402
from rald_amd import postprocess as PP  # noqa: E402

VIEW = (0.0, 0.0, 0.0)


def write(rows, path):
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            json.dump(rows, fh, indent=1)


def normals_case(section, pts, n, B, k, edge, a, rows):
    grid = PP.voxel_grid(BK.LO, BK.HI, edge)
    off = torch.arange(B + 1, device="cuda", dtype=torch.int64) * n
    calls = {"normals": lambda: PP.estimate_normals_ragged(pts, off, k, grid, n, view=VIEW, return_curvature=True, return_eigenvalues=True,
                                                           return_found=True),
             "knn": lambda: PP.knn_ragged(pts, off, k, grid, n, return_found=True)}
    times, out = BK.time_calls(calls, a.warmup, a.reps)
    med = {name: statistics.median(v) for name, v in times.items()}
    nrm, curv, _, found = out["normals"]
    row = {"section": section, "n": n, "B": B, "k": k, "cell_m": round(edge, 5), "cells": grid[2][0] * grid[2][1] * grid[2][2],
           "defined_share": round(float((found >= 2).float().mean()), 5), "mean_curvature": round(float(curv.nan_to_num(0.0).mean()), 5),
           "same_found_as_knn": bool(torch.equal(found, out["knn"][2])), "reps": a.reps, **{name: BK.stats(v) for name, v in times.items()},
           "normals_over_knn": round(med["normals"] / med["knn"], 3), "device": torch.cuda.get_device_name(0)}
    print(json.dumps(row), flush=True)
    rows.append(row)
    write(rows, a.out)
    return nrm


def consistency_case(section, pts, nrm, other, other_nrm, n, B, a, rows):
    off = torch.arange(B + 1, device="cuda", dtype=torch.int64) * n
    calls = {"consistency": lambda: PP.normal_consistency_ragged(pts, nrm, off, other, other_nrm, off, n, n),
             "nn_twice": lambda: (PP.nearest_neighbors_ragged(pts, off, other, off, n, n), PP.nearest_neighbors_ragged(other, off, pts, off, n, n))}
    times, out = BK.time_calls(calls, a.warmup, a.reps)
    med = {name: statistics.median(v) for name, v in times.items()}
    row = {"section": section + "_consistency", "n": n, "B": B, "nc_cloud0": [round(v, 6) for v in out["consistency"][0][0].tolist()],
           "reps": a.reps, **{name: BK.stats(v) for name, v in times.items()}, "consistency_over_nn_twice": round(med["consistency"] / med["nn_twice"], 3),
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(row), flush=True)
    rows.append(row)
    write(rows, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[45000, 480000])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--k", type=int, nargs="+", default=[8, 20, 32])
    ap.add_argument("--edge-factor", type=float, default=0.5)
    ap.add_argument("--consistency-max-rows", type=int, default=45000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip", nargs="*", default=[], choices=["uniform", "clustered", "scattered", "consistency"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normals.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_normals needs a GPU"
    rows = []
    edge_of = lambda n, k, volume=BK.VOLUME: a.edge_factor * (volume * k / n) ** (1.0 / 3.0)
    clouds = []
    for n in a.sizes:
        for B in a.batches:
            if "uniform" not in a.skip:
                clouds.append(("uniform", BK.uniform(B, n, 1000 + B), BK.uniform(B, n, 3000 + B), n, B, BK.VOLUME))
            if "scattered" not in a.skip:
                clouds.append(("scattered", BK.scattered(B, n, 2000 + B)[0], BK.scattered(B, n, 4000 + B)[0], n, B, BK.VOLUME / 8))
    if "clustered" not in a.skip:
        clouds.append(("clustered", BK.clustered(480000, 7), None, 480000, 1, BK.VOLUME))
    for section, pts, other, n, B, volume in clouds:
        nrm = None
        for k in a.k:
            nrm = normals_case(section, pts, n, B, k, edge_of(n, k, volume), a, rows)
        if "consistency" not in a.skip and other is not None and n <= a.consistency_max_rows:
            k = a.k[0]
            other_nrm = PP.estimate_normals_ragged(other, torch.arange(B + 1, device="cuda", dtype=torch.int64) * n, k,
                                                   PP.voxel_grid(BK.LO, BK.HI, edge_of(n, k, volume)), n, view=VIEW)
            consistency_case(section, pts, nrm, other, other_nrm, n, B, a, rows)
    if a.out:
        print(f"wrote {len(rows)} rows to {a.out}")


if __name__ == "__main__":
    main()
