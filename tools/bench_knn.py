#!/usr/bin/env python3
"""Times the k-nearest-neighbour search and the statistical outlier filter per call in the cartesian box of
section 14 ([0, 15.8] x [-15.8, 15.8] x [-5.4, 5.4] m), these calls in one process on the same clouds:

  knn          postprocess.knn_ragged with the distances: the sort, the gather, the search, the [T,k] tables
  filter       postprocess.remove_statistical_outliers_ragged(std_ratio = --std-ratio): the search with the mean folded in, the
               statistics, the compaction
  filter_rmax  the same with max_radius = three times the radius that holds k rows at the cloud's mean density
  radius       yardstick (b): the parent's postprocess.remove_radius_outliers_ragged on the same cloud, with the radius that holds
               about k rows at the cloud's mean density (grid cell = that radius, min_neighbors = 2)
  torch_ops    yardstick (a): k nearest by torch device ops - torch.cdist in blocks of 2048 rows against the whole cloud, then
               topk(k + 1).  It runs for clouds of up to --torch-max-rows rows in all (default 45 000); `torch_ops: null` elsewhere

Clouds: `uniform` ones of --sizes rows x --batches clouds, one `clustered` cloud of 480 000 rows with half its rows in 1 % of the box,
`scattered` clouds with 99 % of the rows in one eighth of the box and 1 % uniform over all of it (the rows the filter exists for: their
boxes of cells grow far), and `one_cell` clouds with every row inside one cell of every grid - the limit: every row meets every other.
Per shape three cell edges: the edge e that holds --k rows per cell at the cloud's mean density, e / 2 and 2 e.
Device events around every call, --warmup warm-ups, then --reps repetitions in which the compared calls alternate in rotating order;
median, minimum and maximum in ms.  Prints one JSON line per case and rewrites --out (default profiles/knn.json) after each.  Run it
under `timeout`."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from rald_amd import postprocess as PP  # noqa: E402

LO, HI = (0.0, -15.8, -5.4), (15.8, 15.8, 5.4)
VOLUME = math.prod(h - l for l, h in zip(LO, HI))


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


def torch_knn(points, n, B, k, block=2048):
    """The k nearest other rows of B dense clouds of n rows by cdist and topk: not the definition's bits, a yardstick for the time."""
    out = torch.empty(B * n, k, device=points.device, dtype=torch.int64)
    for b in range(B):
        p = points[b * n:(b + 1) * n]
        for s in range(0, n, block):
            e = min(s + block, n)
            d = torch.cdist(p[s:e], p)
            out[b * n + s:b * n + e] = d.topk(min(k + 1, n), dim=1, largest=False).indices[:, 1:k + 1]
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


def scattered(B, n, seed):
    """99 % of every cloud's rows in the corner eighth of the box, every hundredth row uniform over the whole box."""
    pts = uniform(B, n, seed)
    far = torch.arange(B * n, device="cuda") % 100 == 0
    span = torch.tensor([h - l for l, h in zip(LO, HI)], device="cuda")
    lo = torch.tensor(LO, device="cuda")
    return torch.where(far[:, None], pts, (pts - lo) * 0.5 + lo), span


def one_cell(n, seed):
    gen = torch.Generator("cuda").manual_seed(seed)
    return torch.rand(n, 3, device="cuda", generator=gen) * 0.04 + torch.tensor([7.005, 0.005, 0.005], device="cuda")


def case(section, pts, n, B, k, edge, a, reps, with_torch, rows, dense_volume=VOLUME):
    grid = PP.voxel_grid(LO, HI, edge)
    off = torch.arange(B + 1, device="cuda", dtype=torch.int64) * n
    r_k = (3.0 * k * dense_volume / (4.0 * math.pi * n)) ** (1.0 / 3.0)                 # the ball that holds k rows at the mean density
    rgrid = PP._radius_grid(LO, HI, r_k)
    calls = {"knn": lambda: PP.knn_ragged(pts, off, k, grid, n, return_found=True),
             "filter": lambda: PP.remove_statistical_outliers_ragged(pts, off, k, a.std_ratio, grid, n, return_stats=True),
             "filter_rmax": lambda: PP.remove_statistical_outliers_ragged(pts, off, k, a.std_ratio, grid, n, max_radius=3.0 * r_k),
             "radius": lambda: PP.remove_radius_outliers_ragged(pts, off, r_k, 2, rgrid, n)}
    if with_torch:
        calls["torch_ops"] = lambda: torch_knn(pts, n, B, k)
    times, out = time_calls(calls, a.warmup, reps)
    med = {name: statistics.median(v) for name, v in times.items()}
    idx, dist2, found = out["knn"]
    row = {"section": section, "n": n, "B": B, "k": k, "cell_m": round(edge, 5), "cells": grid[2][0] * grid[2][1] * grid[2][2],
           "rows_per_cell": round(n / (dense_volume / edge ** 3), 3), "radius_m": round(r_k, 5), "kept": int(out["filter"][1][-1].item()),
           "kept_rmax": int(out["filter_rmax"][1][-1].item()), "kept_radius": int(out["radius"][1][-1].item()),
           "mean_found": round(float(found.clamp(min=0).float().mean()), 3), "stats_cloud0": [round(v, 6) for v in out["filter"][2][0].tolist()],
           "reps": reps, **{name: stats(v) for name, v in times.items()}, "radius_over_filter": round(med["radius"] / med["filter"], 3)}
    if with_torch:
        row["torch_ops_over_knn"] = round(med["torch_ops"] / med["knn"], 3)
        row["torch_same_index_share"] = round(float((out["torch_ops"] == idx).float().mean()), 5)
    else:
        row["torch_ops"] = None
    row["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(row), flush=True)
    rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[45000, 480000])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--k", type=int, nargs="+", default=[8, 20, 32])
    ap.add_argument("--edge-factors", type=float, nargs="+", default=[0.5, 1.0, 2.0])
    ap.add_argument("--std-ratio", type=float, default=2.0)
    ap.add_argument("--torch-max-rows", type=int, default=45000)
    ap.add_argument("--limit-sizes", type=int, nargs="*", default=[45000])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--limit-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip", nargs="*", default=[], choices=["uniform", "clustered", "scattered", "one_cell"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_knn needs a GPU"
    rows = []
    edge_of = lambda n, k, volume=VOLUME: (volume * k / n) ** (1.0 / 3.0)
    if "uniform" not in a.skip:
        for n in a.sizes:
            for B in a.batches:
                pts = uniform(B, n, 1000 + B)
                for k in a.k:
                    for f in a.edge_factors:
                        case("uniform", pts, n, B, k, f * edge_of(n, k), a, a.reps, B * n <= a.torch_max_rows and f == 1.0, rows)
    if "clustered" not in a.skip:
        pts = clustered(480000, 7)
        for k in a.k:
            for f in a.edge_factors:
                case("clustered", pts, 480000, 1, k, f * edge_of(480000, k), a, a.reps, False, rows)
    if "scattered" not in a.skip:
        for n in a.sizes:
            for B in a.batches:
                pts, _ = scattered(B, n, 2000 + B)
                for k in a.k:
                    for f in a.edge_factors:                                       # the edge that suits the dense eighth
                        case("scattered", pts, n, B, k, f * edge_of(n, k, VOLUME / 8), a, a.reps, False, rows, VOLUME / 8)
    if "one_cell" not in a.skip:
        for n in a.limit_sizes:
            for k in a.k:
                case("one_cell", one_cell(n, 5), n, 1, k, 0.05, a, a.limit_reps, n <= a.torch_max_rows, rows, 0.04 ** 3)
    if a.out:
        print(f"wrote {len(rows)} rows to {a.out}")


if __name__ == "__main__":
    main()
