#!/usr/bin/env python3
"""Times voxel-grid down-sampling per call on uniform clouds in the cartesian box of section 14
([0, 15.8] x [-15.8, 15.8] x [-5.4, 5.4] m), three ways in one process on the same clouds:

  (a) split        postprocess.voxel_downsample_ragged with the split sort (one workgroup per chunk; --chunk rows, default 4096)
  (b) one_wg       the same call forced onto its one-workgroup sort (chunk >= n): what the split across workgroups buys
  (c) torch_ops    the yardstick: the same result by torch device ops - the keys by elementwise ops, torch.unique(key,
                   return_inverse=True, return_counts=True), index_add_ in float64.  Its sums use atomics, so values are compared to
                   1e-6 only (max_abs_diff), and torch.unique reads its output size back (a host synchronisation the kernels do not need)
  (d) auto         the call as users make it (chunk 0: the automatic rule)

Sections: `shapes` (n in --sizes x B in --batches x cell in --cells), `rule` (the sweep the automatic chunk rule is set from: small and
middle n, split at --rule-chunks against one_wg), `degenerate` (every row in one cell, once) and `resample` (the tail's
resample=k on one 480 000-row frame with and without thin).  Device events around every call, --warmup warm-ups, then --reps
repetitions in which the compared calls alternate in rotating order; median, minimum and maximum in ms.  Prints one JSON line per case
and writes them all to --out (default profiles/voxel_downsample.json).  Run it under `timeout`."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from rald_amd import engine_generation as E, postprocess as PP  # noqa: E402

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


def torch_ops(points, n, B, grid):
    """points [B*n,3] -> (centroids [M,3], counts [M]) for the whole batch, clouds told apart by b * cells in the key."""
    lo3, v3, dims3 = grid
    dev = points.device
    c = torch.floor((points - torch.tensor(lo3, device=dev)) / torch.tensor(v3, device=dev))
    d = torch.tensor(dims3, device=dev, dtype=torch.float32)
    inside = ((c >= 0) & (c < d)).all(dim=1)
    ci = c.to(torch.int64)
    key = (ci[:, 0] * dims3[1] + ci[:, 1]) * dims3[2] + ci[:, 2]
    key = key + (torch.arange(B * n, device=dev) // n) * (dims3[0] * dims3[1] * dims3[2])
    key, p = key[inside], points[inside]
    uniq, inv, cnt = torch.unique(key, return_inverse=True, return_counts=True)
    s = torch.zeros(uniq.numel(), 3, device=dev, dtype=torch.float64).index_add_(0, inv, p.double())
    return (s / cnt[:, None]).float(), cnt


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


def cloud(B, n, seed):
    gen = torch.Generator("cuda").manual_seed(seed)
    span = torch.tensor([h - l for l, h in zip(LO, HI)], device="cuda")
    return torch.rand(B * n, 3, device="cuda", generator=gen) * span + torch.tensor(LO, device="cuda")


def case(section, n, B, cell, chunks, a, with_torch=True, points=None):
    grid = PP.voxel_grid(LO, HI, cell)
    pts = cloud(B, n, 1000 + B) if points is None else points
    off = torch.arange(B + 1, device="cuda", dtype=torch.int64) * n
    one = -(-n // 1024) * 1024
    calls = {"auto": lambda: PP.voxel_downsample_ragged(pts, off, grid, n, return_count=True),
             "one_wg": lambda: PP.voxel_downsample_ragged(pts, off, grid, n, return_count=True, chunk=one)}
    for ch in chunks:
        if ch < n:
            calls[f"split_{ch}"] = (lambda ch: lambda: PP.voxel_downsample_ragged(pts, off, grid, n, return_count=True, chunk=ch))(ch)
    if with_torch:
        calls["torch_ops"] = lambda: torch_ops(pts, n, B, grid)
    times, out = time_calls(calls, a.warmup, a.reps)
    med = {k: statistics.median(v) for k, v in times.items()}
    m = int(out["auto"][1][-1].item())
    row = {"section": section, "n": n, "B": B, "cell_m": cell, "cells": grid[2][0] * grid[2][1] * grid[2][2],
           "passes": -(-(grid[2][0] * grid[2][1] * grid[2][2]).bit_length() // 8), "voxels": m, "reps": a.reps,
           **{k: stats(v) for k, v in times.items()}, "one_wg_over_auto": round(med["one_wg"] / med["auto"], 3)}
    for k in calls:
        if k.startswith("split_") or k == "one_wg":
            same = torch.equal(out[k][0][:m], out["auto"][0][:m]) and torch.equal(out[k][1], out["auto"][1])
            row.setdefault("same_bits_as_auto", True)
            row["same_bits_as_auto"] = row["same_bits_as_auto"] and bool(same)
    if with_torch:
        tp, tc = out["torch_ops"]
        row["torch_ops_over_auto"] = round(med["torch_ops"] / med["auto"], 3)
        row["torch_same_voxels"] = bool(tp.shape[0] == m and torch.equal(tc.int(), out["auto"][2][:m]))
        row["torch_max_abs_diff"] = float((tp - out["auto"][0][:m]).abs().max()) if tp.shape[0] == m and m else None
    row["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(row), flush=True)
    return row


def resample_case(a, n=480000, k=2048, cell=0.5):
    grid = PP.voxel_grid(LO, HI, cell)
    pts = cloud(1, n, 77)
    off = torch.tensor([0, n], device="cuda", dtype=torch.int64)

    def thin_then_sample():
        t = E._thin(pts, off, grid, n)
        return E._resample(t[0], t[1], k, E._thin_bound(n, grid))
    calls = {"resample_only": lambda: E._resample(pts, off, k, n), "thin_then_resample": thin_then_sample,
             "thin_only": lambda: E._thin(pts, off, grid, n)}
    times, out = time_calls(calls, a.warmup, a.reps)
    row = {"section": "resample", "n": n, "k": k, "cell_m": cell, "cells": grid[2][0] * grid[2][1] * grid[2][2],
           "voxels": int(out["thin_only"][1][-1].item()), "rows_sampled_without_thin": min(n, PP.FPS_MAX_POINTS), "reps": a.reps,
           **{name: stats(v) for name, v in times.items()}, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[45000, 480000])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--cells", type=float, nargs="+", default=[0.05, 0.1, 0.2])
    ap.add_argument("--chunk", type=int, nargs="+", default=[4096], help="chunk lengths of the split sort in the `shapes` section")
    ap.add_argument("--rule-sizes", type=int, nargs="*", default=[1024, 2048, 4096, 8192, 16384, 32768, 65536])
    ap.add_argument("--rule-batches", type=int, nargs="*", default=[1, 8, 64, 256])
    ap.add_argument("--rule-chunks", type=int, nargs="*", default=[1024, 2048, 4096, 8192, 16384])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip", nargs="*", default=[], choices=["shapes", "rule", "degenerate", "resample"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_downsample.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_voxel_downsample needs a GPU"
    rows = []
    if "rule" not in a.skip:
        for n in a.rule_sizes:
            for B in a.rule_batches:
                rows.append(case("rule", n, B, 0.1, a.rule_chunks, a, with_torch=False))
    if "shapes" not in a.skip:
        for n in a.sizes:
            for B in a.batches:
                for cell in a.cells:
                    rows.append(case("shapes", n, B, cell, a.chunk, a))
    if "degenerate" not in a.skip:
        n = 480000
        pts = torch.rand(n, 3, device="cuda", generator=torch.Generator("cuda").manual_seed(5)) * 0.04 + torch.tensor([7.01, 0.01, 0.01], device="cuda")
        rows.append(case("degenerate", n, 1, 0.1, a.chunk, a, points=pts))
        assert rows[-1]["voxels"] == 1
    if "resample" not in a.skip:
        rows.append(resample_case(a))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
