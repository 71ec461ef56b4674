#!/usr/bin/env python3
"""Times ICP registration per call against its two yardsticks on the same target, in the cartesian box of
section 14 ([0, 15.8] x [-15.8, 15.8] x [-5.4, 5.4] m), these calls in one process:

  <src>_<mode>_i<k>  postprocess.register_icp_ragged(max_distance = --radius, tolerance = 0, max_iterations = k) for the source `small`
                     (the first 10 000 rows of every cloud) and `full` (every row), both the target moved by --degrees about z and
                     --shift m, mode point and plane (the target's normals are estimated once, outside the timing), k = 1 and 30: the
                     target's index, then k + 1 times the move and the radius walk, the 29 block sums and the solve
  index              the target's index on its own: the same call with a source of ONE row per cloud and one iteration - the index
                     build plus seven launches of one workgroup each
  radius_filter      yardstick 1: postprocess.remove_radius_outliers_ragged(radius = --radius, min_neighbors = 4) on the target
  nn_<src>           yardstick 2: postprocess.nearest_neighbors_ragged(source -> target), the exact brute-force search that one
                     iteration's correspondence replaces (--nn-reps repetitions: it is slow)

Clouds: `frames` (8 uniform clouds of 45 000 rows) and `uniform` (one of 480 000 rows) of tools/bench_cluster.py.  Device events
around every call, --warmup warm-ups, then --reps repetitions in which the compared calls alternate in rotating order; median, minimum
and maximum in ms.  `<src>_<mode>_per_iteration_ms` is (median of 30 iterations - median of 1) / 29, and its ratios to both yardsticks
follow.  Prints one JSON line per case and writes them all to --out (default profiles/icp.json) beside the per-kernel resources the
compiler reports (--resources, a JSON file, is copied in when given).  Run it under `timeout`."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from bench_radius_filter import HI, LO, stats, time_calls, uniform  # noqa: E402
from rald_amd import postprocess as PP  # noqa: E402


def moved_copy(pts, degrees, shift):
    """The target rotated about z through the box's centre and shifted along (1, 1, 0) / sqrt 2, in float64, rounded to fp32."""
    c, s = math.cos(math.radians(degrees)), math.sin(math.radians(degrees))
    R = torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], device="cuda", dtype=torch.float64)
    centre = torch.tensor([(l + h) / 2 for l, h in zip(LO, HI)], device="cuda", dtype=torch.float64)
    t = torch.tensor([shift / math.sqrt(2), shift / math.sqrt(2), 0.0], device="cuda", dtype=torch.float64)
    return ((pts.double() - centre) @ R.T + centre + t).float()


def case(section, tgt, n, B, a):
    r = a.radius
    grid = PP.voxel_grid(LO, HI, r)
    t_off = torch.arange(B + 1, device="cuda", dtype=torch.int64) * n
    nrm = PP.estimate_normals_ragged(tgt, t_off, 8, PP._knn_grid(LO, HI, n, 8), n, view=(0.0, 0.0, 0.0))
    full = moved_copy(tgt, a.degrees, a.shift)
    m = min(10000, n)
    small = full.reshape(B, n, 3)[:, :m].reshape(-1, 3).contiguous()
    sources = {"small": (small, torch.arange(B + 1, device="cuda", dtype=torch.int64) * m, m), "full": (full, t_off, n)}
    calls = {}
    for sname, (src, s_off, ms) in sources.items():
        for mode in ("point", "plane"):
            for k in (1, 30):
                calls[f"{sname}_{mode}_i{k}"] = (lambda src=src, s_off=s_off, ms=ms, mode=mode, k=k: PP.register_icp_ragged(
                    src, s_off, tgt, t_off, r, grid, ms, n, target_normals=nrm if mode == "plane" else None, mode=mode, max_iterations=k,
                    tolerance=0.0))
    one, one_off = full.reshape(B, n, 3)[:, :1].reshape(-1, 3).contiguous(), torch.arange(B + 1, device="cuda", dtype=torch.int64)
    calls["index"] = lambda: PP.register_icp_ragged(one, one_off, tgt, t_off, r, grid, 1, n, mode="point", max_iterations=1, tolerance=0.0)
    calls["radius_filter"] = lambda: PP.remove_radius_outliers_ragged(tgt, t_off, r, 4, grid, n)
    times, out = time_calls(calls, a.warmup, a.reps)
    nn = {f"nn_{sname}": (lambda src=src, s_off=s_off, ms=ms: PP.nearest_neighbors_ragged(src, s_off, tgt, t_off, ms, n))
          for sname, (src, s_off, ms) in sources.items()}
    nn_times, _ = time_calls(nn, 1, a.nn_reps)
    times.update(nn_times)
    med = {name: statistics.median(v) for name, v in times.items()}
    row = {"section": section, "n": n, "B": B, "source_small": m, "max_distance_m": r, "degrees": a.degrees, "shift_m": a.shift, "reps": a.reps,
           "nn_reps": a.nn_reps, **{name: stats(v) for name, v in times.items()}}
    for sname in sources:
        for mode in ("point", "plane"):
            per = (med[f"{sname}_{mode}_i30"] - med[f"{sname}_{mode}_i1"]) / 29.0
            res = out[f"{sname}_{mode}_i30"]
            row.update({f"{sname}_{mode}_per_iteration_ms": round(per, 4),
                        f"{sname}_{mode}_per_iteration_over_radius_filter": round(per / med["radius_filter"], 3),
                        f"{sname}_{mode}_per_iteration_over_nn": round(per / med[f"nn_{sname}"], 5),
                        f"{sname}_{mode}_fitness": [round(v, 4) for v in res["fitness"].tolist()],
                        f"{sname}_{mode}_status": res["status"].tolist(), f"{sname}_{mode}_step": res["step"].tolist()})
    row["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--radius", type=float, default=0.1)
    ap.add_argument("--degrees", type=float, default=0.1)
    ap.add_argument("--shift", type=float, default=0.02)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--nn-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip", nargs="*", default=[], choices=["frames", "uniform"])
    ap.add_argument("--resources", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_icp needs a GPU"
    clouds = {"frames": lambda: (uniform(8, 45000, 1008), 45000, 8), "uniform": lambda: (uniform(1, 480000, 1001), 480000, 1)}
    rows = []
    for section, make in clouds.items():
        if section in a.skip:
            continue
        pts, n, B = make()
        rows.append(case(section, pts, n, B, a))
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
