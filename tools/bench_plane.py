#!/usr/bin/env python3
"""Times the RANSAC plane segmentation per call against the radius outlier filter on the same cloud, in the
cartesian box of section 14 ([0, 15.8] x [-15.8, 15.8] x [-5.4, 5.4] m), these calls in one process:

  H<h>_K<k>_r<0|1>  postprocess.segment_planes_ragged(threshold = --threshold, num_hypotheses = h, max_planes = k, refine) for h in 256,
                    1024, k in 1, 3, refine off and on: per round the compaction of the live rows, the hypotheses, the scoring
                    kernel rows x hypotheses, the argmax, the marks and fits, the labels
  remove            postprocess.remove_planes_ragged at H = 1024, K = 1, refine on, with index and labels
  radius_filter     the yardstick: postprocess.remove_radius_outliers_ragged(radius = --radius, min_neighbors = 4)

Clouds: `frames` (8 uniform clouds of 45 000 rows) and `uniform` (one of 480 000 rows) of tools/bench_cluster.py, and `ground` (480 000
rows: 40 % within 2 cm of the plane z = -1.5 m, the others uniform in the box).  Device events around every call, --warmup warm-ups,
then --reps repetitions in which the compared calls alternate in rotating order; median, minimum and maximum in ms and each call's
median over the yardstick's.  `score_768h_ms` is the median of H = 1024 less that of H = 256 at K = 1 without refine - 768 hypotheses
of pln_score, the only launch whose work grows with H beside the one-lane-per-hypothesis kernels - and `score_gflops` the fp32 rate
that gives at 11 operations per (row, hypothesis).  Prints one JSON line per case and writes them all to --out (default
profiles/plane.json) beside the per-kernel resources the compiler reports (--resources, a JSON file, is copied in when given).  Run it
under `timeout`."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from bench_radius_filter import HI, LO, stats, time_calls, uniform  # noqa: E402
from rald_amd import postprocess as PP  # noqa: E402

OPS_PER_PAIR = 11                                                        # 3 subtracts, 3 multiplies, 2 adds, 1 square, 1 compare, 1 count


def ground(n, seed):
    """40 % of the rows within 2 cm of z = -1.5 m, the others uniform in the box, in random order."""
    pts = uniform(1, n, seed)
    gen = torch.Generator("cuda").manual_seed(seed + 1)
    on = torch.rand(n, device="cuda", generator=gen) < 0.4
    pts[on, 2] = -1.5 + (torch.rand(int(on.sum()), device="cuda", generator=gen) - 0.5) * 0.04
    return pts


def case(section, pts, n, B, a):
    grid = PP.voxel_grid(LO, HI, a.radius)
    off = torch.arange(B + 1, device="cuda", dtype=torch.int64) * n
    t = a.threshold
    calls = {f"H{h}_K{k}_r{r}": (lambda h=h, k=k, r=r: PP.segment_planes_ragged(pts, off, t, n, num_hypotheses=h, max_planes=k, refine=bool(r)))
             for h in (256, 1024) for k in (1, 3) for r in (0, 1)}
    calls["remove"] = lambda: PP.remove_planes_ragged(pts, off, t, n, num_hypotheses=1024, return_index=True, return_labels=True)
    calls["radius_filter"] = lambda: PP.remove_radius_outliers_ragged(pts, off, a.radius, 4, grid, n)
    times, out = time_calls(calls, a.warmup, a.reps)
    med = {name: statistics.median(v) for name, v in times.items()}
    score = med["H1024_K1_r0"] - med["H256_K1_r0"]
    row = {"section": section, "n": n, "B": B, "threshold_m": t, "radius_m": a.radius, "reps": a.reps,
           "num_planes_H1024_K3_r1": out["H1024_K3_r1"][2].tolist(), "inliers_H1024_K3_r1": out["H1024_K3_r1"][3].tolist(),
           "kept_remove": int(out["remove"][1][-1].item()), "kept_radius_filter": int(out["radius_filter"][1][-1].item()),
           **{name: stats(v) for name, v in times.items()},
           **{name + "_over_radius_filter": round(med[name] / med["radius_filter"], 3) for name in calls if name != "radius_filter"},
           "score_768h_ms": round(score, 4),
           "score_gflops": round(OPS_PER_PAIR * 768.0 * n * B / (score * 1e6), 1) if score > 0 else None,
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--radius", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip", nargs="*", default=[], choices=["frames", "uniform", "ground"])
    ap.add_argument("--resources", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plane.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_plane needs a GPU"
    clouds = {"frames": lambda: (uniform(8, 45000, 1008), 45000, 8), "uniform": lambda: (uniform(1, 480000, 1001), 480000, 1),
              "ground": lambda: (ground(480000, 9), 480000, 1)}
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
