#!/usr/bin/env python3
"""Times the point-cloud metrics against the Chamfer path they sit beside, on the shape of the inference tail
(section 14): --pred predicted points against --gt surface points per frame, for B in --batches frames, three calls alternating in one
process on the same clouds:

  (a) cal_metrics_ragged                                  the existing Chamfer sums (row-decomposed, double atomics)
  (b) cloud_metrics_ragged, no thresholds, no per-point   the same pair work: register-blocked, chunked over the candidates
  (c) cloud_metrics_ragged, 3 thresholds and the four per-point outputs

Device events around every call; every repetition runs all three, in an order that rotates from one repetition to the next, so
neither drift nor the call that ran just before favours one of them.  Prints one JSON line per B
(median, minimum and maximum in ms); --out PATH also writes them there.  Run it under `timeout`."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from rald_amd import postprocess as PP  # noqa: E402


def event_ms(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--pred", type=int, default=480000)
    ap.add_argument("--gt", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_cloud_metrics needs a GPU"
    taus = (0.05, 0.1, 0.2)
    rows = []
    for B in a.batches:
        gen = torch.Generator("cuda").manual_seed(100 + B)
        box = torch.tensor([15.8, 31.6, 10.8], device="cuda")
        pred = (torch.rand(B * a.pred, 3, device="cuda", generator=gen) - 0.5) * box
        gt = (torch.rand(B * a.gt, 3, device="cuda", generator=gen) - 0.5) * box
        po = torch.arange(B + 1, dtype=torch.int64, device="cuda") * a.pred
        go = torch.arange(B + 1, dtype=torch.int64, device="cuda") * a.gt
        calls = {"a_cal_metrics_ragged": lambda: PP.cal_metrics_ragged(pred, po, gt, go, a.pred, a.gt),
                 "b_cloud_metrics": lambda: PP.cloud_metrics_ragged(pred, po, gt, go, a.pred, a.gt),
                 "c_cloud_metrics_thresholds_per_point": lambda: PP.cloud_metrics_ragged(pred, po, gt, go, a.pred, a.gt, taus, per_point=True)}
        times = {k: [] for k in calls}
        names = list(calls)
        for rep in range(a.warmup + a.reps):
            for k in names[rep % 3:] + names[:rep % 3]:              # the order rotates, so no call always follows the same one
                ms = event_ms(calls[k])
                if rep >= a.warmup:
                    times[k].append(ms)
        cd_a = calls["a_cal_metrics_ragged"]()
        cd_b = calls["b_cloud_metrics"]()["cd"]
        row = {"B": B, "pred": a.pred, "gt": a.gt, "reps": a.reps, **{k: stats(v) for k, v in times.items()},
               "b_over_a": round(statistics.median(times["b_cloud_metrics"]) / statistics.median(times["a_cal_metrics_ragged"]), 4),
               "cd_max_rel_diff": float(((cd_a - cd_b).abs() / cd_a).max()), "device": torch.cuda.get_device_name(0)}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del pred, gt
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
