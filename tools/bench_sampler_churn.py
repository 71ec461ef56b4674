#!/usr/bin/env python3
"""Times the 18-step sampler of the shipped 24-block denoiser with and without churn, at B in --batches, three
calls alternating in one process on the same condition cache and initial latents:

  det     S_churn = 0                          the deterministic sampler (35 NFEs)
  host    the paper's churn values, rng='host'  per-sample CPU generators draw one [512, 32] block per step and sample (the reference's
                                                streams), the churned steps' draws are stacked and copied to the device, then the
                                                sampler runs - the draw and the copy are inside the timed window
  device  the paper's churn values, seeds       the noise is generated inside the churn kernel; nothing is drawn or copied

Host clock around each call, ending in a device synchronise (the host draw is CPU work: device events would not see it).  Every
repetition runs all the modes, in an order that rotates.  Prints one JSON line per B (median, minimum and maximum in ms and the
overheads over `det`); --out PATH also writes them there.  --package-root PATH imports rald_amd from another checkout (with
--modes det: the deterministic sampler of an older commit, on the same box, in the same call).  Run it under `timeout`."""
import argparse
import json
import os
import statistics
import sys
import time

CHURN = dict(S_churn=40, S_min=0.05, S_max=50, S_noise=1.003)


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--modes", nargs="+", default=["det", "host", "device"], choices=["det", "host", "device"])
    ap.add_argument("--depth", type=int, default=24)
    ap.add_argument("--steps", type=int, default=18)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
    import torch
    from rald_amd import config, models_radar_generation as G, synth, weights
    assert torch.cuda.is_available(), "bench_sampler_churn needs a GPU"
    m = G.EDMPrecond(n_latents=512, channels=32, depth=a.depth, configs=config.shipped_generation_config())
    m.load_state_dict(weights.make_state_dict(weights.dit_spec(depth=a.depth), 0), strict=True)
    m = m.cuda()
    h = m._handle()
    rows = []
    with torch.no_grad():
        for B in a.batches:
            cube = synth.radar_cube(1).cuda().expand(B, -1, -1, -1, -1).contiguous()
            _, cache = h.encode_cond(cube, want_tokens=False)
            seed_list = list(range(B))
            latents = synth.latents(seed_list).cuda()
            seeds = torch.tensor(seed_list, dtype=torch.int64).cuda()
            copied = {}

            def det():
                return h.sample(latents, cache, a.steps)

            def host():
                rnd = G.StackedRandomGenerator(latents.device, seed_list)
                churn = G._churn_inputs(rnd.randn_like, latents, a.steps, 0.002, 80.0, 7.0, **CHURN)
                copied["bytes"] = churn["noise"].numel() * 4
                return h.sample(latents, cache, a.steps, **churn)

            def device():
                return h.sample(latents, cache, a.steps, seeds=seeds, **CHURN)
            calls = {k: v for k, v in (("det", det), ("host", host), ("device", device)) if k in a.modes}
            names = list(calls)
            times = {k: [] for k in names}
            for rep in range(a.warmup + a.reps):
                r = rep % len(names)
                for k in names[r:] + names[:r]:                  # the order rotates, so no mode always follows the same one
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = calls[k]()
                    torch.cuda.synchronize()
                    ms = (time.perf_counter() - t0) * 1e3
                    assert torch.isfinite(out).all()
                    if rep >= a.warmup:
                        times[k].append(ms)
            row = {"label": a.label, "B": B, "depth": a.depth, "num_steps": a.steps, "reps": a.reps, "graph_replay": B <= 16,
                   **{k: stats(v) for k, v in times.items()}, "device_name": torch.cuda.get_device_name(0)}
            if "det" in times:
                base = statistics.median(times["det"])
                for k in names:
                    if k != "det":
                        row[f"{k}_overhead_ms"] = round(statistics.median(times[k]) - base, 3)
                        row[f"{k}_over_det"] = round(statistics.median(times[k]) / base, 4)
            if "host" in times:
                row["host_noise_bytes_copied"] = copied["bytes"]
            print(json.dumps(row), flush=True)
            rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
