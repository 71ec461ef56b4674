#!/usr/bin/env python3
"""Times the first-return beam scan on the flagship decoder shape (dim 512, 512 latents, depth-1 latent stack: it
is not timed) for a 64 x 1024 beam grid, S = 256 march steps and 8 bisection steps, at B = 1 and B = 8, three legs alternating in one
process on the same decoder context:

  (a) cast_rays                     the fused launch
  (b) composition                   what a user would write without it: per step a torch axpy for the sample points, decode_queries, and the
                                    first-hit bookkeeping in torch; S + 1 + n_refine times, no early exit (that would need a host read)
  (c) decode_queries                the plain decoder on B * R * (S + 1 + n_refine) points in one call: the per-point rate to approach

The context is a synthetic sample (seeded weights and latents) whose output bias is moved so that about half of the beams return; the
hit shares are recorded, and so are the points the fused launch really evaluates (a wave stops marching when its 64 beams have all
returned and skips the bisection when none crossed between two samples).  Device events around every call after --warmup repetitions.
A side column compares the scan with infer_point_clouds on the same latents against a synthetic surface (Chamfer, F-score): it
records, it does not gate.  Prints one JSON line per batch size; --out PATH also writes them (profiles/ray_scan.json).  Run it under
`timeout`."""
import argparse
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from rald_amd import engine_generation as E, models_ae as A, query_points as QP, synth, weights  # noqa: E402

PC_RANGE = [0, -90, -20, 15.8, 90, 20]


def _ns(**kw):
    return types.SimpleNamespace(**kw)


def event_ms(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def build(shift):
    m = A.KLAutoEncoder(depth=1, dim=512, queries_dim=512, num_latents=512, latent_dim=32, num_inputs=1000, query_type="mix")
    sd = weights.make_state_dict(weights.spec_of_state_dict(m.state_dict()), 0)
    sd["to_outputs.bias"] = sd["to_outputs.bias"] - shift
    m.load_state_dict(sd, strict=True)
    return m.cuda().eval()


def composition(h, ctx, B, o, d, S, n_refine):
    """cast_rays' rule from decode_queries and torch: one axpy, one decode and the bookkeeping per step"""
    dev = o.device
    oo, dd = o.expand(B, -1, -1), d.expand(B, -1, -1)
    R = o.shape[-2]
    step = torch.full((B, R), -1, dtype=torch.int32, device=dev)
    lo, hi = torch.zeros(B, R, device=dev), torch.zeros(B, R, device=dev)
    lh = torch.full((B, R), float("nan"), device=dev)
    t_prev = 0.0
    for k in range(S + 1):
        t = k / S
        lg = h.decode_queries(ctx, torch.addcmul(oo, dd, torch.tensor(t, device=dev)))
        new = (step < 0) & (lg > 0)
        step = torch.where(new, torch.full_like(step, k), step)
        hi = torch.where(new, torch.full_like(hi, t), hi)
        lo = torch.where(new, torch.full_like(lo, t_prev), lo)
        lh = torch.where(new, lg, lh)
        t_prev = t
    cross = step >= 1
    for _ in range(n_refine):
        te = torch.where(cross, 0.5 * (lo + hi), torch.where(step == 0, hi, torch.ones_like(hi)))
        lg = h.decode_queries(ctx, torch.addcmul(oo, dd, te[..., None]))
        pos = lg > 0
        hi = torch.where(cross & pos, te, hi)
        lh = torch.where(cross & pos, lg, lh)
        lo = torch.where(cross & ~pos, te, lo)
    return torch.where(step >= 0, hi, torch.full_like(hi, -1.0)), lh, step


def evaluated_points(step, S, n_refine):
    """the points the fused launch evaluates: per 64-beam chunk of a sample, the samples up to the last first return (all S + 1 when a beam
    has none) + the bisection steps when a beam of the chunk crossed between two samples"""
    B, R = step.shape
    pad = (-R) % 64
    if pad:
        step = torch.cat([step, step[:, -1:].expand(B, pad)], dim=1)                         # the tail chunk repeats the last beam
    c = step.view(B, -1, 64)
    marched = torch.where((c >= 0).all(-1), c.max(-1).values + 1, torch.full_like(c[..., 0], S + 1))
    refined = (c >= 1).any(-1).int() * n_refine
    return int(((marched + refined) * 64).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-az", type=int, default=1024)
    ap.add_argument("--n-el", type=int, default=64)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--refine", type=int, default=8)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ray_scan needs a GPU"
    S, n_refine = a.steps, a.refine
    args = _ns(eval=_ns(inference=_ns(num_query_points=1200000, refine_query=False, query_helper=False), use_cart_query=False,
                        skip_eval_metric=False),
               dataset=_ns(lidar=_ns(pc_range=PC_RANGE, pc_range_cart=[0, -15.8, -5.4, 15.8, 15.8, 5.4], voxel_size=[0.05, 0.25, 0.5],
                                     norm_anisotropy=True, norm_isotropy=False, view_cone_mode=True)))
    az, el = QP.beam_grid(-90.0, 90.0, a.n_az, -20.0, 20.0, a.n_el)
    o, d = QP.beam_segments(args, az, el)
    R = o.shape[0]
    # the bias shift: the median over a probe of 4096 beams of the largest logit along the beam (33 samples), on the largest batch
    zs = synth.latents(range(max(a.batches))).contiguous().cuda()
    probe = build(0.0)
    sel = torch.randperm(R, generator=torch.Generator().manual_seed(1))[:4096].cuda()
    top = torch.stack([probe.decode(zs[:1], (o[sel] + (k / 32) * d[sel])[None]).reshape(-1) for k in range(33)]).max(0).values
    m = build(float(top.median()))
    del probe
    h = m._handle()
    rows = []
    for B in a.batches:
        z = zs[:B].contiguous()
        ctx = h.decode_latents(z)
        n_upper = B * R * (S + 1 + n_refine)
        flat = torch.rand(B, R * (S + 1 + n_refine), 3, device="cuda", generator=torch.Generator("cuda").manual_seed(7)) * 2 - 1
        calls = {"a_fused": lambda: h.cast_rays(ctx, B, o, d, S, n_refine),
                 "b_composition": lambda: composition(h, ctx, B, o, d, S, n_refine),
                 "c_plain_decode": lambda: h.decode_queries(ctx, flat)}
        times = {k: [] for k in calls}
        names = list(calls)
        for rep in range(a.warmup + a.reps):
            for k in names[rep % 3:] + names[:rep % 3]:              # the order rotates, so no call always follows the same one
                ms = event_ms(calls[k])
                if rep >= a.warmup:
                    times[k].append(ms)
        t, lg, step, _ = calls["a_fused"]()
        tc, _, sc = calls["b_composition"]()
        n_eval = evaluated_points(step, S, n_refine)
        med = {k: statistics.median(v) for k, v in times.items()}
        row = {"B": B, "beams": R, "n_steps": S, "n_refine": n_refine, "reps": a.reps,
               "hit_share": round(float((step >= 0).float().mean()), 4), "hit_at_0_share": round(float((step == 0).float().mean()), 4),
               "points_upper_bound": n_upper, "points_evaluated_fused": n_eval, **{k: stats(v) for k, v in times.items()},
               "fused_Mpoints_per_s_evaluated": round(n_eval / med["a_fused"] / 1e3, 1),
               "composition_Mpoints_per_s": round(n_upper / med["b_composition"] / 1e3, 1),
               "plain_Mpoints_per_s": round(n_upper / med["c_plain_decode"] / 1e3, 1),
               "b_over_a": round(med["b_composition"] / med["a_fused"], 3), "c_over_a": round(med["c_plain_decode"] / med["a_fused"], 3),
               # the composition's t_k and axpy are torch's (a double k / S rounded once, a fused multiply-add), so a few beams may differ
               "composition_steps_equal_share": round(float((sc == step).float().mean()), 6),
               "composition_t_max_abs_diff": float((tc - t).abs().max()),
               "device": torch.cuda.get_device_name(0)}
        if B == a.batches[0]:
            # side column: the scan and the thresholded volume of infer_point_clouds on the same latents, against a synthetic surface
            surf = synth.structured_cloud(B, 4096).cuda().clamp(-1, 1)
            taus = (0.1, 0.5)
            scan = E.scan_point_clouds(m, z, args, az, el, S, n_refine, surfaces=surf, metric_thresholds=taus)
            vol = E.infer_point_clouds(m, z, args, surfaces=surf, rng=torch.Generator("cuda").manual_seed(11), metric_thresholds=taus)
            row["side_metrics"] = {"thresholds_m": list(taus),
                                   "scan": {"points": [int(p.shape[0]) for p in scan["pred"]], "cd": scan["cd"],
                                            "f_score": [f["f_score"] for f in scan["metrics"]]},
                                   "volume": {"points": [int(p.shape[0]) for p in vol["pred"]], "cd": vol["cd"],
                                              "f_score": [f["f_score"] for f in vol["metrics"]]}}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del flat
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
