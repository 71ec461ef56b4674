#!/usr/bin/env python3
"""Times the inference tail behind the sampler (engine_generation.py:250-322 of the reference) on the shipped autoencoder
(rald_amd.bench_ae.build_ae, synthetic weights with the output bias moved so that ~5 % of the grid is occupied): 1.2 M grid queries
plus a synthetic helper set per frame (500 .. 3 500 points, a different size per frame), the refine pass with 500 000 queries and the
Chamfer distance against 10 000 surface points, for B in {1, 8, 64} frames, both ways on the same latents and in one process:

  (a) loop:    infer_point_cloud frame by frame (4-6 host round trips per frame)
  (b) batched: infer_point_clouds on the whole batch (ragged kernels, one host read per batch)

Both draw from a device generator.  Wall-clock per call between device synchronisations, the latent stack's context included in
both (a fresh latent tensor per repetition).  Prints one JSON line per B; --out PATH also writes them there.  Run it under `timeout`."""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from rald_amd import bench_ae, engine_generation as E, synth  # noqa: E402


def _ns(**kw):
    return types.SimpleNamespace(**kw)


def tail_args(n_grid, aug_num):
    return _ns(eval=_ns(inference=_ns(num_query_points=n_grid, refine_query=True, refine_query_aug_num=aug_num, refine_query_scale=10,
                                      query_helper=True), use_cart_query=False, skip_eval_metric=False),
               dataset=_ns(lidar=_ns(pc_range=[0, -90, -20, 15.8, 90, 20], voxel_size=[0.05, 0.25, 0.5], norm_anisotropy=True,
                                     norm_isotropy=False, view_cone_mode=True)))


def wall_ms(fn, reps, warmup):
    for i in range(warmup):
        fn(-1 - i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(reps):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--grid", type=int, default=1200000)
    ap.add_argument("--aug", type=int, default=500000)
    ap.add_argument("--surface", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_infer_tail needs a GPU"
    vae = bench_ae.build_ae().eval()
    probe = vae.decode(synth.latents([1]).cuda(), synth.queries(1, 65536, seed=5).cuda()).flatten()
    sd = vae.state_dict()
    sd["to_outputs.bias"] = sd["to_outputs.bias"] - torch.quantile(probe, 0.95)
    vae.load_state_dict(sd)
    args = tail_args(a.grid, a.aug)
    rows = []
    for B in a.batches:
        z = synth.latents(range(B)).cuda()
        helpers = [synth.queries(1, 3500, seed=200 + b)[0][:500 + (b * 977) % 3001].cuda() for b in range(B)]
        surfaces = synth.point_cloud(B, a.surface, seed=7).cuda()
        rng = torch.Generator("cuda").manual_seed(11)
        found = {}

        def loop(i):
            zz = z.clone()                                           # a new tensor object: the context is built again, as per batch of an evaluation
            out = [E.infer_point_cloud(vae, zz[b:b + 1], args, helper_points=helpers[b], surface=surfaces[b], rng=rng) for b in range(B)]
            found["loop"] = sum(o["pred"].shape[0] for o in out) / B

        def batched(i):
            out = E.infer_point_clouds(vae, z.clone(), args, helper_points=helpers, surfaces=surfaces, rng=rng)
            found["batched"] = sum(p.shape[0] for p in out["pred"]) / B
        t_loop = wall_ms(loop, a.reps, a.warmup)
        t_batch = wall_ms(batched, a.reps, a.warmup)
        row = {"B": B, "grid": a.grid, "aug": a.aug, "surface": a.surface, "loop_ms_per_frame": round(t_loop / B, 3),
               "batched_ms_per_frame": round(t_batch / B, 3), "speedup": round(t_loop / t_batch, 3),
               "points_per_frame_loop": round(found["loop"]), "points_per_frame_batched": round(found["batched"]),
               "device": torch.cuda.get_device_name(0)}
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
