#!/usr/bin/env python3
"""Times the surface-nets meshing per call against two yardsticks measured in the same process:

  count          the counting call of rald_post_surface_nets (NULL outputs): the sign words, the masks, the scans
  full           postprocess.extract_surface_batch with the exact capacity given: no host read
  two_call       postprocess.extract_surface_batch(capacity=None): the counting call, one host read, the allocation, the full call
  clone          the traffic yardstick: torch.clone of the same volume, one read and one write of its bytes
  decode_volume  what the extraction follows in practice: KLAutoEncoder.decode_volume of the same grid (kl_d512_m512_l32_mix with
                 seeded weights, the context memoised), timed apart with --decode-reps repetitions

Volumes on the grid over [-1, 1]^3: `sphere` (value = 0.6 - |p|, a sparse surface) and `noisy` (the same plus 0.2 x standard normal
noise: many active cells), at 128^3 and 256^3 with B = 1 and 128^3 with B = 8.  Device events around every call, --warmup warm-ups, then
--reps repetitions in which the compared calls alternate in rotating order; median, minimum and maximum in ms and each call's median
over both yardsticks'.  Prints one JSON line per case and writes them all to --out (default profiles/surface.json) beside the per-kernel
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

from bench_radius_filter import event_ms, stats, time_calls  # noqa: E402
from rald_amd import postprocess as PP, query_points as QP  # noqa: E402


def volume(kind, B, n, seed):
    lo, h, dims = QP.field_grid(n)
    p = QP.grid_queries(lo, h, dims)
    v = (0.6 - p.norm(dim=1)).view(1, n, n, n).repeat(B, 1, 1, 1)
    if kind == "noisy":
        v = v + 0.2 * torch.randn(v.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(seed))
    return v.contiguous(), lo, h, dims


def autoencoder(B):
    from rald_amd import models_ae as A, synth, weights
    m = A.kl_d512_m512_l32_mix(N=2048)
    m.load_state_dict(weights.make_state_dict(weights.spec_of_state_dict(m.state_dict()), 0), strict=True)
    return m.cuda().eval(), synth.latents(range(B)).contiguous().cuda()


def case(kind, B, n, a):
    vol, lo, h, dims = volume(kind, B, n, 7)
    iso, lo3, h3, _ = PP._surface_args(vol, 0.0, lo, h, None, 4)
    v_off, f_off = (torch.empty(B + 1, device="cuda", dtype=torch.int64) for _ in range(2))
    PP._surface_call(vol, iso, lo3, h3, None, v_off, None, f_off, None)
    V, F = int(v_off[B]), int(f_off[B])
    calls = {"count": lambda: PP._surface_call(vol, iso, lo3, h3, None, v_off, None, f_off, None),
             "full": lambda: PP.extract_surface_batch(vol, 0.0, lo, h, capacity=(V, F)),
             "two_call": lambda: PP.extract_surface_batch(vol, 0.0, lo, h),
             "clone": lambda: vol.clone()}
    times, _ = time_calls(calls, a.warmup, a.reps)
    row = {"volume": kind, "B": B, "n": n, "nodes": B * n ** 3, "volume_MiB": round(vol.numel() * 4 / 2 ** 20, 1), "vertices": V, "faces": F,
           "reps": a.reps, **{name: stats(v) for name, v in times.items()}}
    med = {name: statistics.median(v) for name, v in times.items()}
    if not a.no_decode:
        m, z = autoencoder(B)
        m.decode_volume(z, lo, h, dims)                                    # the latent stack and the context once: memoised from here on
        dec = [event_ms(lambda: m.decode_volume(z, lo, h, dims))[0] for _ in range(a.decode_reps)]
        row["decode_volume"], med["decode_volume"] = stats(dec), statistics.median(dec)
        del m, z
    for name in ("count", "full", "two_call"):
        row[name + "_over_clone"] = round(med[name] / med["clone"], 3)
        if "decode_volume" in med:
            row[name + "_over_decode_volume"] = round(med[name] / med["decode_volume"], 5)
    row["clone_GBps"] = round(2 * vol.numel() * 4 / (med["clone"] * 1e6), 1)
    row["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--decode-reps", type=int, default=3)
    ap.add_argument("--no-decode", action="store_true")
    ap.add_argument("--resources", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_surface needs a GPU"
    rows = [case(kind, B, n, a) for B, n in ((1, 128), (1, 256), (8, 128)) for kind in ("sphere", "noisy")]
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
