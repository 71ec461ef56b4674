#!/usr/bin/env python3
"""Times the gradient decoder next to the plain streaming decoder it extends, on the flagship decoder shape
(dim 512, 512 latents) and one decoder context, three calls alternating in one process on the same queries:

  (a) decode_queries[_ragged]                       the plain kernel: its time must be what it was before the gradient kernel existed
  (b) decode_queries_grad[_ragged]                  logit + gradient
  (c) decode_queries_grad[_ragged], project=True    logit + gradient + one Newton step

for Q = 1.2 M and 100 k queries at B = 1 (dense), and B = 8 ragged (segments of 0.5 .. 1.5 times --ragged queries).  Device events
around every call after --warmup repetitions; every repetition runs all three in an order that rotates.  The latent stack has depth 1:
it is not timed, the context it writes has the flagship layout.  Prints one JSON line per shape (median, minimum and maximum in ms,
and the ratios to (a)); --out PATH also writes them there (profiles/decode_grad.json).  There is no time gate.  Run it under `timeout`."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from rald_amd import models_ae as A, synth, weights  # noqa: E402


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
    ap.add_argument("--dense", type=int, nargs="+", default=[1200000, 100000])
    ap.add_argument("--ragged", type=int, default=100000)
    ap.add_argument("--ragged-batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_decode_grad needs a GPU"
    m = A.KLAutoEncoder(depth=1, dim=512, queries_dim=512, num_latents=512, latent_dim=32, num_inputs=1000, query_type="mix")
    m.load_state_dict(weights.make_state_dict(weights.spec_of_state_dict(m.state_dict()), 0), strict=True)
    m = m.cuda().eval()
    h = m._handle()
    gen = torch.Generator("cuda").manual_seed(7)
    shapes = [("dense", 1, Q) for Q in a.dense] + [("ragged", a.ragged_batch, a.ragged)]
    rows = []
    for kind, B, Q in shapes:
        z = synth.latents(range(B)).contiguous().cuda()
        ctx = h.decode_latents(z)
        if kind == "dense":
            q = torch.rand(B, Q, 3, device="cuda", generator=gen) * 2 - 1
            total = B * Q
            calls = {"a_plain": lambda: h.decode_queries(ctx, q),
                     "b_grad": lambda: h.decode_queries_grad(ctx, q),
                     "c_grad_projected": lambda: h.decode_queries_grad(ctx, q, project=True)}
        else:
            lengths = [int(Q * (0.5 + b / max(B - 1, 1))) for b in range(B)]
            total, longest = sum(lengths), max(lengths)
            off = torch.tensor([0] + list(torch.tensor(lengths).cumsum(0)), dtype=torch.int64, device="cuda")
            q = torch.rand(total, 3, device="cuda", generator=gen) * 2 - 1
            calls = {"a_plain": lambda: h.decode_queries_ragged(ctx, q, off, longest),
                     "b_grad": lambda: h.decode_queries_grad_ragged(ctx, q, off, longest),
                     "c_grad_projected": lambda: h.decode_queries_grad_ragged(ctx, q, off, longest, project=True)}
        times = {k: [] for k in calls}
        names = list(calls)
        for rep in range(a.warmup + a.reps):
            for k in names[rep % 3:] + names[:rep % 3]:              # the order rotates, so no call always follows the same one
                ms = event_ms(calls[k])
                if rep >= a.warmup:
                    times[k].append(ms)
        plain, grad = calls["a_plain"](), calls["b_grad"]()
        med = {k: statistics.median(v) for k, v in times.items()}
        row = {"layout": kind, "B": B, "queries": total, "reps": a.reps, **{k: stats(v) for k, v in times.items()},
               "b_over_a": round(med["b_grad"] / med["a_plain"], 3), "c_over_a": round(med["c_grad_projected"] / med["a_plain"], 3),
               "grad_Mq_per_s": round(total / med["b_grad"] / 1e3, 1), "logits_equal": bool(torch.equal(plain.reshape(-1), grad[0].reshape(-1))),
               "device": torch.cuda.get_device_name(0)}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del q
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
