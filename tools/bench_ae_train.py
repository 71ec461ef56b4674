"""Time one autoencoder training iteration (stage 1, engine_ae.py:33-104) through the autograd route: KLAutoEncoder.forward in train()
mode + the reference's loss + backward, and the same with a torch.optim.AdamW step.  Shipped shape: kl_d512_m512_l32_mix, depth 24,
N = Q = 10 000 points / queries (point_cloud_size, num_samples), B = 1 and 4 (batch_size in ae_indoor_cfg_aniso_mix_view_cone.yml).

    python tools/bench_ae_train.py [--batches 1 4] [--iters 5] [--warmup 2] [--depth 24] [--points 10000]

Prints one JSON line per batch size: ms per iteration (device events after warm-up), peak memory, and the achieved rate against the
FLOP count of the shapes (forward: latent stack 2*M*(4*512*512 + 2*M*512 + 3*512*2048)*depth... see flops()).

    python tools/bench_ae_train.py --route autograd step graph [--repeats 3] ...

compares the routes of the whole iteration in one process: ``autograd`` (the route above with the reference's loop around it: BCE, clip,
torch.optim.AdamW, the Python EMA loop), ``step`` (train_ae.AeStepTrainer on FlatAdamW storage) and ``graph`` (train_ae.GraphedAeStep).
Every route runs the full iteration including the optimizer, the EMA and the loop's one host read of the loss; the routes alternate over
``--repeats`` rounds of ``--iters`` timed iterations.  One JSON line per route and batch: the median ms per iteration, the min - max
spread over the rounds, the route's peak memory (its own model, optimizer state and activations) and the achieved rate."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def flops(B, N, Q, depth, M=512, D=512):
    """Forward multiply-add FLOPs (2 per MAC) of the products; backward counted as 2x forward."""
    lin = lambda rows, k, n: 2 * rows * k * n
    ff = lambda rows: lin(rows, D, 8 * D) + lin(rows, 4 * D, D)
    stack = depth * (lin(M, D, 3 * D) + 2 * 2 * M * M * D + lin(M, D, D) + ff(M))
    attn = lambda nq, nk: lin(nq, D, D) + lin(nk, D, 2 * D) + 2 * 2 * nq * nk * D + lin(nq, D, D)
    enc = lin(N, 64, D) + attn(M, N) + lin(M, D, D) + attn(M, N) + ff(M)
    dec = lin(Q, 64, D) + attn(Q, M)
    fwd = B * (stack + enc + dec)
    return fwd, 3 * fwd


def _model(a):
    from rald_amd import models_ae as A, weights
    m = A.KLAutoEncoder(depth=a.depth, dim=512, queries_dim=512, output_dim=1, num_inputs=a.points, num_latents=512, latent_dim=32,
                        heads=8, dim_head=64, query_type="mix")
    m.load_state_dict(weights.make_state_dict(weights.spec_of_state_dict(m.state_dict()), 0), strict=True)
    return m.cuda().train()


def _autograd_iteration(a, pc, q, labels, n_in):
    """The reference's loop body (engine_ae.py:55-116) around the autograd route."""
    import copy
    m = _model(a)
    opt = torch.optim.AdamW(m.parameters(), lr=1e-6)
    ema = copy.deepcopy(list(m.parameters()))
    crit = torch.nn.BCEWithLogitsLoss()
    B = pc.shape[0]

    def it():
        out = m(pc, q)
        loss = crit(out["logits"][:, :n_in], labels[:, :n_in]) + 0.1 * crit(out["logits"][:, n_in:], labels[:, n_in:]) \
            + 1e-3 * out["kl"].sum() / B
        value = loss.item()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(m.parameters(), 10.0)
        opt.step()
        with torch.no_grad():
            for t, s in zip(ema, m.parameters()):
                t.detach().mul_(0.999).add_(s, alpha=1 - 0.999)
        return value
    return it


def _step_iteration(a, pc, q, labels, n_in, graph):
    from rald_amd.train_ae import AeStepTrainer, GraphedAeStep
    from rald_amd.train_utils import FlatAdamW
    m = _model(a)
    st = AeStepTrainer(m, FlatAdamW(m.parameters(), lr=1e-6, ema=True))
    run = GraphedAeStep(st, pc.shape[0], a.points, a.points) if graph else st.step

    def it():
        losses, _, _ = run(pc, q, labels, n_in, max_norm=10.0)
        return losses.tolist()[0]                                  # the loop's one host read (engine_ae.train_one_epoch)
    return it


def compare_routes(a):
    """The chosen routes alternately, ``a.repeats`` rounds of ``a.iters`` timed iterations each, per batch size."""
    from rald_amd import synth
    for B in a.batches:
        pc, q = synth.point_cloud(B, a.points).cuda(), synth.queries(B, a.points).cuda()
        labels = (torch.rand(B, a.points, generator=torch.Generator().manual_seed(0)) < 0.3).float().cuda()
        n_in = a.points * 15 // 16
        its, own, peak = {}, {}, {}
        for r in a.route:                                          # build + warm up; what a route keeps and its peak above the others' memory
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            its[r] = _autograd_iteration(a, pc, q, labels, n_in) if r == "autograd" else _step_iteration(a, pc, q, labels, n_in, r == "graph")
            for _ in range(a.warmup):
                its[r]()
            torch.cuda.synchronize()
            peak[r] = torch.cuda.max_memory_allocated() - base
            own[r] = torch.cuda.memory_allocated() - base
        ms = {r: [] for r in a.route}
        for _ in range(a.repeats):
            for r in a.route:
                its[r]()
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated() - own[r]
                torch.cuda.reset_peak_memory_stats()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    value = its[r]()
                e1.record()
                torch.cuda.synchronize()
                ms[r].append(e0.elapsed_time(e1) / a.iters)
                peak[r] = max(peak[r], torch.cuda.max_memory_allocated() - base)
                assert value == value, f"route {r}: the loss is NaN"
        _, total = flops(B, a.points, a.points, a.depth)
        for r in a.route:
            v = sorted(ms[r])
            mid = v[len(v) // 2]
            res = dict(route=r, B=B, N=a.points, Q=a.points, depth=a.depth, ms_iteration=mid, ms_min=v[0], ms_max=v[-1], spread_ms=v[-1] - v[0],
                       repeats=a.repeats, iters=a.iters, peak_GiB=peak[r] / 2 ** 30, iter_GFLOP=total / 1e9,
                       TFLOPs_achieved=total / (mid * 1e-3) / 1e12)
            print(json.dumps({k: (round(v_, 3) if isinstance(v_, float) else v_) for k, v_ in res.items()}), flush=True)
        del its
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--depth", type=int, default=24)
    ap.add_argument("--points", type=int, default=10000)
    ap.add_argument("--route", nargs="+", choices=["autograd", "step", "graph"], default=["autograd"])
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if a.route != ["autograd"]:
        if a.repeats < 3:
            ap.error("--repeats must be at least 3: the spread is the yardstick")
        return compare_routes(a)
    from rald_amd import synth
    m = _model(a)
    opt = torch.optim.AdamW(m.parameters(), lr=1e-6)
    crit = torch.nn.BCEWithLogitsLoss()
    for B in a.batches:
        pc, q = synth.point_cloud(B, a.points).cuda(), synth.queries(B, a.points).cuda()
        labels = (torch.rand(B, a.points, generator=torch.Generator().manual_seed(0)) < 0.3).float().cuda()
        n_in = a.points * 15 // 16

        def it(step):
            out = m(pc, q)
            loss = crit(out["logits"][:, :n_in], labels[:, :n_in]) + 0.1 * crit(out["logits"][:, n_in:], labels[:, n_in:]) \
                + 1e-3 * out["kl"].sum() / B
            opt.zero_grad(set_to_none=True)
            loss.backward()
            if step:
                opt.step()

        res = {}
        for step in (False, True):
            for _ in range(a.warmup):
                it(step)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                it(step)
            e1.record()
            torch.cuda.synchronize()
            res["ms_fwd_bwd_adamw" if step else "ms_fwd_bwd"] = e0.elapsed_time(e1) / a.iters
            res["peak_GiB" + ("_adamw" if step else "")] = torch.cuda.max_memory_allocated() / 2 ** 30
        fwd, total = flops(B, a.points, a.points, a.depth)
        res.update(B=B, N=a.points, Q=a.points, depth=a.depth, fwd_GFLOP=fwd / 1e9, iter_GFLOP=total / 1e9,
                   TFLOPs_achieved=total / (res["ms_fwd_bwd"] * 1e-3) / 1e12)
        print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()}), flush=True)


if __name__ == "__main__":
    main()
