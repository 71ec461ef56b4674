#!/usr/bin/env python3
"""Generate tests/golden/g24_sample_churn.npz: the reference's stochastic sampler (model/models_radar_generation.py:235-275
edm_sampler with the EDM paper's churn values of its comment at :238, S_churn=40, S_min=0.05, S_max=50, S_noise=1.003) on CPU, fp32.

Needs a checkout of the reference; its root directory is the one argument.  Import stubs (timm DropPath, torch_cluster.fps) and the
name-seeded weights are those of make_golden.py.  18 steps, seeds [0, 1], rald_amd.synth.radar_cube(2); the initial latents and the
per-step `randn_like` come from the reference's own StackedRandomGenerator on the CPU, latents first, then one draw per step (:260).
The radar condition is hoisted out of the loop (bit-identical, as make_golden.py does for its long horizons).

Stored:
  sample_d2, sample_d24   edm_sampler output [2, 512, 32] of the depth-2 and the depth-24 EDMPrecond
  t_steps [19], t_hat [18] the noise levels the sampler used (what it passed through net.round_sigma, :249 and :259), float32
  churn                    (S_churn, S_min, S_max, S_noise) as float64
The noise is not stored: the same CPU generators reproduce it.

Usage:  python tests/golden/make_golden_churn.py REFERENCE_ROOT
"""
import argparse
import os
import sys
import time
import types

sys.dont_write_bytecode = True
import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from rald_amd import synth, weights  # noqa: E402

CHURN = dict(S_churn=40, S_min=0.05, S_max=50, S_noise=1.003)
NUM_STEPS = 18
SEEDS = [0, 1]


def import_reference(ref):
    class DropPath(nn.Module):
        def __init__(self, p=0.0):
            super().__init__()
            self.p = p

        def forward(self, x):
            assert (not self.training) or self.p == 0
            return x

    tl = types.ModuleType("timm.models.layers")
    tl.DropPath = DropPath
    sys.modules["timm"] = types.ModuleType("timm")
    sys.modules["timm.models"] = types.ModuleType("timm.models")
    sys.modules["timm.models.layers"] = tl
    tc = types.ModuleType("torch_cluster")

    def fps(*a, **k):
        raise NotImplementedError("torch_cluster.fps is not available (query_type='point' is out of scope)")

    tc.fps = fps
    sys.modules["torch_cluster"] = tc
    sys.path.insert(0, ref)
    from model import models_radar_generation
    return models_radar_generation


class Cfg(dict):
    __getattr__ = dict.__getitem__


CFG = Cfg(cond_type="radar", use_radar_enc=True, unfreeze_radar_enc=True,
          enc_radar_r_dim=8, enc_radar_a_dim=4, enc_radar_e_dim=2, enc_radar_ch=16,
          enc_hidden_ch=64, input_radar_r_dim=128, input_radar_a_dim=64, input_radar_e_dim=32,
          radar_token_channel=512)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference", help="root of the reference checkout (holds model/)")
    ref = os.path.abspath(ap.parse_args().reference)
    G = import_reference(ref)
    torch.set_num_threads(os.cpu_count())
    out = {"churn": np.array([CHURN[k] for k in ("S_churn", "S_min", "S_max", "S_noise")], np.float64)}
    with torch.no_grad():
        for depth in (2, 24):
            m = G.EDMPrecond(n_latents=512, channels=32, depth=depth, configs=CFG)
            spec = weights.spec_of_state_dict(m.state_dict())
            m.load_state_dict(weights.make_state_dict(spec, 0), strict=True)
            m.eval()
            cube = synth.radar_cube(2)
            cond = m.process_radar_cond(cube)
            m.process_radar_cond = lambda c, _cond=cond: _cond
            seen = []
            m.round_sigma = lambda s, _seen=seen: (_seen.append(torch.as_tensor(s).clone()), torch.as_tensor(s))[1]
            rnd = G.StackedRandomGenerator(torch.device("cpu"), SEEDS)
            latents = rnd.randn([2, m.n_latents, m.channels], device=torch.device("cpu"))
            t0 = time.time()
            s = G.edm_sampler(m, latents, cube, "radar", randn_like=rnd.randn_like, num_steps=NUM_STEPS, **CHURN).to(torch.float32)
            print(f"  reference edm_sampler depth {depth}, churn {CHURN}: {time.time() - t0:.0f}s")
            t_steps = torch.cat([seen[0], torch.zeros_like(seen[0][:1])]).numpy()
            t_hat = torch.stack(seen[1:]).numpy()
            assert t_steps.shape == (NUM_STEPS + 1,) and t_hat.shape == (NUM_STEPS,) and t_hat.dtype == np.float32
            if "t_steps" in out:
                assert np.array_equal(out["t_steps"], t_steps) and np.array_equal(out["t_hat"], t_hat)
            out["t_steps"], out["t_hat"] = t_steps, t_hat
            out[f"sample_d{depth}"] = s.numpy()
            del m
    print("  churned steps:", [int(i) for i in np.nonzero(out["t_hat"] != out["t_steps"][:-1])[0]])
    path = os.path.join(HERE, "g24_sample_churn.npz")
    np.savez_compressed(path, **out)
    print(f"  wrote g24_sample_churn.npz  ({os.path.getsize(path) / 1024:.0f} KB)")


if __name__ == "__main__":
    main()
