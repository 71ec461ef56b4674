"""Stochastic EDM sampling (S_churn > 0), the parts that need no GPU: the host schedule of the library against the reference's recorded
noise levels (G24, tests/golden/make_golden_churn.py), the numpy restatement of the Philox generator against the published known
answers, a float restatement of the churned sampler around the oracle's fp32 denoiser against the reference's output, and
`edm_sampler`'s handling of `randn_like` with a stub in place of the module."""
import math

import numpy as np
import pytest
import torch

import churn_ref
from conftest import load_golden, rel_l2
from oracle import rald_oracle as O
from rald_amd import models_radar_generation as G, synth, weights
from rald_amd._handles import edm_schedule

CHURN = dict(S_churn=40, S_min=0.05, S_max=50, S_noise=1.003)        # the EDM paper's values (the reference's comment at :238)


@pytest.fixture(scope="module")
def g24():
    return load_golden("g24_sample_churn.npz")


def test_edm_schedule_equals_the_reference_levels_bit_for_bit(g24):
    assert [float(v) for v in g24["churn"]] == [40.0, 0.05, 50.0, 1.003]
    t, t_hat = edm_schedule(18, 0.002, 80.0, 7.0, 40.0, 0.05, 50.0)
    assert t.dtype == np.float32 and t.shape == (19,) and t_hat.shape == (18,)
    assert np.array_equal(t.view(np.uint32), g24["t_steps"].numpy().view(np.uint32))
    assert np.array_equal(t_hat.view(np.uint32), g24["t_hat"].numpy().view(np.uint32))
    churned = [i for i in range(18) if t_hat[i] != t[i]]
    assert churned == list(range(2, 15))                     # t_0 = 80 and t_1 = 57.6 lie above S_max, t_15.. below S_min
    gamma = np.float32(math.sqrt(2) - 1)
    for i in churned:                                        # gamma = sqrt(2) - 1 (40 / 18 is larger)
        assert t_hat[i] == np.float32(t[i] + np.float32(gamma * t[i]))
    t0, th0 = edm_schedule(18, 0.002, 80.0, 7.0, 0.0, 0.0, float("inf"))
    assert np.array_equal(t0, t) and np.array_equal(th0, t0[:-1])
    t1, th1 = edm_schedule(18, 0.002, 80.0, 7.0, 1.8, 0.0, float("inf"))          # gamma = S_churn / num_steps = 0.1, every step
    assert all(th1[i] == np.float32(t1[i] + np.float32(np.float32(1.8 / 18) * t1[i])) for i in range(18)) and np.all(th1 > t1[:-1])
    for bad in (1, 2049):
        with pytest.raises(RuntimeError, match="num_steps"):
            edm_schedule(bad)


def test_philox_restatement_reproduces_the_known_answers():
    out = churn_ref.philox4x32_10([0, 0, 0, 0], [0, 0])
    assert [f"{int(v):08x}" for v in out] == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    out = churn_ref.philox4x32_10([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0])
    assert [f"{int(v):08x}" for v in out] == ["d16cfe09", "94fdcceb", "5001e420", "24126ea1"]
    both = churn_ref.philox4x32_10([[0, 0, 0, 0], [0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344]], [[0, 0], [0xa4093822, 0x299f31d0]])
    assert both.shape == (2, 4) and int(both[0, 0]) == 0x6627e8d5 and int(both[1, 3]) == 0x24126ea1      # vectorised form


def test_restated_normals_have_unit_moments():
    z = churn_ref.normals([0, 7, 3], 16384, tag=1, step=5)
    assert z.shape == (3, 16384) and np.isfinite(z).all()
    mean, var = float(z.mean()), float(z.var())
    print(f"restated normals: mean {mean:.4f}, var {var:.4f}, max |z| {np.abs(z).max():.3f}")
    assert abs(mean) < 0.03 and abs(var - 1) < 0.05          # standard errors: 0.0045 and 0.0064
    assert np.abs(z).max() <= 5.77                           # sqrt(-2 ln 2^-24)
    assert not np.array_equal(z[0], z[1]) and not np.array_equal(z[0], churn_ref.normals([0], 16384, 1, 4)[0])
    assert np.array_equal(churn_ref.normals([7 + 2 ** 32], 2048, 1, 5), churn_ref.normals([7], 2048, 1, 5))


def churned_sampler_restated(denoise, latents, randn_like, num_steps=18, sigma_min=0.002, sigma_max=80.0, rho=7.0,
                             S_churn=0, S_min=0, S_max=float("inf"), S_noise=1):
    """edm_sampler :246-275 in fp32 torch, `denoise(x, sigma)` one NFE; one `randn_like` per step like the reference."""
    t = O.edm_sigma_schedule(num_steps, sigma_min, sigma_max, rho)
    x_next = latents * t[0]
    for i in range(num_steps):
        t_cur, t_next = t[i], t[i + 1]
        gamma = min(S_churn / num_steps, np.sqrt(2) - 1) if S_min <= t_cur <= S_max else 0
        t_hat = t_cur + gamma * t_cur
        x_hat = x_next + (t_hat ** 2 - t_cur ** 2).sqrt() * S_noise * randn_like(x_next)
        d_cur = (x_hat - denoise(x_hat, t_hat)) / t_hat
        x_next = x_hat + (t_next - t_hat) * d_cur
        if i < num_steps - 1:
            d_prime = (x_next - denoise(x_next, t_next)) / t_next
            x_next = x_hat + (t_next - t_hat) * (0.5 * d_cur + 0.5 * d_prime)
    return x_next


def test_restated_churned_sampler_matches_the_reference_golden(g24):
    """Validates G24 without a GPU: the reference's generators reproduce its noise (latents first, then one draw per step)."""
    sd = weights.make_state_dict(weights.dit_spec(depth=2), seed=0)
    cond = O.process_radar_cond(sd, synth.radar_cube(2))
    rnd = G.StackedRandomGenerator("cpu", [0, 1])
    latents = rnd.randn([2, 512, 32])
    assert torch.equal(latents, synth.latents([0, 1]))
    s = churned_sampler_restated(lambda x, sig: O.edm_precond(sd, x, sig, cond, depth=2), latents, rnd.randn_like, **CHURN)
    err = rel_l2(s, g24["sample_d2"])
    print("restated churned sampler vs G24 (depth 2): rel_l2", err)
    assert err < 1e-4                                        # the bound test_oracle_golden.py sets for its sampler goldens
    assert rel_l2(g24["sample_d2"], load_golden("g1_depth2.npz")["sample100"]) > 5e-2     # and G24 is not a deterministic run


class _StubNet:
    """Stands where the EDMPrecond stands in edm_sampler: records what reaches the handle."""
    sigma_min, sigma_max = 0, float("inf")

    def __init__(self):
        self.calls = []

    def _sample_from(self, *args, **kwargs):
        self.calls.append((args, kwargs))
        return args[0]


def test_edm_sampler_draws_once_per_step_and_keeps_the_churned_steps():
    net, lat, cube = _StubNet(), torch.zeros(2, 512, 32), torch.zeros(2, 1)
    draws = []

    def randn_like(x):
        assert x is lat
        draws.append(len(draws))
        return torch.full_like(x, float(len(draws) - 1))
    out = G.edm_sampler(net, lat, cube, "radar", randn_like=randn_like, **CHURN)
    assert out is lat and draws == list(range(18))           # exactly num_steps draws, in step order, churned or not
    (args, kw), = net.calls
    assert args[1] is cube and args[2:] == ("radar", 18, 0.002, 80, 7)
    assert {k: kw[k] for k in CHURN} == CHURN and "seeds" not in kw
    assert kw["noise"].shape == (13, 2, 512, 32)
    assert [float(n[0, 0, 0]) for n in kw["noise"]] == [float(i) for i in range(2, 15)]     # the churned steps' draws, in order
    # fewer steps, every one churned
    net.calls.clear(); draws.clear()
    G.edm_sampler(net, lat, cube, "radar", randn_like=randn_like, num_steps=5, S_churn=0.5)
    assert draws == list(range(5)) and net.calls[0][1]["noise"].shape[0] == 5
    # no step inside [S_min, S_max]: the draws are still consumed, nothing is kept
    net.calls.clear(); draws.clear()
    G.edm_sampler(net, lat, cube, "radar", randn_like=randn_like, num_steps=5, S_churn=3, S_min=100, S_max=200)
    assert draws == list(range(5)) and net.calls[0][1]["noise"] is None


def test_edm_sampler_refusals_and_the_unchanged_deterministic_path():
    net, lat, cube = _StubNet(), torch.zeros(1, 512, 32), torch.zeros(1, 1)

    def never(x):
        raise AssertionError("randn_like must not be consumed at S_churn=0")
    for kw in ({}, dict(S_churn=40), dict(S_churn=-1)):
        with pytest.raises(NotImplementedError):             # unconditional sampling stays unbuilt, whatever else is asked
            G.edm_sampler(net, lat, None, "radar", **kw)
    with pytest.raises(ValueError):
        G.edm_sampler(net, lat, cube, "radar", S_churn=-1)
    with pytest.raises(ValueError):
        G.edm_sampler(net, lat, cube, "radar", S_churn=1, S_noise=-0.5)
    assert net.calls == []
    G.edm_sampler(net, lat, cube, "radar", randn_like=never, num_steps=7)
    assert net.calls == [((lat, cube, "radar", 7, 0.002, 80, 7), {})]            # today's call, argument for argument
