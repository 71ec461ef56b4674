"""Seeded synthetic inputs of the shapes the reference's data pipeline produces
(SURVEY.md §8d).  All draws come from CPU ``torch.Generator`` streams so the golden script,
the oracle tests, the GPU parity tests and bench.py see identical tensors.
"""
from __future__ import annotations

import numpy as np
import torch


def latents(batch_seeds, n_latents: int = 512, channels: int = 32) -> torch.Tensor:
    """Initial sampler noise.  The reference seeds one torch.Generator(device) per sample
    (models_radar_generation.py:297-304, :446-447); device streams are not portable across
    CPU/CUDA/HIP, so 'identical noise seeds' = the CPU generator stream, which is what the
    reference itself produces when run on CPU (SURVEY.md §8b RNG)."""
    outs = []
    for s in batch_seeds:
        g = torch.Generator("cpu").manual_seed(int(s) % (1 << 32))
        outs.append(torch.randn([n_latents, channels], generator=g, dtype=torch.float32))
    return torch.stack(outs)


def radar_cube(batch: int, seed: int = 1234, rae=(128, 64, 32)) -> torch.Tensor:
    """[B,R,A,E,2] in U[0,1): real cubes are clipped to [0,45] dB and divided by 45
    (datasets/aligned_coloradar/Coloradar_dataset.py:447-451)."""
    g = torch.Generator("cpu").manual_seed(seed)
    return torch.rand([batch, *rae, 2], generator=g, dtype=torch.float32)


def point_cloud(batch: int, n_points: int = 10000, seed: int = 2024) -> torch.Tensor:
    """[B,P,3] in U(-1,1)^3: real clouds are polar view-cone coordinates normalised per axis
    to [-1,1] (Coloradar_dataset.py:376-379)."""
    g = torch.Generator("cpu").manual_seed(seed)
    return torch.rand([batch, n_points, 3], generator=g, dtype=torch.float32) * 2 - 1


def queries(batch: int, n_queries: int, seed: int = 4242) -> torch.Tensor:
    """Decoder query points, U(-1,1)^3 (utils/utils.py:171-175)."""
    g = torch.Generator("cpu").manual_seed(seed)
    return torch.rand([batch, n_queries, 3], generator=g, dtype=torch.float32) * 2 - 1


def cond_tokens(batch: int, n_tokens: int = 64, dim: int = 512, seed: int = 777) -> torch.Tensor:
    """Stand-in radar condition tokens [B,64,C] for denoiser-only workloads."""
    g = torch.Generator("cpu").manual_seed(seed)
    return torch.randn([batch, n_tokens, dim], generator=g, dtype=torch.float32)


def normal(shape, seed: int) -> torch.Tensor:
    g = torch.Generator("cpu").manual_seed(seed)
    return torch.randn(list(shape), generator=g, dtype=torch.float32)


def structured_cloud(batch: int, n_points: int = 10000, seed: int = 3031) -> torch.Tensor:
    """[B,P,3] cloud with the structure real frustum scans have and U(-1,1)^3 lacks (stress input of the folded AE kernels,
    tests/golden/make_golden.py G18): 40 % of the points on three planes (x = 0.25, y = -0.5 and the z = +1 face), 10 % on
    the +-1 faces of the cube (one coordinate exactly +-1), 30 % uniform, then 20 % EXACT duplicates of earlier points."""
    g = torch.Generator("cpu").manual_seed(seed)
    out = []
    for _ in range(batch):
        n_dup = n_points // 5
        n_base = n_points - n_dup
        p = torch.rand([n_base, 3], generator=g, dtype=torch.float32) * 2 - 1
        n_plane, n_face = (2 * n_points) // 5, n_points // 10
        third = n_plane // 3
        p[:third, 0] = 0.25
        p[third:2 * third, 1] = -0.5
        p[2 * third:n_plane, 2] = 1.0
        axis = torch.randint(0, 3, [n_face], generator=g)
        sign = torch.randint(0, 2, [n_face], generator=g).float() * 2 - 1
        p[n_plane + torch.arange(n_face), axis] = sign
        src = torch.randint(0, n_base, [n_dup], generator=g)
        full = torch.cat([p, p[src]])
        out.append(full[torch.randperm(n_points, generator=g)])
    return torch.stack(out)


def structured_queries(batch: int, n_queries: int, seed: int = 3032) -> torch.Tensor:
    """[B,Q,3] decoder queries: a quarter on the +-1 faces, a quarter on the planes of `structured_cloud`, half uniform."""
    g = torch.Generator("cpu").manual_seed(seed)
    q = torch.rand([batch, n_queries, 3], generator=g, dtype=torch.float32) * 2 - 1
    n4 = n_queries // 4
    axis = torch.randint(0, 3, [batch, n4], generator=g)
    sign = torch.randint(0, 2, [batch, n4], generator=g).float() * 2 - 1
    for b in range(batch):
        q[b, torch.arange(n4), axis[b]] = sign[b]
        q[b, n4:n4 + n4 // 3, 0] = 0.25
        q[b, n4 + n4 // 3:n4 + 2 * (n4 // 3), 1] = -0.5
        q[b, n4 + 2 * (n4 // 3):2 * n4, 2] = 1.0
    return q


# AWR1843 layout of the reference's config/antenna_array.txt: rows {data index, azimuth, elevation} in half wavelengths
AWR1843_TX = ((0, 0, 0), (2, 2, 1), (1, 4, 0))
AWR1843_RX = ((0, 0, 0), (1, 1, 0), (2, 2, 0), (3, 3, 0))


def radar_adc(batch: int, seed: int = 5151, ntx: int = 3, nrx: int = 4, n_chirps: int = 128, n_samples: int = 128, n_targets: int = 4,
              tx=AWR1843_TX, rx=AWR1843_RX) -> torch.Tensor:
    """Raw ADC frames int16 [B, ntx, nrx, n_chirps, n_samples, 2] (I, Q; dataset_preprocessor/radar.py:64-70): complex Gaussian
    noise (sigma 40 counts) on a DC offset, plus `n_targets` point targets per frame.  A target is a complex tone with a range beat
    (cycles per sample), a Doppler phase per chirp (including the TDM slot of its transmitter) and the phase of each virtual
    element, exp(i pi (az sin(theta) cos(phi) + el sin(phi))), at amplitudes of 150-1500 counts."""
    g = torch.Generator("cpu").manual_seed(seed)
    s = torch.arange(n_samples, dtype=torch.float64)
    c = torch.arange(n_chirps, dtype=torch.float64)
    frames = []
    for _ in range(batch):
        dc = (torch.rand(2, generator=g, dtype=torch.float64) - 0.5) * 120
        x = torch.randn([ntx, nrx, n_chirps, n_samples, 2], generator=g, dtype=torch.float64) * 40 + dc
        for _ in range(n_targets):
            fr, fd, amp, th, ph = torch.rand(5, generator=g, dtype=torch.float64).tolist()
            fr, fd = 0.08 + 0.35 * fr, fd - 0.5                     # range beat in the uncropped bins; Doppler anywhere
            amp, th, ph = 150 + 1350 * amp, (th - 0.5) * 2.4, (ph - 0.5) * 0.6
            for t_idx, taz, tel in tx:
                for r_idx, raz, rel in rx:
                    ang = torch.pi * ((taz + raz) * torch.sin(torch.tensor(th)) * torch.cos(torch.tensor(ph)) +
                                      (tel + rel) * torch.sin(torch.tensor(ph)))
                    phase = 2 * torch.pi * (fr * s[None, :] + fd * (c[:, None] + t_idx / ntx)) + ang
                    x[t_idx, r_idx, ..., 0] += amp * torch.cos(phase)
                    x[t_idx, r_idx, ..., 1] += amp * torch.sin(phase)
        frames.append(x.round().clamp(-32768, 32767).to(torch.int16))
    return torch.stack(frames)


def lidar_scan(batch: int, seed: int = 2301, n: int = 65536) -> list:
    """Raw LiDAR scans, float32 [n, 4] (x, y, z, intensity in the sensor frame; the layout of lidar/pointclouds/*.bin) per frame,
    a list of `batch` numpy arrays.  Rays from the sensor hit a room (walls, floor, ceiling) with boxes in it; the room reaches past
    the crop range along one axis.  Mixed in, so that every branch of the crop is taken: 6 % all-zero points, rays in every azimuth
    (a third of them behind the radar once the extrinsic turns the frame about z) and elevations up to +-35 degrees (outside the
    +-20 degree FOV)."""
    rng = np.random.default_rng(seed)
    lo = np.array([-22.0, -7.0, -1.3])          # room box around the sensor; -x is the radar's forward direction
    hi = np.array([9.0, 6.0, 2.1])
    out = []
    for _ in range(batch):
        boxes = []
        for _ in range(4):
            c = np.array([rng.uniform(-14, -2), rng.uniform(-5, 4), -1.3])
            s = rng.uniform([0.4, 0.4, 0.5], [1.5, 1.5, 1.6])
            boxes.append((c - s * [1, 1, 0], c + s * [1, 1, 2]))
        az = rng.uniform(-np.pi, np.pi, n)
        az = np.where(rng.random(n) < 0.7, rng.uniform(np.pi - 1.4, np.pi + 1.4, n), az)   # more rays toward -x
        el = np.deg2rad(np.where(rng.random(n) < 0.8, rng.uniform(-19, 19, n), rng.uniform(-35, 35, n)))
        d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(d > 0, (hi - 0) / d, np.where(d < 0, (lo - 0) / d, np.inf)).min(axis=1)   # exit of the room
            for bl, bh in boxes:
                t1, t2 = (bl - 0) / d, (bh - 0) / d
                tn = np.minimum(t1, t2).max(axis=1)
                tf = np.maximum(t1, t2).min(axis=1)
                hit = (tn <= tf) & (tn > 0)
                t = np.where(hit & (tn < t), tn, t)
        p = d * (t * (1 + rng.normal(0, 0.003, n)))[:, None]
        inten = rng.uniform(0, 60, n)
        pts = np.concatenate([p, inten[:, None]], axis=1).astype(np.float32)
        pts[rng.random(n) < 0.06] = 0.0
        out.append(pts)
    return out
