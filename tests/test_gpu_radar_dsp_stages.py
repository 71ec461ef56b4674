"""The radar front end (rald_amd/csrc/radar_dsp.hip) per stage and across its configuration space, against the float64 reference
of tests/radar_dsp_ref.py: the range-Doppler map per element (RadarDSP.range_doppler), the cube, the two input routes, two exact
frames (every Doppler bin tied; everything in one Doppler bin) and the layouts the host refuses.

Frames are rald_amd.synth.radar_adc(B, 3100, ...); the radar constants are the c8x2 config of g21_radar_dsp.npz with the sizes,
the crop and the channel counts of the case.  CASES says what each one reaches in the kernels."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import radar_dsp_ref as REF
from conftest import GOLDEN
from test_radar_dsp import _config

SEED = 3100
AWR_TX = ((0, 0, 0), (2, 2, 1), (1, 4, 0))
AWR_RX = ((0, 0, 0), (1, 1, 0), (2, 2, 0), (3, 3, 0))
ONE = ((0, 0, 0),)
TX2 = ((0, 0, 0), (1, 1, 0))
RX8 = tuple((i, i % 4, i // 4) for i in range(8))          # virtual positions overlap (tx 1 + rx i lands on tx 0 + rx i + 5), nrx != 4
AWR, SINGLE = (AWR_TX, AWR_RX), (ONE, ONE)

# name: (layout, n_chirps, n_samples, range_fft, doppler_fft, A, E, crop_low, crop_high)
CASES = {
    "small":    (SINGLE, 4, 8, 8, 2, 1, 1, 0.0, 0.125),        # smallest FFTs, crop_lo = 0, one cell, G = nd = 2
    "pad":      (AWR, 12, 20, 32, 16, 8, 2, 0.05, 0.05),       # zero-padding in both FFTs, workspace rows the range FFT never wrote
    "cut":      (AWR, 40, 80, 64, 32, 8, 2, 0.05, 0.05),       # both inputs longer than the FFT
    "tiles":    (AWR, 100, 200, 256, 128, 8, 2, 0.05, 0.05),   # 13 chirp tiles of 8 with a 4-row remainder; samples cut, chirps padded
    "r256d256": (AWR, 256, 256, 256, 256, 4, 2, 0.05, 0.05),   # largest FFTs, tstep = 1; A = 4 < 8 drops antenna pairs
    "r256d2":   (AWR, 2, 256, 256, 2, 8, 2, 0.0, 0.01),        # nd = 2 < G
    "odd5x3":   (AWR, 16, 32, 32, 16, 5, 3, 0.05, 0.05),       # odd sizes, 15 cells: cpp = 15, G = 16
    "a3e1":     (AWR, 16, 32, 32, 16, 3, 1, 0.05, 0.05),       # E = 1 drops the raised tx row, A = 3 truncates azimuth
    "a64e1":    (AWR, 16, 32, 32, 16, 64, 1, 0.05, 0.05),      # exactly one full 64-cell chunk
    "c9x8":     (AWR, 16, 32, 32, 16, 9, 8, 0.05, 0.05),       # 72 cells: a full chunk and an 8-cell one
    "tx2rx8":   ((TX2, RX8), 16, 32, 32, 16, 8, 4, 0.05, 0.05),    # overlapping virtual cells (+=), ch / nrx with nrx = 8
    "crop40":   (AWR, 16, 64, 64, 16, 8, 2, 0.25, 0.15),       # 400 of 1024 cells are zero: the quantile lies inside the tie, noise = 0
    "straddle": (SINGLE, 8, 64, 64, 8, 1, 1, 0.15, 0.16),      # 19 zeros of 64, k = 18: v_k the last zero, v_{k+1} the smallest positive S
}
RUNS = [(name, 1) for name in CASES] + [(name, 3) for name in ("pad", "odd5x3", "crop40")]
RUN_IDS = [f"{n}-B{b}" for n, b in RUNS]

# Asserted bounds: 2 x the largest figure measured on an MI355X over the case's runs (B = 1 and, where there is one, B = 3),
# rounded up.  (k of the range-Doppler map, rel-L2 of a channel's map, |dB error| of the cube); the measurements are in the
# docstrings of the tests that assert them.
BOUNDS = {
    "small":    (2.1, 1.2e-07, 1.8e-06),
    "pad":      (5.8, 2.8e-07, 1.9e-05),
    "cut":      (4.8, 2.8e-07, 1.9e-05),
    "tiles":    (6.6, 3.7e-07, 1.8e-05),
    "r256d256": (5.8, 3.6e-07, 1.5e-05),
    "r256d2":   (4.5, 2.6e-07, 1.6e-04),
    "odd5x3":   (5.0, 2.7e-07, 1.9e-05),
    "a3e1":     (4.2, 2.7e-07, 1.7e-05),
    "a64e1":    (4.2, 2.7e-07, 1.9e-05),
    "c9x8":     (4.2, 2.7e-07, 3.5e-05),
    "tx2rx8":   (5.0, 2.7e-07, 3.4e-05),
    "crop40":   (8.0, 3.6e-07, 4.8e-05),
    "straddle": (2.0, 2.1e-07, 3.2e-05),
}


@functools.lru_cache(maxsize=None)
def _g21():
    with np.load(os.path.join(GOLDEN, "g21_radar_dsp.npz"), allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def _radar_config(layout, nc, ns, nr, nd, A, E, crop_low, crop_high):
    cfg = _config(_g21(), "c8x2")
    cfg.update(numTxChan=len(layout[0]), numRxChan=len(layout[1]), numChirpsPerFrame=nc, numAdcSamples=ns, range_fftsize=nr,
               doppler_fftsize=nd, ANGLE_fftsize=A, ELEVATION_fftsize=E, crop_low=crop_low, crop_high=crop_high)
    return cfg


def _handle(cfg, layout):
    from rald_amd import radar_dsp as RD
    h = RD.RadarDSP(cfg, np.array(layout[0]), np.array(layout[1]))
    np.testing.assert_array_equal(h.vbins, RD.velocity_bins(cfg))
    return h


def _run_poisoned(run, h, x):
    """run(x) with the workspace's map block holding NaN beforehand (a first run allocates it), so that a read of a row the range
    FFT never wrote shows in the result whatever the allocator handed out"""
    run(x)
    h.range_doppler().fill_(float("nan"))
    return run(x)


def _mean_removed_f32(adc):
    """int16 [B, ntx, nrx, nc, ns, 2] -> float32 of (sample - frame mean), the mean as the exact integer sum divided in double:
    the values dsp_range_fft forms from the int16 frame"""
    sums = adc.astype(np.int64).reshape(len(adc), -1, 2).sum(1)
    mean = sums / (adc[0].size // 2)
    return (adc.astype(np.float64) - mean.reshape(len(adc), 1, 1, 1, 1, 2)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _reference(name, B):
    """(frames int16 [B, ...], [reference dict per frame]); computed once, shared by every test of the run and left unchanged"""
    from rald_amd import radar_dsp as RD, synth
    layout, nc, ns, nr, nd, A, E, lo, hi = CASES[name]
    frames = synth.radar_adc(B, SEED, len(layout[0]), len(layout[1]), nc, ns, tx=layout[0], rx=layout[1]).numpy()
    vb = RD.velocity_bins(_radar_config(*CASES[name]))
    return frames, [REF.raeivv(REF.frame_iq(frames[b]), layout[0], layout[1], vb, nr, nd, A, E, lo, hi) for b in range(B)]


@functools.lru_cache(maxsize=None)
def _device(name, B):
    """one int16 run and one float run of the case on the device: (cube, range-Doppler map, cube of the float route), numpy"""
    frames, _ = _reference(name, B)
    h = _handle(_radar_config(*CASES[name]), CASES[name][0])
    cube = _run_poisoned(h.cubes, h, torch.from_numpy(frames).cuda())
    rd = h.range_doppler().cpu().numpy()
    cube_iq = _run_poisoned(h.cubes_iq, h, torch.from_numpy(_mean_removed_f32(frames)).cuda())
    return cube.cpu().numpy(), rd, cube_iq.cpu().numpy()


def _map_figures(name, B):
    """(k, rel-L2): the largest |got - ref| of the range-Doppler map in units of 2^-24 max|ref| of its channel's map, and the largest
    rel-L2 of a channel's map"""
    _, refs = _reference(name, B)
    _, rd, _ = _device(name, B)
    k = l2 = 0.0
    for b, r in enumerate(refs):
        assert rd[b].shape == r["rd"].shape and np.isfinite(rd[b].view(np.float32)).all()
        err = np.abs(rd[b].astype(np.complex128) - r["rd"])
        peak = np.abs(r["rd"]).max(axis=(1, 2))
        assert (peak > 0).all()
        k = max(k, float((err / (2.0 ** -24 * peak[:, None, None])).max()))
        l2 = max(l2, float((np.sqrt((err ** 2).sum((1, 2))) / np.sqrt((np.abs(r["rd"]) ** 2).sum((1, 2)))).max()))
    return k, l2


def _cube_figures(got, refs):
    """(max |dB error|, velocity mismatches at a margin > 1e-4, validity mismatches at a margin > 1e-4, all velocity mismatches,
    all validity mismatches) of cubes [B, R, A, E, 3] against the reference frames"""
    db = 0.0
    bad = [0, 0, 0, 0]
    for b, r in enumerate(refs):
        ref = r["cube"]
        assert got[b].shape == ref.shape and np.isfinite(got[b]).all()
        db = max(db, float(np.abs(got[b][..., 0].astype(np.float64) - ref[..., 0]).max()))
        vel_ne = got[b][..., 1] != ref[..., 1].astype(np.float32)
        val_ne = got[b][..., 2] != ref[..., 2].astype(np.float32)
        for i, m in enumerate((vel_ne & (r["gap"] > 1e-4), val_ne & (r["thr"] > 1e-4), vel_ne, val_ne)):
            bad[i] += int(m.sum())
    return (db, *bad)


def figures(name, B):
    """every measured figure of one run, for the test output and for measuring scripts"""
    _, refs = _reference(name, B)
    cube, _, cube_iq = _device(name, B)
    k, l2 = _map_figures(name, B)
    db, vel_r, val_r, vel_all, val_all = _cube_figures(cube, refs)
    live = [r["S"] > 0 for r in refs]
    return dict(k=k, l2=l2, db=db, db_iq=_cube_figures(cube_iq, refs)[0],
                db_rel=max(float((np.abs(cube[b][..., 0] - r["cube"][..., 0])[live[b]] / r["cube"][..., 0][live[b]]).max()) for b, r in enumerate(refs)),
                db_max=max(float(r["cube"][..., 0].max()) for r in refs), routes_db=float(np.abs(cube[..., 0] - cube_iq[..., 0]).max()),
                routes_equal=bool((cube == cube_iq).all()), vel_bad_robust=vel_r, val_bad_robust=val_r, vel_bad=vel_all, val_bad=val_all,
                robust_v=min(float((r["gap"] > 1e-4)[live[b]].mean()) for b, r in enumerate(refs)),
                robust_m=min(float((r["thr"] > 1e-4)[live[b]].mean()) for b, r in enumerate(refs)),
                noise=[r["noise"] for r in refs], zeros=[int((~l).sum()) for l in live])


# ---- per case: the range-Doppler map, the cube, the two routes ---------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name, B", RUNS, ids=RUN_IDS)
def test_range_doppler_map_per_element(name, B):
    """|got - ref| of every (channel, range, Doppler) element of the map after the compensation, in units of 2^-24 x the peak of
    its channel's reference map, and the rel-L2 of every channel's map.  The unit is the peak because the float32 window and
    compensation tables are the kernel's design and their rounding scales with the targets' peaks through leakage.
    Measured on an MI355X (k, rel-L2; the bound is twice the larger of the B = 1 and B = 3 figures, rounded up):
    small-B1     1.02, 5.81e-08;  pad-B1       2.68, 1.35e-07
    cut-B1       2.36, 1.37e-07;  tiles-B1     3.27, 1.84e-07
    r256d256-B1  2.87, 1.77e-07;  r256d2-B1    2.21, 1.30e-07
    odd5x3-B1    2.05, 1.34e-07;  a3e1-B1      2.05, 1.34e-07
    a64e1-B1     2.05, 1.34e-07;  c9x8-B1      2.05, 1.34e-07
    tx2rx8-B1    2.50, 1.31e-07;  crop40-B1    2.22, 1.42e-07
    straddle-B1  0.98, 1.02e-07;  pad-B3       2.86, 1.35e-07
    odd5x3-B3    2.46, 1.34e-07;  crop40-B3    3.96, 1.79e-07"""
    k, l2 = _map_figures(name, B)
    print(f"{name} B={B}: range-Doppler k {k:.3f}, rel-L2 {l2:.3e}")
    k_bound, l2_bound, _ = BOUNDS[name]
    assert k < k_bound
    assert l2 < l2_bound


@pytest.mark.gpu
@pytest.mark.parametrize("name, B", RUNS, ids=RUN_IDS)
def test_cube_against_reference(name, B):
    """dB per element within the case's bound; velocity and validity equal wherever the reference's margin exceeds 1e-4; at least
    99.5 % of the live cells (S > 0) have such a margin, for both decisions (a property of the inputs); cropped bins are exactly
    (0 dB, vbins[0], invalid).  With crop40's noise of 0 the dB values reach 196, where half a float32 ulp is 7.6e-6: its
    absolute bound is measured like the others.  r256d2 has the largest figure: the map's error scales with the channel's peak
    (k above), the weakest live map elements lie at 1e-5 of it, and with two Doppler bins per cell nothing averages that down;
    a random error of that size put on the float64 map moves its dB by 1e-4.
    Measured on an MI355X, max |dB error| (largest dB of the reference cube):
    small-B1     8.91e-07 (17);  pad-B1       8.05e-06 (48)
    cut-B1       9.36e-06 (49);  tiles-B1     8.75e-06 (57)
    r256d256-B1  7.19e-06 (55);  r256d2-B1    7.60e-05 (61)
    odd5x3-B1    9.10e-06 (49);  a3e1-B1      8.43e-06 (45)
    a64e1-B1     9.17e-06 (50);  c9x8-B1      1.74e-05 (51)
    tx2rx8-B1    1.65e-05 (51);  crop40-B1    1.70e-05 (192)
    straddle-B1  1.56e-05 (46);  pad-B3       9.28e-06 (48)
    odd5x3-B3    9.10e-06 (49);  crop40-B3    2.35e-05 (196)"""
    _, refs = _reference(name, B)
    cube, _, _ = _device(name, B)
    db, vel_robust, val_robust, vel_all, val_all = _cube_figures(cube, refs)
    print(f"{name} B={B}: max dB err {db:.3e}, velocity mismatches {vel_all} ({vel_robust} robust), validity mismatches {val_all} "
          f"({val_robust} robust)")
    from rald_amd import radar_dsp as RD
    nr, lo, hi = CASES[name][3], int(CASES[name][3] * CASES[name][7]), int(CASES[name][3] * CASES[name][8])
    cropped = np.array([0.0, RD.velocity_bins(_radar_config(*CASES[name]))[0], 0.0], np.float32)
    for b, r in enumerate(refs):
        live = r["S"] > 0
        assert not live[:lo].any() and not live[nr - hi:].any() and live[lo:nr - hi].all()
        assert (r["gap"] > 1e-4)[live].mean() >= 0.995 and (r["thr"] > 1e-4)[live].mean() >= 0.995
        assert (cube[b][~live] == cropped).all()
    assert db < BOUNDS[name][2]
    assert vel_robust == 0 and val_robust == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name, B", RUNS, ids=RUN_IDS)
def test_int16_and_float_routes_agree(name, B):
    """cubes_iq on float32(sample - frame mean) against cubes on the int16 frame: the two feed dsp_range_fft the same float32
    values, so dB agrees within the case's bound (measured on an MI355X: identical bits in every run), the decisions are the same in
    every cell, and the float route meets the reference like the int16 one."""
    _, refs = _reference(name, B)
    cube, _, cube_iq = _device(name, B)
    db_iq, vel_robust, val_robust, _, _ = _cube_figures(cube_iq, refs)
    diff = float(np.abs(cube[..., 0] - cube_iq[..., 0]).max())
    print(f"{name} B={B}: routes differ by {diff:.3e} dB, float route max dB err {db_iq:.3e}")
    assert diff < BOUNDS[name][2] and db_iq < BOUNDS[name][2]
    assert (cube[..., 1:] == cube_iq[..., 1:]).all()
    assert vel_robust == 0 and val_robust == 0


# ---- exact frames through cubes_iq ------------------------------------------------------------------------------------------
def _exact_run(layout, nr, nd, A, E, iq):
    """float32 frame [ntx, nrx, nd, nr, 2] (n_chirps = nd, n_samples = nr), crop 0.125 / 0.125 -> (cube, map, vbins, live range bins)"""
    h = _handle(_radar_config(layout, nd, nr, nr, nd, A, E, 0.125, 0.125), layout)
    cube = _run_poisoned(h.cubes_iq, h, torch.from_numpy(iq).cuda()).cpu().numpy()
    return cube, h.range_doppler()[0].cpu().numpy(), h.vbins.astype(np.float32), slice(nr // 8, nr - nr // 8)


@pytest.mark.gpu
@pytest.mark.parametrize("A, E", [(1, 1), (5, 3), (64, 1), (9, 8)], ids=["1cell", "15cells", "64cells", "72cells"])
@pytest.mark.parametrize("nr, nd", [(8, 2), (16, 16), (256, 256)], ids=["nd2", "nd16", "nd256"])
def test_all_doppler_bins_tied(nr, nd, A, E):
    """One antenna, one nonzero sample in chirp 0: the Doppler FFT of [v, 0, ...] is v in every bin without rounding (every
    butterfly adds a zero) and transmitter 0's compensation is exactly 1, so every Doppler bin of a cell has the same power, bit
    for bit.  numpy's argmax takes the first maximum: bin 0, whichever of the G Doppler groups holds it and in whatever order they
    merge; top2 = top1 makes every cell invalid."""
    iq = np.zeros((1, 1, nd, nr, 2), np.float32)
    iq[0, 0, 0, 3] = (1000.0, -700.0)
    cube, rd, vbins, live = _exact_run(SINGLE, nr, nd, A, E, iq)
    assert (np.abs(rd[0, :, 0]) > 0).all()
    assert (rd.view(np.uint64) == rd[:, :, :1].view(np.uint64)).all()
    assert (cube[live, ..., 0] > 0).all()
    assert (cube[live, ..., 1] == vbins[0]).all()
    assert (cube[live, ..., 2] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("nr, nd", [(8, 2), (32, 16), (256, 256)], ids=["nd2", "nd16", "nd256"])
def test_identical_chirps_land_in_the_zero_doppler_bin(nr, nd):
    """Every chirp the same: the first butterfly stage subtracts equal values, so every Doppler bin but the shifted bin nd/2 is
    exactly 0 (and stays 0 under the compensation); there the compensation is exactly 1.  Every live cell takes vbins[nd/2] and is
    valid (top2 = 0)."""
    rng = np.random.default_rng(nd)
    chirp = rng.integers(-2000, 2000, (3, 4, 1, nr, 2)).astype(np.float32)
    iq = np.ascontiguousarray(np.broadcast_to(chirp, (3, 4, nd, nr, 2)))
    cube, rd, vbins, live = _exact_run(AWR, nr, nd, 8, 2, iq)
    others = np.arange(nd) != nd // 2
    assert (rd[:, :, others] == 0.0).all()
    assert (np.abs(rd[:, :, nd // 2]) > 0).all()
    assert (cube[live, ..., 0] > 0).all()
    assert (cube[live, ..., 1] == vbins[nd // 2]).all()
    assert (cube[live, ..., 2] == 1).all()


# ---- refused on the host, before any launch (no GPU needed) --------------------------------------------------------------------
WIDE_TX = ((0, 0, 0), (1, 0, 4), (2, 8, 0))         # with the AWR1843 receivers: 5 elevation rows x 12 azimuth positions


@pytest.mark.parametrize("change, tx, rx, msg", [
    # velocity_bins has range_fftsize entries (the reference's swapped _get_bins arguments): a longer Doppler FFT would index past them
    ({"range_fftsize": 64, "doppler_fftsize": 128}, AWR_TX, AWR_RX, "need a velocity for each of the 128 Doppler bins, got 64"),
    ({"range_fftsize": 2, "doppler_fftsize": 4, "crop_high": 0.5}, AWR_TX, AWR_RX, "need a velocity for each of the 4 Doppler bins, got 2"),
    ({"ANGLE_fftsize": 32, "ELEVATION_fftsize": 16}, WIDE_TX, AWR_RX, "has 60 cells; at most 32 are supported"),
    ({"ANGLE_fftsize": 16, "ELEVATION_fftsize": 3}, WIDE_TX, AWR_RX, "has 36 cells; at most 32 are supported"),
    ({}, ((0, 0, 0), (3, 2, 1), (1, 4, 0)), AWR_RX, "tx layout row 1 out of range"),
    ({}, ((0, 0, 0), (2, 2, 1), (-1, 4, 0)), AWR_RX, "tx layout row 2 out of range"),
    ({}, AWR_TX, ((0, 0, 0), (1, 1, 0), (2, 2, 0), (4, 3, 0)), "rx layout row 3 out of range"),
    ({}, AWR_TX, ((-1, 0, 0), (1, 1, 0), (2, 2, 0), (3, 3, 0)), "rx layout row 0 out of range"),
    ({}, AWR_TX, ((0, 0, 0), (1, 1, 0), (2, 64, 0), (3, 3, 0)), "rx layout row 2 out of range"),
])
def test_unsupported_layouts_and_velocity_tables_raise_at_creation(change, tx, rx, msg):
    """radar_dsp_plan refuses on the host: creation fails before any allocation."""
    from rald_amd import radar_dsp as RD
    cfg = _config(_g21(), "c8x2")
    cfg.update(change)
    with pytest.raises(RuntimeError, match=re.escape(msg)):
        RD.RadarDSP(cfg, np.array(tx), np.array(rx))
