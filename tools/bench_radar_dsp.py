#!/usr/bin/env python3
"""Times the radar front end (rald_amd.radar_dsp.RadarDSP.cubes: int16 ADC frames -> RAEIVV cubes) for B in {1, 8, 64} and
both shipped DSP configs (angle x elevation 8 x 2 and 32 x 16), with device events after warm-up.  Prints one JSON line per
(config, B), and with --out PATH also writes them there as one JSON list.  hbm_bytes_per_frame is the traffic the five kernels need,
from shapes (each kernel's reads and writes counted once; the quantile passes re-read the intensity channel)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from rald_amd import radar_dsp as RD, synth  # noqa: E402

# the AWR1843 values of the ColoRadar single-chip config (1843_coloradar.yml); the test-set config differs in the angle sizes
BASE = dict(numTxChan=3, numRxChan=4, numChirpsPerFrame=128, numAdcSamples=128, StartFrequency=77.0e9, Ideltime=110.0e-6,
            range_fftsize=128, doppler_fftsize=128, Fs=10666000, SamplePerChripUp=128, Kr=1.00000000377e14, adc_start_time=7.0e-6,
            crop_low=0.05, crop_high=0.05)


def config(A, E):
    cfg = RD.RadarConfig(BASE, ANGLE_fftsize=A, ELEVATION_fftsize=E)
    cfg.chirpRampTime = cfg.SamplePerChripUp / cfg.Fs
    return cfg


def hbm_bytes(cfg):
    nch, nc, ns = cfg.numTxChan * cfg.numRxChan, cfg.numChirpsPerFrame, cfg.numAdcSamples
    nr, nd = cfg.range_fftsize, cfg.doppler_fftsize
    cells = nr * cfg.ANGLE_fftsize * cfg.ELEVATION_fftsize
    adc = nch * nc * ns * 4
    spec = nch * nr * nd * 8
    return (adc                      # channel sums
            + adc + spec             # range FFT
            + 2 * spec               # Doppler FFT (in place)
            + spec + cells * 12      # angle transform + Doppler reductions
            + 5 * cells * 12 + cells * 4)   # quantile passes (strided intensity reads) + dB writes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the rows to this JSON file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_radar_dsp needs a GPU"
    torch.cuda.set_device(0)
    base = synth.radar_adc(8, 4242).cuda()
    rows = []
    for A, E in ((8, 2), (32, 16)):
        cfg = config(A, E)
        h = RD.RadarDSP(cfg, synth.AWR1843_TX, synth.AWR1843_RX)
        for B in (1, 8, 64):
            frames = base.repeat((B + 7) // 8, 1, 1, 1, 1, 1)[:B].contiguous()
            for _ in range(args.warmup):
                h.cubes(frames)
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.iters):
                h.cubes(frames)
            t1.record()
            torch.cuda.synchronize()
            ms = t0.elapsed_time(t1) / args.iters
            rows.append(dict(config=f"{A}x{E}", batch=B, ms_per_call=round(ms, 4), ms_per_frame=round(ms / B, 5),
                             hbm_bytes_per_frame=hbm_bytes(cfg), gbps=round(hbm_bytes(cfg) * B / ms / 1e6, 1)))
            print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
