#!/usr/bin/env python3
"""Generate tests/golden/g21_radar_dsp.npz: the reference's radar front end (dataset_preprocessor/radar.py:64-76
load_radar_data + utils/radar_preprocessing.py:6-62 RAEIVVmap) on seeded synthetic ADC frames (rald_amd.synth.radar_adc).

Needs a checkout of the reference; its root directory is the one argument.  radar.py imports `easydict`; it is stubbed
in memory (a dict with attribute access), as make_golden.py stubs the packages it may lack.  The frames are not
stored: tests regenerate them from the seeds below.

Stored, per DSP config (`c8x2` = 1843_coloradar.yml, 4 frames; `c32x16` = 1843_coloradar_test_set.yml, 1 frame):
  <tag>_cube    the reference's cubes [B, R, A, E, 3] float32
  <tag>_vbins   the reference's vbins (float64)
  <tag>_cfg     the config values the front end reads, as float64 (names in `cfg_keys`)
  <tag>_gap     (top1 - top2) / top1 of the Doppler power per (R, A, E): how far the argmax decision is from a tie
  <tag>_thr     |0.7 top1 - top2| / top1: how far the validity decision is from its threshold
plus the parsed antenna layout (`tx`, `rx`).

Usage:  python tests/golden/make_golden_radar_dsp.py REFERENCE_ROOT
"""
import argparse
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from rald_amd import synth  # noqa: E402

SEEDS = {"c8x2": (2101, 4), "c32x16": (2102, 1)}
YML = {"c8x2": "1843_coloradar.yml", "c32x16": "1843_coloradar_test_set.yml"}
CFG_KEYS = ["numTxChan", "numRxChan", "numChirpsPerFrame", "numAdcSamples", "range_fftsize", "doppler_fftsize", "ANGLE_fftsize",
            "ELEVATION_fftsize", "crop_low", "crop_high", "StartFrequency", "Ideltime", "adc_start_time", "Fs", "SamplePerChripUp", "Kr",
            "chirpRampTime", "chirpBandwidth", "max_range"]


def import_reference(ref):
    class ED(dict):
        __getattr__ = dict.__getitem__

        def __setattr__(self, k, v):
            self[k] = v
    ed = types.ModuleType("easydict")
    ed.EasyDict = ED
    sys.modules["easydict"] = ed
    sys.path.insert(0, os.path.join(ref, "dataset_preprocessor"))
    sys.path.insert(0, ref)
    import yaml
    from dataset_preprocessor import radar as R
    from dataset_preprocessor.utils import radar_preprocessing as P, radardsp as D
    return R, P, D, ED, yaml


def margins(adc, cfg, tx, rx, D):
    """The reference chain up to FFT_power (radar_preprocessing.py:21-46, its own helper functions), for the decision margins."""
    ntx, nrx, nc, ns = adc.shape
    x = adc * np.blackman(ns).reshape(1, 1, 1, -1)
    dfft = np.fft.fftshift(np.fft.fft(np.fft.fft(x, cfg.range_fftsize, -1), cfg.doppler_fftsize, -2), -2)
    dfft = dfft * D.velocity_compensation(ntx, cfg.doppler_fftsize)
    va = D.virtual_array(dfft, tx, rx)
    efft = np.fft.fftshift(np.fft.fft(np.fft.fftshift(np.fft.fft(va, cfg.ANGLE_fftsize, 1), 1), cfg.ELEVATION_fftsize, 0), 0)
    efft[:, :, :, 0:int(efft.shape[-1] * cfg.crop_low)] = 0
    efft[:, :, :, -int(efft.shape[-1] * cfg.crop_high):] = 0
    p = np.sort(np.abs(efft) ** 2, axis=2)                         # (E, A, D, R)
    top1, top2 = p[:, :, -1], p[:, :, -2]
    den = np.where(top1 > 0, top1, 1.0)
    gap = np.where(top1 > 0, (top1 - top2) / den, 0.0)
    thr = np.where(top1 > 0, np.abs(0.7 * top1 - top2) / den, 0.0)
    return gap.transpose(2, 1, 0).astype(np.float32), thr.transpose(2, 1, 0).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference", help="root of the reference checkout (holds dataset_preprocessor/)")
    ref = os.path.abspath(ap.parse_args().reference)
    R, P, D, ED, yaml = import_reference(ref)
    cfg_dir = os.path.join(ref, "dataset_preprocessor", "config")
    tx, rx = R.antenna_array(os.path.join(cfg_dir, "antenna_array.txt"))
    out = {"tx": tx.astype(np.int32), "rx": rx.astype(np.int32), "cfg_keys": np.array(CFG_KEYS)}
    for tag, (seed, B) in SEEDS.items():
        with open(os.path.join(cfg_dir, YML[tag]), "r", encoding="utf-8") as fid:
            cfg = ED(yaml.load(fid, Loader=yaml.FullLoader))
        cfg.chirpRampTime = cfg.SamplePerChripUp / cfg.Fs                 # radar.py:145-147
        cfg.chirpBandwidth = cfg.Kr * cfg.chirpRampTime
        cfg.max_range = (3e8 * cfg.chirpRampTime * cfg.Fs) / (2 * cfg.chirpBandwidth)
        frames = synth.radar_adc(B, seed).numpy()
        cubes, gaps, thrs = [], [], []
        with tempfile.TemporaryDirectory() as tmp:
            for b in range(B):
                path = os.path.join(tmp, f"frame_{b}.bin")
                frames[b].tofile(path)
                adc = R.load_radar_data(cfg, path)
                g, t = margins(adc.copy(), cfg, tx, rx, D)
                cubes.append(P.RAEIVVmap(adc, cfg, tx, rx))
                gaps.append(g)
                thrs.append(t)
        _, vbins, _, _ = D._get_bins(cfg.doppler_fftsize, cfg.range_fftsize, cfg.ANGLE_fftsize, cfg.ELEVATION_fftsize, cfg)
        out[f"{tag}_cube"] = np.stack(cubes)
        out[f"{tag}_vbins"] = vbins
        out[f"{tag}_cfg"] = np.array([float(cfg[k]) for k in CFG_KEYS])
        out[f"{tag}_gap"] = np.stack(gaps)
        out[f"{tag}_thr"] = np.stack(thrs)
        print(tag, out[f"{tag}_cube"].shape, "valid", out[f"{tag}_cube"][..., 2].mean(), "dB max", out[f"{tag}_cube"][..., 0].max(),
              "min gap", out[f"{tag}_gap"].min(), "min thr", out[f"{tag}_thr"].min())
    np.savez_compressed(os.path.join(HERE, "g21_radar_dsp.npz"), **out)


if __name__ == "__main__":
    main()
