#!/usr/bin/env python3
"""Generate tests/golden/g22_radar_points.npz: the reference's CFAR helper points (dataset_preprocessor/cache_test_cfar.py:68-93 with
cache_test_cfar_utils.py rae_interpo / weighted_allocation / RA2DDetectorTensor / cube_idx2coord and lidar.filter_points_polar) on
32 x 16 cubes that the reference's own RAEIVVmap makes from seeded synthetic ADC frames (rald_amd.synth.radar_adc).

Needs a checkout of the reference; its root directory is the one argument.  `easydict` and `skimage.feature` are stubbed in memory
(peak_local_max is imported but unused on this path).  The ADC frames are not stored: tests regenerate them from the seed below.

Stored:
  cube            input intensity cubes (channel 0) [B, 128, 32, 16] float32
  radar_cfg       the radar config values the tests rebuild a YAML from (names in `radar_keys`), float64
  fov_az, fov_el  angles_DOA_az / angles_DOA_ele;  max_range
  dims            input_r/a/e, tgt_r/a/e of coloradar_config_test_set.yaml;  num_point_str  its cfar_num_point string
  axis_r/a/e      the reference's float32 coordinate of each target index (cube_idx2coord);  keep_r/a/e  filter_points_polar per axis
  per frame, shipped config (256 x 256 x 128, 8e5 points):
    prefloor      fp32 ratios * total of weighted_allocation, as float64 [B, 256];  counts  the allocation [B, 256]
    kept          len(filter_points_polar(...)) [B];  selected  packed bitmask of the chosen voxels [B, 256 * 256 * 128 / 8]
  two reduced configs on frame 0 (`p2` 64 x 64 x 32 with 2e4 points, `nd` 200 x 96 x 40 with 5e4 points):
    <tag>_dims, <tag>_num, <tag>_counts, <tag>_prefloor, <tag>_points (after the FOV filter)
    <tag>_flat    the reference's peaks in its order as uint16 flat indices a * tgt_e + e; the range index of peak j is the slice
                  whose share of <tag>_counts holds j (RA2DDetector emits the slices in ascending order)
  The reference's intensities are not stored: they are its fp32 F.interpolate values at its peaks, which is asserted here bit for
  bit, so a test recomputes them exactly with F.interpolate on the stored cube.  The file stays well under 1 MB.

Usage:  python tests/golden/make_golden_radar_points.py REFERENCE_ROOT
"""
import argparse
import os
import sys
import tempfile
import time
import types

sys.dont_write_bytecode = True
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from rald_amd import synth  # noqa: E402

SEED, FRAMES = 2201, 2
REDUCED = {"p2": ((64, 64, 32), 20000), "nd": ((200, 96, 40), 50000)}
RADAR_KEYS = ["numTxChan", "numRxChan", "numChirpsPerFrame", "numAdcSamples", "range_fftsize", "doppler_fftsize", "ANGLE_fftsize",
              "ELEVATION_fftsize", "crop_low", "crop_high", "StartFrequency", "Ideltime", "adc_start_time", "Fs", "SamplePerChripUp", "Kr"]


def import_reference(ref):
    class ED(dict):
        __getattr__ = dict.__getitem__

        def __setattr__(self, k, v):
            self[k] = v
    ed = types.ModuleType("easydict")
    ed.EasyDict = ED
    sys.modules["easydict"] = ed
    sk = types.ModuleType("skimage")
    skf = types.ModuleType("skimage.feature")
    skf.peak_local_max = None
    sk.feature = skf
    sys.modules["skimage"] = sk
    sys.modules["skimage.feature"] = skf
    sys.path.insert(0, os.path.join(ref, "dataset_preprocessor"))
    sys.path.insert(0, ref)
    import yaml
    from dataset_preprocessor import radar as R, lidar as L
    from dataset_preprocessor import cache_test_cfar_utils as U
    from dataset_preprocessor.utils import radar_preprocessing as P
    return R, L, U, P, ED, yaml


def prefloor(cube_b, total):
    """weighted_allocation's pre-floor values as RA2DDetectorTensor feeds it (fp32 torch)"""
    import torch
    w = (cube_b.sum(axis=[1, 2]) / cube_b.sum()).to(torch.float32)
    return (w / w.sum() * total).double().numpy()


def run_chain(U, L, cfg, up):
    """cache_test_cfar.py:80-90 from the upsampled cube [1, R, A, E]: peaks, intensities, filtered points"""
    peaks, inten = U.RA2DDetectorTensor(up, num=cfg.cfar_num_point)
    coords = U.cube_idx2coord(peaks, cfg, return_in_degrees=True)
    return peaks.numpy(), inten.numpy(), L.filter_points_polar(coords, cfg.fov)


def axis_tables(U, L, cfg):
    import torch
    R, A, E = cfg.target_r_size, cfg.target_a_size, cfg.target_e_size
    n = max(R, A, E)
    i = np.arange(n)
    idx = torch.from_numpy(np.stack([np.minimum(i, R - 1), np.minimum(i, A - 1), np.minimum(i, E - 1)], 1))
    c = U.cube_idx2coord(idx, cfg, return_in_degrees=True)
    ax = [c[:R, 0].copy(), c[:A, 1].copy(), c[:E, 2].copy()]
    keep = []
    for d, t in enumerate(ax):
        pts = np.zeros((len(t), 3), np.float32)
        pts[:, 0] = float(cfg.max_range) / 2
        pts[:, d] = t
        m = L.filter_points_polar(pts, cfg.fov)
        keep.append(np.isin(t, m[:, d]))
    return ax, keep


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("reference", help="root of the reference checkout (holds dataset_preprocessor/)")
    ref = os.path.abspath(ap.parse_args().reference)
    R, L, U, P, ED, yaml = import_reference(ref)
    cfg_dir = os.path.join(ref, "dataset_preprocessor", "config")
    tx, rx = R.antenna_array(os.path.join(cfg_dir, "antenna_array.txt"))
    with open(os.path.join(cfg_dir, "coloradar_config_test_set.yaml"), "r", encoding="utf-8") as fid:
        ds = ED(yaml.load(fid, Loader=yaml.FullLoader))
    with open(os.path.join(cfg_dir, "1843_coloradar_test_set.yml"), "r", encoding="utf-8") as fid:
        cfg = ED(yaml.load(fid, Loader=yaml.FullLoader))
    cfg.chirpRampTime = cfg.SamplePerChripUp / cfg.Fs                 # cache_test_cfar.py:132-140
    cfg.chirpBandwidth = cfg.Kr * cfg.chirpRampTime
    cfg.max_range = (3e8 * cfg.chirpRampTime * cfg.Fs) / (2 * cfg.chirpBandwidth)
    cfg.fov = [[0, cfg.max_range], cfg.angles_DOA_az, cfg.angles_DOA_ele]
    cf = ds["single_chip_mode"]["radar"]["cfar"]
    cfg.target_r_size, cfg.target_a_size, cfg.target_e_size = cf["tgt_r_dim"], cf["tgt_a_dim"], cf["tgt_e_dim"]
    cfg.input_r_size, cfg.input_a_size, cfg.input_e_size = cf["input_r_dim"], cf["input_a_dim"], cf["input_e_dim"]
    cfg.cfar_num_point = int(float(cf["cfar_num_point"]))

    frames = synth.radar_adc(FRAMES, SEED).numpy()
    cubes = []
    with tempfile.TemporaryDirectory() as tmp:
        for b in range(FRAMES):
            path = os.path.join(tmp, f"frame_{b}.bin")
            frames[b].tofile(path)
            cubes.append(P.RAEIVVmap(R.load_radar_data(cfg, path), cfg, tx, rx)[..., 0])
    cube = np.stack(cubes).astype(np.float32)
    ax, keep = axis_tables(U, L, cfg)
    out = {"cube": cube, "radar_keys": np.array(RADAR_KEYS), "radar_cfg": np.array([float(cfg[k]) for k in RADAR_KEYS]),
           "fov_az": np.array(cfg.angles_DOA_az, np.float64), "fov_el": np.array(cfg.angles_DOA_ele, np.float64),
           "max_range": np.float64(cfg.max_range), "num_point_str": np.array(str(cf["cfar_num_point"])),
           "dims": np.array([cfg.input_r_size, cfg.input_a_size, cfg.input_e_size, cfg.target_r_size, cfg.target_a_size, cfg.target_e_size]),
           "axis_r": ax[0], "axis_a": ax[1], "axis_e": ax[2], "keep_r": keep[0], "keep_a": keep[1], "keep_e": keep[2]}
    pre, counts, kept, sel = [], [], [], []
    for b in range(FRAMES):
        t0 = time.perf_counter()
        up = U.rae_interpo(torch.from_numpy(cube[b:b + 1]), cfg.target_r_size, cfg.target_a_size, cfg.target_e_size)
        t1 = time.perf_counter()
        peaks, inten, pts = run_chain(U, L, cfg, up)
        t2 = time.perf_counter()
        print(f"frame {b}: rae_interpo {1e3 * (t1 - t0):.1f} ms, detector + coords + filter {1e3 * (t2 - t1):.1f} ms, "
              f"total {1e3 * (t2 - t0):.1f} ms; kept {len(pts)}")
        pre.append(prefloor(up[0], cfg.cfar_num_point))
        c = U.weighted_allocation(up[0].sum(axis=[1, 2]) / up[0].sum(), cfg.cfar_num_point).numpy()
        counts.append(c)
        assert np.array_equal(np.bincount(peaks[:, 0], minlength=cfg.target_r_size), c)
        kept.append(len(pts))
        m = np.zeros((cfg.target_r_size, cfg.target_a_size, cfg.target_e_size), bool)
        m[peaks[:, 0], peaks[:, 1], peaks[:, 2]] = True
        sel.append(np.packbits(m.ravel()))
    out.update(prefloor=np.stack(pre), counts=np.stack(counts).astype(np.int64), kept=np.array(kept), selected=np.stack(sel))
    for tag, (dims, num) in REDUCED.items():
        c2 = ED(dict(cfg))
        c2.target_r_size, c2.target_a_size, c2.target_e_size = dims
        c2.cfar_num_point = num
        up = U.rae_interpo(torch.from_numpy(cube[:1]), *dims)
        peaks, inten, pts = run_chain(U, L, c2, up)
        out[f"{tag}_dims"] = np.array(dims)
        out[f"{tag}_num"] = np.int64(num)
        out[f"{tag}_counts"] = U.weighted_allocation(up[0].sum(axis=[1, 2]) / up[0].sum(), num).numpy().astype(np.int64)
        out[f"{tag}_prefloor"] = prefloor(up[0], num)
        assert np.array_equal(peaks[:, 0], np.repeat(np.arange(dims[0]), out[f"{tag}_counts"]))
        assert np.array_equal(inten, up[0].numpy()[peaks[:, 0], peaks[:, 1], peaks[:, 2]])
        out[f"{tag}_flat"] = (peaks[:, 1] * dims[2] + peaks[:, 2]).astype(np.uint16)
        out[f"{tag}_points"] = pts.astype(np.float32)
        print(tag, dims, num, "kept", len(pts))
    np.savez_compressed(os.path.join(HERE, "g22_radar_points.npz"), **out)


if __name__ == "__main__":
    main()
