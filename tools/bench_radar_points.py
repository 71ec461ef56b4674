#!/usr/bin/env python3
"""Times the helper-point extractor (rald_amd.radar_points.RadarPoints: 32 x 16 RAEIVV cubes -> CFAR query points, shipped config
256 x 256 x 128 with 8e5 points) and the whole ADC -> RadarDSP.cubes -> RadarPoints chain, for B in {1, 8, 64}, with device events
after warm-up.  Prints one JSON line per (stage, B), and with --out PATH also writes them there as one JSON list.
hbm_bytes_per_frame is an upper bound of the extractor's traffic from shapes: the cube is read by three kernels (slice sums, select,
emit), the 16-bit indices are written once, moved by up to four sort passes (two reads, one write each) and read once, and every
point is written (12 bytes); the chain adds the front end's bytes (tools/bench_radar_dsp.py)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from bench_radar_dsp import config as dsp_config, hbm_bytes as dsp_hbm_bytes  # noqa: E402
from rald_amd import radar_dsp as RD, radar_points as RP, synth  # noqa: E402


def cfar_config(dsp_cfg):
    """coloradar_config_test_set.yaml's cfar block and the FOV of 1843_coloradar_test_set.yml"""
    cfg = RD.RadarConfig(dsp_cfg)
    cfg.chirpBandwidth = cfg.Kr * cfg.chirpRampTime
    cfg.max_range = (3e8 * cfg.chirpRampTime * cfg.Fs) / (2 * cfg.chirpBandwidth)
    cfg.fov = [[0, cfg.max_range], [-90, 90], [-20, 20]]
    cfg.input_r_size, cfg.input_a_size, cfg.input_e_size = 128, 32, 16
    cfg.target_r_size, cfg.target_a_size, cfg.target_e_size = 256, 256, 128
    cfg.cfar_num_point = int(float("8e5"))
    return cfg


def hbm_bytes(cfg, channels=3):
    cube = cfg.input_r_size * cfg.input_a_size * cfg.input_e_size * channels * 4
    num = cfg.cfar_num_point
    return 3 * cube + 2 * num + 4 * 6 * num + 2 * num + 12 * num


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the rows to this JSON file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_radar_points needs a GPU"
    torch.cuda.set_device(0)
    dcfg = dsp_config(32, 16)
    dsp = RD.RadarDSP(dcfg, synth.AWR1843_TX, synth.AWR1843_RX)
    cfg = cfar_config(dcfg)
    pts = RP.RadarPoints(cfg, 3)
    base = synth.radar_adc(8, 4242).cuda()
    rows = []
    for B in (1, 8, 64):
        frames = base.repeat((B + 7) // 8, 1, 1, 1, 1, 1)[:B].contiguous()
        cubes = dsp.cubes(frames)
        _, counts, _, _ = pts.run(cubes)                    # raises on a rejected frame
        kept = float(counts.float().mean())
        for stage, fn, hb in (("extractor", lambda: pts.run(cubes, check_frames=False), hbm_bytes(cfg)),
                              ("adc_to_helper_points", lambda: pts.run(dsp.cubes(frames), check_frames=False),
                               hbm_bytes(cfg) + dsp_hbm_bytes(dcfg))):
            ms = timed(fn, args.iters, args.warmup)
            rows.append(dict(stage=stage, config="32x16->256x256x128", num_points=cfg.cfar_num_point, batch=B, ms_per_call=round(ms, 4),
                             ms_per_frame=round(ms / B, 5), mean_kept_points=round(kept, 1), hbm_bytes_per_frame=hb,
                             gbps=round(hb * B / ms / 1e6, 1)))
            print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
