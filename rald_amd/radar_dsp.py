"""Radar front end on the device: raw AWR1843 ADC frames -> the RAEIVV cubes the model reads.

The reference makes each ``radarcube_raw/*.bin`` with a complex128 numpy chain on the host
(``dataset_preprocessor/radar.py:64-76`` parses a frame, ``:108-115`` drives
``utils/radar_preprocessing.py:6-62`` ``RAEIVVmap``).  Here that chain is ``rald_radar_dsp_run``
(``rald_amd/csrc/radar_dsp.hip``): range FFT, Doppler FFT, virtual array, azimuth x elevation
transform, argmax / validity / power over Doppler and the 30 % noise quantile, batched over frames.

* ``antenna_array`` / ``load_radar_config`` / ``velocity_bins``: the reference's host-side set-up;
* ``RadarDSP``: the device handle, ``cubes(adc)`` on a CUDA int16 tensor ``[B, ntx, nrx, nc, ns, 2]``
  (``range_doppler()`` reads the range-Doppler stage of the latest run);
* ``load_adc_frames``, ``RAEIVVmap`` (drop-in, numpy in / numpy out), ``process_adc_files``
  (``{i:04d}.bin`` files byte-compatible with ``save_radarcube``, radar.py:56-62).
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path
from typing import Dict, Sequence, Tuple

import numpy as np
import torch

from ._handles import _Handle, _cached_workspace, _nbytes, _need_cuda, _stream
from ._lib import RadarDspConfig, check, lib

class RadarConfig(dict):
    """The radar YAML as a dict with attribute access (the reference wraps it in an EasyDict)."""
    __getattr__ = dict.__getitem__

    def __setattr__(self, k, v):
        self[k] = v


def antenna_array(path) -> Tuple[np.ndarray, np.ndarray]:
    """config/antenna_array.txt -> (tx [ntx,3], rx [nrx,3]) int rows {index, azimuth, elevation} (radar.py:35-54)."""
    txl, rxl = [], []
    with open(path, "r") as fh:
        for line in fh:
            if line.startswith("# "):
                continue
            chunks = line.strip().split(" ")
            if chunks[0] == "rx":
                rxl.append([int(x) for x in chunks[1:]])
            elif chunks[0] == "tx":
                txl.append([int(x) for x in chunks[1:]])
    return np.array(txl), np.array(rxl)


def virtual_positions(tx_array, rx_array) -> Tuple[np.ndarray, np.ndarray]:
    """(elevation, azimuth) of the virtual element each (tx row, rx row) pair lands on: radardsp.py:54-111
    adds channel [tidx, ridx] into va[tel + rel, taz + raz] (colliding pairs add up)."""
    tx, rx = np.asarray(tx_array), np.asarray(rx_array)
    return tx[:, 2:3] + rx[None, :, 2], tx[:, 1:2] + rx[None, :, 1]


def load_radar_config(path) -> RadarConfig:
    """The radar YAML (1843_coloradar*.yml) with the values radar.py:145-147 derives from it."""
    import yaml
    with open(path, "r", encoding="utf-8") as fid:
        cfg = RadarConfig(yaml.load(fid, Loader=yaml.FullLoader))
    cfg.chirpRampTime = cfg.SamplePerChripUp / cfg.Fs
    cfg.chirpBandwidth = cfg.Kr * cfg.chirpRampTime
    cfg.max_range = (3e8 * cfg.chirpRampTime * cfg.Fs) / (2 * cfg.chirpBandwidth)
    return cfg


def velocity_bins(radar_config) -> np.ndarray:
    """The ``vbins`` RAEIVVmap indexes with the Doppler argmax (radar_preprocessing.py:45).  The reference calls
    ``_get_bins(nv, nr, ...)`` with its first two arguments swapped, so the bin count is the RANGE FFT size
    (radardsp.py:135-207, get_velocity_bins :285-304, get_max_velocity :209-217)."""
    c = 299792458.0
    ntx, fstart = radar_config["numTxChan"], radar_config["StartFrequency"]
    te = radar_config["chirpRampTime"] + radar_config["adc_start_time"]
    tc = radar_config["Ideltime"] + te
    vmax = (c / fstart) / (4.0 * tc * ntx)
    vres = (2 * vmax) / radar_config["range_fftsize"]
    return np.arange(-vmax, vmax, vres)


def dsp_config(radar_config) -> RadarDspConfig:
    g = radar_config.__getitem__
    return RadarDspConfig(int(g("numTxChan")), int(g("numRxChan")), int(g("numChirpsPerFrame")), int(g("numAdcSamples")),
                          int(g("range_fftsize")), int(g("doppler_fftsize")), int(g("ANGLE_fftsize")), int(g("ELEVATION_fftsize")),
                          float(g("crop_low")), float(g("crop_high")))


def workspace_bytes(radar_config, batch: int) -> int:
    """Device workspace of one run over `batch` frames (host arithmetic, no device call)."""
    return _nbytes(lib().rald_radar_dsp_workspace_bytes(C.byref(dsp_config(radar_config)), int(batch)))


class RadarDSP(_Handle):
    """rald_radar_dsp*: every size, the crop and the antenna layout are checked, and the tables built, here."""

    def __init__(self, radar_config, tx_array, rx_array):
        self.config = radar_config
        self.cfg = dsp_config(radar_config)
        c = self.cfg
        self.shape_in = (c.ntx, c.nrx, c.n_chirps, c.n_samples, 2)
        self.shape_out = (c.range_fft, c.angle_fft, c.elevation_fft, 3)
        tx = np.ascontiguousarray(np.asarray(tx_array, dtype=np.int32).reshape(-1, 3))
        rx = np.ascontiguousarray(np.asarray(rx_array, dtype=np.int32).reshape(-1, 3))
        if tx.shape[0] != c.ntx or rx.shape[0] != c.nrx:
            raise ValueError(f"antenna layout has {tx.shape[0]} tx / {rx.shape[0]} rx rows, the config {c.ntx} / {c.nrx}")
        self.vbins = np.ascontiguousarray(velocity_bins(radar_config), dtype=np.float64)
        super().__init__("radar_dsp", C.byref(c), tx.ctypes.data, rx.ctypes.data, self.vbins.ctypes.data, len(self.vbins))
        self._ws: Dict[torch.device, torch.Tensor] = {}
        self._last = None                                    # (batch, device) of the latest run

    def _run(self, frames: torch.Tensor, kind: int) -> torch.Tensor:
        _need_cuda(frames, "the ADC frames")
        squeeze = frames.dim() == 5
        x = frames.unsqueeze(0) if squeeze else frames
        if tuple(x.shape[1:]) != self.shape_in:
            raise ValueError(f"ADC frames must be [B, {', '.join(map(str, self.shape_in))}], got {list(frames.shape)}")
        x = x.contiguous()
        B = x.shape[0]
        out = torch.empty((B, *self.shape_out), dtype=torch.float32, device=x.device)
        ws = _cached_workspace(self._ws, _nbytes(lib().rald_radar_dsp_workspace_bytes(C.byref(self.cfg), B)), x.device)
        check(lib().rald_radar_dsp_run(self._h, x.data_ptr(), kind, B, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
        self._last = (B, x.device)
        return out[0] if squeeze else out

    def range_doppler(self) -> torch.Tensor:
        """The range-Doppler stage of the latest cubes() / cubes_iq() call: complex64 [B, ntx * nrx, range_fft, doppler_fft], after
        the Doppler fftshift and the velocity compensation; channel = tx data index * nrx + rx data index.  A view of the cached
        workspace (radar_dsp_run's layout: the integer channel sums, 16 bytes per frame and channel rounded up to 256 bytes, then this
        array), valid until the next run on that device."""
        if self._last is None:
            raise RuntimeError("range_doppler(): no run yet")
        B, device = self._last
        c = self.cfg
        nch = c.ntx * c.nrx
        off, n = (B * nch * 16 + 255) // 256 * 256, B * nch * c.range_fft * c.doppler_fft
        return torch.view_as_complex(self._ws[device][off:off + n * 8].view(torch.float32).view(B, nch, c.range_fft, c.doppler_fft, 2))

    def cubes(self, adc: torch.Tensor) -> torch.Tensor:
        """int16 [B, ntx, nrx, nc, ns, 2] (or one frame without B) -> [B, R, A, E, 3] float32 (intensity dB, velocity,
        validity): load_radar_data's mean removal (radar.py:72-75) + RAEIVVmap."""
        if adc.dtype != torch.int16:
            raise TypeError(f"cubes() takes the raw int16 ADC samples, got {adc.dtype}")
        return self._run(adc, 0)

    def cubes_iq(self, iq: torch.Tensor) -> torch.Tensor:
        """float32 [B, ntx, nrx, nc, ns, 2] interleaved I/Q, used as given (no mean removal) -> [B, R, A, E, 3]."""
        return self._run(iq.to(torch.float32), 1)


def load_adc_frames(paths: Sequence, radar_config=None) -> np.ndarray:
    """Raw ADC files (int16 I/Q, radar.py:64-70) -> int16 [B, ntx, nrx, nc, ns, 2]."""
    g = (radar_config or RadarConfig(numTxChan=3, numRxChan=4, numChirpsPerFrame=128, numAdcSamples=128)).__getitem__
    shape = (g("numTxChan"), g("numRxChan"), g("numChirpsPerFrame"), g("numAdcSamples"), 2)
    return np.stack([np.fromfile(str(p), dtype=np.int16).reshape(shape) for p in paths])


_DROPIN: Dict[tuple, RadarDSP] = {}


def _dropin_handle(radar_config, tx_array, rx_array) -> RadarDSP:
    keys = ("numTxChan", "numRxChan", "numChirpsPerFrame", "numAdcSamples", "range_fftsize", "doppler_fftsize", "ANGLE_fftsize",
            "ELEVATION_fftsize", "crop_low", "crop_high", "StartFrequency", "chirpRampTime", "adc_start_time", "Ideltime")
    key = (tuple(radar_config[k] for k in keys), np.asarray(tx_array).tobytes(), np.asarray(rx_array).tobytes(), torch.cuda.current_device())
    h = _DROPIN.get(key)
    if h is None:
        h = _DROPIN[key] = RadarDSP(radar_config, tx_array, rx_array)
    return h


def RAEIVVmap(radar_adc_data, radar_config, tx_array, rx_array) -> np.ndarray:
    """Drop-in for utils/radar_preprocessing.py RAEIVVmap: complex (ntx, nrx, nc, ns) (load_radar_data's mean-removed
    frame) -> float32 (range, azimuth, elevation, 3) numpy.  Runs on the current GPU in fp32; unlike the reference it
    leaves its input unchanged (the reference windows it in place)."""
    x = np.asarray(radar_adc_data)
    h = _dropin_handle(radar_config, tx_array, rx_array)
    iq = np.stack([x.real, x.imag], axis=-1).astype(np.float32)
    out = h.cubes_iq(torch.from_numpy(iq).cuda())
    return out.cpu().numpy()


def process_adc_files(paths: Sequence, out_dir, radar_config, tx_array, rx_array, batch: int = 64) -> int:
    """The per-frame loop of radar.py:108-115 on the device: each ADC file -> out_dir/{i:04d}.bin (float32
    [R, A, E, 3], save_radarcube's bytes).  Frames go through in batches of `batch`; returns the count written."""
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    h = _dropin_handle(radar_config, tx_array, rx_array)
    paths = list(paths)
    for i0 in range(0, len(paths), batch):
        frames = torch.from_numpy(load_adc_frames(paths[i0:i0 + batch], radar_config)).cuda()
        cubes = h.cubes(frames).cpu().numpy()
        for j, cube in enumerate(cubes):
            cube.astype(np.float32).tofile(out_dir / f"{i0 + j:04d}.bin")
    return len(paths)
