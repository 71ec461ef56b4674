"""Helper points on the device: RAEIVV intensity cubes -> the CFAR query points the decoder's ``aug_query_helper`` reads.

The reference makes each ``radar_cfar_low_thrd/{i:04d}.bin`` on the host (``dataset_preprocessor/cache_test_cfar.py:68-93``):
trilinear upsampling (``rae_interpo``), a per-range-slice share of the points in proportion to slice energy
(``weighted_allocation``), a top-k per slice sorted by intensity (``RA2DDetectorTensor``), the index -> polar lookup
(``cube_idx2coord``) and the FOV filter (``lidar.filter_points_polar``).  Here that chain is ``rald_radar_points_run``
(``rald_amd/csrc/radar_points.hip``), batched over frames, with the upsampled cube never stored.

Tie rule (the reference leaves it to np.argpartition / np.argsort): among equal values at a slice's k-th value the lowest flat
index ``a * tgt_e + e`` is chosen, and a slice's points come by value descending, then flat index ascending.

* ``load_cfar_config`` / ``coordinate_axes`` / ``keep_masks``: the reference's host-side set-up, computed in numpy exactly as it
  does (float64 tables, float32 comparisons), so the coordinates and the filter are bit-exact by construction;
* ``RadarPoints``: the device handle, ``points(cubes)`` / ``points_padded(cubes)`` on CUDA cubes ``[B, R, A, E, C]``;
* ``RA2DDetectorTensor`` (drop-in), ``process_cube_files`` (``{i:04d}.bin`` files byte-compatible with ``save_lidar_data``),
  ``helper_points_from_adc`` (ADC -> ``RadarDSP.cubes`` -> ``RadarPoints.points`` on the device).
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from ._handles import _Handle, _cached_workspace, _nbytes, _need_cuda, _opt, _stream
from ._lib import RadarPointsConfig, check, lib
from .radar_dsp import RadarConfig, load_radar_config

WAVELENGTH_TO_APERTURE_RATIO = 0.4972   # dataset_preprocessor/constants.py


def load_cfar_config(dataset_yaml, radar_config) -> RadarConfig:
    """coloradar_config_test_set.yaml (``single_chip_mode.radar.cfar``) + the radar YAML (a path, or a config already loaded
    with ``radar_dsp.load_radar_config``) -> the radar config with the values cache_test_cfar.py:132-154 adds: ``fov``,
    ``input_*_size``, ``target_*_size`` and ``cfar_num_point`` (PyYAML reads ``8e5`` as a string: ``int(float(...))``)."""
    import yaml
    with open(dataset_yaml, "r", encoding="utf-8") as fid:
        ds = yaml.load(fid, Loader=yaml.FullLoader)
    cfg = RadarConfig(radar_config) if isinstance(radar_config, dict) else load_radar_config(radar_config)
    cf = ds["single_chip_mode"]["radar"]["cfar"]
    cfg.fov = [[0, cfg.max_range], cfg.angles_DOA_az, cfg.angles_DOA_ele]
    cfg.target_r_size, cfg.target_a_size, cfg.target_e_size = int(cf["tgt_r_dim"]), int(cf["tgt_a_dim"]), int(cf["tgt_e_dim"])
    cfg.input_r_size, cfg.input_a_size, cfg.input_e_size = int(cf["input_r_dim"]), int(cf["input_a_dim"]), int(cf["input_e_dim"])
    cfg.cfar_num_point = int(float(cf["cfar_num_point"]))
    return cfg


def _angle_axis(n: int) -> np.ndarray:
    w = np.flip(np.linspace(-np.pi, np.pi, n))
    ax = np.arcsin(np.clip(w / (2 * np.pi * WAVELENGTH_TO_APERTURE_RATIO), -1, 1))
    ax[0] = np.pi / 2
    ax[-1] = -np.pi / 2
    return np.rad2deg(-ax)


def coordinate_axes(cfg) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The float64 range (m), azimuth and elevation (degrees) of each target index: cube_idx2coord(return_in_degrees=True).
    The reference casts them to float32 when it stores a point."""
    cell = cfg.max_range / cfg.target_r_size
    r = np.arange(cell, cfg.max_range + cell / 2, cell)
    return r, _angle_axis(cfg.target_a_size), _angle_axis(cfg.target_e_size)


def keep_masks(cfg) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Per axis, whether filter_points_polar(points, cfg.fov) keeps the float32 coordinate (numpy compares in float32)."""
    out = []
    for t, (lo, hi) in zip(coordinate_axes(cfg), cfg.fov):
        v = t.astype(np.float32)
        out.append((v >= lo) & (v <= hi))
    return tuple(out)


def points_config(cfg, in_channels: int = 1) -> RadarPointsConfig:
    g = cfg.__getitem__
    return RadarPointsConfig(int(g("input_r_size")), int(g("input_a_size")), int(g("input_e_size")), int(in_channels),
                             int(g("target_r_size")), int(g("target_a_size")), int(g("target_e_size")), int(g("cfar_num_point")))


def workspace_bytes(cfg, batch: int) -> int:
    """Device workspace of one run over `batch` frames (host arithmetic, no device call)."""
    return _nbytes(lib().rald_radar_points_workspace_bytes(C.byref(points_config(cfg)), int(batch)))


def _raise_rejected(counts: torch.Tensor) -> None:
    c = counts.cpu()
    bad = torch.nonzero(c < 0).flatten().tolist()
    if not bad:
        return
    b = bad[0]
    if int(c[b]) == -1:
        raise ValueError(f"radar_points: frame {b} has no positive finite total intensity (the reference's weights are 0/0 there)")
    raise AssertionError(f"radar_points: frame {b} needs more points in one range slice than the slice has voxels")


class RadarPoints(_Handle):
    """rald_radar_points*: the sizes are checked, and the interpolation tables built, at creation.  `in_channels` is the channel
    count of the cubes given to it (channel 0, the intensity, is read): 3 for RadarDSP.cubes() output, 1 for intensity only."""

    def __init__(self, cfg, in_channels: int = 3, axes=None, masks=None):
        self.config = cfg
        self.cfg = points_config(cfg, in_channels)
        c = self.cfg
        self.num = int(c.num_points)
        self.shape_in = (c.in_r, c.in_a, c.in_e, c.in_channels)
        axes = coordinate_axes(cfg) if axes is None else axes
        masks = keep_masks(cfg) if masks is None else masks
        self._axes = [np.ascontiguousarray(np.asarray(a, dtype=np.float64).astype(np.float32)) for a in axes]
        self._masks = [np.ascontiguousarray(np.asarray(m).astype(np.uint8)) for m in masks]
        for name, t, m, n in zip("rae", self._axes, self._masks, (c.tgt_r, c.tgt_a, c.tgt_e)):
            if t.ndim != 1 or len(t) < n or m.ndim != 1 or len(m) < n:
                raise ValueError(f"the {name} axis table and keep mask need {n} entries (tgt_{name}), got {t.shape} and {m.shape}")
        super().__init__("radar_points", C.byref(c), *[t.ctypes.data for t in self._axes], *[m.ctypes.data for m in self._masks])
        self._ws: Dict[torch.device, torch.Tensor] = {}

    def _frames(self, cubes: torch.Tensor) -> torch.Tensor:
        _need_cuda(cubes, "the radar cubes")
        if cubes.dtype != torch.float32:
            raise TypeError(f"radar cubes must be float32, got {cubes.dtype}")
        x = cubes
        if self.shape_in[3] == 1 and tuple(x.shape[-3:]) == self.shape_in[:3]:
            x = x.unsqueeze(-1)
        if x.dim() == 4:
            x = x.unsqueeze(0)
        if x.dim() != 5 or tuple(x.shape[1:]) != self.shape_in:
            raise ValueError(f"radar cubes must be [B, {', '.join(map(str, self.shape_in))}], got {list(cubes.shape)}")
        return x.contiguous()

    def run(self, cubes: torch.Tensor, with_peaks: bool = False, check_frames: bool = True):
        """-> (points [B, num, 3], counts [B] int32, peaks [B, num, 3] int32 or None, intensities [B, num] or None), all on the
        device.  Rows of points past counts[b] are unspecified.  A rejected frame raises (ValueError: no positive finite total;
        AssertionError: a slice over-allocated) unless check_frames=False, where its count is -1 / -2."""
        x = self._frames(cubes)
        B, dev = x.shape[0], x.device
        points = torch.empty((B, self.num, 3), dtype=torch.float32, device=dev)
        counts = torch.empty((B,), dtype=torch.int32, device=dev)
        peaks = torch.empty((B, self.num, 3), dtype=torch.int32, device=dev) if with_peaks else None
        inten = torch.empty((B, self.num), dtype=torch.float32, device=dev) if with_peaks else None
        ws = _cached_workspace(self._ws, _nbytes(lib().rald_radar_points_workspace_bytes(C.byref(self.cfg), B)), dev)
        check(lib().rald_radar_points_run(self._h, x.data_ptr(), B, points.data_ptr(), counts.data_ptr(),
                                          _opt(peaks), _opt(inten),
                                          ws.data_ptr(), ws.numel(), _stream()))
        if check_frames:
            _raise_rejected(counts)
        return points, counts, peaks, inten

    def points_padded(self, cubes: torch.Tensor, with_peaks: bool = False):
        """-> (points [B, num, 3], counts [B]) and, with with_peaks, also (peaks, intensities)."""
        points, counts, peaks, inten = self.run(cubes, with_peaks)
        return (points, counts, peaks, inten) if with_peaks else (points, counts)

    def points(self, cubes: torch.Tensor) -> List[torch.Tensor]:
        """-> one [N_b, 3] float32 device tensor of polar (r, az deg, el deg) points per frame."""
        points, counts, _, _ = self.run(cubes)
        return [points[b, :n] for b, n in enumerate(counts.cpu().tolist())]


_DROPIN: Dict[tuple, RadarPoints] = {}


def RA2DDetectorTensor(ramap_cube, num=10000):
    """Drop-in for cache_test_cfar_utils.RA2DDetectorTensor: (B, R, A, E) -> (peaks (B, num, 3) int32, intensities (B, num)), both
    squeezed at B = 1, CPU tensors.  Runs on the current GPU with target dims = input dims (the interpolation is then the identity).
    Ties at a slice's k-th value take the lowest flat index, where the reference's order is undefined."""
    x = torch.as_tensor(ramap_cube)
    B, R, A, E = x.shape
    key = (R, A, E, int(num), torch.cuda.current_device())
    h = _DROPIN.get(key)
    if h is None:
        cfg = RadarConfig(input_r_size=R, input_a_size=A, input_e_size=E, target_r_size=R, target_a_size=A, target_e_size=E,
                          cfar_num_point=int(num))
        h = _DROPIN[key] = RadarPoints(cfg, 1, axes=[np.zeros(R), np.zeros(A), np.zeros(E)],
                                       masks=[np.ones(R, bool), np.ones(A, bool), np.ones(E, bool)])
    _, _, peaks, inten = h.run(x.to(torch.float32).cuda(), with_peaks=True)
    return peaks.cpu().squeeze(0), inten.cpu().squeeze(0)


def sorted_cube_files(paths: Sequence) -> List[Path]:
    """The reference's order of the radarcube_high_res files: int(stem.split('_')[-1]) (cache_test_cfar.py:166)."""
    return sorted((Path(p) for p in paths), key=lambda p: int(p.stem.split("_")[-1]))


def process_cube_files(paths: Sequence, out_dir, cfg, batch: int = 64) -> int:
    """The per-frame loop of cache_test_cfar.py:68-93 on the device: each cube file (float32 [R, A, E, C], the RAEIVV .bin) ->
    out_dir/{i:04d}.bin, float32 [N, 3] polar points (save_lidar_data's bytes).  Files go in the order given (sorted_cube_files
    gives the reference's), in batches of `batch`; returns the count written."""
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    paths = list(paths)
    shape = (cfg.input_r_size, cfg.input_a_size, cfg.input_e_size)
    h = None
    for i0 in range(0, len(paths), batch):
        cubes = np.stack([np.fromfile(str(p), dtype=np.float32).reshape(*shape, -1)[..., 0] for p in paths[i0:i0 + batch]])
        if h is None:
            h = RadarPoints(cfg, 1)
        for j, pts in enumerate(h.points(torch.from_numpy(cubes).cuda())):
            pts.cpu().numpy().astype(np.float32).tofile(out_dir / f"{i0 + j:04d}.bin")
    return len(paths)


def helper_points_from_adc(frames: torch.Tensor, dsp, pts: RadarPoints) -> List[torch.Tensor]:
    """int16 ADC frames [B, ntx, nrx, nc, ns, 2] on the device -> RadarDSP.cubes -> RadarPoints.points: one [N_b, 3] polar point
    tensor per frame, on the device, for query_points.aug_query_helper / infer_point_cloud(helper_points=...)."""
    return pts.points(dsp.cubes(frames))
