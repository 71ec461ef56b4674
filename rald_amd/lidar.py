"""LiDAR front end on the device: raw scans -> the dict the reference's loader hands to the engines.

The reference runs this on the host: the offline crop ``dataset_preprocessor/lidar.py:123-194`` (remove_empty_points, the
lidar -> radar extrinsic in float64, cartesian2polar, filter_points_polar, polar2cartesian, ``lidar_sc/{i:04d}.bin``), then per
sample ``ColoRadarDataset.__getitem__`` (``datasets/aligned_coloradar/Coloradar_dataset.py:70-135``): float32 polar, spconv's
voxelization (``datasets/utils/voxelize.py``), point sampling, occupancy queries (:237-294, :335-363) and normalisation
(:365-418).  Here those run as ``rald_lidar_crop`` / ``_voxelize`` / ``_queries`` (``rald_amd/csrc/lidar.hip``), batched over
frames of different lengths.

* ``load_lidar_config``, ``T_RADAR_TO_LIDAR``: the configuration and the extrinsic (built in numpy from the calibration data);
* ``remove_empty_points`` / ``transform_lidar_data`` / ``cartesian2polar`` / ``filter_points_polar``: device drop-ins for the
  single-step functions of lidar.py (elementwise torch plumbing in float64; the fused kernel is ``LidarFrames.crop``);
* ``process_lidar_files``: the lidar.py main loop, batched, writing the reference's ``.bin`` files;
* ``VoxelGeneratorWrapper``: drop-in for datasets/utils/voxelize.py (numpy in, numpy out, spconv's Point2VoxelCPU3d rules);
* ``LidarFrames``: the handle; ``batch(scans, loader_type)`` returns what ``default_collate`` makes of the reference's dicts.

Random numbers (the ``query_points.py`` rule): ``rng=None`` makes the reference's draws on the host, in its calls and order, frame
by frame (a fresh ``np.random.default_rng()`` per numpy call, ``torch.randint`` on torch's global CPU generator); an
``np.random.Generator`` serves every numpy draw (replaying the reference with ``default_rng`` patched to one seeded generator); a
``torch.Generator`` draws on the device.  ``batch`` reads N (points per frame) and V (kept voxels per frame) back to the host once
per batch: the draws' sizes depend on them, and the reference raises on the same values.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path
from typing import Dict, Optional, Sequence, Union

import numpy as np
import torch

from ._handles import _Handle, _cached_workspace, _nbytes, _need_cuda, _opt, _stream
from ._lib import LidarConfig, check, lib
from .config import Config

# dataset_preprocessor/constants.py: calibration data (calib/base_to_lidar.txt, calib/base_to_single_chip.txt), quaternions x y z w
BASE_TO_RADAR = {"translation": [-0.145, 0.09, -0.025], "quaternion": [0.0, 0.0, 0.706825181105, 0.707388269167]}
BASE_TO_LIDAR = {"translation": [-0.075, -0.02, 0.03618], "quaternion": [0.0, 0.0, 0.721382357437, -0.692536998563]}
# dataset_preprocessor/config/coloradar_config.yaml, single_chip_mode.lidar.FOV
SHIPPED_FOV = {"max_range": 15.863025538680999, "az_range": [-90, 90], "el_range": [-20, 20]}
NUMBER_RECORDING_ATTRIBUTES = 4


def quaternion_matrix(q) -> np.ndarray:
    """Rotation matrix of a scalar-last quaternion (x, y, z, w), normalised first (scipy's Rotation.from_quat(q).as_matrix())."""
    x, y, z, w = np.asarray(q, dtype=np.float64) / np.linalg.norm(np.asarray(q, dtype=np.float64))
    x2, y2, z2, w2 = x * x, y * y, z * z, w * w
    xy, zw, xz, yw, yz, xw = x * y, z * w, x * z, y * w, y * z, x * w
    return np.array([[x2 - y2 - z2 + w2, 2 * (xy - zw), 2 * (xz + yw)],
                     [2 * (xy + zw), -x2 + y2 - z2 + w2, 2 * (yz - xw)],
                     [2 * (xz - yw), 2 * (yz + xw), -x2 - y2 + z2 + w2]])


def _pose(cal) -> np.ndarray:
    T = np.eye(4)
    T[:3, :3] = quaternion_matrix(cal["quaternion"])
    T[:3, 3] = cal["translation"]
    return T


T_RADAR_TO_LIDAR = np.linalg.inv(_pose(BASE_TO_RADAR)) @ _pose(BASE_TO_LIDAR)


def _section(cfg, key):
    return cfg[key] if isinstance(cfg, dict) and key in cfg else None


def load_lidar_config(dataset_cfg, preprocessor_yaml=None) -> Config:
    """The `dataset.lidar` section of a training / eval config (a YAML path, the whole config, the `dataset` section or the `lidar`
    section itself) plus the crop FOV of the preprocessor YAML (`single_chip_mode.lidar.FOV`; the shipped values without one).
    Returns a Config with the section's keys, `grid_size` (round((hi - lo) / voxel_size), numpy float64 as the dataset computes it),
    `fov` ([[0, max_range], az_range, el_range]) and `extrinsic` (T_RADAR_TO_LIDAR)."""
    import yaml
    if isinstance(dataset_cfg, (str, Path)):
        with open(dataset_cfg, "r", encoding="utf-8") as fid:
            dataset_cfg = yaml.load(fid, Loader=yaml.FullLoader)
    sec = dataset_cfg
    for key in ("dataset", "lidar"):
        s = _section(sec, key)
        if s is not None:
            sec = s
    for key in ("pc_range", "voxel_size", "max_points_per_voxel", "max_number_of_voxels", "num_point_features"):
        if key not in sec:
            raise KeyError(f"the lidar config has no '{key}'")
    cfg = Config(dict(sec))
    cfg.setdefault("view_cone_mode", False)
    cfg.setdefault("norm_anisotropy", False)
    cfg.setdefault("norm_isotropy", False)
    cfg.setdefault("sampling", True)
    cfg.setdefault("num_samples", 10000)
    cfg.setdefault("query_ratio", 0.0625)
    cfg.grid_size = grid_size(cfg)
    fov = SHIPPED_FOV
    if preprocessor_yaml is not None:
        with open(preprocessor_yaml, "r", encoding="utf-8") as fid:
            fov = yaml.load(fid, Loader=yaml.FullLoader)["single_chip_mode"]["lidar"]["FOV"]
    cfg.fov = [[0, fov["max_range"]], [fov["az_range"][0], fov["az_range"][1]], [fov["el_range"][0], fov["el_range"][1]]]
    cfg.extrinsic = T_RADAR_TO_LIDAR
    return cfg


def lidar_config_struct(cfg) -> LidarConfig:
    c = LidarConfig()
    for i, v in enumerate(cfg.pc_range):
        c.pc_range[i] = float(v)
    for i, v in enumerate(cfg.voxel_size):
        c.voxel_size[i] = float(v)
    c.max_points_per_voxel = int(cfg.max_points_per_voxel)
    c.max_voxels = int(cfg.max_number_of_voxels)
    c.num_point_features = int(cfg.num_point_features)
    c.view_cone_mode = int(bool(cfg.get("view_cone_mode", False)))
    c.norm_anisotropy = int(bool(cfg.get("norm_anisotropy", False)))
    c.norm_isotropy = int(bool(cfg.get("norm_isotropy", False)))
    T = np.asarray(cfg.get("extrinsic", T_RADAR_TO_LIDAR), dtype=np.float64).reshape(16)
    for i in range(16):
        c.extrinsic[i] = float(T[i])
    fov = cfg.get("fov", [[0, SHIPPED_FOV["max_range"]], SHIPPED_FOV["az_range"], SHIPPED_FOV["el_range"]])
    for i, v in enumerate(np.asarray(fov, dtype=np.float64).reshape(6)):
        c.fov[i] = float(v)
    return c


def fps_scale(cfg):
    """Per-axis factors that make farthest-point distances those of the normalised coordinates the encoder sees: 1 / half extent per
    axis with norm_anisotropy, 1 / the largest half extent with norm_isotropy (both: their product), None when neither is on.
    float64 arithmetic, rounded to float32 once."""
    pc = np.array(cfg.pc_range, dtype=np.float64)
    half = (pc[3:6] - pc[0:3]) / 2
    s = np.ones(3, dtype=np.float64)
    if cfg.get("norm_anisotropy", False):
        s = s / half
    if cfg.get("norm_isotropy", False):
        s = s / half.max()
    if not (cfg.get("norm_anisotropy", False) or cfg.get("norm_isotropy", False)):
        return None
    return [float(v) for v in s.astype(np.float32)]


def grid_size(cfg) -> np.ndarray:
    """round((hi - lo) / voxel_size) in float64, as the dataset computes it (Coloradar_dataset.py:57-58); create checks the sizes."""
    pc = np.array(cfg.pc_range, dtype=np.float64)
    with np.errstate(all="ignore"):
        g = np.round((pc[3:6] - pc[0:3]) / np.array(cfg.voxel_size, dtype=np.float64))
    return np.where(np.isfinite(g), g, 0).astype(np.int64)


def workspace_bytes(cfg, batch: int, total_points: int) -> int:
    """Device workspace of one crop / voxelize / queries call over `batch` frames of `total_points` points (host arithmetic)."""
    return _nbytes(lib().rald_lidar_workspace_bytes(C.byref(lidar_config_struct(cfg)), int(batch), int(total_points)))


def empty_cell(kept_keys: np.ndarray, r) -> np.ndarray:
    """The r-th empty cell (row-major) of a grid whose occupied cells are the sorted `kept_keys`: the smallest j with
    kept_keys[j] - j > r gives cell r + j.  Host form of what lid_queries does per out-voxel query."""
    k = np.asarray(kept_keys, dtype=np.int64)
    j = np.searchsorted(k - np.arange(len(k)), np.asarray(r, dtype=np.int64), side="right")
    return np.asarray(r, dtype=np.int64) + j


# ---------------------------------------------------------------------------------------------------- drop-ins (lidar.py)
def _dev(points) -> torch.Tensor:
    t = torch.as_tensor(points)
    return t if t.is_cuda else t.cuda()


def remove_empty_points(points) -> torch.Tensor:
    """lidar.py:111-121: rows whose xyz norm (in the input dtype) is 0 are dropped."""
    p = _dev(points)
    return p[(p[:, :3] * p[:, :3]).sum(dim=1) > 0]


def transform_lidar_data(points) -> torch.Tensor:
    """lidar.py:46-50: [x y z 1] @ T_RADAR_TO_LIDAR.T in float64 -> float64 [N, 3]."""
    p = _dev(points)
    assert p.shape[1] == 3
    T = torch.as_tensor(T_RADAR_TO_LIDAR, dtype=torch.float64, device=p.device)
    h = torch.cat([p.double(), torch.ones(p.shape[0], 1, dtype=torch.float64, device=p.device)], dim=1)
    return (h @ T.T)[:, :3]


def cartesian2polar(points) -> torch.Tensor:
    """lidar.py:52-58 in the input's dtype (float32 or float64); transcendentals in float64, rounded once."""
    p = _dev(points)
    assert p.shape[1] == 3
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    r = torch.sqrt(x * x + y * y + z * z)
    r2d = torch.tensor(np.rad2deg(np.ones(1, dtype=np.float64 if p.dtype == torch.float64 else np.float32)), device=p.device)
    az = -(torch.atan2(y.double(), x.double()).to(p.dtype) * r2d)
    el = torch.asin((z / r).double()).to(p.dtype) * r2d
    return torch.stack([r, az, el], dim=1)


def filter_points_polar(points, range) -> torch.Tensor:  # noqa: A002 - the reference's argument name
    """lidar.py:95-109: inclusive bounds on r, az, el."""
    p = _dev(points)
    assert p.shape[1] == 3, "Input points must be in polar coordinates"
    m = (p[:, 0] >= range[0][0]) & (p[:, 0] <= range[0][1]) & (p[:, 1] >= range[1][0]) & (p[:, 1] <= range[1][1]) & \
        (p[:, 2] >= range[2][0]) & (p[:, 2] <= range[2][1])
    return p[m]


# ---------------------------------------------------------------------------------------------------- the handle
def _pack(scans: Sequence, cols: int) -> tuple:
    arrs = [np.ascontiguousarray(np.asarray(s.cpu() if torch.is_tensor(s) else s, dtype=np.float32)) for s in scans]
    for a in arrs:
        if a.ndim != 2 or a.shape[1] < cols:
            raise ValueError(f"each scan must be [N, >= {cols}] float32, got {a.shape}")
    n = np.array([a.shape[0] for a in arrs], dtype=np.int64)
    offs = np.zeros(len(arrs) + 1, dtype=np.int64)
    offs[1:] = np.cumsum(n)
    width = max(a.shape[1] for a in arrs) if arrs else cols
    if any(a.shape[1] != width for a in arrs):
        raise ValueError("all scans of a batch must have the same number of columns")
    flat = np.concatenate(arrs, axis=0) if arrs else np.zeros((0, width), np.float32)
    return flat, offs, width


class LidarFrames(_Handle):
    """rald_lidar*: the configuration is checked at creation (positive voxel sizes, a grid below 2^31 cells).  Frames are packed
    [total, F] float32 CUDA tensors with host int64 offsets [B + 1]; the workspace is owned here and grows on demand."""

    def __init__(self, cfg):
        self.config = cfg
        self.cfg = lidar_config_struct(cfg)
        self.grid = grid_size(cfg)
        self.cells = int(np.prod(self.grid))
        self.maxv = int(self.cfg.max_voxels)
        self.maxp = int(self.cfg.max_points_per_voxel)
        self.F = int(self.cfg.num_point_features)
        super().__init__("lidar", C.byref(self.cfg))
        self._ws: Dict[torch.device, torch.Tensor] = {}

    def _workspace(self, batch: int, total: int, device) -> torch.Tensor:
        return _cached_workspace(self._ws, _nbytes(lib().rald_lidar_workspace_bytes(C.byref(self.cfg), int(batch), int(total))), device)

    @staticmethod
    def _offs(offsets) -> np.ndarray:
        o = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64))
        if o.ndim != 1 or len(o) < 2:
            raise ValueError("offsets must be int64 [B + 1]")
        return o

    @staticmethod
    def _rows(points: torch.Tensor, o: np.ndarray) -> None:
        if points.shape[0] < o[-1]:
            raise ValueError(f"offsets reach row {int(o[-1])} of a tensor of {points.shape[0]} rows")

    def crop(self, points: torch.Tensor, offsets):
        """lidar.py:170-182 on packed scans [total, >= 3] (x, y, z first; raw [N, 4] scans as they are): -> (out [total, 3] float32,
        counts [B] int32), frame b's survivors in input order at rows offsets[b] .. offsets[b] + counts[b]."""
        _need_cuda(points, "the scans")
        if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] < 3:
            raise ValueError(f"scans must be float32 [total, >= 3], got {points.dtype} {list(points.shape)}")
        points = points.contiguous()
        o = self._offs(offsets)
        self._rows(points, o)
        B, dev = len(o) - 1, points.device
        out = torch.empty((max(points.shape[0], 1), 3), dtype=torch.float32, device=dev)
        counts = torch.empty((B,), dtype=torch.int32, device=dev)
        ws = self._workspace(B, points.shape[0], dev)
        check(lib().rald_lidar_crop(self._h, points.data_ptr(), points.shape[1], o.ctypes.data, B, out.data_ptr(),
                                    counts.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
        return out, counts

    def voxelize(self, points: torch.Tensor, offsets, counts: Optional[torch.Tensor] = None, to_polar: bool = False,
                 with_voxels: bool = True) -> dict:
        """Point2VoxelCPU3d per frame on packed points [total, F].  -> dict of device tensors: voxels [B, max_voxels, max_points, F]
        (zero-filled; None unless with_voxels), coords [B, max_voxels, 3] int32 zyx, num_points [B, max_voxels] int32, kept_keys
        [B, max_voxels] int32 (ascending), voxel_counts [B] int32 and, with to_polar, polar [total, 3] (numpy's float32
        cartesian2polar of every point).  Rows past voxel_counts[b] are unspecified."""
        _need_cuda(points, "the points")
        if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != self.F:
            raise ValueError(f"points must be float32 [total, {self.F}], got {points.dtype} {list(points.shape)}")
        points = points.contiguous()
        o = self._offs(offsets)
        self._rows(points, o)
        B, dev, T = len(o) - 1, points.device, points.shape[0]
        i32 = dict(dtype=torch.int32, device=dev)
        voxels = torch.empty((B, self.maxv, self.maxp, self.F), dtype=torch.float32, device=dev) if with_voxels else None
        res = dict(voxels=voxels, coords=torch.empty((B, self.maxv, 3), **i32), num_points=torch.empty((B, self.maxv), **i32),
                   kept_keys=torch.empty((B, self.maxv), **i32), voxel_counts=torch.empty((B,), **i32),
                   polar=torch.empty((max(T, 1), 3), dtype=torch.float32, device=dev) if to_polar else None)
        if counts is not None:
            _need_cuda(counts, "counts")
            counts = counts.to(torch.int32).contiguous()
        ws = self._workspace(B, T, dev)
        check(lib().rald_lidar_voxelize(self._h, points.data_ptr(), o.ctypes.data, _opt(counts), B, int(bool(to_polar)), _opt(res["polar"]),
                                        _opt(voxels), res["coords"].data_ptr(), res["num_points"].data_ptr(), res["kept_keys"].data_ptr(),
                                        res["voxel_counts"].data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
        return res

    def queries(self, points: torch.Tensor, offsets, num_samples: int, in_num: int, sample_idx, u_in, voxel_idx, u_out, empty_rank,
                vox: dict):
        """rald_lidar_queries: -> (lidar_points [B, S, 3], query_points [B, S, 3], query_labels [B, S]) on the device."""
        o = self._offs(offsets)
        _need_cuda(points, "the points")
        if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 3:
            raise ValueError(f"points must be float32 [total, 3], got {points.dtype} {list(points.shape)}")
        self._rows(points, o)
        B, dev = len(o) - 1, points.device
        S = int(num_samples)
        lp = torch.empty((B, S, 3), dtype=torch.float32, device=dev)
        qp = torch.empty((B, S, 3), dtype=torch.float32, device=dev)
        lab = torch.empty((B, S), dtype=torch.float32, device=dev)
        ws = self._workspace(B, 0, dev)
        check(lib().rald_lidar_queries(self._h, points.contiguous().data_ptr(), o.ctypes.data, B, S, int(in_num), _opt(sample_idx), _opt(u_in),
                                       _opt(voxel_idx), _opt(u_out), _opt(empty_rank), _opt(vox["coords"]), _opt(vox["kept_keys"]),
                                       _opt(vox["voxel_counts"]), lp.data_ptr(), qp.data_ptr(), lab.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
        return lp, qp, lab

    def batch(self, scans: Sequence, loader_type: str = "train", load_query: bool = True,
              rng: Union[None, np.random.Generator, torch.Generator] = None, crop: bool = False, polar: bool = False,
              point_sampling: str = "random") -> dict:
        """ColoRadarDataset.__getitem__'s LiDAR part for a batch, collated.  `scans`: cartesian float32 [N_b, 3] (the lidar_sc files),
        or raw [N_b, 4] scans with crop=True (lidar.py's crop first); polar=True: float32 polar rows that are used as they are (the
        view-cone conversion skipped).  Returns (device tensors) lidar_points [B, S, 3] and, with load_query, query_points,
        raw_query_points (the same tensor: the reference normalises its alias in place), query_labels [B, S], in_voxel_num [B]
        int64; for loaders other than 'train' also raw_lidar_points, the cartesian scans (a list: their lengths differ).
        point_sampling: 'random' (the reference's permutation draw, and the default: the same draws bit for bit) or 'fps': the S
        encoder points of a frame are its farthest-point sample (postprocess.farthest_point_sample_ragged over the rows the queries
        sample from, distances scaled as the point normalisation scales them: fps_scale), started at one index drawn from `rng` in
        place of the permutation; every other draw is unchanged.  'fps' takes frames of up to 65536 points."""
        cfg = self.config
        if point_sampling not in ("random", "fps"):
            raise ValueError("point_sampling must be 'random' or 'fps'")
        fps = point_sampling == "fps"
        if loader_type not in ("train", "val", "test"):
            raise AssertionError(f"Invalid loader type {loader_type}")
        if cfg.get("shuffle_pts", False) or cfg.get("DOUBLE_FLIP", False):
            raise NotImplementedError("shuffle_pts and DOUBLE_FLIP (both off in the shipped configs) are not built")
        if not cfg.get("sampling", True):
            raise NotImplementedError("sampling: False is not built (frames of different lengths would not collate)")
        if crop and polar:
            raise ValueError("crop and polar exclude each other")
        view_cone = bool(cfg.get("view_cone_mode", False))
        flat, offs, width = _pack(scans, 3)
        if not crop:
            flat = np.ascontiguousarray(flat[:, :3])
        dev = torch.device("cuda", torch.cuda.current_device()) if not isinstance(rng, torch.Generator) else rng.device
        x = torch.from_numpy(flat).to(dev)
        counts = None
        if crop:
            x, counts = self.crop(x, offs)
        vox = self.voxelize(x, offs, counts, to_polar=view_cone and not polar, with_voxels=False)
        src = vox["polar"] if vox["polar"] is not None else x
        # the one device -> host read of the batch: N and V size the draws
        n_host = (counts.cpu().numpy().astype(np.int64) if counts is not None else np.diff(offs))
        v_host = vox["voxel_counts"].cpu().numpy().astype(np.int64)
        B = len(n_host)
        S = int(cfg.num_samples)
        train = loader_type == "train"
        in_ratio = int(S * cfg.query_ratio)
        in_num = in_ratio if train else S
        out_num = S - in_num if train else 0
        vsize = np.array(cfg.voxel_size)
        G = self.cells
        sidx, uin, vidx, uout, erank = [], [], [], [], []
        for b in range(B):
            N, V = int(n_host[b]), int(v_host[b])
            if isinstance(rng, torch.Generator):
                if N < S:
                    raise ValueError(f"Error sampling points from {N} points")
                sidx.append(torch.randint(0, N, (1,), generator=rng, device=dev)[0] if fps else
                            torch.randperm(N, generator=rng, device=dev)[:S])
                if load_query:
                    if V == 0:
                        raise ValueError("a cannot be empty unless no samples are taken")
                    lo = torch.tensor(-vsize / 2, device=dev)
                    uin.append(torch.rand((in_num, 3), dtype=torch.float64, generator=rng, device=dev) * (2 * -lo) + lo)
                    uout.append(torch.rand((out_num, 3), dtype=torch.float64, generator=rng, device=dev) * (2 * -lo) + lo)
                    vidx.append(torch.randint(0, V, (in_num,), generator=rng, device=dev))
                    erank.append(torch.randint(0, G - V, (out_num,), generator=rng, device=dev) if out_num else
                                 torch.zeros(0, dtype=torch.int64, device=dev))
                continue
            g = (lambda: rng) if isinstance(rng, np.random.Generator) else np.random.default_rng
            if fps:
                if N < S:
                    raise ValueError(f"Error sampling points from {N} points")
                sidx.append(int(g().integers(0, N)))
            else:
                try:
                    sidx.append(g().choice(N, S, replace=False))
                except ValueError:
                    raise ValueError(f"Error sampling points from {N} points")
            if not load_query:
                continue
            if train:
                uin.append(g().uniform(low=-vsize / 2, high=vsize / 2, size=(in_num, 3)))
                uout.append(g().uniform(low=-vsize / 2, high=vsize / 2, size=(out_num, 3)))
                vidx.append(g().choice(V, in_num, replace=True))
                erank.append(torch.randint(0, G - V, (out_num,)).numpy())
            else:
                uin.append(g().uniform(low=-vsize / 2, high=vsize / 2, size=(S, 3)))
                vidx.append(g().choice(V, S, replace=True))
        up = lambda xs, dt: (torch.stack([torch.as_tensor(v) for v in xs]).to(device=dev, dtype=dt).contiguous() if xs else None)
        sample_idx = up(sidx, torch.int64)
        if fps:                                 # sidx: one start per frame; the S rows come from the sampler, on the device
            from . import postprocess as PP
            longest = int(n_host.max())
            if longest > PP.FPS_MAX_POINTS:
                raise ValueError(f"point_sampling='fps' takes frames of up to {PP.FPS_MAX_POINTS} points, got {longest}")
            sample_idx = PP.farthest_point_sample_ragged(src, torch.from_numpy(offs).to(dev), S, longest, counts=counts, start=sample_idx,
                                                         scale=fps_scale(cfg))
        if load_query:
            u_in, voxel_idx = up(uin, torch.float64), up(vidx, torch.int64)
            u_out, empty_rank = (up(uout, torch.float64), up(erank, torch.int64)) if out_num else (None, None)
            q_in = in_num
        else:                                   # queries off: the samples only (labels / queries of the call are discarded)
            u_in = voxel_idx = u_out = empty_rank = None
            q_in = S
            u_in = torch.zeros((B, S, 3), dtype=torch.float64, device=dev)
            voxel_idx = torch.zeros((B, S), dtype=torch.int64, device=dev)
        lp, qp, lab = self.queries(src, offs, S, q_in, sample_idx, u_in, voxel_idx, u_out, empty_rank, vox)
        out = {}
        if not train:
            n_rows = n_host
            out["raw_lidar_points"] = [x[offs[b]:offs[b] + int(n_rows[b])] for b in range(B)]
        out["lidar_points"] = lp
        if load_query:
            out["query_points"] = qp
            out["query_labels"] = lab
            out["in_voxel_num"] = torch.full((B,), in_ratio, dtype=torch.int64)
            out["raw_query_points"] = qp
        return out


# ---------------------------------------------------------------------------------------------------- files and drop-ins
def load_lidar_data(path, return_xyz: bool = True) -> np.ndarray:
    """lidar.py:38-44."""
    pts = np.fromfile(str(path), dtype=np.float32).reshape(-1, NUMBER_RECORDING_ATTRIBUTES)
    return pts[:, :3] if return_xyz else pts


def process_lidar_files(lidar_files: Sequence, lindex: Sequence[int], out_dir, cfg, batch: int = 64) -> int:
    """The lidar.py main loop (:160-182) on the device: for i, index in enumerate(lindex), lidar_files[index] (raw float32 [N, 4]) ->
    out_dir/{i:04d}.bin, float32 [M, 3] cartesian in the radar frame (save_lidar_data's bytes).  `cfg` is a load_lidar_config
    result (its `fov` and `extrinsic` are used).  Returns the number of files written."""
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    h = LidarFrames(cfg)
    lindex = [int(i) for i in lindex]
    for i0 in range(0, len(lindex), batch):
        scans = [load_lidar_data(lidar_files[k], return_xyz=False) for k in lindex[i0:i0 + batch]]
        flat, offs, _ = _pack(scans, 3)
        out, counts = h.crop(torch.from_numpy(flat).cuda(), offs)
        out, counts = out.cpu().numpy(), counts.cpu().numpy()
        for j in range(len(scans)):
            out[offs[j]:offs[j] + counts[j]].astype(np.float32).tofile(out_dir / f"{i0 + j:04d}.bin")
    return len(lindex)


_VOX: Dict[tuple, LidarFrames] = {}


class VoxelGeneratorWrapper:
    """Drop-in for datasets/utils/voxelize.py (spconv's Point2VoxelCPU3d): the same constructor; generate(points) takes numpy
    [N, num_point_features] float32 and returns numpy (voxels [V, max_points, F] float32, coordinates [V, 3] int32 in z, y, x order,
    num_points [V] int32), run on the current GPU."""

    def __init__(self, vsize_xyz, coors_range_xyz, num_point_features, max_num_points_per_voxel, max_num_voxels):
        self.cfg = Config(pc_range=[float(v) for v in coors_range_xyz], voxel_size=[float(v) for v in vsize_xyz],
                          num_point_features=int(num_point_features), max_points_per_voxel=int(max_num_points_per_voxel),
                          max_number_of_voxels=int(max_num_voxels))
        self.spconv_ver = 2
        self._h = LidarFrames(self.cfg)

    def generate(self, points):
        pts = np.ascontiguousarray(np.asarray(points, dtype=np.float32))
        res = self._h.voxelize(torch.from_numpy(pts).cuda(), [0, pts.shape[0]])
        V = int(res["voxel_counts"][0].item())
        return (res["voxels"][0, :V].cpu().numpy(), res["coords"][0, :V].cpu().numpy(), res["num_points"][0, :V].cpu().numpy())
