"""The ~15 lines of the reference's generation engine that call the hot path
(engine_generation.py:183-232, :274-300), restated as a batch-sharded driver: radar cube ->
EDMPrecond.sample -> vae.decode on query sets -> occupancy = logits > 0, plus the per-frame
inference tail (:250-322: query generation, helper points, refine pass, Chamfer) kept on the device.
Data loading and PLY writing are out of scope."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import distributed as D
from . import postprocess as PP
from . import query_points as QP
from .postprocess import _positive, _whole


@torch.no_grad()
def sample_and_decode(model, vae, radar_cube: torch.Tensor, query_sets: Sequence[torch.Tensor],
                      batch_seeds: Optional[torch.Tensor] = None, sampler_kwargs: Optional[dict] = None) -> Dict[str, object]:
    """One evaluation batch on ONE rank: `model.sample` (18 Heun steps, condition encoded once),
    then every query set decoded against the same latents (the 24-layer latent stack runs once:
    rald_amd.models_ae memoises the decoder context per latent tensor).  `sampler_kwargs` goes to `model.sample`
    (num_steps, S_churn, S_min, S_max, S_noise, rng).
    Returns {'latents': [B,512,C], 'logits': [ [B,Q_i] ... ], 'occupied': [bool masks]}."""
    sampled = model.sample(cond=radar_cube, batch_seeds=batch_seeds, cond_type='radar', **(sampler_kwargs or {}))        # :195
    logits = [vae.decode(sampled, q).squeeze(-1) for q in query_sets]                          # :204, :275, :300
    return {"latents": sampled, "logits": logits, "occupied": [l > 0 for l in logits]}        # :229-232


@torch.no_grad()
def chamfer_of_decode(logits: torch.Tensor, queries: torch.Tensor, surface: torch.Tensor, lidar_pc_range,
                      norm_anisotropy: bool = True, norm_isotropy: bool = False, view_cone_mode: bool = True) -> float:
    """engine_generation.py:283-322 for one sample, on the device: positives of `logits` [Q] ->
    metric (cartesian) coordinates, ground-truth `surface` [P,3] likewise, Chamfer distance."""
    pred = PP.occupied_points(logits, queries, lidar_pc_range, norm_anisotropy, norm_isotropy, view_cone_mode)
    gt = PP.inverse_norm_points(surface, lidar_pc_range, norm_anisotropy, norm_isotropy)
    if view_cone_mode:
        gt = PP.polar2cartesian(gt)
    return PP.cal_metrics(pred, gt)


def _get(ns, name, default=None):
    return ns.get(name, default) if hasattr(ns, "get") else getattr(ns, name, default)


@torch.no_grad()
def infer_point_cloud(vae, sampled_tokens: torch.Tensor, args, helper_points: Optional[torch.Tensor] = None,
                      surface: Optional[torch.Tensor] = None, rng: Optional[torch.Generator] = None) -> Dict[str, object]:
    """engine_generation.py:250-322 for ONE sample (the reference asserts batch 1 when helper points are
    used), everything between the sampler and the metric on the device:
    uniform (or cartesian-box) queries [+ helper points] -> vae.decode -> positives -> un-normalised polar
    points -> [refine: jittered copies -> normalise -> decode -> positives] -> cartesian if view_cone_mode
    -> Chamfer distance against `surface` (normalised ground truth [P,3]) unless skip_eval_metric.
    `rng=None` consumes numpy's global RNG in the reference's order; a device generator avoids host draws.
    Returns {'pred': [n,3] metric coordinates, 'cd': float or None, 'n_queries': int}."""
    if sampled_tokens.shape[0] != 1:
        raise AssertionError("Batch size should be 1 when using query helper points")          # :265
    lidar, inf = args.dataset.lidar, args.eval.inference
    aniso, iso = lidar.norm_anisotropy, lidar.norm_isotropy
    dev = sampled_tokens.device
    if _get(args.eval, "use_cart_query", False):
        grid = QP.generate_cart_query_points(args, device=dev, rng=rng)                        # :251-256
    else:
        grid = QP.generate_query_points(args, device=dev, rng=rng)                             # :258
    if _get(inf, "query_helper", False) and helper_points is not None:
        grid = torch.cat((grid, helper_points.to(dev, torch.float32).reshape(-1, 3)), dim=0)    # :264-271
    output = vae.decode(sampled_tokens, grid[None]).squeeze(-1)[0]                              # :275
    pred = PP.occupied_points(output, grid, lidar.pc_range, aniso, iso, view_cone_mode=False)   # :283-289
    n_queries = grid.shape[0]
    if _get(inf, "refine_query", False):
        refined = QP.refine_queries(pred, args, rng=rng)                                        # :292-297
        out_r = vae.decode(sampled_tokens, refined[None]).squeeze(-1)[0]                        # :300
        pred = PP.occupied_points(out_r, refined, lidar.pc_range, aniso, iso, view_cone_mode=False)   # :304-310
        n_queries += refined.shape[0]
    view_cone = bool(_get(lidar, "view_cone_mode", False))
    if view_cone:
        pred = PP.polar2cartesian(pred)                                                         # :313-315
    cd = None
    if surface is not None and not _get(args.eval, "skip_eval_metric", False):
        gt = PP.inverse_norm_points(surface.to(dev), lidar.pc_range, aniso, iso)                 # :290
        cd = PP.cal_metrics(pred, PP.polar2cartesian(gt) if view_cone else gt)                   # :320
    return {"pred": pred, "cd": cd, "n_queries": n_queries}


def offsets_from_lengths(lengths: Sequence[int]) -> List[int]:
    """Host offsets [B+1] of a ragged layout from its B segment lengths (offsets[0] = 0; a length of 0 is an empty segment)."""
    out = [0]
    for n in lengths:
        n = int(n)
        if n < 0:
            raise ValueError("segment lengths must be non-negative")
        out.append(out[-1] + n)
    return out


def _check_batch_inputs(sampled_tokens, helper_points, surfaces) -> List[Optional[torch.Tensor]]:
    """The shape and length rules of infer_point_clouds, all on the host: raises ValueError before any GPU work."""
    if not isinstance(sampled_tokens, torch.Tensor) or sampled_tokens.dim() != 3:
        raise ValueError("sampled_tokens must be [B, M, C]")
    B = sampled_tokens.shape[0]
    if B < 1:
        raise ValueError("sampled_tokens must hold at least one frame")
    helpers: List[Optional[torch.Tensor]] = [None] * B
    if helper_points is not None:
        if isinstance(helper_points, torch.Tensor) or len(helper_points) != B:
            raise ValueError(f"helper_points must be a list of {B} tensors [H_b, 3], one per frame")
        for b, h in enumerate(helper_points):
            if not isinstance(h, torch.Tensor) or h.dim() != 2 or h.shape[1] != 3:
                raise ValueError(f"helper_points[{b}] must be a tensor [H_b, 3]")
        helpers = list(helper_points)
    if surfaces is not None:
        if not isinstance(surfaces, torch.Tensor) or surfaces.dim() != 3 or surfaces.shape[2] != 3:
            raise ValueError("surfaces must be [B, P, 3]")
        if surfaces.shape[0] != B:
            raise ValueError(f"surfaces holds {surfaces.shape[0]} frames, sampled_tokens {B}")
        if surfaces.shape[1] < 1:
            raise ValueError("surfaces must hold at least one point per frame")
    return helpers


def _batch_queries(grid: torch.Tensor, n_grid, helpers: List[Optional[torch.Tensor]], B: int):
    """The ragged query sets of the first decode: every frame = the shared grid + its own helper points.
    grid [n_cap,3]; n_grid = n_cap as an int, or (use_cart_query) a device int64 [1] count of the valid grid rows.
    -> (queries [T_cap,3], offsets int64 [B+1] on the device, max_per_sample)."""
    dev = grid.device
    n_cap = grid.shape[0]
    h_len = [0 if h is None else h.shape[0] for h in helpers]
    parts = [h.to(dev, torch.float32) for h in helpers if h is not None and h.shape[0]]
    if isinstance(n_grid, int):
        rows = []
        for h in helpers:
            rows.append(grid)
            if h is not None and h.shape[0]:
                rows.append(h.to(dev, torch.float32))
        offsets = torch.tensor(offsets_from_lengths([n_cap + n for n in h_len]), dtype=torch.int64, device=dev)
        return torch.cat(rows, dim=0), offsets, n_cap + max(h_len)
    # the FoV filter leaves a number of grid rows only the device knows: gather every frame's rows out of [grid | all helper points]
    # by index arithmetic on the device (row r of frame b is grid row r below the count, else the frame's helper row r - count)
    h_off = torch.tensor(offsets_from_lengths(h_len), dtype=torch.int64, device=dev)
    offsets = torch.arange(B + 1, dtype=torch.int64, device=dev) * n_grid + h_off
    source = torch.cat([grid] + parts, dim=0) if parts else grid
    t_cap = B * n_cap + sum(h_len)
    pos = torch.arange(t_cap, dtype=torch.int64, device=dev)
    frame = (torch.searchsorted(offsets, pos, right=True) - 1).clamp_(0, B - 1)
    local = pos - offsets[frame]
    src = torch.where(local < n_grid, local, n_cap + h_off[frame] + (local - n_grid)).clamp_(0, source.shape[0] - 1)
    return source[src], offsets, n_cap + max(h_len)


@torch.no_grad()
def infer_point_clouds_device(vae, sampled_tokens: torch.Tensor, args, helper_points=None, surfaces: Optional[torch.Tensor] = None,
                              rng: Optional[torch.Generator] = None, draws: Optional[dict] = None, metric_thresholds=None,
                              normals: bool = False, surface_steps: int = 0, surface_max_step: float = 0.05, resample: Optional[int] = None,
                              thin=None, denoise=None, denoise_statistical=None, normal_consistency=None, denoise_cluster=None,
                              remove_planes=None):
    """infer_point_clouds (see there for the options) without its readback -> a tuple, all on the device, in this order:
    points [T_cap,3], offsets int64 [B+1], cd float64 [B] or None: frame b's prediction is points[offsets[b]:offsets[b+1]];
    with `metric_thresholds` (a sequence of distances, () included) the dict of postprocess.cloud_metrics_ragged (None where no metric
    is computed), whose 'cd' is the third element; with `normals` or `surface_steps` the unit normals [T_cap,3]; with
    `normal_consistency` normal_consistency float64 [B,3] and the surfaces' estimated normals [B*P,3];
    with `denoise`, `denoise_statistical` or `denoise_cluster`: denoised [T_cap,3], denoise_offsets int64 [B+1], denoise_index int64
    [T_cap], cd_denoised float64 [B] or None and, with `metric_thresholds`, the dict of the denoised clouds' metrics (or None); behind
    them denoise_stats float64 [B,3] (mu, sigma, the threshold) of the statistical filter, or denoise_labels int32 [T_cap] (per row of
    `denoised`) and n_clusters int32 [B] of the cluster filter, or with `remove_planes` denoise_labels int32 [T_cap], planes float64
    [B, max_planes, 4] and num_planes int32 [B]; thin and resample then run on the denoised clouds, their indices count its rows;
    with `thin`: thinned [T_cap,3], thin_offsets int64 [B+1], thin_count int32 [T_cap], thin_first int64 [T_cap] - frame b's voxels are
    rows thin_offsets[b] .. thin_offsets[b+1]-1; with `resample=k`, last, the resampled clouds [B,k,3] and their row indices [B,k]
    (rows of the frame's thinned cloud with `thin`).  With a device generator (`rng`) or explicit `draws` nothing is read to the host
    and the device is not synchronised."""
    t, thinned, resampled = _tail_on_device(vae, sampled_tokens, args, helper_points, surfaces, rng, draws, metric_thresholds, normals,
                                            surface_steps, surface_max_step, resample, thin, denoise, denoise_statistical, normal_consistency,
                                            denoise_cluster, remove_planes)
    with_metrics, den = metric_thresholds is not None, t.denoised
    out = (t.points, t.offsets, t.cd) + ((t.metrics,) if with_metrics else ()) + ((t.normals,) if t.normals is not None else ()) + (t.ncons or ())
    if den is not None:
        out += (den.points, den.offsets, den.index, den.cd) + ((den.metrics,) if with_metrics else ())
        out += ((den.stats,) if den.stats is not None else ()) + ((den.labels, den.n_clusters) if den.n_clusters is not None else ())
        out += (den.labels, den.planes, den.n_planes) if den.planes is not None else ()
    return out + (thinned or ()) + (resampled or ())


@dataclass
class _Denoised:
    """The tail's clouds behind one of the four filters, on the device: the kept rows, their offsets int64 [B+1], their rows in the full
    cloud, cd / metrics against the same surfaces; stats float64 [B,3] (statistical), labels int32 per kept row (cluster, plane),
    n_clusters int32 [B] (cluster), planes float64 [B,K,4] and n_planes int32 [B] (plane)."""
    points: torch.Tensor; offsets: torch.Tensor; index: torch.Tensor; cd: Optional[torch.Tensor] = None; metrics: Optional[dict] = None
    stats: Optional[torch.Tensor] = None; labels: Optional[torch.Tensor] = None; n_clusters: Optional[torch.Tensor] = None
    planes: Optional[torch.Tensor] = None; n_planes: Optional[torch.Tensor] = None


@dataclass
class _Tail:
    """The batched tail's results on the device: the final clouds, their offsets int64 [B+1], cd float64 [B], the frames' query counts int64
    [B], cloud_metrics_ragged's dict, the unit normals, the host bound of the longest final cloud, the denoised clouds, the pair (normal
    consistency float64 [B,3], the surfaces' estimated normals); None for what was not asked for or not computed."""
    points: torch.Tensor; offsets: torch.Tensor; cd: Optional[torch.Tensor]; n_queries: torch.Tensor
    metrics: Optional[dict]; normals: Optional[torch.Tensor]; longest: int; denoised: Optional[_Denoised]; ncons: Optional[tuple]
    aligned: Optional["_Aligned"] = None


@dataclass
class _Aligned:
    """The final clouds registered onto their surfaces, on the device: register_icp_ragged's transform float64 [B,4,4], fitness and
    inlier_rmse float64 [B], status int32 [B], the final clouds under the transform (laid out like the tail's points), and cd / metrics
    of those against the same surfaces."""
    transform: torch.Tensor; fitness: torch.Tensor; rmse: torch.Tensor; status: torch.Tensor; points: torch.Tensor
    cd: Optional[torch.Tensor] = None; metrics: Optional[dict] = None


class _Align(NamedTuple):
    mode: int; max_distance: float; max_iterations: int; grid: tuple; normals_of: Optional[tuple]


# the four filters as _check_denoise, _check_denoise_statistical, _check_denoise_cluster and _check_remove_planes return them, plain
# tuples with names: each
# run(points, offsets, bound) -> the _Denoised clouds, with the kept rows' indices and what its filter adds
class _RadiusFilter(NamedTuple):
    radius: float; min_neighbors: int; grid: tuple

    def run(self, points, offsets, bound) -> _Denoised:
        return _Denoised(*PP.remove_radius_outliers_ragged(points, offsets, self.radius, self.min_neighbors, self.grid, bound, return_index=True))


class _StatisticalFilter(NamedTuple):
    kind: str; k: int; std_ratio: float; grid: tuple; max_radius: Optional[float]

    def run(self, points, offsets, bound) -> _Denoised:
        pts, off, idx, stats = PP.remove_statistical_outliers_ragged(points, offsets, self.k, self.std_ratio, self.grid, bound,
                                                                     max_radius=self.max_radius, return_index=True, return_stats=True)
        return _Denoised(pts, off, idx, stats=stats)


class _ClusterFilter(NamedTuple):
    kind: str; eps: float; min_points: int; min_cluster_size: int; largest_only: bool; grid: tuple

    def run(self, points, offsets, bound) -> _Denoised:
        pts, off, idx, labels, num = PP.remove_small_clusters_ragged(points, offsets, self.eps, self.min_points, self.min_cluster_size,
                                                                     self.grid, bound, largest_only=self.largest_only, return_index=True,
                                                                     return_labels=True)
        return _Denoised(pts, off, idx, labels=labels, n_clusters=num)


class _PlaneFilter(NamedTuple):
    kind: str; threshold: float; num_hypotheses: int; max_planes: int; keep_planes: bool; seed: int

    def run(self, points, offsets, bound) -> _Denoised:
        pts, off, idx, labels, planes, num = PP.remove_planes_ragged(points, offsets, self.threshold, bound, self.num_hypotheses,
                                                                     self.max_planes, seed=self.seed, view=(0.0, 0.0, 0.0),
                                                                     keep_planes=self.keep_planes, return_index=True, return_labels=True)
        return _Denoised(pts, off, idx, labels=labels, planes=planes, n_planes=num)


def _check_resample(resample) -> Optional[int]:
    if resample is None:
        return None
    if isinstance(resample, bool) or int(resample) != resample or resample < 1:
        raise ValueError("resample must be None or a positive integer")
    return int(resample)


def _thin_grid(thin, args):
    """The grid of `thin` (None, or the cell edge: a number or 3) in the final clouds' coordinates -> None or postprocess.voxel_grid's
    triple: the cube [-r_max, r_max]^3 (r_max = pc_range[3]) in view-cone mode, where the clouds are cartesian, else pc_range itself.
    ValueError for a bad edge or too many cells, on the host."""
    if thin is None:
        return None
    lidar = args.dataset.lidar
    rng = [float(v) for v in lidar.pc_range]
    if bool(_get(lidar, "view_cone_mode", False)):
        return PP.voxel_grid([-rng[3]] * 3, [rng[3]] * 3, thin)
    return PP.voxel_grid(rng[:3], rng[3:], thin)


def _check_denoise(denoise, args):
    """`denoise` (None, or (radius, min_neighbors)) -> None or (radius, min_neighbors, grid): the search grid is _thin_grid's box with
    the cell edge `radius`.  ValueError for anything else, and for a radius so small that the box has more than 2^31 - 1 cells, on the
    host."""
    if denoise is None:
        return None
    try:
        radius, k = denoise
    except (TypeError, ValueError):
        raise ValueError("denoise must be None or (radius, min_neighbors)") from None
    radius = _positive(radius, "denoise: radius must be a finite number > 0")
    return _RadiusFilter(radius, _whole(k, 1, None, "denoise: min_neighbors must be an integer >= 1"), _thin_grid(radius, args))


def _three_or_four(option, fourth, message: str):
    """A sequence of three or four -> its four values, `fourth` where it has three; ValueError(message) for anything else."""
    try:
        a, b, c = option[:3]
        if len(option) in (3, 4):
            return a, b, c, (option[3] if len(option) == 4 else fourth)
    except (TypeError, ValueError):
        pass
    raise ValueError(message)


def _check_denoise_statistical(stat, denoise, args):
    """`denoise_statistical` (None, or (k, std_ratio, cell) or (k, std_ratio, cell, max_radius)) -> None or ('statistical', k, std_ratio,
    grid, max_radius or None): the search grid is _thin_grid's box with the cell edge `cell`.  ValueError for anything else, for a cell
    that gives the box more than 2^31 - 1 cells, and for `denoise` given as well (chaining the two filters is not offered), on the host."""
    if stat is None:
        return None
    if denoise is not None:
        raise ValueError("denoise and denoise_statistical exclude each other")
    k, ratio, cell, max_radius = _three_or_four(stat, None, "denoise_statistical must be None, (k, std_ratio, cell) or "
                                                            "(k, std_ratio, cell, max_radius)")
    k, ratio = PP._knn_k(k), PP._knn_ratio(ratio)
    if max_radius is not None:
        PP._knn_radius(max_radius)
        max_radius = float(max_radius)
    cell = _positive(cell, "denoise_statistical: cell must be a finite number > 0")
    return _StatisticalFilter("statistical", k, ratio, _thin_grid(cell, args), max_radius)


def _check_denoise_cluster(clu, denoise, stat, args):
    """`denoise_cluster` (None, or (eps, min_points, min_cluster_size) or (eps, min_points, min_cluster_size, largest_only)) -> None or
    ('cluster', eps, min_points, min_cluster_size, largest_only, grid): the search grid is _thin_grid's box with the cell edge eps.
    ValueError for anything else, for an eps that gives the box more than 2^31 - 1 cells, and for `denoise` or `denoise_statistical`
    given as well (chaining the filters is not offered), on the host."""
    if clu is None:
        return None
    if denoise is not None or stat is not None:
        raise ValueError("denoise_cluster excludes denoise and denoise_statistical")
    eps, min_points, min_size, largest = _three_or_four(clu, False, "denoise_cluster must be None, (eps, min_points, min_cluster_size) or "
                                                                    "(eps, min_points, min_cluster_size, largest_only)")
    eps = _positive(eps, "denoise_cluster: eps must be a finite number > 0")
    min_points = _whole(min_points, 0, None, "denoise_cluster: min_points must be an integer >= 0")
    if not isinstance(largest, (bool, int)):
        raise ValueError("denoise_cluster: largest_only must be a bool")
    return _ClusterFilter("cluster", eps, min_points, PP._cluster_size(min_size), bool(largest), _thin_grid(eps, args))


def _check_remove_planes(rp, denoise, stat, clu, rng):
    """`remove_planes` (None, or (threshold, num_hypotheses), (threshold, num_hypotheses, max_planes) or (threshold, num_hypotheses,
    max_planes, keep_planes)) -> None or ('plane', threshold, num_hypotheses, max_planes, keep_planes, seed): the seed is the low 32 bits
    of `rng`'s initial seed (a host value) if the call has a generator, else 0.  ValueError for anything else and for any of the three
    other filters given as well (chaining the filters is not offered), on the host."""
    if rp is None:
        return None
    if denoise is not None or stat is not None or clu is not None:
        raise ValueError("remove_planes excludes denoise, denoise_statistical and denoise_cluster")
    message = ("remove_planes must be None, (threshold, num_hypotheses), (threshold, num_hypotheses, max_planes) or "
               "(threshold, num_hypotheses, max_planes, keep_planes)")
    try:
        rp = tuple(rp)
    except TypeError:
        raise ValueError(message) from None
    if len(rp) not in (2, 3, 4):
        raise ValueError(message)
    threshold, H = rp[:2]
    K, keep = (rp[2] if len(rp) >= 3 else 1), (rp[3] if len(rp) == 4 else False)
    threshold = _positive(threshold, "remove_planes: threshold must be a finite number > 0")
    H = _whole(H, 1, PP.PLANE_MAX_HYPOTHESES, f"remove_planes: num_hypotheses must be an integer in 1 .. {PP.PLANE_MAX_HYPOTHESES}")
    K = _whole(K, 1, PP.PLANE_MAX_PLANES, f"remove_planes: max_planes must be an integer in 1 .. {PP.PLANE_MAX_PLANES}")
    if not isinstance(keep, (bool, int)) or keep not in (0, 1):
        raise ValueError("remove_planes: keep_planes must be a bool")
    return _PlaneFilter("plane", threshold, H, K, bool(keep), int(rng.initial_seed()) & 0xFFFFFFFF if rng is not None else 0)


def _check_normal_consistency(nc, args, surfaces, normals, surface_steps):
    """`normal_consistency` (None, or (k, cell)) -> None or (k, grid): the search grid of the surfaces' normals is _thin_grid's box with
    the cell edge `cell`.  ValueError for anything else, for a cell that gives the box more than 2^31 - 1 cells, and where the tail has
    no `surfaces` to estimate normals on or no predicted normals (`normals` / `surface_steps`) to compare them with, on the host."""
    if nc is None:
        return None
    try:
        k, cell = nc
    except (TypeError, ValueError):
        raise ValueError("normal_consistency must be None or (k, cell)") from None
    k = PP._knn_k(k)
    cell = _positive(cell, "normal_consistency: cell must be a finite number > 0")
    if surfaces is None:
        raise ValueError("normal_consistency needs surfaces")
    if not (bool(normals) or int(surface_steps) > 0):
        raise ValueError("normal_consistency needs the predicted normals: normals=True or surface_steps > 0")
    return k, _thin_grid(float(cell), args)


def _check_align(align, args, surfaces, normal_consistency):
    """`align` (None, or (mode, max_distance), (mode, max_distance, max_iterations) or, for plane mode without `normal_consistency`,
    (mode, max_distance, max_iterations, k, cell)) -> None or (mode 0 / 1, max_distance, max_iterations, grid, (k, normals grid) or
    None): the search grid is _thin_grid's box with the cell edge max_distance; plane mode estimates the surfaces' normals from (k,
    cell), its own or `normal_consistency`'s.  ValueError for anything else, for too many cells, and without `surfaces`, on the host."""
    if align is None:
        return None
    message = "align must be None, (mode, max_distance), (mode, max_distance, max_iterations) or (mode, max_distance, max_iterations, k, cell)"
    try:
        align = tuple(align)
    except TypeError:
        raise ValueError(message) from None
    if len(align) not in (2, 3, 5):
        raise ValueError(message)
    mode = PP._icp_mode(align[0])
    max_distance = _positive(align[1], "align: max_distance must be a finite number > 0")
    iterations = _whole(align[2] if len(align) >= 3 else 30, 1, PP.ICP_MAX_ITERATIONS,
                        f"align: max_iterations must be an integer in 1 .. {PP.ICP_MAX_ITERATIONS}")
    if surfaces is None:
        raise ValueError("align needs surfaces")
    normals_of = None
    if mode == 1:
        knn = align[3:] if len(align) == 5 else normal_consistency
        if knn is None:
            raise ValueError("align: plane mode needs (k, cell) for the surfaces' normals, as its fourth and fifth entry or from normal_consistency")
        try:
            k, cell = knn
        except (TypeError, ValueError):
            raise ValueError(message) from None
        normals_of = (PP._knn_k(k), _thin_grid(_positive(cell, "align: cell must be a finite number > 0"), args))
    return _Align(mode, max_distance, iterations, _thin_grid(max_distance, args), normals_of)


def _thin(pts: torch.Tensor, off: torch.Tensor, grid, longest: int):
    """The final clouds, one centroid per occupied cell -> (thinned [T,3], thin_offsets [B+1], thin_count [T], thin_first [T]); after
    the metric, which keeps the full cloud."""
    return PP.voxel_downsample_ragged(pts, off, grid, max(1, int(longest)), return_count=True, return_first=True)


def _thin_bound(longest: int, grid) -> int:
    """Host bound of the longest thinned cloud: no more voxels than rows, nor than cells."""
    return min(int(longest), grid[2][0] * grid[2][1] * grid[2][2])


def _resample(pts: torch.Tensor, off: torch.Tensor, k: int, longest: int):
    """The final clouds as k evenly spread points each -> (resampled [B,k,3], index [B,k]); after the metric, which keeps the full cloud."""
    return PP.resample_points_ragged(pts, off, k, max(1, min(int(longest), PP.FPS_MAX_POINTS)), return_index=True)


def _metric(pts, off, gt, gt_off, max_pred, max_gt, thresholds):
    """The tail's metric stage -> (cd float64 [B], metrics): Chamfer alone, or with thresholds cloud_metrics_ragged's dict and its 'cd'."""
    if thresholds is None:
        return PP.cal_metrics_ragged(pts, off, gt, gt_off, max_pred, max_gt), None                 # :320
    metrics = PP.cloud_metrics_ragged(pts, off, gt, gt_off, max_pred, max_gt, thresholds)
    return metrics["cd"], metrics


class _HostPack:
    """One host read of many small device tensors: add(name, group) (or a keyword each) collects them - a tensor, cloud_metrics_ragged's
    dict (its METRIC_KEYS in order) or None (not computed: no group) - and read() makes the one copy (everything as float64,
    concatenated) -> {name: the flat list of its values as floats}; integer groups are cast back by the caller."""
    def __init__(self, **groups):
        self.groups = {}
        for name, group in groups.items():
            self.add(name, group)

    def add(self, name: str, group) -> None:
        if group is not None:
            tensors = [group[k] for k in PP.METRIC_KEYS] if isinstance(group, dict) else [group]
            self.groups[name] = [t.reshape(-1).double() for t in tensors]

    def read(self) -> Dict[str, list]:
        host = torch.cat([t for group in self.groups.values() for t in group]).cpu().tolist()       # the one host read
        ends = np.cumsum([sum(t.numel() for t in group) for group in self.groups.values()]).tolist()
        return {name: host[lo:hi] for name, lo, hi in zip(self.groups, [0] + ends, ends)}


def _tail_on_device(vae, sampled_tokens, args, helper_points, surfaces, rng, draws, metric_thresholds, normals, surface_steps, surface_max_step,
                    resample, thin, denoise, denoise_statistical, normal_consistency, denoise_cluster, remove_planes=None, align=None):
    """What both batched entry points do, with their arguments -> (_Tail, _thin's four or None, _resample's pair or None): every option
    checked on the host, the batched tail on the device, the filter chosen behind the metric of the full cloud with a metric of its own,
    then the finishing chain on the denoised clouds if there are any, else on the full ones: thin, then resample."""
    resample, thin_grid = _check_resample(resample), _thin_grid(thin, args)
    # at most one of the four filters: each check refuses the ones named before it ("exclude each other" / "excludes")
    denoise = (_check_remove_planes(remove_planes, denoise, denoise_statistical, denoise_cluster, rng)
               or _check_denoise_cluster(denoise_cluster, denoise, denoise_statistical, args)
               or _check_denoise_statistical(denoise_statistical, denoise, args) or _check_denoise(denoise, args))
    ncons = _check_normal_consistency(normal_consistency, args, surfaces, normals, surface_steps)
    al = _check_align(align, args, surfaces, normal_consistency)
    oriented = bool(normals) or int(surface_steps) > 0
    if metric_thresholds is not None:
        metric_thresholds = PP._thresholds(metric_thresholds)
    helpers = _check_batch_inputs(sampled_tokens, helper_points, surfaces)
    B = sampled_tokens.shape[0]
    lidar, inf = args.dataset.lidar, args.eval.inference
    aniso, iso = lidar.norm_anisotropy, lidar.norm_isotropy
    if not (aniso or iso):
        raise ValueError("one of norm_anisotropy / norm_isotropy is required")
    dev = sampled_tokens.device
    n = int(inf.num_query_points)
    refine = bool(_get(inf, "refine_query", False))
    aug_num = int(inf.refine_query_aug_num) if refine else 0
    host_draws = draws is None and rng is None
    if draws is None and rng is not None:
        draws = QP.draw_tail_randoms(B, n, aug_num, int(inf.refine_query_scale) if refine else 1, rng)
    u3n = torch.from_numpy(np.random.random_sample((3, n))).to(dev) if host_draws else draws["u3n"]
    if u3n.dtype != torch.float64 or tuple(u3n.shape) != (3, n) or not u3n.is_cuda:
        raise ValueError(f"draws['u3n'] must be a float64 tensor [3, {n}] on the GPU")
    if _get(args.eval, "use_cart_query", False):                                                   # :251-256
        grid, n_grid = QP.cart_queries_from_uniform_device(u3n, args)
    else:
        grid, n_grid = QP.uniform_queries_from(u3n, lidar.pc_range, aniso, iso), n                 # :258
    if not _get(inf, "query_helper", False):
        helpers = [None] * B
    queries, offsets, longest = _batch_queries(grid, n_grid, helpers, B)                           # :264-271
    logits = vae.decode_ragged(sampled_tokens, queries, offsets, longest)                          # :275
    pts, p_off, p_idx = PP.occupied_points_ragged(logits, queries, offsets, lidar.pc_range, aniso, iso, view_cone_mode=False,
                                                  return_index=oriented and not refine)                                    # :283-289
    kept_src, kept_off = queries, offsets
    n_queries = offsets[1:] - offsets[:-1]
    if refine:
        if host_draws:
            draws = _numpy_refine_draws(p_off, aug_num, int(inf.refine_query_scale), dev)
        refined, r_off = QP.refine_queries_ragged(pts, p_off, args, draws)                         # :292-297
        logits_r = vae.decode_ragged(sampled_tokens, refined, r_off, aug_num)                      # :300
        pts, p_off, p_idx = PP.occupied_points_ragged(logits_r, refined, r_off, lidar.pc_range, aniso, iso, view_cone_mode=False,
                                                      return_index=oriented)                                               # :304-310
        kept_src, kept_off = refined, r_off
        n_queries = n_queries + (r_off[1:] - r_off[:-1])
        longest = aug_num
    view_cone = bool(_get(lidar, "view_cone_mode", False))
    nrm = None
    if oriented:
        # the kept queries in normalised coordinates (row r of frame b is query p_idx[r] of that frame's set), moved onto the surface if
        # asked, then the gradient there: positions and normals in one pass.  All by device offsets; rows past the last frame unspecified
        pos = torch.arange(pts.shape[0], dtype=torch.int64, device=dev)
        frame = (torch.searchsorted(p_off, pos, right=True) - 1).clamp_(0, B - 1)
        kept = kept_src[(kept_off[frame] + p_idx).clamp_(0, kept_src.shape[0] - 1)]
        kept, _, grad = QP.project_to_surface_ragged(vae, sampled_tokens, kept, p_off, longest, int(surface_steps), surface_max_step)
        pts, nrm = PP.oriented_points_ragged(kept, grad, p_off, lidar.pc_range, aniso, iso, view_cone_mode=view_cone)
    elif view_cone:
        pts = PP.polar2cartesian(pts)                                                              # :313-315 (rows past the last frame: unspecified)
    cd = metrics = den = ncd = thinned = resampled = aligned = None
    with_metric = surfaces is not None and not _get(args.eval, "skip_eval_metric", False)
    if with_metric or ncons is not None or al is not None:
        P = surfaces.shape[1]
        gt = PP.inverse_norm_points(surfaces.to(dev).reshape(-1, 3), lidar.pc_range, aniso, iso)   # :290
        if view_cone:
            gt = PP.polar2cartesian(gt)
        gt_off = torch.arange(B + 1, dtype=torch.int64, device=dev) * P
    if ncons is not None:                                                                          # the sensor sits at the origin of the final frame
        gt_nrm = PP.estimate_normals_ragged(gt, gt_off, ncons[0], ncons[1], max(1, int(P)), view=(0.0, 0.0, 0.0))
        ncd = (PP.normal_consistency_ragged(pts, nrm, p_off, gt, gt_nrm, gt_off, longest, P)[0], gt_nrm)
    if with_metric:
        cd, metrics = _metric(pts, p_off, gt, gt_off, longest, P, metric_thresholds)
    if denoise is not None:                                                                        # after the metric, which keeps the full cloud
        den = denoise.run(pts, p_off, max(1, int(longest)))
        if with_metric:
            den.cd, den.metrics = _metric(den.points, den.offsets, gt, gt_off, longest, P, metric_thresholds)
    if al is not None:                                                                             # the full cloud onto its surfaces
        gt_nrm = None
        if al.mode == 1:
            gt_nrm = ncd[1] if ncd is not None and al.normals_of == ncons else \
                PP.estimate_normals_ragged(gt, gt_off, al.normals_of[0], al.normals_of[1], max(1, int(P)), view=(0.0, 0.0, 0.0))
        reg = PP.register_icp_ragged(pts, p_off, gt, gt_off, al.max_distance, al.grid, max(1, int(longest)), max(1, int(P)),
                                     target_normals=gt_nrm, max_iterations=al.max_iterations, mode=al.mode, return_moved=True)
        aligned = _Aligned(reg["transform"], reg["fitness"], reg["inlier_rmse"], reg["status"], reg["moved"])
        if with_metric:
            aligned.cd, aligned.metrics = _metric(aligned.points, p_off, gt, gt_off, longest, P, metric_thresholds)
    tail = _Tail(pts, p_off, cd, n_queries, metrics, nrm, longest, den, ncd, aligned)
    if den is not None:
        pts, p_off = den.points, den.offsets
    if thin_grid is not None:
        thinned = _thin(pts, p_off, thin_grid, longest)
        pts, p_off, longest = thinned[0], thinned[1], _thin_bound(longest, thin_grid)
    if resample is not None:
        resampled = _resample(pts, p_off, resample, longest)
    return tail, thinned, resampled


def _numpy_refine_draws(p_off: torch.Tensor, aug_num: int, scale: int, dev) -> dict:
    """The refine draws of every frame from numpy's global RNG, frame by frame in the reference's order (query_helper.py:3-42): the
    one host read of the numpy mode - the frames' positive counts - happens here."""
    counts = (p_off[1:] - p_off[:-1]).cpu().numpy()
    B = len(counts)
    sel = np.zeros((B, aug_num), np.int64)
    scales = np.ones((B, aug_num), np.int64)
    u = np.zeros((B, aug_num, 3), np.float64)
    for b, N in enumerate(int(c) for c in counts):
        gen = aug_num - N
        if N > 0 and gen > 0:
            sel[b, :gen] = np.random.choice(N, size=gen, replace=True)
            scales[b, :gen] = np.random.choice(np.arange(scale, step=1) + 1, size=gen)
            u[b, :gen] = np.random.rand(gen, 3)
    return {"sel": torch.from_numpy(sel).to(dev), "scales": torch.from_numpy(scales).to(dev), "u_bias": torch.from_numpy(u).to(dev)}


@torch.no_grad()
def infer_point_clouds(vae, sampled_tokens: torch.Tensor, args, helper_points=None, surfaces: Optional[torch.Tensor] = None,
                       rng: Optional[torch.Generator] = None, draws: Optional[dict] = None, metric_thresholds=None, normals: bool = False,
                       surface_steps: int = 0, surface_max_step: float = 0.05, resample: Optional[int] = None,
                       thin=None, denoise=None, denoise_statistical=None, normal_consistency=None, denoise_cluster=None,
                       remove_planes=None, align=None) -> Dict[str, object]:
    """engine_generation.py:250-322 for a whole batch of frames, on the device from the sampler's latents to the metric:
    one query grid for the batch (the reference repeats its grid over the batch) [+ each frame's helper points] -> ragged decode ->
    positives per frame -> un-normalised polar points -> [refine: jittered copies per frame -> normalise -> ragged decode ->
    positives] -> cartesian if view_cone_mode -> Chamfer distance per frame against `surfaces` [B,P,3] unless skip_eval_metric.
    The frames' sizes differ from the first step on (helper points, positives); every step takes them from device offsets.

    sampled_tokens [B,M,C]; helper_points: None or a list of B tensors [H_b,3] (normalised; H_b may be 0); random numbers from
    `draws` (QP.draw_tail_randoms) or a device generator `rng` - then the ONLY host read is the one at the end, which copies the
    offsets, the query counts and the Chamfer values together.  `rng=None` with `draws=None` replays numpy's global RNG in the
    reference's order - the grid once, then frame by frame the refine pass's three draws - and passes explicit selected indices;
    that mode reads the B positive counts to the host once more, before it draws (numpy's draw sizes depend on them).

    A frame whose first decode has no positive gets no refine queries and ends with an empty prediction and cd = inf; the
    single-frame infer_point_cloud raises there.  Shape and length errors raise ValueError before any GPU work.  Every option below is
    off by default (None, False, 0) and then changes neither the calls, the dict nor the host read; none of them adds a host read.
    `metric_thresholds` (None, or a sequence of up to 8 distances, () included): when given, the metric comes from
    postprocess.cloud_metrics_ragged instead of cal_metrics_ragged - 'cd' keeps its meaning, and 'metrics' holds one dict per frame
    (postprocess.cloud_metrics' keys: accuracy, completeness, cd, cd_l2, hausdorff, mhd as floats; precision, recall, f_score as lists
    per threshold), copied in the same single host read; None where no metric is computed.
    `normals` / `surface_steps`: with either, the queries that the last thresholding kept are gathered in normalised coordinates, moved
    onto the decoder's surface by `surface_steps` Newton steps of at most `surface_max_step` (query_points.project_to_surface_ragged;
    0 = left where they are), and decoded once more with the logit's gradient (KLAutoEncoder.decode_ragged_with_gradient); 'pred' then
    holds those points and a new 'normals' list one unit vector per point [n_b,3] (occupied -> empty; zero where undefined), both from
    postprocess.oriented_points_ragged, and the metric is computed on those points.
    `resample` (None, or k >= 1): every final cloud additionally as exactly k evenly spread points - 'resampled' [B,k,3] (metric
    coordinates, on the device) and 'resample_index' int64 [B,k] (rows of the frame's 'pred'; -1 in padded slots), from
    postprocess.resample_points_ragged (farthest-point sampling from row 0) after the metric, which stays on the full
    cloud.  A frame with fewer than k points repeats its points in order, an empty one gives NaN rows.  The sampler takes clouds of
    up to 65536 points: a frame LONGER than that is sampled from its first 65536 rows only (the rows are in query order, so that is a
    spatial bias) - a caller who expects such frames thins first, with `thin`.
    `thin` (None, or the cell edge in the final clouds' coordinates, a number or 3): every final cloud additionally with one point per
    occupied cell of a fixed grid - the cube [-r_max, r_max]^3, r_max = pc_range[3], in view_cone_mode, else pc_range - from
    postprocess.voxel_downsample_ragged after the metric, which stays on the full cloud: 'thinned' a list of B
    tensors [m_b,3] (the cells' centroids in ascending cell-key order), 'thin_count' a list of int32 [m_b] (rows per cell), 'thin_first'
    a list of int64 [m_b] (the cell's first row of the frame's 'pred'), and with normals / surface_steps 'thinned_normals' [m_b,3], the
    normals of the thin_first rows.  Too many cells (more than 2^31 - 1) raise ValueError before any GPU work.  The thinned offsets join
    the one host read.  With `resample` as well the sampler runs on the THINNED clouds and 'resample_index' counts rows of 'thinned'; a
    thinned cloud above 65536 voxels is still truncated to its first 65536 - now in cell-key order, a slab of the grid - so a coarser
    cell is the remedy.
    `denoise` (None, or (radius, min_neighbors) in the final clouds' coordinates): every final cloud additionally without its isolated
    rows - a row stays iff at least min_neighbors OTHER rows of its frame lie within radius of it, from
    postprocess.remove_radius_outliers_ragged on the box `thin` uses, cell edge = radius (a radius that gives that
    box more than 2^31 - 1 cells raises ValueError before any GPU work).  'pred', 'cd' and 'metrics' stay on the full cloud, untouched.
    Added: 'denoised' a list of B tensors [m_b,3] (the kept rows in their order), 'denoise_index' a list of int64 [m_b] (rows of the
    frame's 'pred'), with normals / surface_steps 'denoised_normals' [m_b,3], with surfaces 'cd_denoised' (B floats, None where no
    metric is computed) and with metric_thresholds 'metrics_denoised' (as 'metrics').  The denoised offsets and metrics join the one
    host read.  `thin` and `resample` then run on the DENOISED clouds: 'thin_first' and (without thin) 'resample_index' count rows of
    'denoised', not of 'pred' - 'denoise_index' maps them back - and 'thinned_normals' are those of the rows thin_first names in 'denoised'.
    `denoise_statistical` (None, or (k, std_ratio, cell) or (k, std_ratio, cell, max_radius)): the statistical outlier filter in
    `denoise`'s place - a row stays iff the mean distance to its k nearest other rows of its frame (within max_radius, if given) is at
    most mu + std_ratio * sigma of its frame's means, from postprocess.remove_statistical_outliers_ragged; it adapts
    to the cloud's density, which thins out with range, where `denoise` needs one radius in metres.  `cell` is the search grid's edge
    over the box `thin` uses (it does not show in the result; k / 8 to k rows per cell is a good edge; a cell that gives the box more
    than 2^31 - 1 cells raises ValueError before any GPU work).  It fills the keys of `denoise` - 'denoised', 'denoise_index',
    'denoised_normals', 'cd_denoised', 'metrics_denoised' - feeds `thin` and `resample` as `denoise` does, and adds 'denoise_stats': B
    triples (mu, sigma, threshold) as floats, NaN for a frame without a row that has a neighbour, carried in the one host read.  Given
    together with `denoise` it raises ValueError: the two filters are not chained.
    `denoise_cluster` (None, or (eps, min_points, min_cluster_size) or (eps, min_points, min_cluster_size, largest_only)): small-cluster
    removal in `denoise`'s place - the frame's rows are clustered by density (a row with at least min_points OTHER rows within eps is a
    core row, core rows within eps of each other share a cluster, other rows join their nearest core row's) and a row stays iff its
    cluster has at least min_cluster_size rows, with largest_only only the frame's largest cluster, from
    postprocess.remove_small_clusters_ragged on the box `thin` uses, cell edge = eps.  It drops the floating blobs
    that both other filters keep, because inside a blob every row has ordinary neighbours.  It fills the keys of `denoise`, feeds `thin`
    and `resample` as `denoise` does, and adds 'denoise_labels', a list of int32 [m_b] (per row of 'denoised' its cluster in the frame's
    numbering before the filter), and 'n_clusters', B ints carried in the one host read.  Given together with `denoise` or
    `denoise_statistical` it raises ValueError.
    `remove_planes` (None, or (threshold, num_hypotheses), (threshold, num_hypotheses, max_planes) or (threshold, num_hypotheses,
    max_planes, keep_planes)): RANSAC plane removal in `denoise`'s place - up to max_planes (default 1) planes are found in turn, each
    the best of num_hypotheses (a fixed number) three-row hypotheses by its rows within `threshold`, re-fitted to them, from
    postprocess.remove_planes_ragged (min_inliers 3, the planes turned towards the sensor at the origin) - and the
    rows of no plane stay (ground removal), with keep_planes the rows of the planes (the faces of an indoor scene).  The hypotheses'
    seed is the low 32 bits of `rng.initial_seed()` when the call has a generator `rng`, else 0: the same call gives the same planes.
    It fills the keys of `denoise`, feeds `thin` and `resample` as `denoise` does, and adds 'denoise_labels', a list of int32 [m_b]
    (per row of 'denoised' the plane that took it, -1 for none), 'planes', per frame the list of its planes found as 4-tuples (a, b, c,
    d) of floats, and 'num_planes', B ints, both carried in the one host read.  Given together with any of the three other filters it
    raises ValueError.
    `normal_consistency` (None, or (k, cell)): the third standard metric of occupancy-field work beside Chamfer and F-score.  It needs
    `surfaces` and the predicted normals (`normals` or `surface_steps`), else ValueError before any GPU work.  The ground-truth clouds
    carry coordinates only, so their normals are estimated first - PCA over each row's k nearest
    other rows and itself, turned towards the sensor at the origin, from postprocess.estimate_normals_ragged over the
    box `thin` uses with the search cell `cell` (it does not show in the result) - and then compared with the normals of 'pred' by
    postprocess.normal_consistency_ragged: |n . n'| with the nearest row of the other cloud, averaged per direction.  Computed on the
    full cloud, skip_eval_metric or not.  Added: 'normal_consistency', B triples (pred -> gt, gt -> pred, their mean; NaN where no row
    has two usable normals) carried in the one host read, and 'surface_normals', a list of B tensors [P,3] on the device.
    `align` (None, or (mode, max_distance), (mode, max_distance, max_iterations) or (mode, max_distance, max_iterations, k, cell); mode
    'point' or 'plane'): every final cloud is additionally registered onto its frame's `surfaces` cloud by ICP - a small extrinsic or
    timing error between the sensors shows up in 'cd' as shape error; the metric after a rigid alignment tells the two apart - from
    postprocess.register_icp_ragged over the box `thin` uses with the cell edge max_distance, at most
    max_iterations (default 30) iterations, all on the device.  It needs `surfaces`, else ValueError before any GPU work.  Plane mode
    estimates the surfaces' normals as `normal_consistency` does, from its own (k, cell) or, without them, from `normal_consistency`'s.
    'pred', 'cd', 'metrics' and every other key stay untouched.  Added: 'align_transform' (B 4 x 4 nested lists of floats: surfaces ~ R
    pred + t), 'align_fitness', 'align_rmse' (B floats), 'align_status' (B ints: postprocess.ICP_STATUS), 'aligned' (a list of B tensors
    [n_b,3], 'pred' under the transform), 'cd_aligned' (B floats, None where no metric is computed) and with metric_thresholds
    'metrics_aligned' (as 'metrics'), all host values carried in the one host read.
    Returns {'pred': list of B tensors [n_b,3] (metric coordinates, on the device), 'cd': list of B floats or None,
    'n_queries': list of B ints} and the keys that the options above add."""
    t, thinned, resampled = _tail_on_device(vae, sampled_tokens, args, helper_points, surfaces, rng, draws, metric_thresholds, normals,
                                            surface_steps, surface_max_step, resample, thin, denoise, denoise_statistical, normal_consistency,
                                            denoise_cluster, remove_planes, align)
    B, den, nrm, al = sampled_tokens.shape[0], t.denoised, t.normals, t.aligned
    groups = {"offsets": t.offsets, "n_queries": t.n_queries, "cd": t.cd, "metrics": t.metrics,
              "normal_consistency": t.ncons and t.ncons[0], "thin_offsets": thinned and thinned[1]}
    if den is not None:
        groups.update(denoise_offsets=den.offsets, cd_denoised=den.cd, metrics_denoised=den.metrics, denoise_stats=den.stats, n_clusters=den.n_clusters,
                      planes=den.planes, num_planes=den.n_planes)
    if al is not None:
        groups.update(align_transform=al.transform, align_fitness=al.fitness, align_rmse=al.rmse, align_status=al.status, cd_aligned=al.cd,
                      metrics_aligned=al.metrics)
    host = _HostPack(**groups).read()
    ints = lambda name: [int(v) for v in host[name]]
    frames = lambda rows, name: [rows[lo:hi] for lo, hi in zip(ints(name), ints(name)[1:])]         # a ragged tensor by its offsets' host copy
    triples = lambda name: [tuple(host[name][3 * b:3 * b + 3]) for b in range(B)]
    frame_metrics = lambda name: PP._metrics_to_host(host[name], B, len(metric_thresholds)) if name in host else None
    o = ints("offsets")
    out = {"pred": frames(t.points, "offsets"), "cd": host.get("cd"), "n_queries": ints("n_queries")}
    if metric_thresholds is not None:
        out["metrics"] = frame_metrics("metrics")
    if nrm is not None:
        out["normals"] = frames(nrm, "offsets")
    if den is not None:
        out["denoised"], out["denoise_index"] = frames(den.points, "denoise_offsets"), frames(den.index, "denoise_offsets")
        if nrm is not None:
            out["denoised_normals"] = [nrm[o[b] + out["denoise_index"][b]] for b in range(B)]
        if surfaces is not None:
            out["cd_denoised"] = host.get("cd_denoised")
        if metric_thresholds is not None:
            out["metrics_denoised"] = frame_metrics("metrics_denoised")
        if den.stats is not None:
            out["denoise_stats"] = triples("denoise_stats")
        if den.labels is not None:
            out["denoise_labels"] = frames(den.labels, "denoise_offsets")
        if den.n_clusters is not None:
            out["n_clusters"] = ints("n_clusters")
        if den.planes is not None:
            K, flat = den.planes.shape[1], host["planes"]
            out["num_planes"] = ints("num_planes")
            out["planes"] = [[tuple(flat[(b * K + k) * 4:(b * K + k) * 4 + 4]) for k in range(out["num_planes"][b])] for b in range(B)]
    if t.ncons is not None:
        out["normal_consistency"], out["surface_normals"] = triples("normal_consistency"), list(t.ncons[1].split(surfaces.shape[1]))
    if al is not None:
        flat = host["align_transform"]
        out["align_transform"] = [[flat[b * 16 + 4 * r:b * 16 + 4 * r + 4] for r in range(4)] for b in range(B)]
        out["align_fitness"], out["align_rmse"], out["align_status"] = host["align_fitness"], host["align_rmse"], ints("align_status")
        out["aligned"], out["cd_aligned"] = frames(al.points, "offsets"), host.get("cd_aligned")
        if metric_thresholds is not None:
            out["metrics_aligned"] = frame_metrics("metrics_aligned")
    if thinned is not None:
        for key, rows in zip(("thinned", "thin_count", "thin_first"), (thinned[0], thinned[2], thinned[3])):
            out[key] = frames(rows, "thin_offsets")
        if nrm is not None:
            rows = out["thin_first"] if den is None else [out["denoise_index"][b][out["thin_first"][b]] for b in range(B)]
            out["thinned_normals"] = [nrm[o[b] + rows[b]] for b in range(B)]
    if resampled is not None:
        out["resampled"], out["resample_index"] = resampled
    return out


def _check_scan_inputs(sampled_tokens, args, az_deg, el_deg, n_steps, n_refine, surfaces):
    """The argument rules of scan_point_clouds, all on the host: ValueError before any library call -> (az, el, n_steps, n_refine)."""
    from ._handles import _ray_counts
    _check_batch_inputs(sampled_tokens, None, surfaces)
    az, el = QP._beam_tables(args, az_deg, el_deg)
    n_steps, n_refine = _ray_counts(n_steps, n_refine)
    return az, el, n_steps, n_refine


@torch.no_grad()
def scan_point_clouds(vae, sampled_tokens: torch.Tensor, args, az_deg, el_deg, n_steps: int = 256, n_refine: int = 8,
                      surfaces: Optional[torch.Tensor] = None, metric_thresholds=None, normals: bool = False) -> Dict[str, object]:
    """A LiDAR-like scan of every frame's decoder field instead of the thresholded volume of infer_point_clouds: one first return per
    sensor beam (az_deg / el_deg [R], degrees: query_points.beam_grid), view-cone mode only.

    beam_segments (the beams as segments of the normalised (r, az, el) cube, from pc_range[0] to pc_range[3]) -> KLAutoEncoder.cast_rays
    (one launch: the beam is sampled at n_steps + 1 ranges, returns at the first positive logit, and the return is bisected n_refine
    times) -> the existing compaction and un-normalisation (postprocess.occupied_points_ragged on the returned logits
    and points) -> [normals: the logit's gradient at the returned points, postprocess.oriented_points_ragged] -> cartesian -> the
    Chamfer / cloud_metrics_ragged tail of infer_point_clouds against `surfaces` [B,P,3] (normalised ground truth) unless
    skip_eval_metric.  One host read at the end, packed as infer_point_clouds packs it.  Shape and range errors raise ValueError before
    any GPU work.

    Returns {'pred': list of B tensors [n_b,3] (metric, cartesian, on the device, in beam order), 'range': [B,R] metres on the device
    (NaN = no return; the r column of the un-normalised polar hit point), 'beam_index': list of B int64 tensors [n_b] (the beam of
    every row of 'pred'), 'cd': list of B floats or None (inf for a frame without returns), 'n_queries': list of B ints}
    (+ 'metrics' with metric_thresholds, + 'normals' with normals: unit vectors [n_b,3], zero where undefined).
    'n_queries' counts evaluated points as R * (n_steps + 1 + n_refine): an UPPER bound, a wave whose 64 beams have all returned stops
    marching and a wave without a return between two samples skips the bisection."""
    az, el, n_steps, n_refine = _check_scan_inputs(sampled_tokens, args, az_deg, el_deg, n_steps, n_refine, surfaces)
    if metric_thresholds is not None:
        metric_thresholds = PP._thresholds(metric_thresholds)
    lidar = args.dataset.lidar
    aniso, iso = lidar.norm_anisotropy, lidar.norm_isotropy
    B, dev = sampled_tokens.shape[0], sampled_tokens.device
    origins, dirs = QP.beam_segments(args, az, el, device=dev)
    R = origins.shape[0]
    _, logit, step, hit = vae.cast_rays(sampled_tokens, origins, dirs, n_steps, n_refine, points=True)
    offsets = torch.arange(B + 1, dtype=torch.int64, device=dev) * R
    flat = hit.reshape(-1, 3)
    pts, p_off, p_idx = PP.occupied_points_ragged(logit.reshape(-1), flat, offsets, lidar.pc_range, aniso, iso, view_cone_mode=False,
                                                  return_index=True)
    polar = PP.inverse_norm_points(flat, lidar.pc_range, aniso, iso)
    rng_m = torch.where(step.reshape(-1) >= 0, polar[:, 0], torch.full_like(polar[:, 0], float("nan"))).view(B, R)
    nrm = None
    if normals:
        pos = torch.arange(pts.shape[0], dtype=torch.int64, device=dev)
        frame = (torch.searchsorted(p_off, pos, right=True) - 1).clamp_(0, B - 1)
        kept = flat[(offsets[frame] + p_idx).clamp_(0, flat.shape[0] - 1)]
        _, grad = vae.decode_ragged_with_gradient(sampled_tokens, kept, p_off, R)
        pts, nrm = PP.oriented_points_ragged(kept, grad, p_off, lidar.pc_range, aniso, iso, view_cone_mode=True)
    else:
        pts = PP.polar2cartesian(pts)                                                              # rows past the last frame: unspecified
    cd, metrics = None, None
    if surfaces is not None and not _get(args.eval, "skip_eval_metric", False):
        P = surfaces.shape[1]
        gt = PP.polar2cartesian(PP.inverse_norm_points(surfaces.to(dev).reshape(-1, 3), lidar.pc_range, aniso, iso))
        gt_off = torch.arange(B + 1, dtype=torch.int64, device=dev) * P
        cd, metrics = _metric(pts, p_off, gt, gt_off, R, P, metric_thresholds)
    host = _HostPack(offsets=p_off, cd=cd, metrics=metrics).read()
    o = [int(v) for v in host["offsets"]]
    out = {"pred": [pts[o[b]:o[b + 1]] for b in range(B)], "range": rng_m, "beam_index": [p_idx[o[b]:o[b + 1]] for b in range(B)],
           "cd": host.get("cd"), "n_queries": [R * (n_steps + 1 + n_refine)] * B}
    if metric_thresholds is not None:
        out["metrics"] = PP._metrics_to_host(host["metrics"], B, len(metric_thresholds)) if metrics is not None else None
    if nrm is not None:
        out["normals"] = [nrm[o[b]:o[b + 1]] for b in range(B)]
    return out


def _check_mesh_inputs(sampled_tokens, args, resolution, threshold, surface_steps, surface_max_step, capacity, surfaces, metric_thresholds):
    """The argument rules of extract_meshes, all on the host: ValueError before any device use -> (the grid, threshold, surface_steps,
    capacity, the metric's thresholds or None)."""
    _check_batch_inputs(sampled_tokens, None, surfaces)
    lidar = args.dataset.lidar
    if not (lidar.norm_anisotropy or lidar.norm_isotropy):
        raise ValueError("one of norm_anisotropy / norm_isotropy is required")
    grid = QP.field_grid(resolution)
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float)) or not np.isfinite(threshold):
        raise ValueError("threshold must be a finite number")
    surface_steps = _whole(surface_steps, 0, 64, "surface_steps must be an integer in 0 .. 64")
    _positive(surface_max_step, "surface_max_step must be a finite number > 0")
    B, (nx, ny, nz) = sampled_tokens.shape[0], grid[2]
    if B > 65535 or B * nx * ny * nz > PP.SURFACE_MAX_NODES:
        raise ValueError(f"batch * resolution^3 must be at most {PP.SURFACE_MAX_NODES} nodes and the batch at most 65535")
    if capacity is not None:
        try:
            ok = len(capacity) == 2
            capacity = (_whole(capacity[0], 0, 2 ** 31 - 1, ""), _whole(capacity[1], 0, 2 ** 40, ""))
        except (TypeError, ValueError, IndexError):
            ok = False
        if not ok:
            raise ValueError("capacity must be (max_vertices, max_faces), two non-negative integers (max_vertices below 2^31), or None")
    thresholds = PP._thresholds(metric_thresholds) if metric_thresholds is not None and len(metric_thresholds) else None
    return grid, float(threshold), surface_steps, capacity, thresholds


@torch.no_grad()
def extract_meshes(vae, sampled_tokens: torch.Tensor, args, resolution, threshold: float = 0.0, normals: bool = False, surface_steps: int = 0,
                   surface_max_step: float = 0.05, capacity=None, surfaces: Optional[torch.Tensor] = None,
                   metric_thresholds=()) -> List[Dict[str, object]]:
    """Every frame's decoder field as a triangle mesh instead of the thresholded cloud of infer_point_clouds.

    query_points.field_grid(resolution) (the node grid over the normalised box) -> KLAutoEncoder.decode_volume (the logits on its nodes,
    decode's bit for bit) -> postprocess.extract_surface_batch (surface nets at logit = threshold) -> [surface_steps >
    0: the vertices moved onto logit = 0 by that many clamped Newton steps, query_points.project_to_surface_ragged; the faces keep
    their numbers] -> metric coordinates (cartesian in view-cone mode), the faces' winding kept counter-clockwise seen from the empty
    side (postprocess.mesh_to_metric) -> [normals: the logit's gradient at the final vertices, postprocess.oriented_points_ragged] ->
    [surfaces [B,P,3], the normalised ground truth: the Chamfer distance of the vertices, with metric_thresholds the whole
    cloud_metrics_ragged row, unless skip_eval_metric].
    capacity = (max_vertices, max_faces) over the batch: everything stays on the device until ONE host read at the end (the offsets and
    the metric), and a capacity the meshes do not fit raises RuntimeError naming the counts.  capacity = None adds
    extract_surface_batch's read of the two totals.  Argument errors raise ValueError before any device use.

    Returns a list of B dicts {'vertices' [V_b,3] float32 metric, 'faces' [F_b,3] int32 into them} on the device (+ 'normals' [V_b,3]
    unit vectors from occupied to empty, zero where undefined; + 'cd' a float, inf for an empty mesh; + 'metrics' with thresholds)."""
    grid, threshold, surface_steps, capacity, thresholds = _check_mesh_inputs(sampled_tokens, args, resolution, threshold, surface_steps,
                                                                              surface_max_step, capacity, surfaces, metric_thresholds)
    lidar = args.dataset.lidar
    aniso, iso = lidar.norm_anisotropy, lidar.norm_isotropy
    view_cone = bool(_get(lidar, "view_cone_mode", False))
    B, dev = sampled_tokens.shape[0], sampled_tokens.device
    lo, spacing, dims = grid
    volume = vae.decode_volume(sampled_tokens, lo, spacing, dims)
    v, v_off, f, f_off = PP.extract_surface_batch(volume, threshold, lo, spacing, capacity)
    cap_v, cap_f = v.shape[0], f.shape[0]
    row_off = v_off.clamp(max=cap_v)                                                               # what the later stages may read
    longest = max(1, min(cap_v, (dims[0] - 1) * (dims[1] - 1) * (dims[2] - 1)))
    nrm = None
    if cap_v == 0:                                                                                 # no vertex anywhere: nothing to decode
        normals, surface_steps, nrm = False, 0, (v if normals else None)
    if normals or surface_steps > 0:
        v, _, grad = QP.project_to_surface_ragged(vae, sampled_tokens, v, row_off, longest, surface_steps, surface_max_step)
    pts, faces = PP.mesh_to_metric(v, f, lidar.pc_range, aniso, iso, view_cone)
    if normals:
        pts, nrm = PP.oriented_points_ragged(v, grad, row_off, lidar.pc_range, aniso, iso, view_cone_mode=view_cone)
    cd = metrics = None
    if surfaces is not None and not _get(args.eval, "skip_eval_metric", False):
        P = surfaces.shape[1]
        gt = PP.inverse_norm_points(surfaces.to(dev).reshape(-1, 3), lidar.pc_range, aniso, iso)
        if view_cone:
            gt = PP.polar2cartesian(gt)
        gt_off = torch.arange(B + 1, dtype=torch.int64, device=dev) * P
        cd, metrics = _metric(pts, row_off, gt, gt_off, longest, P, thresholds)
    host = _HostPack(v_off=v_off, f_off=f_off, cd=cd, metrics=metrics).read()                      # the one host read
    vo, fo = [int(x) for x in host["v_off"]], [int(x) for x in host["f_off"]]
    if vo[B] > cap_v or fo[B] > cap_f:
        raise RuntimeError(f"extract_meshes: the batch has {vo[B]} vertices and {fo[B]} faces, the capacity is ({cap_v}, {cap_f})")
    out = []
    for b in range(B):
        mesh = {"vertices": pts[vo[b]:vo[b + 1]], "faces": faces[fo[b]:fo[b + 1]]}
        if nrm is not None:
            mesh["normals"] = nrm[vo[b]:vo[b + 1]]
        if cd is not None:
            mesh["cd"] = host["cd"][b]
        if metrics is not None:
            mesh["metrics"] = PP._metrics_to_host(host["metrics"], B, len(thresholds))[b]
        out.append(mesh)
    return out


@torch.no_grad()
def evaluate_sharded(model, vae, cubes: torch.Tensor, queries: torch.Tensor, eval_batch_size: int = 1,
                     metric_fn: Optional[Callable[[torch.Tensor, int], float]] = None,
                     sampler_kwargs: Optional[dict] = None) -> Dict[str, float]:
    """Batch-sharded evaluation: every rank owns the samples DistributedSampler would give it,
    runs them in eval batches with seeds = global sample index, and the only collective is the
    final metric reduction (utils/misc.py:45-47).  `cubes` [N,R,A,E,2] and `queries` [N,Q,3] are the
    full (host) arrays; each rank moves only its shard to the device.  `sampler_kwargs`: see sample_and_decode."""
    rank = torch.distributed.get_rank() if D.is_dist() else 0
    world = D.world_size()
    mine = D.shard_sample_indices(cubes.shape[0], rank, world)
    total, count = 0.0, 0.0
    occupied_fraction = []
    dev = next(model.parameters()).device
    for i in range(0, len(mine), eval_batch_size):
        idx = mine[i:i + eval_batch_size]
        out = sample_and_decode(model, vae, cubes[idx].to(dev), [queries[idx].to(dev)],
                                batch_seeds=torch.tensor(idx), sampler_kwargs=sampler_kwargs)
        occ = out["occupied"][0].float().mean(dim=1)
        for j, gi in enumerate(idx):
            val = metric_fn(out["logits"][0][j], gi) if metric_fn else float(occ[j])
            total += val
            count += 1
            occupied_fraction.append(float(occ[j]))
    total, count = D.reduce_sum_count(total, count)
    return {"metric_mean": total / max(count, 1.0), "n_samples": count}
