"""Device counterparts of the host post-processing the reference runs after ``vae.decode``
(engine_generation.py:229-243, :283-322): same function names and argument meaning as
``utils/utils.py`` (``inverse_norm_points``, ``cal_metrics``) and
``dataset_preprocessor/lidar.py`` (``polar2cartesian``), operating on CUDA tensors through
``rald_post_*`` (include/rald_hip.h).  ``occupied_points`` is the fused form of
``np.where(output > 0)`` -> ``grid[ind]`` -> ``inverse_norm_points`` -> ``polar2cartesian``.

Beyond the reference's one metric: ``nearest_neighbors*`` and ``cloud_metrics*`` (exact nearest neighbours per point, and accuracy,
completeness, both Chamfer variants, (modified) Hausdorff distance and precision / recall / F-score per frame),
``farthest_point_sample*`` / ``resample_points_ragged`` (k evenly spread points per cloud, the device counterpart of
``torch_cluster.fps``), ``voxel_grid`` / ``voxel_downsample*`` (one centroid per occupied cell of a fixed
grid, the device counterpart of Open3D's ``voxel_down_sample``), and ``radius_neighbor_count_ragged`` /
``remove_radius_outliers*`` (neighbours within a radius inside a cloud and the outlier filter on them, the device counterpart of
Open3D's ``remove_radius_outlier``), ``knn_ragged`` / ``remove_statistical_outliers*`` (the k nearest other rows
inside a cloud and the outlier filter on their mean distance), and ``estimate_normals*`` /
``normal_consistency*`` (PCA normals, surface variation and eigenvalues from those neighbours, and the normal-consistency metric of two
clouds with normals), ``cluster_dbscan*`` / ``remove_small_clusters*`` (density clustering; DESIGN.md section
25), and ``segment_plane*`` / ``remove_planes*`` (RANSAC plane segmentation with a fixed number of counter-based hypotheses, the device
counterpart of Open3D's ``segment_plane``, and plane removal), and ``register_icp*`` / ``transform_points*``
(ICP registration of one ragged batch onto another, point-to-point and point-to-plane, iterated on the device, the device counterpart
of Open3D's ``registration_icp``, and the rigid transform that applies its result), and ``extract_surface*`` /
``mesh_to_metric`` (a dense volume, such as the decoder's field on a grid, to a triangle mesh by naive surface nets, and the mesh in
metric coordinates).
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple

import torch

from ._handles import _doubles, _f32c, _nbytes, _need_cuda, _opt, _ragged_batch, _scratch, _stream
from ._lib import check, lib


_PC_RANGE = " [min0,min1,min2,max0,max1,max2]"          # the layout named when a pc_range has the wrong length


def occupied_points(logits: torch.Tensor, queries: torch.Tensor, lidar_pc_range, norm_anisotropy: bool, norm_isotropy: bool,
                    view_cone_mode: bool = True, threshold: float = 0.0, return_index: bool = False):
    """logits [Q], queries [Q,3] (normalised) -> positive queries in metric (cartesian if view_cone_mode)
    coordinates, in ascending query order: [n_pos, 3] (and their indices)."""
    _need_cuda(logits, "logits")
    logits, queries = _f32c(logits).reshape(-1), _f32c(queries).reshape(-1, 3)
    Q = logits.numel()
    if queries.shape[0] != Q:
        raise ValueError("one logit per query expected")
    pts = torch.empty(Q, 3, device=logits.device, dtype=torch.float32)
    idx = torch.empty(Q, device=logits.device, dtype=torch.int64) if return_index else None
    cnt = torch.zeros(1, device=logits.device, dtype=torch.int64)
    scratch = torch.empty(lib().rald_post_scratch_bytes(Q), device=logits.device, dtype=torch.uint8)
    check(lib().rald_post_occupied_points(logits.data_ptr(), queries.data_ptr(), Q, _doubles(lidar_pc_range, 6, "pc_range", _PC_RANGE),
                                          int(norm_anisotropy), int(norm_isotropy), int(view_cone_mode), float(threshold),
                                          pts.data_ptr(), _opt(idx), cnt.data_ptr(),
                                          scratch.data_ptr(), _stream()))
    n = int(cnt.item())                                   # the only host sync: the reference syncs on the full D2H here
    return (pts[:n], idx[:n]) if return_index else pts[:n]


def occupied_points_ragged(logits: torch.Tensor, queries: torch.Tensor, offsets: torch.Tensor, lidar_pc_range, norm_anisotropy: bool,
                           norm_isotropy: bool, view_cone_mode: bool = True, threshold: float = 0.0, return_index: bool = False):
    """occupied_points for a ragged batch: logits [T], queries [T,3], offsets int64 [B+1] on the device ->
    (points [T,3], out_offsets int64 [B+1], index [T] or None), all on the device and sized for the worst case: sample b's positives
    are rows out_offsets[b] .. out_offsets[b+1]-1, in ascending query order, `index` counting from the sample's first query; rows
    from out_offsets[B] on are unspecified.  No host read."""
    _need_cuda(logits, "logits")
    logits, queries = _f32c(logits).reshape(-1), _f32c(queries).reshape(-1, 3)
    T = logits.numel()
    if queries.shape[0] != T:
        raise ValueError("one logit per query expected")
    B = _ragged_batch(offsets, "offsets")
    dev = logits.device
    pts = torch.empty(T, 3, device=dev, dtype=torch.float32)
    idx = torch.empty(T, device=dev, dtype=torch.int64) if return_index else None
    out_offsets = torch.empty(B + 1, device=dev, dtype=torch.int64)
    scratch = torch.empty(lib().rald_post_scratch_bytes(T), device=dev, dtype=torch.uint8)
    check(lib().rald_post_occupied_points_ragged(logits.data_ptr(), queries.data_ptr(), offsets.data_ptr(), B, T,
                                                 _doubles(lidar_pc_range, 6, "pc_range", _PC_RANGE), int(norm_anisotropy), int(norm_isotropy),
                                                 int(view_cone_mode), float(threshold), pts.data_ptr(), _opt(idx), out_offsets.data_ptr(),
                                                 scratch.data_ptr(), _stream()))
    return pts, out_offsets, idx


def _transform(points: torch.Tensor, lidar_pc_range, aniso: bool, iso: bool, view_cone: bool) -> torch.Tensor:
    _need_cuda(points, "points")
    points = _f32c(points).reshape(-1, 3)
    out = torch.empty_like(points)
    if points.shape[0]:
        check(lib().rald_post_transform_points(points.data_ptr(), points.shape[0], _doubles(lidar_pc_range, 6, "pc_range", _PC_RANGE), int(aniso),
                                               int(iso), int(view_cone), out.data_ptr(), _stream()))
    return out


def oriented_points(points_norm: torch.Tensor, grad: torch.Tensor, lidar_pc_range, norm_anisotropy: bool, norm_isotropy: bool,
                    view_cone_mode: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """Normalised points [n,3] and the logit's gradients there [n,3] (KLAutoEncoder.decode_with_gradient) -> (points, normals): the
    points in metric coordinates, bit for bit what inverse_norm_points (+ polar2cartesian) gives, and one unit normal each, pointing
    from occupied to empty: -J^-T grad normalised, J the Jacobian of that transform.  (0,0,0) where the transform is singular (range 0,
    the view cone's poles) or the gradient vanishes."""
    return oriented_points_ragged(points_norm, grad, None, lidar_pc_range, norm_anisotropy, norm_isotropy, view_cone_mode)


def oriented_points_ragged(points_norm: torch.Tensor, grad: torch.Tensor, offsets: Optional[torch.Tensor], lidar_pc_range,
                           norm_anisotropy: bool, norm_isotropy: bool, view_cone_mode: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """oriented_points for a ragged batch held in worst-case sized arrays: offsets int64 [B+1] on the device, rows from offsets[B] on
    are not read and stay unspecified.  No host read."""
    _need_cuda(points_norm, "points")
    points, grad = _f32c(points_norm).reshape(-1, 3), _f32c(grad).reshape(-1, 3)
    if grad.shape != points.shape or grad.device != points.device:
        raise ValueError("one gradient per point expected, on the points' device")
    out, normals = torch.empty_like(points), torch.empty_like(points)
    n = points.shape[0]
    rng = _doubles(lidar_pc_range, 6, "pc_range", _PC_RANGE)
    if offsets is None:
        if n:
            check(lib().rald_post_oriented_points(points.data_ptr(), grad.data_ptr(), n, rng, int(norm_anisotropy), int(norm_isotropy),
                                                  int(view_cone_mode), out.data_ptr(), normals.data_ptr(), _stream()))
    else:
        B = _ragged_batch(offsets, "offsets")
        check(lib().rald_post_oriented_points_ragged(points.data_ptr(), grad.data_ptr(), offsets.data_ptr(), B, n, rng, int(norm_anisotropy),
                                                     int(norm_isotropy), int(view_cone_mode), out.data_ptr(), normals.data_ptr(), _stream()))
    return out, normals


def inverse_norm_points(points, lidar_pc_range, norm_anisotropy, norm_isotropy):
    """utils/utils.py:50-75."""
    return _transform(points, lidar_pc_range, norm_anisotropy, norm_isotropy, False)


def polar2cartesian(points):
    """dataset_preprocessor/lidar.py:57-63 ((r, az deg, el deg) -> (x, y, z))."""
    # identity normalisation: scale 1, offset 0 on every axis
    return _transform(points, [-1, -1, -1, 1, 1, 1], True, False, True)


def cal_metrics(y_pred: torch.Tensor, y_gt: torch.Tensor) -> float:
    """utils/utils.py:116-142 - Chamfer distance; inf for an empty prediction, like the reference."""
    if y_pred.shape[0] == 0:
        return float("inf")
    _need_cuda(y_pred, "y_pred")
    y_pred, y_gt = _f32c(y_pred).reshape(-1, 3), _f32c(y_gt).reshape(-1, 3).to(y_pred.device)
    sums = torch.zeros(2, device=y_pred.device, dtype=torch.float64)
    check(lib().rald_post_chamfer_sums(y_pred.data_ptr(), y_pred.shape[0], y_gt.data_ptr(), y_gt.shape[0],
                                       sums.data_ptr(), _stream()))
    s = sums.cpu()
    return float(0.5 * s[1] / y_gt.shape[0] + 0.5 * s[0] / y_pred.shape[0])


def cal_metrics_ragged(y_pred: torch.Tensor, pred_offsets: torch.Tensor, y_gt: torch.Tensor, gt_offsets: torch.Tensor, max_pred: int,
                       max_gt: int) -> torch.Tensor:
    """cal_metrics per sample of a ragged batch -> float64 [B] on the device (inf where the prediction is empty); max_pred / max_gt
    are host upper bounds of the longest prediction / ground truth (trusted: a bound below a frame's size silently leaves the rows behind
    it out of the sums).  No host read."""
    _need_cuda(y_pred, "y_pred")
    y_pred, y_gt = _f32c(y_pred).reshape(-1, 3), _f32c(y_gt).reshape(-1, 3).to(y_pred.device)
    B = _ragged_batch(pred_offsets, "pred_offsets")
    if _ragged_batch(gt_offsets, "gt_offsets") != B:
        raise ValueError("pred_offsets and gt_offsets must describe the same batch")
    sums = torch.empty(B, 2, device=y_pred.device, dtype=torch.float64)
    check(lib().rald_post_chamfer_sums_ragged(y_pred.data_ptr(), pred_offsets.data_ptr(), y_gt.data_ptr(), gt_offsets.data_ptr(), B,
                                              int(max_pred), int(max_gt), sums.data_ptr(), _stream()))
    n_pred = (pred_offsets[1:] - pred_offsets[:-1]).double()
    n_gt = (gt_offsets[1:] - gt_offsets[:-1]).double()
    cd = 0.5 * sums[:, 1] / n_gt + 0.5 * sums[:, 0] / n_pred
    return torch.where(n_pred == 0, torch.full_like(cd, float("inf")), cd)


MAX_THRESHOLDS = 8                                       # K of rald_post_cloud_metrics_ragged
METRIC_KEYS = ("accuracy", "completeness", "cd", "cd_l2", "hausdorff", "mhd", "precision", "recall", "f_score")


def _xyz(t, what: str) -> None:
    if not (isinstance(t, torch.Tensor) and t.dim() == 2 and t.shape[1] == 3):
        raise ValueError(f"{what} must be a tensor [n, 3]")


def _offsets_shape(t, what: str) -> int:
    """B of int64 offsets [B+1], by shape and dtype alone (before anything asks where the tensor lives)."""
    if not (isinstance(t, torch.Tensor) and t.dtype == torch.int64 and t.dim() == 1 and t.numel() >= 2):
        raise ValueError(f"{what} must be an int64 tensor [B+1]")
    return t.numel() - 1


def _positive(x, message: str) -> float:
    """A finite number > 0 (no bool, no string) -> float; else ValueError(message)."""
    if isinstance(x, bool) or not isinstance(x, (int, float)) or not math.isfinite(x) or x <= 0:
        raise ValueError(message)
    return float(x)


def _whole(x, lo: int, hi, message: str) -> int:
    """A number (no bool, no string) that is a whole number in lo .. hi (hi None: no upper end) -> int; else ValueError(message)."""
    if isinstance(x, bool) or not isinstance(x, (int, float)) or not math.isfinite(x) or int(x) != x or x < lo or (hi is not None and x > hi):
        raise ValueError(message)
    return int(x)


def _bound(v, what: str) -> int:
    if int(v) != v or v < 0:
        raise ValueError(f"{what} must be a non-negative integer")
    return int(v)


def _thresholds(thresholds) -> list:
    taus = [float(t) for t in thresholds]
    if len(taus) > MAX_THRESHOLDS:
        raise ValueError(f"at most {MAX_THRESHOLDS} thresholds")
    if any(not math.isfinite(t) or t < 0 for t in taus):
        raise ValueError("thresholds must be finite and >= 0")
    return taus


def _ragged_pair(a, a_offsets, b, b_offsets, names) -> int:
    """The shape rules of a ragged pair of clouds (ValueError), then the device rules; -> B."""
    _xyz(a, names[0])
    _xyz(b, names[2])
    B = _offsets_shape(a_offsets, names[1])
    if _offsets_shape(b_offsets, names[3]) != B:
        raise ValueError(f"{names[1]} and {names[3]} must describe the same batch")
    _need_cuda(a, names[0])
    _ragged_batch(a_offsets, names[1])
    _ragged_batch(b_offsets, names[3])
    return B


def nearest_neighbors_ragged(a: torch.Tensor, a_offsets: torch.Tensor, b: torch.Tensor, b_offsets: torch.Tensor, max_a: int, max_b: int,
                             b_chunk: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per row of a [Ta,3] the exact nearest row of b [Tb,3] in the same frame (offsets int64 [B+1] on the device; max_a / max_b host
    upper bounds of the longest segment, trusted as in cal_metrics_ragged): (dist float64 [Ta], idx int64 [Ta]), idx counting from the
    frame's first b row, the lowest index on equal distances; a frame without b rows gets (inf, -1).  Rows from a_offsets[B] on are
    unspecified.  float64 arithmetic on the fp32 coordinates, no atomics, no host read.  b_chunk (tests): the b rows per workgroup,
    a multiple of 1024, 0 or None = automatic; the result does not depend on it."""
    max_a, max_b = _bound(max_a, "max_a"), _bound(max_b, "max_b")
    B = _ragged_pair(a, a_offsets, b, b_offsets, ("a", "a_offsets", "b", "b_offsets"))
    a, b = _f32c(a), _f32c(b).to(a.device)
    dist = torch.empty(a.shape[0], device=a.device, dtype=torch.float64)
    idx = torch.empty(a.shape[0], device=a.device, dtype=torch.int64)
    if b_chunk is None:
        scratch = _scratch(_nbytes(lib().rald_post_cloud_metrics_scratch_bytes(B, max_a, max_b)), a.device)
        check(lib().rald_post_nn_ragged(a.data_ptr(), a_offsets.data_ptr(), b.data_ptr(), b_offsets.data_ptr(), B, max_a, max_b,
                                        dist.data_ptr(), idx.data_ptr(), scratch.data_ptr(), _stream()))
    else:
        nbytes = _nbytes(lib().rald_op_nn_scratch_bytes(B, max_a, max_b, int(b_chunk)))
        scratch = _scratch(nbytes, a.device)
        check(lib().rald_op_nn_ragged(a.data_ptr(), a_offsets.data_ptr(), b.data_ptr(), b_offsets.data_ptr(), B, max_a, max_b, int(b_chunk),
                                      dist.data_ptr(), idx.data_ptr(), scratch.data_ptr(), nbytes, _stream()))
    return dist, idx


def nearest_neighbors(a: torch.Tensor, b: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(dist float64 [n_a], idx int64 [n_a]): the exact nearest row of b for every row of a (nearest_neighbors_ragged for one frame)."""
    _xyz(a, "a")
    _xyz(b, "b")
    _need_cuda(a, "a")
    off = torch.tensor([[0, a.shape[0]], [0, b.shape[0]]], dtype=torch.int64, device=a.device)
    return nearest_neighbors_ragged(a, off[0], b, off[1], a.shape[0], b.shape[0])


def _derive_cloud_metrics(raw: torch.Tensor, n_pred: torch.Tensor, n_gt: torch.Tensor) -> Dict[str, torch.Tensor]:
    """raw [B,2,3+K] (direction 0 pred -> gt, 1 gt -> pred: sum d, sum d^2, max d, counts below the K thresholds) and the frames'
    sizes (float64 [B]) -> the metrics.  A frame with an empty side: the six distances inf, the three ratios 0."""
    empty = (n_pred == 0) | (n_gt == 0)
    n = torch.stack((n_pred, n_gt), dim=1)                                       # [B,2]
    safe = torch.where(n == 0, torch.ones_like(n), n)
    mean_d, mean_d2, max_d = raw[:, :, 0] / safe, raw[:, :, 1] / safe, raw[:, :, 2]
    inf = torch.full_like(n_pred, float("inf"))
    dist = {"accuracy": mean_d[:, 0], "completeness": mean_d[:, 1], "cd": 0.5 * mean_d[:, 0] + 0.5 * mean_d[:, 1],
            "cd_l2": mean_d2[:, 0] + mean_d2[:, 1], "hausdorff": torch.maximum(max_d[:, 0], max_d[:, 1]),
            "mhd": torch.maximum(mean_d[:, 0], mean_d[:, 1])}
    out = {k: torch.where(empty, inf, v) for k, v in dist.items()}
    ratio = torch.where(empty[:, None, None], torch.zeros_like(raw[:, :, 3:]), raw[:, :, 3:] / safe[:, :, None])     # [B,2,K]
    p, r = ratio[:, 0], ratio[:, 1]
    s = p + r
    out["precision"], out["recall"] = p, r
    out["f_score"] = torch.where(s > 0, 2.0 * p * r / torch.where(s > 0, s, torch.ones_like(s)), torch.zeros_like(s))
    return out


def cloud_metrics_ragged(y_pred: torch.Tensor, pred_offsets: torch.Tensor, y_gt: torch.Tensor, gt_offsets: torch.Tensor, max_pred: int,
                         max_gt: int, thresholds: Sequence[float] = (), per_point: bool = False) -> Dict[str, torch.Tensor]:
    """Per frame of a ragged batch, float64 [B] on the device, from the exact nearest-neighbour distances d of both directions:
    accuracy (mean d over pred), completeness (mean d over gt), cd = 0.5 accuracy + 0.5 completeness (cal_metrics' definition),
    cd_l2 (mean d^2 over pred + mean d^2 over gt), hausdorff (the larger maximum), mhd (the larger mean), and [B,K] per threshold tau:
    precision (share of pred with d < tau), recall (share of gt with d < tau), f_score = 2PR / (P + R), 0 where P + R = 0.
    A frame with an empty prediction or ground truth: the six distances inf, the three ratios 0.  max_pred / max_gt as in
    cal_metrics_ragged.  per_point adds dist_pred / idx_pred [Tp] and dist_gt / idx_gt [Tg] (nearest_neighbors_ragged's outputs of both
    directions).  Bit-reproducible (no atomics; a frame's values do not depend on the batch around it).  No host read."""
    taus = _thresholds(thresholds)
    max_pred, max_gt = _bound(max_pred, "max_pred"), _bound(max_gt, "max_gt")
    B = _ragged_pair(y_pred, pred_offsets, y_gt, gt_offsets, ("y_pred", "pred_offsets", "y_gt", "gt_offsets"))
    y_pred, y_gt = _f32c(y_pred), _f32c(y_gt).to(y_pred.device)
    dev, K = y_pred.device, len(taus)
    raw = torch.empty(B, 2, 3 + K, device=dev, dtype=torch.float64)
    pp = {}
    if per_point:
        for side, t in (("pred", y_pred), ("gt", y_gt)):
            pp["dist_" + side] = torch.empty(t.shape[0], device=dev, dtype=torch.float64)
            pp["idx_" + side] = torch.empty(t.shape[0], device=dev, dtype=torch.int64)
    scratch = _scratch(_nbytes(lib().rald_post_cloud_metrics_scratch_bytes(B, max_pred, max_gt)), dev)
    check(lib().rald_post_cloud_metrics_ragged(y_pred.data_ptr(), pred_offsets.data_ptr(), y_gt.data_ptr(), gt_offsets.data_ptr(), B, max_pred,
                                               max_gt, _doubles(taus, K, "thresholds") if K else None, K, raw.data_ptr(),
                                               _opt(pp.get("dist_pred")), _opt(pp.get("idx_pred")), _opt(pp.get("dist_gt")),
                                               _opt(pp.get("idx_gt")), scratch.data_ptr(), _stream()))
    out = _derive_cloud_metrics(raw, (pred_offsets[1:] - pred_offsets[:-1]).double(), (gt_offsets[1:] - gt_offsets[:-1]).double())
    out.update(pp)
    return out


def _metrics_to_host(values: Sequence[float], B: int, K: int) -> list:
    """The METRIC_KEYS tensors of a batch, flattened and concatenated in that order, as host floats -> one dict per frame."""
    frames = [{} for _ in range(B)]
    at = 0
    for key in METRIC_KEYS:
        width = K if key in ("precision", "recall", "f_score") else None
        for b in range(B):
            if width is None:
                frames[b][key] = values[at + b]
            else:
                frames[b][key] = list(values[at + b * K:at + (b + 1) * K])
        at += B * (width if width is not None else 1)
    return frames


def cloud_metrics(y_pred: torch.Tensor, y_gt: torch.Tensor, thresholds: Sequence[float] = ()) -> dict:
    """cloud_metrics_ragged for one frame, read to the host: Python floats, and lists of K floats for precision / recall / f_score."""
    taus = _thresholds(thresholds)
    _xyz(y_pred, "y_pred")
    _xyz(y_gt, "y_gt")
    _need_cuda(y_pred, "y_pred")
    off = torch.tensor([[0, y_pred.shape[0]], [0, y_gt.shape[0]]], dtype=torch.int64, device=y_pred.device)
    m = cloud_metrics_ragged(y_pred, off[0], y_gt, off[1], y_pred.shape[0], y_gt.shape[0], taus)
    host = torch.cat([m[k].reshape(-1) for k in METRIC_KEYS]).cpu().tolist()
    return _metrics_to_host(host, 1, len(taus))[0]


def accuracy_iou(outputs: torch.Tensor, labels: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """engine_generation.py:229-243 per sample: (accuracy [B], iou [B]); the caller takes .mean()."""
    _need_cuda(outputs, "outputs")
    outputs, labels = _f32c(outputs), _f32c(labels).to(outputs.device)
    B, Q = outputs.shape
    acc = torch.empty(B, device=outputs.device, dtype=torch.float32)
    iou = torch.empty(B, device=outputs.device, dtype=torch.float32)
    check(lib().rald_post_iou(outputs.data_ptr(), labels.data_ptr(), B, Q, acc.data_ptr(), iou.data_ptr(), _stream()))
    return acc, iou


FPS_MAX_POINTS = 65536                                   # the largest max_per_sample of rald_post_fps_ragged
FPS_FORMS = {None: 0, "auto": 0, "resident": 1, "streaming": 2}


def _fps_args(points, dim: int, k, max_per_sample, counts, start, scale, B: Optional[int], form):
    """The shape, dtype and range rules of the farthest-point calls (ValueError, before anything asks where a tensor lives)
    -> (k, max_per_sample, scale as 3 floats or None, form code)."""
    if not (isinstance(points, torch.Tensor) and points.dim() == dim and points.shape[-1] == 3 and points.is_floating_point()):
        raise ValueError("points must be a floating-point tensor " + ("[B, N, 3]" if dim == 3 else "[T, 3]"))
    if isinstance(k, bool) or int(k) != k or k < 1:
        raise ValueError("k must be a positive integer")
    if isinstance(max_per_sample, bool) or int(max_per_sample) != max_per_sample or not 1 <= max_per_sample <= FPS_MAX_POINTS:
        raise ValueError(f"max_per_sample must be an integer in 1 .. {FPS_MAX_POINTS}")
    if B is not None:
        if counts is not None and not (isinstance(counts, torch.Tensor) and counts.dtype == torch.int32 and tuple(counts.shape) == (B,)):
            raise ValueError(f"counts must be an int32 tensor [{B}] (LidarFrames.crop's)")
        if start is not None and not (isinstance(start, torch.Tensor) and start.dtype == torch.int64 and tuple(start.shape) == (B,)):
            raise ValueError(f"start must be an int64 tensor [{B}]")
    if scale is not None:
        scale = [float(v) for v in scale]
        if len(scale) != 3 or any(not math.isfinite(v) for v in scale):
            raise ValueError("scale must be 3 finite numbers")
    if form not in FPS_FORMS:
        raise ValueError("form must be None, 'auto', 'resident' or 'streaming'")
    return int(k), int(max_per_sample), scale, FPS_FORMS[form]


def _fps_call(points, offsets, counts, B, n_dense, max_per_sample, k, start, scale, return_dist, form):
    import ctypes as C
    dev = points.device
    idx = torch.empty(B, k, device=dev, dtype=torch.int64)
    dist = torch.empty(B, k, device=dev, dtype=torch.float32) if return_dist else None
    nbytes = _nbytes(lib().rald_post_fps_scratch_bytes(B, max_per_sample, form))
    scratch = _scratch(nbytes, dev)
    scale3 = (C.c_float * 3)(*scale) if scale is not None else None
    check(lib().rald_post_fps_ragged(points.data_ptr(), _opt(offsets), _opt(counts), B, n_dense, max_per_sample, k, _opt(start), scale3,
                                     idx.data_ptr(), _opt(dist), scratch.data_ptr(), nbytes, form, _stream()))
    return (idx, dist) if return_dist else idx


def farthest_point_sample_ragged(points: torch.Tensor, offsets: torch.Tensor, k: int, max_per_sample: int, counts: Optional[torch.Tensor] = None,
                                 start: Optional[torch.Tensor] = None, scale: Optional[Sequence[float]] = None, return_dist: bool = False,
                                 form: Optional[str] = None):
    """Farthest-point sampling per cloud of a ragged batch (rald_post_fps_ragged): points [T,3], offsets int64
    [B+1] on the device -> idx int64 [B,k] (row indices from the cloud's own first row) and, with return_dist, dist2 float32 [B,k]
    (+inf first, then the squared distance of every choice to the set chosen before it), both on the device.
    The first choice is start[b] mod n (start: int64 [B] on the device; None = row 0), every further one the row with the largest
    squared distance to the rows chosen so far, the SMALLEST index on equal distances; distances are fp32 on points * scale (3 numbers
    per axis, None = 1), every operation rounded, so the result is the same bits in every call and batch.  counts (int32 [B] on the
    device, LidarFrames.crop's): only the first counts[b] rows of a cloud are valid.  max_per_sample: host bound of the longest cloud,
    at most 65536 - it is trusted, a cloud LONGER than it is sampled from its first max_per_sample rows.  A cloud with n < k rows gets
    its n choices, then idx -1 and dist2 NaN; with fewer than k distinct points the smallest index repeats at distance 0.  Coordinates
    must be finite.  form (tests): 'resident' / 'streaming' force the kernel form, the result does not depend on it.
    No host read, no synchronisation; runs on the current stream."""
    k, max_per_sample, scale, form = _fps_args(points, 2, k, max_per_sample, counts, start, scale, _offsets_shape(offsets, "offsets"), form)
    _need_cuda(points, "points")
    B = _ragged_batch(offsets, "offsets")
    for t, what in ((counts, "counts"), (start, "start")):
        if t is not None:
            _need_cuda(t, what)
    points = _f32c(points)
    return _fps_call(points, offsets, None if counts is None else counts.contiguous(), B, 0, max_per_sample, k,
                     None if start is None else start.contiguous(), scale, return_dist, form)


def farthest_point_sample(points: torch.Tensor, k: int, start: Optional[torch.Tensor] = None, scale: Optional[Sequence[float]] = None,
                          return_dist: bool = False, form: Optional[str] = None):
    """farthest_point_sample_ragged for dense clouds: points [B,N,3] (1 <= N <= 65536) -> idx int64 [B,k] (and dist2 float32 [B,k])."""
    if not (isinstance(points, torch.Tensor) and points.dim() == 3):
        raise ValueError("points must be a floating-point tensor [B, N, 3]")
    B, N = points.shape[0], points.shape[1]
    if B < 1 or N < 1:
        raise ValueError("points must hold at least one cloud of at least one point")
    k, N, scale, form = _fps_args(points, 3, k, N, None, start, scale, B, form)
    _need_cuda(points, "points")
    if start is not None:
        _need_cuda(start, "start")
    return _fps_call(_f32c(points), None, None, B, N, N, k, None if start is None else start.contiguous(), scale, return_dist, form)


def resample_points_ragged(points: torch.Tensor, offsets: torch.Tensor, k: int, max_per_sample: int, counts: Optional[torch.Tensor] = None,
                           start: Optional[torch.Tensor] = None, scale: Optional[Sequence[float]] = None, pad: str = "repeat",
                           return_index: bool = False):
    """Every cloud of a ragged batch as exactly k evenly spread points: -> [B,k,3] float32 = the rows farthest_point_sample_ragged
    chooses (same arguments), in the order chosen.  pad='repeat': a cloud with 0 < n < k rows fills slot j >= n with the point of slot
    j mod n; pad='nan': those slots are NaN.  An empty cloud gives NaN rows.  return_index adds idx [B,k] (-1 in the padded slots).
    The gather and the padding are torch indexing on the device; no host read."""
    if pad not in ("repeat", "nan"):
        raise ValueError("pad must be 'repeat' or 'nan'")
    idx = farthest_point_sample_ragged(points, offsets, k, max_per_sample, counts=counts, start=start, scale=scale)
    B, k = idx.shape
    pts = _f32c(points)
    slot = torch.arange(k, dtype=torch.int64, device=idx.device).expand(B, k)
    if pad == "repeat":
        n_sel = (idx >= 0).sum(dim=1, keepdim=True)                              # min(n, k) per cloud
        slot = slot % n_sel.clamp(min=1)
    src = torch.gather(idx, 1, slot)                                             # -1 where nothing can fill the slot
    rows = (offsets[:-1, None] + src).clamp_(0, max(pts.shape[0] - 1, 0))
    if pts.shape[0]:
        out = pts[rows]
    else:
        out = torch.zeros(B, k, 3, device=idx.device, dtype=torch.float32)
    out = torch.where((src >= 0)[:, :, None], out, torch.full_like(out, float("nan")))
    return (out, idx) if return_index else out


VOXEL_MAX_POINTS = 1 << 24                               # the largest max_per_sample of rald_post_voxel_downsample_ragged
VOXEL_MAX_CELLS = (1 << 31) - 1


def _f32(v: float) -> float:
    """v rounded to float32; +-inf where it does not fit, which every caller refuses as it refuses a non-finite result."""
    import struct
    try:
        return struct.unpack("f", struct.pack("f", v))[0]
    except OverflowError:
        return math.copysign(math.inf, v)


def voxel_grid(lo: Sequence[float], hi: Sequence[float], voxel) -> Tuple[Tuple[float, ...], Tuple[float, ...], Tuple[int, ...]]:
    """The fixed grid of the voxel calls -> (lo3, v3, dims3): `voxel` is the cell edge, one number or one per axis; per axis
    dims = floor((hi - lo) / v) + 1 (in double, on the numbers given), so that hi itself lies in the last cell; lo3 and v3 are lo and
    voxel rounded to float32, what the kernels compute with.  ValueError for non-finite bounds, hi < lo, a non-positive or non-finite
    edge (also one that rounds to 0 or inf in float32), and for more than 2^31 - 1 cells."""
    try:
        lo, hi = [float(x) for x in lo], [float(x) for x in hi]
        v = [float(voxel)] * 3 if isinstance(voxel, (int, float)) and not isinstance(voxel, bool) else [float(x) for x in voxel]
    except TypeError:
        raise ValueError("lo, hi must be 3 numbers each, voxel a number or 3 numbers") from None
    if len(lo) != 3 or len(hi) != 3 or len(v) != 3:
        raise ValueError("lo, hi must be 3 numbers each, voxel a number or 3 numbers")
    if any(not math.isfinite(x) for x in lo + hi) or any(h < l for l, h in zip(lo, hi)):
        raise ValueError("lo and hi must be finite with lo <= hi")
    if any(not math.isfinite(x) or x <= 0 for x in v):
        raise ValueError("the cell edge must be finite and > 0")
    lo3, v3 = tuple(_f32(x) for x in lo), tuple(_f32(x) for x in v)
    if any(x <= 0 or not math.isfinite(x) for x in v3) or any(not math.isfinite(x) for x in lo3):
        raise ValueError("lo and the cell edge must fit float32")
    dims = tuple(int(math.floor((h - l) / x)) + 1 for l, h, x in zip(lo, hi, v))
    if dims[0] * dims[1] * dims[2] > VOXEL_MAX_CELLS:
        raise ValueError(f"the grid has {dims[0] * dims[1] * dims[2]} cells, more than 2^31 - 1: use a coarser cell")
    return lo3, v3, dims


def _voxel_grid_arg(grid):
    """(lo3, v3, dims3) of voxel_grid, checked again (a caller may build it by hand) -> three ctypes host arrays."""
    import ctypes as C
    try:
        lo3, v3, dims3 = grid
        lo3, v3 = [float(x) for x in lo3], [float(x) for x in v3]
        ok = len(lo3) == 3 and len(v3) == 3 and len(dims3) == 3 and all(int(d) == d and not isinstance(d, bool) for d in dims3)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("grid must be (lo3, v3, dims3) as voxel_grid returns it")
    dims3 = [int(d) for d in dims3]
    if any(not math.isfinite(x) for x in lo3) or any(not math.isfinite(x) or x <= 0 for x in v3):
        raise ValueError("grid: lo must be finite and every cell edge finite and > 0")
    if any(d < 1 for d in dims3) or dims3[0] * dims3[1] * dims3[2] > VOXEL_MAX_CELLS:
        raise ValueError("grid: every dim must be >= 1 and the grid at most 2^31 - 1 cells")
    return (C.c_float * 3)(*lo3), (C.c_float * 3)(*v3), (C.c_int32 * 3)(*dims3)


def _voxel_args(points, max_per_sample, counts, B: Optional[int], chunk):
    if not (isinstance(points, torch.Tensor) and points.dim() == 2 and points.shape[-1] == 3 and points.is_floating_point()):
        raise ValueError("points must be a floating-point tensor [T, 3]")
    if isinstance(max_per_sample, bool) or int(max_per_sample) != max_per_sample or not 1 <= max_per_sample <= VOXEL_MAX_POINTS:
        raise ValueError(f"max_per_sample must be an integer in 1 .. {VOXEL_MAX_POINTS}")
    if B is not None and counts is not None and not (isinstance(counts, torch.Tensor) and counts.dtype == torch.int32 and tuple(counts.shape) == (B,)):
        raise ValueError(f"counts must be an int32 tensor [{B}] (LidarFrames.crop's)")
    if isinstance(chunk, bool) or int(chunk) != chunk or chunk < 0 or chunk % 1024:
        raise ValueError("chunk must be 0 (automatic) or a multiple of 1024")
    return int(max_per_sample), int(chunk)


def _cloud_batch(points, offsets, counts):
    """What the grid-indexed ragged calls do once their ValueErrors are behind them: every tensor on the device, points as contiguous
    float32 -> (points, counts, B, T, the device)."""
    _need_cuda(points, "points")
    B = _ragged_batch(offsets, "offsets")
    if counts is not None:
        _need_cuda(counts, "counts")
        counts = counts.contiguous()
    points = _f32c(points)
    return points, counts, B, points.shape[0], points.device


def _cloud_call(entry: str, sizes: str, points, offsets, counts, B: int, T: int, dev, max_per_sample: int, grid3, args, chunk: int) -> None:
    """rald_op_<entry> with a chunk, rald_post_<entry> without one, on scratch of the matching rald_*_<sizes>_scratch_bytes; args: the
    entry's own arguments between the grid and the scratch."""
    L = lib()
    pre, tail = ("rald_op_", (chunk,)) if chunk else ("rald_post_", ())
    nbytes = _nbytes(getattr(L, pre + sizes + "_scratch_bytes")(B, T, max_per_sample, *tail))
    scratch = _scratch(nbytes, dev)
    check(getattr(L, pre + entry)(points.data_ptr(), offsets.data_ptr(), _opt(counts), B, 0, T, max_per_sample, *grid3, *args,
                                  scratch.data_ptr(), nbytes, *tail, _stream()))


def _one_cloud_check(points, lo, hi) -> None:
    if not (isinstance(points, torch.Tensor) and points.dim() == 2 and points.shape[-1] == 3 and points.is_floating_point()):
        raise ValueError("points must be a floating-point tensor [N, 3]")
    if (lo is None) != (hi is None):
        raise ValueError("lo and hi come together")


def _one_cloud(points, lo, hi, grid_of):
    """What the one-cloud conveniences share behind _one_cloud_check and their own rules: grid_of(lo, hi, rows) on the box given (before
    anything else, an empty cloud included) or on the cloud's own minimum and maximum (one host read of six numbers) -> the ragged call's
    (points, offsets [0, N], grid, N); None for an empty cloud."""
    N = points.shape[0]
    if lo is not None:
        grid = grid_of(lo, hi, max(N, 1))
    if N == 0:
        return None
    if N > VOXEL_MAX_POINTS:
        raise ValueError(f"at most {VOXEL_MAX_POINTS} points")
    _need_cuda(points, "points")
    points = _f32c(points)
    if lo is None:
        ext = torch.cat([points.min(dim=0).values, points.max(dim=0).values]).tolist()   # the host read
        grid = grid_of(ext[:3], ext[3:], N)
    return points, torch.tensor([0, N], dtype=torch.int64, device=points.device), grid, N


def _one_cloud_rows(points, lo, hi, grid_of, run_ragged) -> torch.Tensor:
    """A filter on one cloud: run_ragged(points, offsets, grid, N) -> (rows, out_offsets) and its first cloud's rows (the second host read)."""
    one = _one_cloud(points, lo, hi, grid_of)
    if one is None:
        return points.new_zeros(0, 3, dtype=torch.float32)
    out, off = run_ragged(*one)
    return out[:int(off[1].item())]


def voxel_downsample_ragged(points: torch.Tensor, offsets: torch.Tensor, grid, max_per_sample: int, counts: Optional[torch.Tensor] = None,
                            return_count: bool = False, return_first: bool = False, return_cells: bool = False, return_inverse: bool = False,
                            chunk: int = 0):
    """Voxel-grid down-sampling per cloud of a ragged batch (rald_post_voxel_downsample_ragged): points [T,3],
    offsets int64 [B+1] on the device, grid = voxel_grid(lo, hi, voxel) -> (points [T,3], out_offsets int64 [B+1], ...), on the device
    and sized for the worst case: cloud b's voxels are rows out_offsets[b] .. out_offsets[b+1]-1, one per occupied cell in ASCENDING
    cell-key order ((c0 * dims1 + c1) * dims2 + c2 - a canonical order, independent of the order of the rows), each the centroid of
    the cell's rows (added in float64 in row order, rounded to float32 once).  Rows past out_offsets[B] are unspecified.
    A row's cell is floor((p - lo) / v) in float32; rows outside the grid (NaN and inf rows included) are dropped.
    Then, in this order, for every flag set: count int32 [T] (rows per voxel), first int64 [T] (the voxel's smallest row index, from
    the cloud's first row: gathers any attribute of a representative row), cells int32 [T,3], inverse int64 [T] (per ROW, laid out
    like points: the rank of its voxel inside its cloud, -1 for a dropped row; rows past offsets[B] or behind counts / the bound are
    unspecified).
    counts (int32 [B] on the device): only the first counts[b] rows of a cloud are valid.  max_per_sample: host bound of the longest
    cloud, at most 2^24 - it is trusted, a cloud LONGER than it is reduced from its first max_per_sample rows.  The result is the same
    bits in every call and batch.  chunk (tests, tools): the chunk length of the split sort, 0 = automatic; the result does not depend
    on it.  No host read, no synchronisation; runs on the current stream."""
    max_per_sample, chunk = _voxel_args(points, max_per_sample, counts, _offsets_shape(offsets, "offsets"), chunk)
    grid3 = _voxel_grid_arg(grid)
    points, counts, B, T, dev = _cloud_batch(points, offsets, counts)
    out = torch.empty(T, 3, device=dev, dtype=torch.float32)
    out_offsets = torch.empty(B + 1, device=dev, dtype=torch.int64)
    cnt = torch.empty(T, device=dev, dtype=torch.int32) if return_count else None
    first = torch.empty(T, device=dev, dtype=torch.int64) if return_first else None
    cells = torch.empty(T, 3, device=dev, dtype=torch.int32) if return_cells else None
    inverse = torch.empty(T, device=dev, dtype=torch.int64) if return_inverse else None
    _cloud_call("voxel_downsample_ragged", "voxel", points, offsets, counts, B, T, dev, max_per_sample, grid3,
                (out.data_ptr(), out_offsets.data_ptr(), _opt(cnt), _opt(first), _opt(cells), _opt(inverse)), chunk)
    return (out, out_offsets) + tuple(t for t in (cnt, first, cells, inverse) if t is not None)


def voxel_downsample(points: torch.Tensor, voxel, lo: Optional[Sequence[float]] = None, hi: Optional[Sequence[float]] = None) -> torch.Tensor:
    """One cloud [N,3] -> [m,3], one centroid per occupied cell of edge `voxel` (a number or 3), in ascending cell-key order: the device
    counterpart of Open3D's voxel_down_sample on the grid voxel_grid(lo, hi, voxel).  Without lo / hi the grid spans the cloud's own
    minimum and maximum - that costs one host read of six numbers (and the cloud must be finite); the result's length is a second
    host read in either case."""
    _one_cloud_check(points, lo, hi)
    if lo is None:
        voxel_grid((0, 0, 0), (0, 0, 0), voxel)                                       # the edge's own rules, before anything is read
    return _one_cloud_rows(points, lo, hi, lambda l, h, n: voxel_grid(l, h, voxel), voxel_downsample_ragged)


def _radius_args(points, radius, grid, max_per_sample, counts, B: Optional[int], chunk, cap, cap_name: str, cap_min: int):
    """The rules of the radius calls beyond the voxel calls' (ValueError, before anything asks where a tensor lives) -> (radius as the
    float32 the kernels use, cap, max_per_sample, chunk, the grid's three ctypes arrays)."""
    max_per_sample, chunk = _voxel_args(points, max_per_sample, counts, B, chunk)
    arrays = _voxel_grid_arg(grid)
    radius = _f32(_positive(radius, "radius must be a finite number > 0"))
    if not radius > 0 or not math.isfinite(radius):
        raise ValueError("radius must fit float32")
    if any(float(v) < radius for v in grid[1]):
        raise ValueError("every cell edge of the grid must be >= radius (build it with voxel_grid(lo, hi, radius))")
    if isinstance(cap, bool) or int(cap) != cap or cap < cap_min or cap > 2 ** 31 - 1:
        raise ValueError(f"{cap_name} must be an integer >= {cap_min}")
    return radius, int(cap), max_per_sample, chunk, arrays


def radius_neighbor_count_ragged(points: torch.Tensor, offsets: torch.Tensor, radius: float, grid, max_per_sample: int,
                                 counts: Optional[torch.Tensor] = None, max_count: int = 0, return_nearest: bool = False, chunk: int = 0):
    """Neighbours within `radius` inside each cloud of a ragged batch (rald_post_radius_count_ragged): points
    [T,3], offsets int64 [B+1] on the device, grid = voxel_grid(lo, hi, voxel) with every cell edge >= radius (voxel=radius is the normal
    use; the grid only indexes the search and does not show in the result beyond its box) -> count int32 [T], laid out like points:
    the number of OTHER rows of the same cloud (by row index: a duplicate counts) with squared float32 distance <= float32(radius)^2,
    min(count, max_count) with max_count > 0 (the search stops there), -1 for a row outside the grid's box (NaN and inf rows
    included; such rows are nobody's neighbour).  return_nearest (needs max_count = 0) adds nn_idx int64 [T] (the nearest other row
    within the radius, from the cloud's first row, the smallest index on equal distances, -1 when there is none) and nn_dist2 float32
    [T] (its squared distance, +inf when there is none).  Rows past offsets[B] or behind counts / the bound are unspecified.
    counts, max_per_sample, chunk: as voxel_downsample_ragged.  Defined to the bit: the same in every call, batch, chunk and grid.
    No host read, no synchronisation; runs on the current stream."""
    radius, max_count, max_per_sample, chunk, grid3 = _radius_args(points, radius, grid, max_per_sample, counts,
                                                                   _offsets_shape(offsets, "offsets"), chunk, max_count, "max_count", 0)
    if return_nearest and max_count:
        raise ValueError("return_nearest needs max_count = 0")
    points, counts, B, T, dev = _cloud_batch(points, offsets, counts)
    cnt = torch.empty(T, device=dev, dtype=torch.int32)
    nn_idx = torch.empty(T, device=dev, dtype=torch.int64) if return_nearest else None
    nn_dist2 = torch.empty(T, device=dev, dtype=torch.float32) if return_nearest else None
    _cloud_call("radius_count_ragged", "radius", points, offsets, counts, B, T, dev, max_per_sample, grid3,
                (radius, max_count, cnt.data_ptr(), _opt(nn_idx), _opt(nn_dist2)), chunk)
    return (cnt, nn_idx, nn_dist2) if return_nearest else cnt


def remove_radius_outliers_ragged(points: torch.Tensor, offsets: torch.Tensor, radius: float, min_neighbors: int, grid, max_per_sample: int,
                                  counts: Optional[torch.Tensor] = None, return_index: bool = False, return_count: bool = False,
                                  chunk: int = 0):
    """Radius outlier removal per cloud of a ragged batch (rald_post_radius_filter_ragged): a row stays iff it
    lies inside the grid's box and at least min_neighbors (>= 1) OTHER rows of its cloud lie within `radius` of it
    (radius_neighbor_count_ragged's count).  -> (points [T,3], out_offsets int64 [B+1], ...) on the device, sized for the worst case:
    cloud b's kept rows are rows out_offsets[b] .. out_offsets[b+1]-1 in their ORIGINAL order, bit for bit the input rows; rows past
    out_offsets[B] are unspecified.  Then, for every flag set: index int64 [T] (per kept row, its row in its cloud), count int32 [T]
    (per INPUT row: min(count, min_neighbors), -1 outside the box).  Arguments as radius_neighbor_count_ragged.
    No host read, no synchronisation; runs on the current stream."""
    radius, min_neighbors, max_per_sample, chunk, grid3 = _radius_args(points, radius, grid, max_per_sample, counts,
                                                                       _offsets_shape(offsets, "offsets"), chunk, min_neighbors, "min_neighbors", 1)
    points, counts, B, T, dev = _cloud_batch(points, offsets, counts)
    out = torch.empty(T, 3, device=dev, dtype=torch.float32)
    out_offsets = torch.empty(B + 1, device=dev, dtype=torch.int64)
    index = torch.empty(T, device=dev, dtype=torch.int64) if return_index else None
    cnt = torch.empty(T, device=dev, dtype=torch.int32) if return_count else None
    _cloud_call("radius_filter_ragged", "radius", points, offsets, counts, B, T, dev, max_per_sample, grid3,
                (radius, min_neighbors, out.data_ptr(), out_offsets.data_ptr(), _opt(index), _opt(cnt)), chunk)
    return (out, out_offsets) + tuple(t for t in (index, cnt) if t is not None)


def remove_radius_outliers(points: torch.Tensor, radius: float, min_neighbors: int, lo: Optional[Sequence[float]] = None,
                           hi: Optional[Sequence[float]] = None) -> torch.Tensor:
    """One cloud [N,3] -> [m,3]: the rows with at least min_neighbors other rows within `radius`, in their order - the device
    counterpart of a radius outlier filter.  lo / hi: the box of the search grid (rows outside it are dropped); without them the box is
    the cloud's own minimum and maximum - that costs one host read of six numbers (and the cloud must be finite); the result's length
    is a second host read in either case.  Where the box would need more than 2^31 - 1 cells of edge `radius` the cells are made
    larger; the result does not depend on that."""
    _one_cloud_check(points, lo, hi)
    _positive(radius, "radius must be a finite number > 0")
    if isinstance(min_neighbors, bool) or int(min_neighbors) != min_neighbors or min_neighbors < 1:
        raise ValueError("min_neighbors must be an integer >= 1")
    return _one_cloud_rows(points, lo, hi, lambda l, h, n: _radius_grid(l, h, radius),
                           lambda p, off, grid, n: remove_radius_outliers_ragged(p, off, radius, int(min_neighbors), grid, n))


def _cluster_size(min_cluster_size) -> int:
    return _whole(min_cluster_size, 1, 2 ** 31 - 1, "min_cluster_size must be an integer >= 1")


def cluster_dbscan_ragged(points: torch.Tensor, offsets: torch.Tensor, eps: float, min_points: int, grid, max_per_sample: int,
                          counts: Optional[torch.Tensor] = None, return_sizes: bool = False, return_count: bool = False, chunk: int = 0):
    """Density clustering (DBSCAN) per cloud of a ragged batch (rald_post_cluster_labels_ragged): points [T,3],
    offsets int64 [B+1] on the device, grid = voxel_grid(lo, hi, voxel) with every cell edge >= eps (the grid only indexes the search
    and does not show in the result beyond its box) -> (labels int32 [T], num_clusters int32 [B], ...) on the device.
    A row is CORE iff it lies inside the box and at least min_points (>= 0) OTHER rows of its cloud lie within eps of it
    (radius_neighbor_count_ragged's count: Open3D's min_points = m is m - 1 here; 0 makes every inside row core, which is Euclidean
    cluster extraction).  A cluster is a connected component of the core rows under "within eps"; a cloud's clusters are numbered
    0 .. C-1 in ascending order of their smallest row index.  A row that is not core but has a core row within eps is a BORDER row of
    the cluster of its NEAREST core row (the smallest row index on equal distances), so the labels are a function of the rows alone.
    labels, laid out like points: the cluster, -1 for noise, -2 for a row outside the box (NaN and inf rows included; such rows are
    nobody's neighbour).  Then, for every flag set: sizes int32 [T] (cloud b's cluster c at row offsets[b] + c: its core and border
    rows; 0 behind the last cluster), count int32 [T] (per row: min(count, min_points), -1 outside the box).  Rows past offsets[B] or
    behind counts / the bound are unspecified.  counts, max_per_sample, chunk: as voxel_downsample_ragged.  Defined to the bit: the
    same in every call, batch, chunk and grid.  No host read, no synchronisation; runs on the current stream."""
    eps, min_points, max_per_sample, chunk, grid3 = _radius_args(points, eps, grid, max_per_sample, counts, _offsets_shape(offsets, "offsets"),
                                                                 chunk, min_points, "min_points", 0)
    points, counts, B, T, dev = _cloud_batch(points, offsets, counts)
    labels = torch.empty(T, device=dev, dtype=torch.int32)
    num = torch.empty(B, device=dev, dtype=torch.int32)
    sizes = torch.empty(T, device=dev, dtype=torch.int32) if return_sizes else None
    cnt = torch.empty(T, device=dev, dtype=torch.int32) if return_count else None
    if T == 0:                                                                       # no rows: an empty tensor has no address to pass
        num.zero_()
    else:
        _cloud_call("cluster_labels_ragged", "cluster", points, offsets, counts, B, T, dev, max_per_sample, grid3,
                    (eps, min_points, labels.data_ptr(), num.data_ptr(), _opt(sizes), _opt(cnt)), chunk)
    return (labels, num) + tuple(t for t in (sizes, cnt) if t is not None)


def remove_small_clusters_ragged(points: torch.Tensor, offsets: torch.Tensor, eps: float, min_points: int, min_cluster_size: int, grid,
                                 max_per_sample: int, counts: Optional[torch.Tensor] = None, largest_only: bool = False,
                                 return_index: bool = False, return_labels: bool = False, chunk: int = 0):
    """Small-cluster removal per cloud of a ragged batch (rald_post_cluster_filter_ragged): a row stays iff
    cluster_dbscan_ragged gives it a cluster (core or border) of at least min_cluster_size (>= 1) rows, with largest_only only the
    cloud's largest cluster (the smallest id on equal sizes).  It drops the floating blobs that the radius and the statistical filter
    keep.  -> (points [T,3], out_offsets int64 [B+1], ...) on the device, sized for the worst case: cloud b's kept rows are rows
    out_offsets[b] .. out_offsets[b+1]-1 in their ORIGINAL order, bit for bit the input rows; rows past out_offsets[B] are unspecified.
    Then, for every flag set: index int64 [T] (per kept row, its row in its cloud), (labels int32 [T], num_clusters int32 [B]) (per
    kept row its cluster in cluster_dbscan_ragged's numbering, NOT renumbered; the clusters before the filter).  Arguments as
    cluster_dbscan_ragged.  No host read, no synchronisation; runs on the current stream."""
    eps, min_points, max_per_sample, chunk, grid3 = _radius_args(points, eps, grid, max_per_sample, counts, _offsets_shape(offsets, "offsets"),
                                                                 chunk, min_points, "min_points", 0)
    min_cluster_size = _cluster_size(min_cluster_size)
    points, counts, B, T, dev = _cloud_batch(points, offsets, counts)
    out = torch.empty(T, 3, device=dev, dtype=torch.float32)
    out_offsets = torch.empty(B + 1, device=dev, dtype=torch.int64)
    index = torch.empty(T, device=dev, dtype=torch.int64) if return_index else None
    labels = torch.empty(T, device=dev, dtype=torch.int32)
    num = torch.empty(B, device=dev, dtype=torch.int32)
    if T == 0:
        out_offsets.zero_()
        num.zero_()
    else:
        _cloud_call("cluster_filter_ragged", "cluster", points, offsets, counts, B, T, dev, max_per_sample, grid3,
                    (eps, min_points, min_cluster_size, int(bool(largest_only)), out.data_ptr(), out_offsets.data_ptr(), _opt(index),
                     labels.data_ptr(), num.data_ptr()), chunk)
    return (out, out_offsets) + ((index,) if return_index else ()) + ((labels, num) if return_labels else ())


def _cluster_one_args(points, eps, min_points, lo, hi) -> None:
    _one_cloud_check(points, lo, hi)
    _positive(eps, "eps must be a finite number > 0")
    _whole(min_points, 0, None, "min_points must be an integer >= 0")


def cluster_dbscan(points: torch.Tensor, eps: float, min_points: int, lo: Optional[Sequence[float]] = None,
                   hi: Optional[Sequence[float]] = None) -> torch.Tensor:
    """One cloud [N,3] -> labels int32 [N] on the device: cluster_dbscan_ragged's - the device counterpart of Open3D's cluster_dbscan
    with min_points counting OTHER rows (Open3D's m is m - 1 here), a canonical numbering and -2 for rows outside the box.  lo / hi:
    the box of the search grid; without them the box is the cloud's own minimum and maximum - that costs one host read of six numbers
    (and the cloud must be finite).  Where the box would need more than 2^31 - 1 cells of edge eps the cells are made larger; the
    result does not depend on that."""
    _cluster_one_args(points, eps, min_points, lo, hi)
    one = _one_cloud(points, lo, hi, lambda l, h, n: _radius_grid(l, h, eps))
    if one is None:
        return torch.zeros(0, dtype=torch.int32, device=points.device)
    p, off, grid, N = one
    return cluster_dbscan_ragged(p, off, eps, int(min_points), grid, N)[0]


def remove_small_clusters(points: torch.Tensor, eps: float, min_points: int, min_cluster_size: int, largest_only: bool = False,
                          lo: Optional[Sequence[float]] = None, hi: Optional[Sequence[float]] = None) -> torch.Tensor:
    """One cloud [N,3] -> [m,3]: remove_small_clusters_ragged's kept rows, in their order.  lo / hi as cluster_dbscan; the result's
    length is a second host read in either case."""
    _cluster_one_args(points, eps, min_points, lo, hi)
    min_cluster_size = _cluster_size(min_cluster_size)
    return _one_cloud_rows(points, lo, hi, lambda l, h, n: _radius_grid(l, h, eps),
                           lambda p, off, grid, n: remove_small_clusters_ragged(p, off, eps, int(min_points), min_cluster_size, grid, n,
                                                                                largest_only=largest_only))


KNN_MAX_K = 32                                           # the largest k of rald_post_knn_ragged


def _knn_args(points, k, grid, max_per_sample, counts, B: Optional[int], chunk, max_radius):
    """The rules of the k-NN calls beyond the voxel calls' (ValueError, before anything asks where a tensor lives) -> (k, max_radius as
    the float32 the kernels use with 0.0 for None, max_per_sample, chunk, the grid's three ctypes arrays)."""
    max_per_sample, chunk = _voxel_args(points, max_per_sample, counts, B, chunk)
    arrays = _voxel_grid_arg(grid)
    k = _knn_k(k)
    return k, _knn_radius(max_radius), max_per_sample, chunk, arrays


def _knn_k(k) -> int:
    return _whole(k, 1, KNN_MAX_K, f"k must be an integer in 1 .. {KNN_MAX_K}")


def _knn_radius(max_radius) -> float:
    if max_radius is None:
        return 0.0
    r = _f32(_positive(max_radius, "max_radius must be None or a finite number > 0"))
    if not r > 0 or not math.isfinite(r):
        raise ValueError("max_radius must fit float32")
    return r


def _knn_ratio(std_ratio) -> float:
    if isinstance(std_ratio, bool) or not isinstance(std_ratio, (int, float)) or not math.isfinite(std_ratio) or std_ratio < 0:
        raise ValueError("std_ratio must be a finite number >= 0")
    return float(std_ratio)


def knn_ragged(points: torch.Tensor, offsets: torch.Tensor, k: int, grid, max_per_sample: int, counts: Optional[torch.Tensor] = None,
               max_radius: Optional[float] = None, return_dist2: bool = True, return_found: bool = False, chunk: int = 0):
    """The k nearest OTHER rows of every row inside its own cloud of a ragged batch (rald_post_knn_ragged):
    points [T,3], offsets int64 [B+1] on the device, 1 <= k <= 32, grid = voxel_grid(lo, hi, cell) - any cell edge: the grid only
    indexes the search and does not show in the result beyond its box; k / 8 to k rows per cell is a good edge -> idx int64 [T,k], laid
    out like points: slot s of row i is the row (from the cloud's first row) of its s-th candidate in the order (squared float32
    distance, row index) ascending, so equal distances come by row index and a duplicate is a neighbour at distance 0; -1 from the
    number of candidates on, and in every slot of a row outside the grid's box (NaN and inf rows included; such rows are nobody's
    neighbour).  max_radius: only rows with squared distance <= float32(max_radius)^2 are candidates.  Then, for every flag set:
    dist2 float32 [T,k] (+inf in the empty slots), found int32 [T] (min(k, candidates), -1 outside).  Rows past offsets[B] or behind
    counts / the bound are unspecified.  counts, max_per_sample, chunk: as voxel_downsample_ragged.  Defined to the bit: the same in
    every call, batch, chunk and grid.  No host read, no synchronisation; runs on the current stream."""
    k, max_radius, max_per_sample, chunk, grid3 = _knn_args(points, k, grid, max_per_sample, counts, _offsets_shape(offsets, "offsets"), chunk,
                                                            max_radius)
    points, counts, B, T, dev = _cloud_batch(points, offsets, counts)
    idx = torch.empty(T, k, device=dev, dtype=torch.int64)
    dist2 = torch.empty(T, k, device=dev, dtype=torch.float32) if return_dist2 else None
    found = torch.empty(T, device=dev, dtype=torch.int32) if return_found else None
    if T:                                                                            # no rows: an empty tensor has no address to pass
        _cloud_call("knn_ragged", "knn", points, offsets, counts, B, T, dev, max_per_sample, grid3,
                    (k, max_radius, idx.data_ptr(), _opt(dist2), _opt(found)), chunk)
    out = (idx,) + tuple(t for t in (dist2, found) if t is not None)
    return out if len(out) > 1 else idx


def remove_statistical_outliers_ragged(points: torch.Tensor, offsets: torch.Tensor, k: int, std_ratio: float, grid, max_per_sample: int,
                                       counts: Optional[torch.Tensor] = None, max_radius: Optional[float] = None, return_index: bool = False,
                                       return_mean: bool = False, return_stats: bool = False, chunk: int = 0):
    """Statistical outlier removal per cloud of a ragged batch (rald_post_statistical_filter_ragged): m[i] is
    the mean distance (float64) from row i to its k nearest other rows (knn_ragged's, fewer where the cloud or max_radius leaves
    fewer); over the rows that have at least one, mu is the mean and sigma the deviation (divided by n - 1) of m; a row stays iff it
    has a neighbour and m[i] <= mu + std_ratio * sigma.  It adapts to the cloud's density, where the radius filter needs a radius.
    -> (points [T,3], out_offsets int64 [B+1], ...) on the device, sized for the worst case: cloud b's kept rows are rows
    out_offsets[b] .. out_offsets[b+1]-1 in their ORIGINAL order, bit for bit the input rows; rows past out_offsets[B] are
    unspecified.  Then, for every flag set: index int64 [T] (per kept row, its row in its cloud), mean float64 [T] (per INPUT row: m,
    +inf without a neighbour, NaN outside the box), stats float64 [B,3] (mu, sigma, the threshold; NaN for a cloud without a row that
    counts).  Unlike Open3D's remove_statistical_outlier, k counts OTHER rows.  Arguments as knn_ragged; std_ratio finite, >= 0.
    Defined to the bit (the sums have one fixed shape): the same in every call, batch, chunk and grid.
    No host read, no synchronisation; runs on the current stream."""
    k, max_radius, max_per_sample, chunk, grid3 = _knn_args(points, k, grid, max_per_sample, counts, _offsets_shape(offsets, "offsets"), chunk,
                                                            max_radius)
    std_ratio = _knn_ratio(std_ratio)
    points, counts, B, T, dev = _cloud_batch(points, offsets, counts)
    out = torch.empty(T, 3, device=dev, dtype=torch.float32)
    out_offsets = torch.empty(B + 1, device=dev, dtype=torch.int64)
    index = torch.empty(T, device=dev, dtype=torch.int64) if return_index else None
    mean = torch.empty(T, device=dev, dtype=torch.float64) if return_mean else None
    stats = torch.empty(B, 3, device=dev, dtype=torch.float64) if return_stats else None
    if T == 0:                                                                       # no rows: an empty tensor has no address to pass
        out_offsets.zero_()
        if stats is not None:
            stats.fill_(float("nan"))
        return (out, out_offsets) + tuple(t for t in (index, mean, stats) if t is not None)
    _cloud_call("statistical_filter_ragged", "statistical", points, offsets, counts, B, T, dev, max_per_sample, grid3,
                (k, max_radius, std_ratio, out.data_ptr(), out_offsets.data_ptr(), _opt(index), _opt(mean), _opt(stats)), chunk)
    return (out, out_offsets) + tuple(t for t in (index, mean, stats) if t is not None)


def remove_statistical_outliers(points: torch.Tensor, k: int, std_ratio: float, lo: Optional[Sequence[float]] = None,
                                hi: Optional[Sequence[float]] = None, cell: Optional[float] = None) -> torch.Tensor:
    """One cloud [N,3] -> [m,3]: remove_statistical_outliers_ragged's kept rows, in their order.  lo / hi: the box of the search grid
    (rows outside it are dropped); without them the box is the cloud's own minimum and maximum - that costs one host read of six
    numbers (and the cloud must be finite); the result's length is a second host read in either case.  cell: the search grid's edge;
    without it half the edge that gives k rows per cell of the box (about k / 8 rows per cell).  The edge grows until the grid fits 2^31 - 1 cells; the result
    does not depend on it for a cloud within lo .. hi (the last cell of voxel_grid reaches beyond hi by less than one edge: a row
    out there is inside for one edge and outside for another)."""
    _one_cloud_check(points, lo, hi)
    k, std_ratio = _knn_k(k), _knn_ratio(std_ratio)
    if cell is not None:
        _positive(cell, "cell must be None or a finite number > 0")
    return _one_cloud_rows(points, lo, hi, lambda l, h, n: _knn_grid(l, h, n, k, cell),
                           lambda p, off, grid, n: remove_statistical_outliers_ragged(p, off, k, std_ratio, grid, n))


def _view_arg(view):
    """view=None -> None; else three finite numbers that fit float32 -> a ctypes float[3]."""
    import ctypes as C
    if view is None:
        return None
    try:
        v = [float(x) for x in view]
    except (TypeError, ValueError):
        raise ValueError("view must be None or 3 finite numbers") from None
    if len(v) != 3 or any(not math.isfinite(x) for x in v):
        raise ValueError("view must be None or 3 finite numbers")
    v = [_f32(x) for x in v]
    if any(not math.isfinite(x) for x in v):
        raise ValueError("view must fit float32")
    return (C.c_float * 3)(*v)


def estimate_normals_ragged(points: torch.Tensor, offsets: torch.Tensor, k: int, grid, max_per_sample: int, counts: Optional[torch.Tensor] = None,
                            max_radius: Optional[float] = None, view: Optional[Sequence[float]] = None, return_curvature: bool = False,
                            return_eigenvalues: bool = False, return_found: bool = False, chunk: int = 0):
    """PCA normals of every row of a ragged batch from its k nearest OTHER rows and itself (rald_post_normals_ragged, DESIGN.md section
    24): points [T,3], offsets int64 [B+1] on the device, k, grid, counts, max_per_sample, max_radius and chunk as knn_ragged ->
    normals float32 [T,3], laid out like points: the unit eigenvector of the smallest eigenvalue of the covariance (float64, a fixed
    six-sweep Jacobi iteration) of the row and its neighbours, turned towards `view` (3 numbers, the sensor's position in the frame of
    the points), without a view (or for a view in the row's tangent plane) so that its largest component is positive.  A row outside
    the grid's box or with fewer than 2 neighbours gets (0, 0, 0).  Then, for every flag set: curvature float32 [T] (the surface
    variation l0 / (l0 + l1 + l2); NaN for such a row), eigenvalues float32 [T,3] (ascending; NaN), found int32 [T] (knn_ragged's).
    Unlike Open3D's estimate_normals, k counts OTHER rows: k = 15 here is knn = 16 there.  Rows past offsets[B] or behind counts / the
    bound are unspecified.  Defined to the bit: the same in every call, batch, chunk and grid; no [T,k] table is built.
    No host read, no synchronisation; runs on the current stream."""
    k, max_radius, max_per_sample, chunk, grid3 = _knn_args(points, k, grid, max_per_sample, counts, _offsets_shape(offsets, "offsets"), chunk,
                                                            max_radius)
    view3 = _view_arg(view)
    points, counts, B, T, dev = _cloud_batch(points, offsets, counts)
    normals = torch.empty(T, 3, device=dev, dtype=torch.float32)
    curv = torch.empty(T, device=dev, dtype=torch.float32) if return_curvature else None
    eig = torch.empty(T, 3, device=dev, dtype=torch.float32) if return_eigenvalues else None
    found = torch.empty(T, device=dev, dtype=torch.int32) if return_found else None
    if T:                                                                            # no rows: an empty tensor has no address to pass
        _cloud_call("normals_ragged", "normals", points, offsets, counts, B, T, dev, max_per_sample, grid3,
                    (k, max_radius, view3, normals.data_ptr(), _opt(curv), _opt(eig), _opt(found)), chunk)
    out = (normals,) + tuple(t for t in (curv, eig, found) if t is not None)
    return out if len(out) > 1 else normals


def estimate_normals(points: torch.Tensor, k: int, view: Optional[Sequence[float]] = None, lo: Optional[Sequence[float]] = None,
                     hi: Optional[Sequence[float]] = None, cell: Optional[float] = None) -> torch.Tensor:
    """One cloud [N,3] -> its normals float32 [N,3] (estimate_normals_ragged's): the device counterpart of Open3D's estimate_normals
    followed by orient_normals_towards_camera_location(view).  lo / hi: the box of the search grid (rows outside it get (0, 0, 0));
    without them the box is the cloud's own minimum and maximum - that costs one host read of six numbers (and the cloud must be
    finite).  cell: the search grid's edge, as in remove_statistical_outliers; the result does not depend on it."""
    _one_cloud_check(points, lo, hi)
    k = _knn_k(k)
    _view_arg(view)
    if cell is not None:
        _positive(cell, "cell must be None or a finite number > 0")
    one = _one_cloud(points, lo, hi, lambda l, h, n: _knn_grid(l, h, n, k, cell))
    if one is None:
        return points.new_zeros(0, 3, dtype=torch.float32)
    p, off, grid, N = one
    return estimate_normals_ragged(p, off, k, grid, N, view=view)


PLANE_MAX_HYPOTHESES = 65536                             # the largest num_hypotheses and max_planes of rald_post_plane_segment_ragged
PLANE_MAX_PLANES = 8


def _plane_args(points, threshold, max_per_sample, num_hypotheses, max_planes, min_inliers, refine, seed, view, counts, B: Optional[int]):
    """The rules of the plane calls (ValueError, before anything asks where a tensor lives) -> (threshold as the float32 the kernels use,
    max_per_sample, H, K, min_inliers, refine as 0 / 1, seed, the view's ctypes array or None)."""
    max_per_sample, _ = _voxel_args(points, max_per_sample, counts, B, 0)
    threshold = _f32(_positive(threshold, "threshold must be a finite number > 0"))
    if not threshold > 0 or not math.isfinite(threshold):
        raise ValueError("threshold must fit float32")
    H = _whole(num_hypotheses, 1, PLANE_MAX_HYPOTHESES, f"num_hypotheses must be an integer in 1 .. {PLANE_MAX_HYPOTHESES}")
    K = _whole(max_planes, 1, PLANE_MAX_PLANES, f"max_planes must be an integer in 1 .. {PLANE_MAX_PLANES}")
    min_inliers = _whole(min_inliers, 3, 2 ** 31 - 1, "min_inliers must be an integer >= 3")
    if not isinstance(refine, (bool, int)) or refine not in (0, 1):
        raise ValueError("refine must be a bool")
    seed = _whole(seed, -2 ** 63, 2 ** 63 - 1, "seed must be an integer that fits int64")
    return threshold, max_per_sample, H, K, min_inliers, int(refine), seed, _view_arg(view)


def _plane_call(entry: str, points, offsets, counts, B: int, T: int, dev, max_per_sample: int, H: int, K: int, args) -> None:
    L = lib()
    nbytes = _nbytes(L.rald_post_plane_scratch_bytes(B, T, max_per_sample, H, K))
    scratch = _scratch(nbytes, dev)
    check(getattr(L, entry)(points.data_ptr(), offsets.data_ptr(), _opt(counts), B, 0, T, max_per_sample, *args, scratch.data_ptr(), nbytes,
                            _stream()))


def segment_planes_ragged(points: torch.Tensor, offsets: torch.Tensor, threshold: float, max_per_sample: int, num_hypotheses: int = 1024,
                          max_planes: int = 1, min_inliers: int = 3, refine: bool = True, seed: int = 0,
                          view: Optional[Sequence[float]] = None, counts: Optional[torch.Tensor] = None, return_best: bool = False):
    """RANSAC plane segmentation per cloud of a ragged batch (rald_post_plane_segment_ragged), the device
    counterpart of Open3D's segment_plane, repeated up to max_planes (1 .. 8) times on what the earlier planes left: points [T,3],
    offsets int64 [B+1] on the device -> (labels int32 [T], planes float64 [B, max_planes, 4], num_planes int32 [B], inliers int32
    [B, max_planes]) on the device.  Every round draws num_hypotheses (1 .. 65536, a FIXED number: no early termination) triples of
    the rows still unlabelled from a counter-based Philox generator keyed by `seed` (mod 2^32) - the same triples in every cloud of
    the same length, in every call - counts for each the rows within `threshold` of its plane (fp32, without a root or a division),
    and takes the hypothesis of the most inliers (the smallest number on equal counts) if it has at least min_inliers (>= 3).  refine
    re-fits the plane to those inliers (float64 centroid and covariance, the smallest eigenvector) and re-marks the inliers in
    float64.  A plane is (a, b, c, d) with a unit normal turned towards `view` (3 numbers, default the origin) and a x + b y + c z +
    d = 0; rows of planes not found are NaN, their inliers 0.  labels, laid out like points: the round that took the row, -1 for a row
    no plane took, -2 for a row with a NaN or an inf.  return_best adds best int32 [B, max_planes], the winning hypothesis of each
    plane (-1: none).  Rows past offsets[B] or behind counts / the bound are unspecified.  counts, max_per_sample: as
    voxel_downsample_ragged.  Defined to the bit: a function of the rows, the arguments and the seed alone.  No host read, no
    synchronisation; runs on the current stream."""
    t, max_per_sample, H, K, min_inliers, refine, seed, view3 = _plane_args(points, threshold, max_per_sample, num_hypotheses, max_planes,
                                                                            min_inliers, refine, seed, view, counts,
                                                                            _offsets_shape(offsets, "offsets"))
    points, counts, B, T, dev = _cloud_batch(points, offsets, counts)
    labels = torch.empty(T, device=dev, dtype=torch.int32)
    planes = torch.empty(B, K, 4, device=dev, dtype=torch.float64)
    num = torch.empty(B, device=dev, dtype=torch.int32)
    inliers = torch.empty(B, K, device=dev, dtype=torch.int32)
    best = torch.empty(B, K, device=dev, dtype=torch.int32)
    if T == 0:                                                                       # no rows: an empty tensor has no address to pass
        planes.fill_(float("nan"))
        num.zero_()
        inliers.zero_()
        best.fill_(-1)
    else:
        _plane_call("rald_post_plane_segment_ragged", points, offsets, counts, B, T, dev, max_per_sample, H, K,
                    (t, H, K, min_inliers, refine, seed, view3, labels.data_ptr(), planes.data_ptr(), num.data_ptr(), inliers.data_ptr(),
                     best.data_ptr()))
    return (labels, planes, num, inliers) + ((best,) if return_best else ())


def remove_planes_ragged(points: torch.Tensor, offsets: torch.Tensor, threshold: float, max_per_sample: int, num_hypotheses: int = 1024,
                         max_planes: int = 1, min_inliers: int = 3, refine: bool = True, seed: int = 0,
                         view: Optional[Sequence[float]] = None, counts: Optional[torch.Tensor] = None, keep_planes: bool = False,
                         return_index: bool = False, return_labels: bool = False):
    """Plane removal per cloud of a ragged batch (rald_post_plane_filter_ragged): segment_planes_ragged, then
    the rows that no plane took stay (ground removal at max_planes = 1) or, with keep_planes, the rows of the planes; rows with a NaN
    or an inf never stay.  -> (points [T,3], out_offsets int64 [B+1], ...) on the device, sized for the worst case: cloud b's kept
    rows are rows out_offsets[b] .. out_offsets[b+1]-1 in their ORIGINAL order, bit for bit the input rows; rows past out_offsets[B]
    are unspecified.  Then, for every flag set: index int64 [T] (per kept row, its row in its cloud), (labels int32 [T], planes
    float64 [B, max_planes, 4], num_planes int32 [B]) (per kept row its label of segment_planes_ragged; the planes and their number).
    Arguments as segment_planes_ragged.  No host read, no synchronisation; runs on the current stream."""
    t, max_per_sample, H, K, min_inliers, refine, seed, view3 = _plane_args(points, threshold, max_per_sample, num_hypotheses, max_planes,
                                                                            min_inliers, refine, seed, view, counts,
                                                                            _offsets_shape(offsets, "offsets"))
    points, counts, B, T, dev = _cloud_batch(points, offsets, counts)
    out = torch.empty(T, 3, device=dev, dtype=torch.float32)
    out_offsets = torch.empty(B + 1, device=dev, dtype=torch.int64)
    index = torch.empty(T, device=dev, dtype=torch.int64) if return_index else None
    labels = torch.empty(T, device=dev, dtype=torch.int32)
    planes = torch.empty(B, K, 4, device=dev, dtype=torch.float64)
    num = torch.empty(B, device=dev, dtype=torch.int32)
    if T == 0:
        out_offsets.zero_()
        planes.fill_(float("nan"))
        num.zero_()
    else:
        _plane_call("rald_post_plane_filter_ragged", points, offsets, counts, B, T, dev, max_per_sample, H, K,
                    (t, H, K, min_inliers, refine, seed, view3, int(bool(keep_planes)), out.data_ptr(), out_offsets.data_ptr(), _opt(index),
                     labels.data_ptr(), planes.data_ptr(), num.data_ptr()))
    return (out, out_offsets) + ((index,) if return_index else ()) + ((labels, planes, num) if return_labels else ())


def _plane_one(points, threshold, num_hypotheses, max_planes, min_inliers, refine, seed, view):
    if not (isinstance(points, torch.Tensor) and points.dim() == 2 and points.shape[-1] == 3 and points.is_floating_point()):
        raise ValueError("points must be a floating-point tensor [N, 3]")
    if points.shape[0] > VOXEL_MAX_POINTS:
        raise ValueError(f"at most {VOXEL_MAX_POINTS} points")
    _plane_args(points, threshold, 1, num_hypotheses, max_planes, min_inliers, refine, seed, view, None, None)


def segment_plane(points: torch.Tensor, threshold: float, num_hypotheses: int = 1024, min_inliers: int = 3, refine: bool = True,
                  seed: int = 0, view: Optional[Sequence[float]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """One cloud [N,3] -> (plane float64 [4], inlier index int64 [m]) on the device, Open3D's shape of segment_plane's result
    (distance_threshold = threshold, num_iterations = num_hypotheses, ransac_n = 3): segment_planes_ragged's one plane and the rows
    it took, ascending.  Without a plane: NaN and no rows.  The index's length is a host read."""
    _plane_one(points, threshold, num_hypotheses, 1, min_inliers, refine, seed, view)
    N = points.shape[0]
    if N == 0:
        return torch.full((4,), float("nan"), dtype=torch.float64, device=points.device), torch.zeros(0, dtype=torch.int64, device=points.device)
    _need_cuda(points, "points")
    off = torch.tensor([0, N], dtype=torch.int64, device=points.device)
    labels, planes, _, _ = segment_planes_ragged(points, off, threshold, N, num_hypotheses, 1, min_inliers, refine, seed, view)
    return planes[0, 0], torch.nonzero(labels == 0).reshape(-1)


def remove_planes(points: torch.Tensor, threshold: float, num_hypotheses: int = 1024, max_planes: int = 1, min_inliers: int = 3,
                  refine: bool = True, seed: int = 0, view: Optional[Sequence[float]] = None, keep_planes: bool = False) -> torch.Tensor:
    """One cloud [N,3] -> [m,3]: remove_planes_ragged's kept rows, in their order.  The result's length is a host read."""
    _plane_one(points, threshold, num_hypotheses, max_planes, min_inliers, refine, seed, view)
    N = points.shape[0]
    if N == 0:
        return points.new_zeros(0, 3, dtype=torch.float32)
    _need_cuda(points, "points")
    off = torch.tensor([0, N], dtype=torch.int64, device=points.device)
    out, out_off = remove_planes_ragged(points, off, threshold, N, num_hypotheses, max_planes, min_inliers, refine, seed, view,
                                        keep_planes=keep_planes)
    return out[:int(out_off[1].item())]


def _normals_of(t, points, what: str) -> None:
    if not (isinstance(t, torch.Tensor) and t.dim() == 2 and t.shape[1] == 3 and t.shape[0] == points.shape[0]):
        raise ValueError(f"{what} must be a tensor [n, 3] with one row per point")


def normal_consistency_ragged(y_pred: torch.Tensor, pred_normals: torch.Tensor, pred_offsets: torch.Tensor, y_gt: torch.Tensor,
                              gt_normals: torch.Tensor, gt_offsets: torch.Tensor, max_pred: int, max_gt: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Normal consistency per frame of two ragged batches with normals (rald_post_normal_consistency_ragged):
    for every row of one side, |n . n'| (float64) with the normal n' of its exact nearest row of the other side in the same frame
    (nearest_neighbors_ragged's), averaged over the rows whose two normals are finite and not zero -> (nc float64 [B,3]: pred -> gt,
    gt -> pred and their mean; counts int64 [B,2]: the rows that counted), on the device.  NaN where no row counts.  max_pred /
    max_gt as in cloud_metrics_ragged.  The sums have one fixed shape: a frame's values are the same bits alone and in any batch.
    No host read, no synchronisation; runs on the current stream."""
    max_pred, max_gt = _bound(max_pred, "max_pred"), _bound(max_gt, "max_gt")
    _xyz(y_pred, "y_pred")
    _xyz(y_gt, "y_gt")
    _normals_of(pred_normals, y_pred, "pred_normals")
    _normals_of(gt_normals, y_gt, "gt_normals")
    B = _ragged_pair(y_pred, pred_offsets, y_gt, gt_offsets, ("y_pred", "pred_offsets", "y_gt", "gt_offsets"))
    dev = y_pred.device
    y_pred, y_gt = _f32c(y_pred), _f32c(y_gt).to(dev)
    pred_normals, gt_normals = _f32c(pred_normals).to(dev), _f32c(gt_normals).to(dev)
    nc = torch.empty(B, 3, device=dev, dtype=torch.float64)
    cnt = torch.empty(B, 2, device=dev, dtype=torch.int64)
    Tp, Tg = y_pred.shape[0], y_gt.shape[0]
    if Tp == 0 or Tg == 0:                                                           # a side without a row: an empty tensor has no address to pass
        nc.fill_(float("nan"))
        cnt.zero_()
        return nc, cnt
    nbytes = _nbytes(lib().rald_post_normal_consistency_scratch_bytes(B, Tp, Tg, max_pred, max_gt))
    scratch = _scratch(nbytes, dev)
    check(lib().rald_post_normal_consistency_ragged(y_pred.data_ptr(), pred_normals.data_ptr(), pred_offsets.data_ptr(), Tp, y_gt.data_ptr(),
                                                    gt_normals.data_ptr(), gt_offsets.data_ptr(), Tg, B, max_pred, max_gt, nc.data_ptr(),
                                                    cnt.data_ptr(), scratch.data_ptr(), nbytes, _stream()))
    return nc, cnt


def normal_consistency(y_pred: torch.Tensor, pred_normals: torch.Tensor, y_gt: torch.Tensor, gt_normals: torch.Tensor) -> dict:
    """normal_consistency_ragged for one frame, read to the host: {'pred_to_gt', 'gt_to_pred', 'mean'} as Python floats."""
    _xyz(y_pred, "y_pred")
    _xyz(y_gt, "y_gt")
    _need_cuda(y_pred, "y_pred")
    off = torch.tensor([[0, y_pred.shape[0]], [0, y_gt.shape[0]]], dtype=torch.int64, device=y_pred.device)
    nc, _ = normal_consistency_ragged(y_pred, pred_normals, off[0], y_gt, gt_normals, off[1], y_pred.shape[0], y_gt.shape[0])
    host = nc[0].cpu().tolist()
    return {"pred_to_gt": host[0], "gt_to_pred": host[1], "mean": host[2]}


def _knn_grid(lo, hi, n: int, k: int, cell=None):
    """voxel_grid(lo, hi, edge) for a k-NN search of n rows: edge = `cell`, or HALF the edge at which a cell of the box holds k rows -
    (volume * k / n)^(1/3) / 2 over the axes that have an extent (1.0 for a box of no extent), about k / 8 rows per cell, the fastest
    of k / 8, k and 8 k rows per cell where it was measured; then the smallest edge * 2^j (j >= 0) that keeps
    the grid within 2^31 - 1 cells."""
    try:
        voxel_grid(lo, hi, 1.0)                                                        # the box's own rules
    except ValueError as e:
        if "cells" not in str(e):
            raise
    if cell is None:
        ext = [float(h) - float(l) for l, h in zip(lo, hi)]
        ext = [e for e in ext if e > 0]
        cell = 0.5 * (math.prod(ext) * k / n) ** (1.0 / len(ext)) if ext else 1.0
        tiny = max(abs(float(x)) for x in list(lo) + list(hi)) * 2.0 ** -20            # never below the coordinates' resolution
        cell = max(cell, tiny, 1e-30)
        if not math.isfinite(cell):
            cell = max(ext)
    return _radius_grid(lo, hi, cell)


def _radius_grid(lo, hi, radius):
    """voxel_grid(lo, hi, edge) with the smallest edge radius * 2^k (k >= 0) that keeps the grid within 2^31 - 1 cells."""
    edge = float(radius)
    for _ in range(64):
        try:
            return voxel_grid(lo, hi, edge)
        except ValueError as e:
            if "cells" not in str(e):
                raise
        edge *= 2.0
    raise ValueError("no grid of at most 2^31 - 1 cells covers lo .. hi")


ICP_MAX_ITERATIONS = 64                                  # the largest max_iterations of rald_post_icp_ragged
ICP_MODES = {"point": 0, "plane": 1, "point_to_point": 0, "point_to_plane": 1, 0: 0, 1: 1}
ICP_STATUS = ("max_iterations", "converged", "too_few_correspondences", "degenerate")


def _icp_mode(mode) -> int:
    if isinstance(mode, bool) or not isinstance(mode, (str, int)) or mode not in ICP_MODES:
        raise ValueError("mode must be 'point' (0) or 'plane' (1)")
    return ICP_MODES[mode]


def _icp_args(source, target, max_distance, grid, max_source, max_target, target_normals, init, mode, max_iterations, tolerance,
              min_correspondences, source_counts, target_counts, B: Optional[int], chunk):
    """The rules of the ICP calls (ValueError, before anything asks where a tensor lives) -> (max_distance as the float32 the kernels
    use, max_source, max_target, mode, max_iterations, tolerance, min_correspondences, chunk, the grid's three ctypes arrays)."""
    for t, what in ((source, "source"), (target, "target")):
        if not (isinstance(t, torch.Tensor) and t.dim() == 2 and t.shape[-1] == 3 and t.is_floating_point()):
            raise ValueError(f"{what} must be a floating-point tensor [T, 3]")
    max_source, chunk = _voxel_args(source, max_source, source_counts, B, chunk)
    max_target, _ = _voxel_args(target, max_target, target_counts, B, 0)
    max_distance = _f32(_positive(max_distance, "max_distance must be a finite number > 0"))
    if not max_distance > 0 or not math.isfinite(max_distance):
        raise ValueError("max_distance must fit float32")
    grid3 = _voxel_grid_arg(grid)
    if any(float(v) < max_distance for v in grid[1]):
        raise ValueError("every cell edge of the grid must be >= max_distance (build it with voxel_grid(lo, hi, max_distance))")
    mode = _icp_mode(mode)
    if mode == 1:
        if target_normals is None:
            raise ValueError("plane mode needs target_normals")
        _normals_of(target_normals, target, "target_normals")
    if init is not None and not (isinstance(init, torch.Tensor) and init.dtype == torch.float64
                                 and (B is None or tuple(init.shape) in ((B, 12), (B, 4, 4), (B, 16)))):
        raise ValueError("init must be a float64 tensor [B, 12] (R row-major, then t), [B, 16] or [B, 4, 4]")
    max_iterations = _whole(max_iterations, 1, ICP_MAX_ITERATIONS, f"max_iterations must be an integer in 1 .. {ICP_MAX_ITERATIONS}")
    if isinstance(tolerance, bool) or not isinstance(tolerance, (int, float)) or not tolerance >= 0:
        raise ValueError("tolerance must be a number >= 0")
    min_correspondences = _whole(min_correspondences, 1, 2 ** 31 - 1, "min_correspondences must be an integer >= 1")
    return max_distance, max_source, max_target, mode, max_iterations, float(tolerance), min_correspondences, chunk, grid3


def _init12(init: torch.Tensor, B: int, dev) -> torch.Tensor:
    """[B,12], [B,16] or [B,4,4] float64 -> contiguous [B,12] on the device (R row-major, then t)."""
    init = init.detach().to(dev)
    if init.dim() == 2 and init.shape[1] == 12:
        return init.contiguous()
    M = init.reshape(B, 4, 4)
    return torch.cat([M[:, :3, :3].reshape(B, 9), M[:, :3, 3]], dim=1).contiguous()


def register_icp_ragged(source: torch.Tensor, source_offsets: torch.Tensor, target: torch.Tensor, target_offsets: torch.Tensor,
                        max_distance: float, grid, max_source: int, max_target: int, target_normals: Optional[torch.Tensor] = None,
                        init: Optional[torch.Tensor] = None, max_iterations: int = 30, tolerance: float = 1e-6,
                        min_correspondences: int = 6, mode=None, source_counts: Optional[torch.Tensor] = None,
                        target_counts: Optional[torch.Tensor] = None, return_correspondences: bool = False, return_moved: bool = False,
                        chunk: int = 0) -> Dict[str, torch.Tensor]:
    """ICP registration of every source cloud onto the target cloud of the same batch position (rald_post_icp_ragged, DESIGN.md
    section 27), the device counterpart of Open3D's registration_icp: source [Ts,3] / target [Tt,3] with int64 offsets [B+1] on the
    device, grid = voxel_grid(lo, hi, max_distance) over the box of the TARGET (target rows outside it are nobody's match; the grid
    does not show otherwise), max_source / max_target the host bounds of the longest cloud.  mode 'point' or 'plane' (default: plane
    iff target_normals [Tt,3] are given).  Each iteration moves the source by the current transform (float64), takes for every row its
    nearest target row within max_distance (float32 distances, the lowest row on equal ones), sums the normal equations of the
    linearised objective in float64 in a fixed shape, solves them by Cholesky and applies the step as an exact rational rotation; it
    stops when every component of the step is <= tolerance, when fewer than min_correspondences rows have a match, or when the
    equations are degenerate (an exactly planar target in plane mode).  init: float64 [B,12] (R row-major then t), [B,16] or
    [B,4,4] on the device.  -> dict of device tensors: 'transform' float64 [B,4,4] (target ~ R source + t), 'fitness' float64 [B]
    (matched / usable source rows under the final transform), 'inlier_rmse' float64 [B], 'step' float64 [B] (the last step's
    largest component), 'residual' float64 [B] (the final sum of squared residuals), 'status' int32 [B] (0 ran all iterations, 1
    converged, 2 too few correspondences, 3 degenerate: ICP_STATUS), 'iterations' int32 [B] (updates applied), 'count' int32 [B];
    with return_correspondences 'correspondences' int64 [Ts] (the target row from the cloud's first target row, -1 for none), with
    return_moved 'moved' float32 [Ts,3] (the source under the final transform).  Rows past the offsets or behind counts / the bounds
    are unspecified.  Defined to the bit: the same in every call, batch, chunk and grid.  All iterations run on the device: no host
    read, no synchronisation; runs on the current stream."""
    B = _offsets_shape(source_offsets, "source_offsets")
    if _offsets_shape(target_offsets, "target_offsets") != B:
        raise ValueError("source_offsets and target_offsets must describe the same batch")
    if mode is None:
        mode = "plane" if target_normals is not None else "point"
    max_distance, max_source, max_target, mode, max_iterations, tolerance, min_correspondences, chunk, grid3 = _icp_args(
        source, target, max_distance, grid, max_source, max_target, target_normals, init, mode, max_iterations, tolerance, min_correspondences,
        source_counts, target_counts, B, chunk)
    source, source_counts, _, Ts, dev = _cloud_batch(source, source_offsets, source_counts)
    target, target_counts, _, Tt, _ = _cloud_batch(target, target_offsets, target_counts)
    normals = _f32c(target_normals).to(dev) if mode == 1 else None
    init = _init12(init, B, dev) if init is not None else None
    transform = torch.empty(B, 4, 4, device=dev, dtype=torch.float64)
    stats = torch.empty(B, 4, device=dev, dtype=torch.float64)
    info = torch.empty(B, 3, device=dev, dtype=torch.int32)
    corr = torch.empty(Ts, device=dev, dtype=torch.int64) if return_correspondences else None
    moved = torch.empty(Ts, 3, device=dev, dtype=torch.float32) if return_moved else None
    L = lib()
    pre, tail = ("rald_op_", (chunk,)) if chunk else ("rald_post_", ())
    nbytes = _nbytes(getattr(L, pre + "icp_scratch_bytes")(B, Ts, max_source, Tt, max_target, *tail))
    scratch = _scratch(nbytes, dev)
    pad = torch.zeros(4, device=dev, dtype=torch.float32)                            # no rows: an empty tensor has no address to pass
    check(getattr(L, pre + "icp_ragged")((source if Ts else pad).data_ptr(), source_offsets.data_ptr(), _opt(source_counts), 0, Ts, max_source,
                                         (target if Tt else pad).data_ptr(), target_offsets.data_ptr(), _opt(target_counts), 0, Tt, max_target,
                                         (normals if Tt else pad).data_ptr() if mode == 1 else None, B, *grid3, mode, max_distance,
                                         max_iterations, tolerance, min_correspondences, _opt(init), transform.data_ptr(), stats.data_ptr(),
                                         info.data_ptr(), _opt(corr) if Ts else None, _opt(moved) if Ts else None, scratch.data_ptr(), nbytes,
                                         *tail, _stream()))
    out = {"transform": transform, "fitness": stats[:, 0], "inlier_rmse": stats[:, 1], "step": stats[:, 2], "residual": stats[:, 3],
           "status": info[:, 0], "iterations": info[:, 1], "count": info[:, 2]}
    if return_correspondences:
        out["correspondences"] = corr
    if return_moved:
        out["moved"] = moved
    return out


def register_icp(source: torch.Tensor, target: torch.Tensor, max_distance: float, target_normals: Optional[torch.Tensor] = None,
                 init: Optional[torch.Tensor] = None, max_iterations: int = 30, tolerance: float = 1e-6, min_correspondences: int = 6,
                 mode=None, lo: Optional[Sequence[float]] = None, hi: Optional[Sequence[float]] = None, return_correspondences: bool = False,
                 return_moved: bool = False) -> Dict[str, torch.Tensor]:
    """One pair: source [n,3] onto target [m,3] -> register_icp_ragged's dict without the batch dimension ('transform' float64 [4,4],
    scalars as 0-d device tensors), the device counterpart of Open3D's registration_icp(source, target, max_distance, init).  init:
    float64 [4,4] or [12].  lo / hi: the box of the target's search grid; without them the target's own minimum and maximum - that
    costs one host read of six numbers (and the target must be finite).  Where the box would need more than 2^31 - 1 cells of edge
    max_distance the cells are made larger; the result does not depend on that.  An empty source or target gives init, status 2."""
    _one_cloud_check(target, lo, hi)
    if mode is None:
        mode = "plane" if target_normals is not None else "point"
    if init is not None:
        if not (isinstance(init, torch.Tensor) and init.dtype == torch.float64 and tuple(init.shape) in ((4, 4), (12,), (16,))):
            raise ValueError("init must be a float64 tensor [4, 4] or [12]")
        init = init.reshape(1, -1)
    _icp_one_check(source, target, max_distance, target_normals, init, mode, max_iterations, tolerance, min_correspondences)
    dev = source.device
    n = source.shape[0]
    one = _one_cloud(target, lo, hi, lambda l, h, rows: _radius_grid(l, h, max_distance))
    if one is None:                                                                  # no target row: nothing to index
        _need_cuda(source, "source")
        grid, m = _radius_grid((0, 0, 0), (0, 0, 0), max_distance), 0
        target = torch.zeros(0, 3, device=dev, dtype=torch.float32)
    else:
        target, _, grid, m = one
    _need_cuda(source, "source")
    off = torch.tensor([[0, n], [0, m]], dtype=torch.int64, device=dev)
    out = register_icp_ragged(source, off[0], target, off[1], max_distance, grid, max(n, 1), max(m, 1), target_normals, init, max_iterations,
                              tolerance, min_correspondences, mode, return_correspondences=return_correspondences, return_moved=return_moved)
    return {k: (v[0] if k not in ("correspondences", "moved") else v) for k, v in out.items()}


def _icp_one_check(source, target, max_distance, target_normals, init, mode, max_iterations, tolerance, min_correspondences) -> None:
    """register_icp's ValueErrors: the ragged call's rules on a grid that every max_distance passes."""
    edge = min(_positive(max_distance, "max_distance must be a finite number > 0") * 2.0, 1e30)
    _icp_args(source, target, max_distance, ((0.0, 0.0, 0.0), (edge,) * 3, (1, 1, 1)), 1, 1, target_normals, init, mode, max_iterations,
              tolerance, min_correspondences, None, None, 1, 0)
    if source.shape[0] > VOXEL_MAX_POINTS or target.shape[0] > VOXEL_MAX_POINTS:
        raise ValueError(f"at most {VOXEL_MAX_POINTS} points a cloud")


def _transform_args(points, transforms, normals, max_per_sample, counts, B: Optional[int]) -> int:
    """The rules of the rigid-transform calls (ValueError) -> max_per_sample."""
    max_per_sample, _ = _voxel_args(points, max_per_sample, counts, B, 0)
    if not (isinstance(transforms, torch.Tensor) and transforms.dtype == torch.float64
            and (B is None or tuple(transforms.shape) in ((B, 12), (B, 16), (B, 4, 4)))):
        raise ValueError("transforms must be a float64 tensor [B, 4, 4], [B, 16] or [B, 12] (R row-major, then t)")
    if normals is not None:
        _normals_of(normals, points, "normals")
    return max_per_sample


def transform_points_ragged(points: torch.Tensor, offsets: torch.Tensor, transforms: torch.Tensor, max_per_sample: int,
                            normals: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None):
    """The rigid transform of every cloud of a ragged batch by its own float64 transform (rald_post_rigid_transform_ragged, DESIGN.md
    section 27): points [T,3], offsets int64 [B+1] and transforms float64 [B,4,4] / [B,16] / [B,12] on the device (register_icp_ragged's
    'transform') -> points float32 [T,3]: R p + t in float64 in the order register_icp_ragged moves its source, rounded to float32
    once, so the result is its 'moved'.  With normals [T,3] -> (points, normals): the normals rotated by R alone.  Rows past
    offsets[B] or behind counts / the bound are unspecified.  No host read, no synchronisation; runs on the current stream."""
    B = _offsets_shape(offsets, "offsets")
    max_per_sample = _transform_args(points, transforms, normals, max_per_sample, counts, B)
    points, counts, B, T, dev = _cloud_batch(points, offsets, counts)
    transforms = transforms.detach().to(dev).reshape(B, -1).contiguous()
    out = torch.empty(T, 3, device=dev, dtype=torch.float32)
    out_normals = torch.empty(T, 3, device=dev, dtype=torch.float32) if normals is not None else None
    if T:                                                                            # no rows: an empty tensor has no address to pass
        nrm = _f32c(normals).to(dev) if normals is not None else None
        check(lib().rald_post_rigid_transform_ragged(points.data_ptr(), offsets.data_ptr(), _opt(counts), B, 0, T, max_per_sample,
                                                     transforms.data_ptr(), transforms.shape[1], _opt(nrm), out.data_ptr(), _opt(out_normals),
                                                     _stream()))
    return out if normals is None else (out, out_normals)


def transform_points(points: torch.Tensor, transform: torch.Tensor, normals: Optional[torch.Tensor] = None):
    """One cloud [N,3] and one float64 transform [4,4] (or [12]: R row-major, then t) on the device -> transform_points_ragged's
    result for it."""
    if not (isinstance(points, torch.Tensor) and points.dim() == 2 and points.shape[-1] == 3 and points.is_floating_point()):
        raise ValueError("points must be a floating-point tensor [N, 3]")
    if not (isinstance(transform, torch.Tensor) and transform.dtype == torch.float64 and tuple(transform.shape) in ((4, 4), (16,), (12,))):
        raise ValueError("transform must be a float64 tensor [4, 4] or [12]")
    N = points.shape[0]
    if N > VOXEL_MAX_POINTS:
        raise ValueError(f"at most {VOXEL_MAX_POINTS} points")
    _transform_args(points, transform.reshape(1, -1), normals, 1, None, 1)
    _need_cuda(points, "points")
    off = torch.tensor([0, N], dtype=torch.int64, device=points.device)
    return transform_points_ragged(points, off, transform.reshape(1, -1), max(N, 1), normals)


# ---- isosurface meshing of dense volumes: naive surface nets ------------------------------------------------------
SURFACE_MAX_DIM = 1024                                   # the largest node count per axis of rald_post_surface_nets
SURFACE_MAX_NODES = (2 ** 31 - 1) // 6                   # batch * nx * ny * nz: six triangles a node at most, counted in int32


def _grid_spec(lo, spacing, dims):
    """The rules of a node grid (ValueError) -> (lo3, h3 as the float32 numbers the kernels use, dims3 as ints)."""
    try:
        lo3, h3 = [_f32(float(x)) for x in lo], [_f32(float(x)) for x in spacing]
        ok = len(lo3) == 3 and len(h3) == 3 and len(dims) == 3 and all(not isinstance(d, bool) and int(d) == d for d in dims)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("lo and spacing must be 3 numbers each, dims 3 integers")
    if any(not math.isfinite(x) for x in lo3) or any(not math.isfinite(x) or x <= 0 for x in h3):
        raise ValueError("lo must be finite and spacing finite and > 0 in float32")
    dims3 = [int(d) for d in dims]
    if any(d < 2 or d > SURFACE_MAX_DIM for d in dims3):
        raise ValueError(f"every dim must be in 2 .. {SURFACE_MAX_DIM}")
    return lo3, h3, dims3


def _surface_args(volume, iso, lo, spacing, capacity, dim: int):
    """The rules of the surface calls (ValueError, before anything asks where the volume lives) -> (iso, lo3, h3, capacity or None)."""
    if not (isinstance(volume, torch.Tensor) and volume.dim() == dim and volume.is_floating_point()):
        raise ValueError("volume must be a floating-point tensor " + ("[B, nx, ny, nz]" if dim == 4 else "[nx, ny, nz]"))
    shape = tuple(volume.shape[-3:])
    B = volume.shape[0] if dim == 4 else 1
    lo3, h3, _ = _grid_spec(lo, spacing, shape)
    if B < 1 or B > 65535 or B * shape[0] * shape[1] * shape[2] > SURFACE_MAX_NODES:
        raise ValueError(f"batch must be 1 .. 65535 and batch * nx * ny * nz at most {SURFACE_MAX_NODES}")
    if isinstance(iso, bool) or not isinstance(iso, (int, float)) or math.isnan(iso):
        raise ValueError("iso must be a number, not a NaN")
    if capacity is not None:
        try:
            mv, mf = capacity
            capacity = (_whole(mv, 0, 2 ** 40, ""), _whole(mf, 0, 2 ** 40, ""))
        except (TypeError, ValueError):
            raise ValueError("capacity must be (max_vertices, max_faces), two integers in 0 .. 2^40, or None") from None
    return _f32(float(iso)), lo3, h3, capacity


def _surface_call(volume, iso, lo3, h3, vertices, v_off, faces, f_off, cells) -> None:
    import ctypes as C
    B, dims = volume.shape[0], [int(d) for d in volume.shape[1:]]
    L = lib()
    nbytes = _nbytes(L.rald_post_surface_scratch_bytes(B, *dims))
    scratch = _scratch(nbytes, volume.device)
    check(L.rald_post_surface_nets(volume.data_ptr(), B, (C.c_int32 * 3)(*dims), (C.c_float * 3)(*lo3), (C.c_float * 3)(*h3), iso,
                                   _opt(vertices), v_off.data_ptr(), 0 if vertices is None else vertices.shape[0], _opt(faces),
                                   f_off.data_ptr(), 0 if faces is None else faces.shape[0], _opt(cells), scratch.data_ptr(), nbytes, _stream()))


def extract_surface_batch(volume: torch.Tensor, iso: float = 0.0, lo: Sequence[float] = (0.0, 0.0, 0.0),
                          spacing: Sequence[float] = (1.0, 1.0, 1.0), capacity: Optional[Tuple[int, int]] = None, return_cells: bool = False):
    """The isosurface value = iso of every volume of a batch as a triangle mesh, by naive surface nets (rald_post_surface_nets, DESIGN.md
    section 28): volume [B, nx, ny, nz] on the device, node (i, j, k) at lo + (i, j, k) * spacing -> (vertices float32 [V, 3], v_offsets
    int64 [B+1], faces int32 [F, 3], f_offsets int64 [B+1][, cells int32 [V]]) on the device.  Volume b's vertices are rows v_offsets[b]
    .. v_offsets[b+1]-1, one per cell whose corners are not all on one side of iso (inside iff value > iso; a NaN is outside), at the
    mean of the cell's edge crossings, in ascending cell order; its triangles rows f_offsets[b] .. f_offsets[b+1]-1, two per grid edge
    that crosses and has four cells around it, with vertex numbers local to the volume, counter-clockwise seen from the outside (value
    <= iso), so normals point from occupied to empty.  A surface that does not touch the grid's border is closed.  cells: each vertex's
    linear cell index (i * (ny - 1) + j) * (nz - 1) + k.
    capacity = (max_vertices, max_faces) over the whole batch: one call, no host read; V, F are the capacities, the offsets hold the
    TRUE counts (compare offsets[B] with the capacity: rows at or beyond it are not written, rows between offsets[B] and the capacity
    are unspecified).  capacity = None: a counting call, ONE host read of the two totals, exact allocation, the full call.
    Defined to the bit: a function of the values, iso, lo, spacing and the dims alone.  Runs on the current stream."""
    iso, lo3, h3, capacity = _surface_args(volume, iso, lo, spacing, capacity, 4)
    _need_cuda(volume, "volume")
    volume = _f32c(volume)
    B, dev = volume.shape[0], volume.device
    v_off = torch.empty(B + 1, device=dev, dtype=torch.int64)
    f_off = torch.empty(B + 1, device=dev, dtype=torch.int64)
    if capacity is None:
        _surface_call(volume, iso, lo3, h3, None, v_off, None, f_off, None)
        capacity = tuple(int(x) for x in torch.stack((v_off[B], f_off[B])).tolist())          # the one host read
    vertices = torch.empty(capacity[0], 3, device=dev, dtype=torch.float32)
    faces = torch.empty(capacity[1], 3, device=dev, dtype=torch.int32)
    cells = torch.empty(capacity[0], device=dev, dtype=torch.int32) if return_cells else None
    # an empty tensor has no address to pass: a NULL output is simply not written
    _surface_call(volume, iso, lo3, h3, vertices if capacity[0] else None, v_off, faces if capacity[1] else None, f_off,
                  cells if capacity[0] else None)
    return (vertices, v_off, faces, f_off) + ((cells,) if return_cells else ())


def extract_surface(volume: torch.Tensor, iso: float = 0.0, lo: Sequence[float] = (0.0, 0.0, 0.0), spacing: Sequence[float] = (1.0, 1.0, 1.0),
                    return_cells: bool = False):
    """extract_surface_batch for one volume [nx, ny, nz] -> (vertices [V, 3], faces int32 [F, 3][, cells]), trimmed (one host read)."""
    _surface_args(volume, iso, lo, spacing, None, 3)
    out = extract_surface_batch(volume.unsqueeze(0), iso, lo, spacing, None, return_cells)
    return (out[0], out[2]) + tuple(out[4:])


def mesh_to_metric(vertices_norm: torch.Tensor, faces: torch.Tensor, lidar_pc_range, norm_anisotropy: bool, norm_isotropy: bool,
                   view_cone_mode: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """A mesh in the decoder's normalised coordinates -> (vertices, faces) in metric coordinates (cartesian if view_cone_mode): the
    vertices by inverse_norm_points (+ polar2cartesian), bit for bit; the faces with the last two vertex numbers of every triangle
    exchanged where the transform reverses orientation, so that they stay counter-clockwise seen from the empty side.  In view-cone
    mode it does: the azimuth is -(y * pi / 180), so the Jacobian determinant of (r, az, el) -> (x, y, z) is negative wherever r > 0 and
    |el| < 90.  Without it the transform is a positive scaling per axis and a shift, which keeps orientation."""
    _xyz(vertices_norm, "vertices_norm")
    if not (isinstance(faces, torch.Tensor) and faces.dim() == 2 and faces.shape[1] == 3 and not faces.is_floating_point()):
        raise ValueError("faces must be an integer tensor [F, 3]")
    if not (norm_anisotropy or norm_isotropy):
        raise ValueError("one of norm_anisotropy / norm_isotropy is required")
    _doubles(lidar_pc_range, 6, "pc_range", _PC_RANGE)
    out = _transform(vertices_norm, lidar_pc_range, norm_anisotropy, norm_isotropy, bool(view_cone_mode))
    return out, (faces[:, [0, 2, 1]].contiguous() if view_cone_mode else faces)
