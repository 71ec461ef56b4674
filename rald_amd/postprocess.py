"""Device counterparts of the host post-processing the reference runs after ``vae.decode``
(engine_generation.py:229-243, :283-322): same function names and argument meaning as
``utils/utils.py`` (``inverse_norm_points``, ``cal_metrics``) and
``dataset_preprocessor/lidar.py`` (``polar2cartesian``), operating on CUDA tensors through
``rald_post_*`` (include/rald_hip.h).  ``occupied_points`` is the fused form of
``np.where(output > 0)`` -> ``grid[ind]`` -> ``inverse_norm_points`` -> ``polar2cartesian``.
"""
from __future__ import annotations

from typing import Tuple

import torch

from ._handles import _doubles, _f32c, _need_cuda, _opt, _ragged_batch, _stream
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


def accuracy_iou(outputs: torch.Tensor, labels: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """engine_generation.py:229-243 per sample: (accuracy [B], iou [B]); the caller takes .mean()."""
    _need_cuda(outputs, "outputs")
    outputs, labels = _f32c(outputs), _f32c(labels).to(outputs.device)
    B, Q = outputs.shape
    acc = torch.empty(B, device=outputs.device, dtype=torch.float32)
    iou = torch.empty(B, device=outputs.device, dtype=torch.float32)
    check(lib().rald_post_iou(outputs.data_ptr(), labels.data_ptr(), B, Q, acc.data_ptr(), iou.data_ptr(), _stream()))
    return acc, iou
