"""The reference's autoencoder engine (engine_ae.py) around the native stage-1 step: ``train_one_epoch`` restates the loop body
(:55-134) around a step object (``train_ae.AeStepTrainer`` or ``train_ae.GraphedAeStep``), ``evaluate_losses`` the loss / IoU part of
``evaluate`` (:185-227) as a forward-only use of ``train_ops.ae_loss``.  Logging, learning-rate schedules (pass ``lr_fn``) and the
Chamfer half of ``evaluate`` (:229-274; ``engine_generation.chamfer_of_decode`` has the pieces) are out of scope."""
from __future__ import annotations

import math
from typing import Callable, Dict, Iterable, Optional

import torch

from . import train_ops as TO
from .engine_generation import _get

KL_WEIGHT = 1e-3                                                   # engine_ae.py:48


def train_one_epoch(step, data_loader: Iterable, args, lr_fn: Optional[Callable[[int], None]] = None) -> Dict[str, float]:
    """engine_ae.train_one_epoch (:55-134) with the iteration handed to ``step``: an ``AeStepTrainer`` (its ``.step`` is called) or a
    ``GraphedAeStep`` / any callable with that signature.  Per batch: ``lr_fn(data_iter_step)`` when an accumulation window starts (:58-59),
    the ``data_dict`` keys of :60-63 with ``in_voxel_num[0]``, ``args.train.vol_weight`` / ``near_weight`` and kl_weight 1e-3 (:48-50),
    an update every ``args.train.accum_iter`` iterations clipped to ``args.train.clip_grad`` (:107-112), the EMA every iteration (:116).
    The loss tensor is read once per iteration for the reference's ``isfinite`` exit (:103-105; raised as FloatingPointError - the step is
    already enqueued then, the reference stops just before it); accuracy and IoU (:96-101) accumulate on the device and are read at the
    end.  Returns the epoch means, as the reference's ``meter.global_avg``."""
    run = step.step if hasattr(step, "step") else step
    accum_iter = int(args.train.accum_iter)
    vol_weight, near_weight = float(args.train.vol_weight), float(args.train.near_weight)
    max_norm = _get(args.train, "clip_grad", None)
    sums = [0.0, 0.0, 0.0, 0.0]
    metrics, n_iter = None, 0
    for data_iter_step, data_dict in enumerate(data_loader):
        if lr_fn is not None and data_iter_step % accum_iter == 0:
            lr_fn(data_iter_step)
        points, labels, surface = data_dict["query_points"], data_dict["query_labels"], data_dict["lidar_points"]
        in_voxel_num = data_dict["in_voxel_num"][0]
        losses, counts, _ = run(surface, points, labels.to(torch.float32), in_voxel_num, update=(data_iter_step + 1) % accum_iter == 0,
                                accum_iter=accum_iter, max_norm=max_norm, vol_weight=vol_weight, near_weight=near_weight, kl_weight=KL_WEIGHT)
        c = counts.to(torch.float64)
        m = torch.stack([(c[:, 0] / labels.shape[1]).mean(), (c[:, 1] / (c[:, 2] + 1e-5)).mean()])      # accuracy, iou (:96-101)
        metrics = m if metrics is None else metrics + m
        values = losses.tolist()                                   # the iteration's one host read
        if not math.isfinite(values[0]):
            raise FloatingPointError(f"Loss is {values[0]}, stopping training")
        sums = [s + v for s, v in zip(sums, values)]
        n_iter += 1
    if n_iter == 0:
        return {}
    acc, iou = (metrics / n_iter).tolist()
    return dict(loss=sums[0] / n_iter, loss_vol=sums[1] / n_iter, loss_near=sums[2] / n_iter, loss_kl=sums[3] / n_iter, iou=iou, accuracy=acc)


@torch.no_grad()
def evaluate_losses(model, surface: torch.Tensor, points: torch.Tensor, labels: torch.Tensor) -> Dict[str, float]:
    """engine_ae.evaluate's loss and metrics for one batch (:200-223): ``model(surface, points)`` on the inference path (call
    ``model.eval()`` first, as :165 does), BCE-with-logits over all of [B, Q], accuracy, and the evaluation IoU
    ``intersection / union + 1e-5`` (:222; the training loop's is ``intersection / (union + 1e-5)``)."""
    out = model(surface, points)
    logits, kl = out["logits"], out["kl"]
    Q = logits.shape[1]
    # one span that covers every query: entry 1 is BCEWithLogitsLoss over all of [B, Q] (the empty 'near' span makes the total NaN: unused)
    losses, counts, _, _ = TO.ae_loss(logits, labels.to(device=logits.device, dtype=torch.float32), kl, Q, 1.0, 0.0, 0.0, want_grad=False)
    c = counts.to(torch.float64)
    values = losses.tolist()
    return dict(loss=values[1], loss_kl=values[3], iou=float((c[:, 1] / c[:, 2] + 1e-5).mean()), accuracy=float((c[:, 0] / Q).mean()))
