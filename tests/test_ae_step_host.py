"""CPU tests of the native stage-1 step's host logic: the header declares the loss op and ``_lib`` binds it, ``AeStepTrainer`` keeps
``AeTrainer``'s refusals, and ``engine_ae.train_one_epoch`` drives a step object in the reference's pattern (engine_ae.py:55-116)."""
import ctypes as C
import math
from types import SimpleNamespace

import pytest
import torch


def _model(**kw):
    from rald_amd import models_ae as A
    args = dict(depth=1, dim=512, queries_dim=512, output_dim=1, num_inputs=64, num_latents=512, latent_dim=32, heads=8, dim_head=64,
                query_type="mix")
    args.update(kw)
    return A.KLAutoEncoder(**args)


def test_header_declares_the_loss_op_and_lib_binds_it():
    from rald_amd import _lib
    with open(_lib.HEADER, encoding="utf-8") as fh:
        text = fh.read()
    assert "int64_t rald_op_ae_loss_scratch_bytes(int32_t batch, int64_t n_queries);" in text
    assert "int rald_op_ae_loss(const float* logits, const float* labels, const float* kl, const int32_t* in_voxel_num_dev," in text
    res, args = _lib.SIGNATURES["rald_op_ae_loss_scratch_bytes"]
    assert res is C.c_int64 and args == [C.c_int32, C.c_int64]
    res, args = _lib.SIGNATURES["rald_op_ae_loss"]
    p, f = C.c_void_p, C.c_float
    assert res is C.c_int32 and args == [p, p, p, p, C.c_int32, C.c_int64, f, f, f, f, p, p, p, p, p, C.c_int64, p]
    L = _lib.lib()
    assert L.rald_op_ae_loss.argtypes == args and L.rald_op_ae_loss_scratch_bytes.restype is C.c_int64
    # host arithmetic: one 32-byte partial (two double sums, three counts) per workgroup of 1 024 queries of one sample
    assert L.rald_op_ae_loss_scratch_bytes(0, 100) == 0 and L.rald_op_ae_loss_scratch_bytes(2, 0) == 0
    assert L.rald_op_ae_loss_scratch_bytes(1, 1) == 32
    assert L.rald_op_ae_loss_scratch_bytes(2, 1024) == 2 * 32
    assert L.rald_op_ae_loss_scratch_bytes(2, 1025) == 2 * 2 * 32
    assert L.rald_op_ae_loss_scratch_bytes(4, 10000) == 4 * 10 * 32


def test_step_trainer_refuses_cpu_parameters():
    from rald_amd.train_ae import AeStepTrainer
    with pytest.raises(RuntimeError):
        AeStepTrainer(_model(), opt=None)


def test_step_trainer_keeps_the_point_refusal():
    from rald_amd.train_ae import AeStepTrainer
    m = _model()
    m.query_type = "point"                                         # KLAutoEncoder itself refuses to build one
    with pytest.raises(NotImplementedError):
        AeStepTrainer(m, opt=None)


def test_ae_loss_refuses_cpu_tensors():
    from rald_amd import train_ops as TO
    with pytest.raises(RuntimeError):
        TO.ae_loss(torch.zeros(2, 8), torch.zeros(2, 8), torch.zeros(2), 4)


class _StubStep:
    """Stands in for AeStepTrainer / GraphedAeStep: records every call, returns finite losses and plausible counts."""

    def __init__(self, nan_at=None):
        self.calls, self.nan_at = [], nan_at

    def __call__(self, surface, points, labels, in_voxel_num, **kw):
        self.calls.append(dict(surface=surface, points=points, labels=labels, in_voxel_num=in_voxel_num, **kw))
        i = len(self.calls)
        total = float("nan") if self.nan_at == i else 1.0 / i
        B, Q = labels.shape
        counts = torch.tensor([[Q // 2, Q // 4, Q // 2]] * B, dtype=torch.int32)
        return torch.tensor([total, 0.5, 0.25, 2.0], dtype=torch.float64), counts, None


def _loader(n_batches, B=2, Q=8):
    return [dict(query_points=torch.zeros(B, Q, 3) + i, query_labels=torch.ones(B, Q, dtype=torch.int64), lidar_points=torch.zeros(B, 5, 3) - i,
                 in_voxel_num=torch.tensor([3 + i, 99])) for i in range(n_batches)]


def _args(accum_iter, **kw):
    return SimpleNamespace(train=SimpleNamespace(accum_iter=accum_iter, vol_weight=2.0, near_weight=0.25, **kw))


@pytest.mark.parametrize("accum_iter", [1, 3])
def test_train_one_epoch_drives_the_step_in_the_reference_pattern(accum_iter):
    from rald_amd import engine_ae
    step, lr_calls = _StubStep(), []
    data = _loader(7)
    stats = engine_ae.train_one_epoch(step, data, _args(accum_iter, clip_grad=10.0), lr_fn=lr_calls.append)
    assert len(step.calls) == 7
    # update_grad = (data_iter_step + 1) % accum_iter == 0 (:110); the lr is adjusted where a window starts (:58)
    assert [c["update"] for c in step.calls] == [(i + 1) % accum_iter == 0 for i in range(7)]
    assert lr_calls == [i for i in range(7) if i % accum_iter == 0]
    for i, c in enumerate(step.calls):
        assert int(c["in_voxel_num"]) == 3 + i                     # in_voxel_num[0] (:63)
        assert (c["vol_weight"], c["near_weight"], c["kl_weight"]) == (2.0, 0.25, 1e-3)
        assert c["accum_iter"] == accum_iter and c["max_norm"] == 10.0
        assert c["surface"] is data[i]["lidar_points"] and c["points"] is data[i]["query_points"]
        assert c["labels"].dtype == torch.float32 and torch.equal(c["labels"], data[i]["query_labels"].float())
    assert math.isclose(stats["loss"], sum(1.0 / i for i in range(1, 8)) / 7)
    assert (stats["loss_vol"], stats["loss_near"], stats["loss_kl"]) == (0.5, 0.25, 2.0)
    assert math.isclose(stats["accuracy"], 0.5) and math.isclose(stats["iou"], 2 / (4 + 1e-5))


def test_train_one_epoch_uses_a_step_method_and_stops_on_a_non_finite_loss():
    from rald_amd import engine_ae
    inner = _StubStep(nan_at=3)
    holder = SimpleNamespace(step=inner)                           # AeStepTrainer's surface: .step(...)
    with pytest.raises(FloatingPointError):
        engine_ae.train_one_epoch(holder, _loader(5), _args(1))
    assert len(inner.calls) == 3
    assert inner.calls[0]["max_norm"] is None                      # no clip_grad in the config: the norm is taken, nothing is clipped
