"""Point-cloud metrics, host side (no GPU): the new C entries are declared in the header and bound from it, argument errors raise
before the library is touched, the derivation from the kernels' raw reductions to every metric, and the engine's metric_thresholds
option - absent, the batched tail makes the calls it made before."""
import ctypes as C
import math
import types

import pytest
import torch

INF = float("inf")


def _ns(**kw):
    return types.SimpleNamespace(**kw)


def test_header_declares_the_cloud_metric_entries():
    from rald_amd import _lib
    P, I32, I64 = C.c_void_p, C.c_int32, C.c_int64
    S = _lib.SIGNATURES
    assert S["rald_post_cloud_metrics_scratch_bytes"] == (I64, [I32, I64, I64])
    assert S["rald_post_nn_ragged"] == (I32, [P] * 4 + [I32, I64, I64] + [P] * 4)
    assert S["rald_post_cloud_metrics_ragged"] == (I32, [P] * 4 + [I32, I64, I64, P, I32] + [P] * 7)
    assert S["rald_op_nn_scratch_bytes"] == (I64, [I32, I64, I64, I64])
    assert S["rald_op_nn_ragged"] == (I32, [P] * 4 + [I32, I64, I64, I64] + [P] * 3 + [I64, P])


def test_scratch_queries_are_host_side_and_refuse_bad_arguments():
    from rald_amd._lib import lib
    L = lib()
    off8 = (C.c_int64 * 2)(0, 0)
    # 480 000 x 10 000 points: the workspace holds (d^2, index) per row and chunk, so at least 16 bytes per predicted point
    assert L.rald_post_cloud_metrics_scratch_bytes(1, 480000, 10000) >= 16 * 480000
    assert L.rald_post_cloud_metrics_scratch_bytes(64, 480000, 10000) >= 64 * 16 * 480000
    assert L.rald_post_cloud_metrics_scratch_bytes(3, 0, 0) > 0
    assert L.rald_post_cloud_metrics_scratch_bytes(0, 10, 10) == -1 and L.rald_post_cloud_metrics_scratch_bytes(1, -1, 10) == -1
    # a workspace that 64 bits could not size is refused, not wrapped around
    big = (1 << 38) - 1
    assert L.rald_post_cloud_metrics_scratch_bytes(65535, big, big) == -1 and L.rald_op_nn_scratch_bytes(65535, big, big, 1024) == -1
    assert L.rald_post_cloud_metrics_ragged(None, off8, None, off8, 65535, big, big, None, 0, off8, None, None, None, None, off8, None) != 0
    assert b"too large" in L.rald_last_error()
    # an explicit chunk length: a multiple of the 1024-point tile; 2500 candidates in chunks of 1024 are 3 chunks
    one, three = L.rald_op_nn_scratch_bytes(2, 1000, 2500, 3072), L.rald_op_nn_scratch_bytes(2, 1000, 2500, 1024)
    assert three - one == 2 * 2 * 1000 * 16
    assert L.rald_op_nn_scratch_bytes(2, 1000, 2500, 1000) == -1 and L.rald_op_nn_scratch_bytes(2, 1000, 2500, -1024) == -1
    # the automatic chunk length is a function of the arguments alone
    assert L.rald_op_nn_scratch_bytes(2, 1000, 2500, 0) == L.rald_op_nn_scratch_bytes(2, 1000, 2500, 0)
    # bad arguments are reported, not crashed, before any launch
    assert L.rald_post_cloud_metrics_ragged(None, None, None, None, 1, 10, 10, None, 0, None, None, None, None, None, None, None) != 0
    tau = (C.c_double * 9)(*([0.1] * 9))
    off = (C.c_int64 * 2)(0, 0)
    raw = (C.c_double * 64)()
    for k, bad in ((9, 0.1), (1, -0.5), (1, INF), (1, float("nan"))):
        tau[0] = bad
        assert L.rald_post_cloud_metrics_ragged(None, off, None, off, 1, 0, 0, tau, k, raw, None, None, None, None, raw, None) != 0
        assert b"threshold" in L.rald_last_error()


def _no_library(monkeypatch):
    from rald_amd import _lib

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_library)
    for mod in ("engine_generation", "postprocess", "query_points", "_handles"):
        m = __import__("rald_amd." + mod, fromlist=["x"])
        if hasattr(m, "lib"):
            monkeypatch.setattr(m, "lib", no_library)


def test_argument_errors_raise_before_the_library_is_touched(monkeypatch):
    from rald_amd import engine_generation as E, postprocess as PP
    _no_library(monkeypatch)
    pts, off = torch.zeros(10, 3), torch.tensor([0, 4, 10])
    ok = dict(y_pred=pts, pred_offsets=off, y_gt=pts, gt_offsets=off, max_pred=6, max_gt=6)
    bad = [dict(y_pred=torch.zeros(10, 2)), dict(y_gt=torch.zeros(30)), dict(y_pred=torch.zeros(2, 5, 3)),      # wrong shapes
           dict(gt_offsets=torch.tensor([0, 4, 7, 10])),                                                        # batches of 2 and 3 frames
           dict(pred_offsets=torch.tensor([0.0, 4.0, 10.0])), dict(pred_offsets=torch.tensor([10])), dict(gt_offsets=[0, 4, 10]),
           dict(thresholds=[0.1] * 9),                                                                          # K > 8
           dict(thresholds=(0.1, -0.1)), dict(thresholds=(INF,)), dict(thresholds=(float("nan"),)),
           dict(max_pred=-1), dict(max_gt=2.5)]
    for kw in bad:
        with pytest.raises(ValueError):
            PP.cloud_metrics_ragged(**{**ok, **kw})
    for a, ao, b, bo in ((torch.zeros(10, 4), off, pts, off), (pts, off, torch.zeros(10), off), (pts, off, pts, torch.tensor([0, 10]))):
        with pytest.raises(ValueError):
            PP.nearest_neighbors_ragged(a, ao, b, bo, 6, 6)
    for a, b in ((torch.zeros(10, 2), pts), (pts, torch.zeros(3, 3, 3))):
        with pytest.raises(ValueError):
            PP.nearest_neighbors(a, b)
        with pytest.raises(ValueError):
            PP.cloud_metrics(a, b)
    for taus in ([0.1] * 9, (-1.0,), (INF,)):
        with pytest.raises(ValueError):
            PP.cloud_metrics(pts, pts, taus)

    class Vae:
        def __getattr__(self, name):
            raise AssertionError("the autoencoder was touched")
    for fn in (E.infer_point_clouds, E.infer_point_clouds_device):
        for taus in ([0.1] * 9, (0.1, -2.0), (float("nan"),)):
            with pytest.raises(ValueError):
                fn(Vae(), torch.zeros(2, 128, 32), None, metric_thresholds=taus)


def test_metrics_derive_from_the_raw_reductions():
    """raw [B,2,3+K] = (sum d, sum d^2, max d, counts) per direction -> every key, worked out by hand; the empty-side conventions and
    P + R = 0."""
    from rald_amd.postprocess import METRIC_KEYS, _derive_cloud_metrics, _metrics_to_host
    raw = torch.tensor([[[10.0, 30.0, 4.0, 2.0, 5.0], [6.0, 12.0, 3.0, 0.0, 3.0]],        # 5 predicted, 3 true points
                        [[8.0, 40.0, 7.0, 0.0, 1.0], [9.0, 27.0, 6.5, 0.0, 1.0]],         # 4 and 2 points; nothing below the first threshold
                        [[0.0, 0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0, 0.0]],           # an empty prediction
                        [[0.0, 0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0, 0.0]]],          # an empty ground truth
                       dtype=torch.float64)
    n_pred = torch.tensor([5.0, 4.0, 0.0, 7.0], dtype=torch.float64)
    n_gt = torch.tensor([3.0, 2.0, 7.0, 0.0], dtype=torch.float64)
    m = _derive_cloud_metrics(raw, n_pred, n_gt)
    assert set(m) == set(METRIC_KEYS) and all(v.dtype == torch.float64 for v in m.values())
    assert m["accuracy"].tolist() == [2.0, 2.0, INF, INF] and m["completeness"].tolist() == [2.0, 4.5, INF, INF]
    assert m["cd"].tolist() == [2.0, 3.25, INF, INF]                         # 0.5 accuracy + 0.5 completeness
    assert m["cd_l2"].tolist() == [6.0 + 4.0, 10.0 + 13.5, INF, INF]         # mean d^2 over pred + mean d^2 over gt
    assert m["hausdorff"].tolist() == [4.0, 7.0, INF, INF] and m["mhd"].tolist() == [2.0, 4.5, INF, INF]
    assert m["precision"].tolist() == [[0.4, 1.0], [0.0, 0.25], [0.0, 0.0], [0.0, 0.0]]
    assert m["recall"].tolist() == [[0.0, 1.0], [0.0, 0.5], [0.0, 0.0], [0.0, 0.0]]
    f = m["f_score"].tolist()
    assert f[0] == [0.0, 1.0] and f[1][0] == 0.0 and math.isclose(f[1][1], 2 * 0.25 * 0.5 / 0.75, rel_tol=1e-15) and f[2:] == [[0.0, 0.0]] * 2
    assert not any(torch.isnan(v).any() for v in m.values())
    # the flat host layout infer_point_clouds reads back: one dict per frame
    flat = torch.cat([m[k].reshape(-1) for k in METRIC_KEYS]).tolist()
    frames = _metrics_to_host(flat, 4, 2)
    assert frames[1] == {"accuracy": 2.0, "completeness": 4.5, "cd": 3.25, "cd_l2": 23.5, "hausdorff": 7.0, "mhd": 4.5,
                         "precision": [0.0, 0.25], "recall": [0.0, 0.5], "f_score": f[1]}
    assert frames[2]["cd"] == INF and frames[3]["f_score"] == [0.0, 0.0]
    # no thresholds: the three ratio keys are empty
    m0 = _derive_cloud_metrics(raw[:, :, :3].contiguous(), n_pred, n_gt)
    assert m0["f_score"].shape == (4, 0) and m0["cd"].tolist() == m["cd"].tolist()
    assert _metrics_to_host(torch.cat([m0[k].reshape(-1) for k in METRIC_KEYS]).tolist(), 4, 0)[0]["precision"] == []


def _stub_tail(monkeypatch):
    """The batched tail with every device function replaced by a recorder that returns CPU tensors of the right shapes (B = 2 frames,
    100 grid queries, 50 refine queries); tensors pass for device tensors.  -> (call names, number of host reads, the arguments)."""
    from rald_amd import engine_generation as E
    calls, reads = [], []
    B, n, aug = 2, 100, 50
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True), raising=False)
    real_cpu = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (reads.append(1), real_cpu(self, *a, **k))[1])

    def rec(name, result):
        def f(*a, **k):
            calls.append(name)
            return result(*a, **k) if callable(result) else result
        return f
    off_q = torch.tensor([0, n, 2 * n])
    off_p = torch.tensor([0, 7, 12])
    off_r = torch.tensor([0, aug, 2 * aug])
    fake_pp = _ns(occupied_points_ragged=rec("occupied_points_ragged", (torch.zeros(2 * n, 3), off_p, None)),
                  polar2cartesian=rec("polar2cartesian", lambda p: p), inverse_norm_points=rec("inverse_norm_points", lambda p, *a: p),
                  cal_metrics_ragged=rec("cal_metrics_ragged", torch.tensor([1.5, 2.5], dtype=torch.float64)),
                  cloud_metrics_ragged=rec("cloud_metrics_ragged", lambda *a: _fake_metrics(a[-1])),
                  _thresholds=E.PP._thresholds, _metrics_to_host=E.PP._metrics_to_host, METRIC_KEYS=E.PP.METRIC_KEYS)
    fake_qp = _ns(uniform_queries_from=rec("uniform_queries_from", torch.zeros(n, 3)),
                  refine_queries_ragged=rec("refine_queries_ragged", (torch.zeros(2 * aug, 3), off_r)))
    monkeypatch.setattr(E, "PP", fake_pp)
    monkeypatch.setattr(E, "QP", fake_qp)
    vae = _ns(decode_ragged=rec("decode_ragged", lambda x, q, o, longest: torch.zeros(q.shape[0])))
    args = _ns(eval=_ns(inference=_ns(num_query_points=n, refine_query=True, refine_query_aug_num=aug, refine_query_scale=10, query_helper=True),
                        use_cart_query=False, skip_eval_metric=False),
               dataset=_ns(lidar=_ns(pc_range=[0, -90, -20, 15.8, 90, 20], voxel_size=[0.05, 0.25, 0.5], norm_anisotropy=True,
                                     norm_isotropy=False, view_cone_mode=True)))
    kw = dict(helper_points=None, surfaces=torch.zeros(B, 20, 3), draws={"u3n": torch.zeros(3, n, dtype=torch.float64)})
    return calls, reads, (vae, torch.zeros(B, 128, 32), args), kw, off_q


def _fake_metrics(taus):
    K = len(taus)
    one = torch.tensor([1.5, 2.5], dtype=torch.float64)
    m = {k: one + i for i, k in enumerate(("accuracy", "completeness", "cd", "cd_l2", "hausdorff", "mhd"))}
    for i, k in enumerate(("precision", "recall", "f_score")):
        m[k] = torch.arange(2 * K, dtype=torch.float64).reshape(2, K) / 10 + i
    return m


TAIL = ["uniform_queries_from", "decode_ragged", "occupied_points_ragged", "refine_queries_ragged", "decode_ragged", "occupied_points_ragged",
        "polar2cartesian", "inverse_norm_points", "polar2cartesian"]


def test_without_metric_thresholds_the_tail_makes_the_calls_it_made_before(monkeypatch):
    from rald_amd import engine_generation as E
    calls, reads, pos, kw, _ = _stub_tail(monkeypatch)
    out = E.infer_point_clouds(*pos, **kw)
    assert calls == TAIL + ["cal_metrics_ragged"] and len(reads) == 1
    assert set(out) == {"pred", "cd", "n_queries"} and out["cd"] == [1.5, 2.5] and out["n_queries"] == [150, 150]
    assert [p.shape[0] for p in out["pred"]] == [7, 5]
    del calls[:]
    assert len(E.infer_point_clouds_device(*pos, **kw)) == 3 and calls == TAIL + ["cal_metrics_ragged"] and len(reads) == 1


def test_with_metric_thresholds_the_metrics_join_the_one_host_read(monkeypatch):
    from rald_amd import engine_generation as E
    calls, reads, pos, kw, _ = _stub_tail(monkeypatch)
    out = E.infer_point_clouds(*pos, metric_thresholds=(0.05, 0.1, 0.2), **kw)
    assert calls == TAIL + ["cloud_metrics_ragged"] and len(reads) == 1
    assert out["cd"] == [3.5, 4.5] and out["n_queries"] == [150, 150] and [p.shape[0] for p in out["pred"]] == [7, 5]
    assert out["metrics"][0] == {"accuracy": 1.5, "completeness": 2.5, "cd": 3.5, "cd_l2": 4.5, "hausdorff": 5.5, "mhd": 6.5,
                                 "precision": [0.0, 0.1, 0.2], "recall": [1.0, 1.1, 1.2], "f_score": [2.0, 2.1, 2.2]}
    assert out["metrics"][1]["accuracy"] == 2.5 and out["metrics"][1]["recall"] == [1.3, 1.4, 1.5]
    del calls[:]
    pts, off, cd, metrics = E.infer_point_clouds_device(*pos, metric_thresholds=(), **kw)
    assert calls == TAIL + ["cloud_metrics_ragged"] and len(reads) == 1 and cd is metrics["cd"] and metrics["precision"].shape == (2, 0)
    # no surfaces: no metric of either kind
    kw["surfaces"] = None
    out = E.infer_point_clouds(*pos, metric_thresholds=(0.1,), **kw)
    assert out["cd"] is None and out["metrics"] is None
