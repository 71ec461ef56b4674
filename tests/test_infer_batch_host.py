"""Batched inference tail, host side (no GPU): the four ragged C entries are declared in the header and bound from it, the batched
entry points exist, and their shape / length rules raise before the library is touched."""
import ctypes as C
import types

import pytest
import torch

RAGGED = ("rald_ae_decode_queries_ragged", "rald_post_occupied_points_ragged", "rald_query_refine_ragged", "rald_post_chamfer_sums_ragged")


def _ns(**kw):
    return types.SimpleNamespace(**kw)


def _args():
    return _ns(eval=_ns(inference=_ns(num_query_points=100, refine_query=True, refine_query_aug_num=50, refine_query_scale=10, query_helper=True)),
               dataset=_ns(lidar=_ns(pc_range=[0, -90, -20, 15.8, 90, 20], pc_range_cart=[0, -15.8, -5.4, 15.8, 15.8, 5.4],
                                     voxel_size=[0.05, 0.25, 0.5], norm_anisotropy=True, norm_isotropy=False, view_cone_mode=True)))


def test_header_declares_the_four_ragged_entries():
    from rald_amd import _lib
    for name in RAGGED:
        assert name in _lib.SIGNATURES, name
        res, argtypes = _lib.SIGNATURES[name]
        assert res is C.c_int32
    # offsets are pointers (device arrays), the grid-sizing bounds 64-bit host scalars
    dec = _lib.SIGNATURES["rald_ae_decode_queries_ragged"][1]
    assert dec == [C.c_void_p] * 4 + [C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]
    cham = _lib.SIGNATURES["rald_post_chamfer_sums_ragged"][1]
    assert cham == [C.c_void_p] * 4 + [C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
    comp = _lib.SIGNATURES["rald_post_occupied_points_ragged"][1]
    assert comp == [C.c_void_p] * 3 + [C.c_int32, C.c_int64, C.c_void_p] + [C.c_int32] * 3 + [C.c_float] + [C.c_void_p] * 5
    ref = _lib.SIGNATURES["rald_query_refine_ragged"][1]
    assert ref == [C.c_void_p] * 2 + [C.c_int32, C.c_int64] + [C.c_void_p] * 6 + [C.c_int32] * 3 + [C.c_void_p] * 3


def test_batched_entry_points_exist():
    from rald_amd import engine_generation as E, models_ae, postprocess as PP, query_points as QP
    from rald_amd._handles import AeHandle
    assert callable(E.infer_point_clouds) and callable(E.infer_point_clouds_device)
    assert callable(AeHandle.decode_queries_ragged) and callable(models_ae.KLAutoEncoder.decode_ragged)
    assert callable(PP.occupied_points_ragged) and callable(PP.cal_metrics_ragged)
    assert callable(QP.refine_queries_ragged) and callable(QP.draw_tail_randoms)


def test_offsets_from_lengths():
    from rald_amd.engine_generation import offsets_from_lengths
    assert offsets_from_lengths([]) == [0]
    assert offsets_from_lengths([3]) == [0, 3]
    assert offsets_from_lengths([0, 0]) == [0, 0, 0]
    assert offsets_from_lengths([130, 0, 1, 63, 0]) == [0, 130, 130, 131, 194, 194]
    assert offsets_from_lengths([2 ** 31, 2 ** 31]) == [0, 2 ** 31, 2 ** 32]          # Python ints: no 32-bit wrap
    with pytest.raises(ValueError):
        offsets_from_lengths([3, -1])


def test_shape_and_length_errors_raise_before_the_library_is_touched(monkeypatch):
    from rald_amd import _lib, engine_generation as E

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_library)
    for mod in ("engine_generation", "postprocess", "query_points", "_handles"):
        m = __import__("rald_amd." + mod, fromlist=["x"])
        if hasattr(m, "lib"):
            monkeypatch.setattr(m, "lib", no_library)

    class Vae:                                                  # any use of the autoencoder is a failure too
        def __getattr__(self, name):
            raise AssertionError("the autoencoder was touched")
    z = torch.zeros(3, 128, 32)
    ok_helpers = [torch.zeros(4, 3), torch.zeros(0, 3), torch.zeros(1, 3)]
    bad = [dict(helper_points=ok_helpers[:2]),                                       # len(helper_points) != B
           dict(helper_points=ok_helpers + [torch.zeros(2, 3)]),
           dict(helper_points=torch.zeros(3, 4, 3)),                                 # a tensor, not a list of B tensors
           dict(helper_points=[torch.zeros(4, 3), torch.zeros(4, 2), torch.zeros(1, 3)]),      # wrong trailing dim
           dict(helper_points=[torch.zeros(4, 3), torch.zeros(12), torch.zeros(1, 3)]),
           dict(surfaces=torch.zeros(2, 10, 3)),                                     # surfaces batch mismatch
           dict(surfaces=torch.zeros(3, 10, 2)),
           dict(surfaces=torch.zeros(30, 3))]
    for fn in (E.infer_point_clouds, E.infer_point_clouds_device):
        for kw in bad:
            with pytest.raises(ValueError):
                fn(Vae(), z, _args(), **kw)
        with pytest.raises(ValueError):
            fn(Vae(), torch.zeros(128, 32), _args())                                  # latents without a batch dimension


def test_single_frame_entry_point_still_refuses_a_batch():
    from rald_amd import engine_generation as E
    with pytest.raises(AssertionError):
        E.infer_point_cloud(None, torch.zeros(2, 128, 32), _args())
