"""First-return scans, host side (no GPU): the beam grid, the argument rules of beam_segments / scan_point_clouds (ValueError before the
library or the autoencoder is touched) and the two C entries in the header-derived binding table."""
import ctypes as C
import types

import pytest
import torch


def _ns(**kw):
    return types.SimpleNamespace(**kw)


def _args(view_cone=True, aniso=True):
    return _ns(eval=_ns(inference=_ns(num_query_points=100), skip_eval_metric=False),
               dataset=_ns(lidar=_ns(pc_range=[0, -90, -20, 15.8, 90, 20], pc_range_cart=[0, -15.8, -5.4, 15.8, 15.8, 5.4],
                                     voxel_size=[0.05, 0.25, 0.5], norm_anisotropy=aniso, norm_isotropy=False, view_cone_mode=view_cone)))


def test_beam_grid_values_and_order():
    from rald_amd.query_points import beam_grid
    az, el = beam_grid(-90.0, 90.0, 5, -20.0, 20.0, 3)
    assert az.shape == el.shape == (15,) and az.dtype == el.dtype == torch.float64
    # elevation-major: beam i has elevation i // n_az and azimuth i % n_az; both ends included
    assert az.tolist() == [-90.0, -45.0, 0.0, 45.0, 90.0] * 3
    assert el.tolist() == [-20.0] * 5 + [0.0] * 5 + [20.0] * 5
    az, el = beam_grid(-30.0, 30.0, 4, 5.0, 9.0, 1)             # one elevation: the minimum
    assert az.tolist() == [-30.0, -10.0, 10.0, 30.0] and el.tolist() == [5.0] * 4
    az, el = beam_grid(7.0, 9.0, 1, -2.0, 2.0, 2)
    assert az.tolist() == [7.0, 7.0] and el.tolist() == [-2.0, 2.0]
    for bad in ((0, 3), (3, 0), (-1, 2)):
        with pytest.raises(ValueError):
            beam_grid(-90.0, 90.0, bad[0], -20.0, 20.0, bad[1])


def test_header_declares_the_ray_entries():
    from rald_amd import _lib
    p, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    res, args = _lib.SIGNATURES["rald_ae_cast_rays"]
    assert res is i32 and args == [p] * 4 + [i64, i32, i64, i32, i32] + [p] * 5
    res, args = _lib.SIGNATURES["rald_op_ae_cast_rays"]
    assert res is i32 and args == [p] * 6 + [f32, p, p, i64, i32, i32] + [p] * 4 + [i32, i64, i32, i32, p, i64, p]


def test_entry_points_exist():
    from rald_amd import engine_generation as E, models_ae, query_points as QP
    from rald_amd._handles import AeHandle, op_ae_cast_rays
    assert callable(E.scan_point_clouds) and callable(QP.beam_grid) and callable(QP.beam_segments)
    assert callable(AeHandle.cast_rays) and callable(models_ae.KLAutoEncoder.cast_rays) and callable(op_ae_cast_rays)


def test_argument_errors_raise_before_the_library_is_touched(monkeypatch):
    from rald_amd import _lib, engine_generation as E, query_points as QP

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
    az, el = QP.beam_grid(-90.0, 90.0, 4, -20.0, 20.0, 2)
    z = torch.zeros(2, 128, 32)
    # beam_segments: not view-cone, no normalisation, mismatched / empty / matrix-shaped beam tables, an empty range interval
    for args, a, e, kw in ((_args(view_cone=False), az, el, {}), (_args(aniso=False), az, el, {}), (_args(), az, el[:-1], {}),
                           (_args(), az[:0], el[:0], {}), (_args(), az.view(2, 4), el.view(2, 4), {}), (_args(), az, el, dict(r_min=5.0, r_max=5.0))):
        with pytest.raises(ValueError):
            QP.beam_segments(args, a, e, **kw)
    # scan_point_clouds: the same beam rules, the step counts, the batch rules of the inference tail
    bad = [dict(args=_args(view_cone=False)), dict(el_deg=el[:-1]), dict(n_steps=0), dict(n_steps=65536), dict(n_steps=2.5), dict(n_refine=-1),
           dict(n_refine=31), dict(surfaces=torch.zeros(3, 10, 3)), dict(surfaces=torch.zeros(2, 10, 2)), dict(sampled_tokens=torch.zeros(128, 32))]
    for kw in bad:
        full = dict(sampled_tokens=z, args=_args(), az_deg=az, el_deg=el)
        full.update(kw)
        with pytest.raises(ValueError):
            E.scan_point_clouds(Vae(), **full)
    # the module's cast_rays checks its counts and tables before it asks for a context
    from rald_amd._handles import AeHandle, _ray_counts
    assert _ray_counts(1, 0) == (1, 0) and _ray_counts(65535, 30) == (65535, 30)
    for n_steps, n_refine in ((0, 0), (65536, 0), (8, -1), (8, 31)):
        with pytest.raises(ValueError):
            AeHandle.cast_rays(Vae(), None, 2, None, None, n_steps, n_refine)
