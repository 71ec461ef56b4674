"""Radius outlier removal, host side (no GPU): the brute-force reference of tests/radius_ref.py against an independent grid walk with
the header's search-range rule on the six constructions the GPU tests use (and that a scan of c-1 .. c+1 is NOT enough on them); the
reference on planted cases; the C entries' declarations, scratch sizes and every refusal (through the built library, before any GPU
work); the Python layer's argument errors; and, with the device functions stubbed, that infer_point_clouds does what it did before
when `denoise` is left alone, and what it should with it."""
import ctypes as C

import numpy as np
import pytest
import torch

import radius_ref as REF

F32 = np.float32


# ---- the reference -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(REF.CONSTRUCTIONS))
def test_reference_agrees_with_the_grid_walk(name):
    p, grid, radius = REF.CONSTRUCTIONS[name]()
    assert 1400 <= len(p) <= 1600
    a = REF.radius_one(p, grid, radius)
    b, widest = REF.grid_walk_one(p, grid, radius)
    assert a["inside"].all() and (a["count"] > 0).any()
    for k in ("count", "nn_idx", "nn_dist2"):
        assert np.array_equal(a[k], b[k]), k
    assert widest <= 4
    if name in ("lattice", "lattice_ulp", "faces"):
        assert widest == 4                                                    # with v = radius the rule does reach four cells


def test_a_scan_of_one_cell_each_side_is_too_narrow():
    """What the constructions are for: on the radius-spaced lattice some row within r2 lies two cells from the row that counts it."""
    p, (lo3, v3, dims3), radius = REF.lattice_ulp_cloud()
    a = REF.radius_one(p, (lo3, v3, dims3), radius)
    cell = np.stack([REF.cell_f(p[:, k], lo3[k], v3[k]) for k in range(3)], axis=1)
    r2 = F32(F32(radius) * F32(radius))
    far = 0
    for i in range(len(p)):
        d2 = REF.d2_rows(p, np.array([i]))[0]
        hit = np.nonzero((d2 <= r2) & (np.arange(len(p)) != i))[0]
        far += int((np.abs(cell[hit] - cell[i]).max(axis=1) >= 2).sum()) if len(hit) else 0
    assert far > 0 and a["count"].sum() > far


def test_reference_on_planted_cases():
    grid = REF.cube_grid(0.0, 1.0, 0.125)
    r = 0.125
    up = np.nextafter(F32(0.25), F32(1))
    p = np.array([[0.25, 0.25, 0.25], [0.375, 0.25, 0.25], [0.25, 0.25, 0.25], [0.375, 0.375, 0.25], [up, 0.25, 0.25], [0.125, 0.25, 0.25],
                  [np.nan, 0.25, 0.25], [0.25, np.inf, 0.25], [2.0, 0.25, 0.25], [-0.01, 0.25, 0.25], [0.9, 0.9, 0.9]], F32)
    a = REF.radius_one(p, grid, r)
    # row 0: its duplicate (2), both face neighbours at exactly r2 (1, 5) and the row one ulp up (4); not the diagonal (3), no outside row
    assert a["count"].tolist() == [4, 4, 4, 1, 3, 2, -1, -1, -1, -1, 0]
    assert a["nn_idx"].tolist() == [2, 4, 0, 1, 0, 0, -1, -1, -1, -1, -1]
    assert a["nn_dist2"][0] == 0 and a["nn_dist2"][1] == F32(F32(0.375) - up) ** 2 and np.isposinf(a["nn_dist2"][[6, 10]]).all()
    assert a["nn_dist2"][3] == F32(0.015625) and a["nn_idx"][5] == 0                  # equal d2 to rows 0 and 2: the smaller index
    assert REF.radius_one(p, grid, r, max_count=3)["count"].tolist() == [3, 3, 3, 1, 3, 2, -1, -1, -1, -1, 0]
    f = REF.filter_ragged(p, [0, len(p)], grid, r, 3, 100)
    assert f["index"].tolist() == [0, 1, 2, 4] and f["offsets"].tolist() == [0, 4] and np.array_equal(f["points"], p[[0, 1, 2, 4]])
    assert f["count"].tolist() == [3, 3, 3, 1, 3, 2, -1, -1, -1, -1, 0]
    # ragged: counts trims, the bound trims, empty clouds; a cloud equals the same cloud alone
    g = REF.filter_ragged(p, [0, 6, 6, 11], grid, r, 1, 4, counts=[5, 3, 9])
    alone = REF.filter_ragged(p[:4], [0, 4], grid, r, 1, 4)
    assert g["offsets"].tolist() == [0, len(alone["index"]), len(alone["index"]), len(alone["index"])]
    assert np.array_equal(g["index"], alone["index"]) and g["untouched"].tolist() == [False] * 4 + [True] * 2 + [False] * 4 + [True]
    # the grid does not show for rows that every grid holds: other cell edges (their boxes differ, so only the inside rows are compared)
    q = p[[0, 1, 2, 3, 4, 5, 10]]
    a = REF.radius_one(q, grid, r)
    for v in ((0.125, 0.25, 0.1875), (8.0, 0.125, 0.125)):
        b = REF.radius_one(q, REF.cube_grid(0.0, 1.0, v), r)
        assert b["inside"].all() and all(np.array_equal(a[k], b[k]) for k in ("count", "nn_idx", "nn_dist2"))


# ---- the C entries -------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entries():
    from rald_amd import _lib
    P, I32, I64, F = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    head = [P, P, P, I32, I64, I64, I64, P, P, P, F, I32]
    assert _lib.SIGNATURES["rald_post_radius_scratch_bytes"] == (I64, [I32, I64, I64])
    assert _lib.SIGNATURES["rald_op_radius_scratch_bytes"] == (I64, [I32, I64, I64, I64])
    assert _lib.SIGNATURES["rald_post_radius_count_ragged"] == (I32, head + [P, P, P, P, I64, P])
    assert _lib.SIGNATURES["rald_op_radius_count_ragged"] == (I32, head + [P, P, P, P, I64, I64, P])
    assert _lib.SIGNATURES["rald_post_radius_filter_ragged"] == (I32, head + [P, P, P, P, P, I64, P])
    assert _lib.SIGNATURES["rald_op_radius_filter_ragged"] == (I32, head + [P, P, P, P, P, I64, I64, P])


def test_scratch_bytes():
    from rald_amd._lib import lib
    L = lib()
    q, qo, qv = L.rald_post_radius_scratch_bytes, L.rald_op_radius_scratch_bytes, L.rald_post_voxel_scratch_bytes
    assert q(1, 1, 1) > 0 and q(1, 0, 1) > 0
    sizes = [q(1, 1000, 1000), q(1, 5000, 1000), q(1, 5000, 5000), q(3, 5000, 5000), q(3, 480000, 480000), q(64, 1 << 21, 1 << 21),
             q(64, 1 << 25, 1 << 24)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])) and all(s % 16 == 0 for s in sizes)
    assert q(3, 480000, 480000) >= qv(3, 480000, 480000) + 20 * 480000                  # the sort's share, the sorted rows, the counts
    assert qo(2, 70000, 70000, 0) == q(2, 70000, 70000) and qo(2, 70000, 70000, 1024) > qo(2, 70000, 70000, 4096)
    for args in ((0, 10, 10), (65536, 10, 10), (1, -1, 10), (1, 1 << 31, 10), (1, 10, 0), (1, 10, (1 << 24) + 1)):
        assert q(*args) == -1 and b"rald_post_radius_scratch_bytes" in L.rald_last_error(), args
    for chunk in (-1024, 1, 1000, 1025):
        assert qo(1, 10, 10, chunk) == -1 and b"rald_op_radius_scratch_bytes" in L.rald_last_error()


def test_every_refusal_comes_before_any_gpu_work():
    """Host buffers stand in for device memory: a refused call touches none of them and launches nothing."""
    from rald_amd._lib import lib
    L = lib()
    pts, out, off = (C.c_float * 64)(), (C.c_float * 64)(), (C.c_int64 * 4)()
    cnt, nn_i, nn_d, idx = (C.c_int32 * 16)(), (C.c_int64 * 16)(), (C.c_float * 16)(), (C.c_int64 * 16)()
    need = L.rald_op_radius_scratch_bytes(1, 4, 4, 0)
    scratch = (C.c_char * (need + 64))()
    base = C.addressof(scratch)
    aligned = base + (-base) % 16
    f3, i3 = lambda *v: (C.c_float * 3)(*v), lambda *v: (C.c_int32 * 3)(*v)
    inf, nan = float("inf"), float("nan")
    layout = dict(points=pts, offsets=None, counts=None, batch=1, n_dense=4, n_total=4, max_per_sample=4, lo=f3(0, 0, 0), v=f3(1, 1, 1),
                  dims=i3(4, 4, 4), radius=0.5)
    tail = dict(scratch=aligned, scratch_bytes=need, chunk=0, stream=None)
    count_ok = {**layout, **dict(max_count=0, out_count=cnt, out_nn_idx=None, out_nn_dist2=None), **tail}
    filter_ok = {**layout, **dict(min_neighbors=2, out_points=out, out_offsets=off, out_index=idx, out_count=None), **tail}
    shared = [(dict(points=None), b"null pointer"), (dict(lo=None), b"null grid"), (dict(v=None), b"null grid"), (dict(dims=None), b"null grid"),
              (dict(radius=0.0), b"radius must be finite and > 0"), (dict(radius=-0.5), b"radius must be finite and > 0"),
              (dict(radius=nan), b"radius must be finite and > 0"), (dict(radius=inf), b"radius must be finite and > 0"),
              (dict(v=f3(0.4, 1, 1)), b"cell edge must be >= radius"), (dict(v=f3(1, 0.4, 1)), b"cell edge must be >= radius"),
              (dict(v=f3(1, 1, 0.4999)), b"cell edge must be >= radius"), (dict(v=f3(1, nan, 1)), b"cell edge must be >= radius"),
              (dict(v=f3(1, 1, inf)), b"cell edge must be finite"), (dict(lo=f3(0, nan, 0)), b"lo must be finite"),
              (dict(batch=0), b"batch must be 1 .. 65535"), (dict(batch=65536), b"batch must be 1 .. 65535"),
              (dict(n_dense=-1), b"n_dense must be >= 0"), (dict(n_total=-1), b"n_total must be"), (dict(n_total=1 << 31), b"n_total must be"),
              (dict(max_per_sample=0), b"max_per_sample must be 1 .. 16777216"), (dict(max_per_sample=(1 << 24) + 1), b"max_per_sample must be"),
              (dict(dims=i3(4, 0, 4)), b"every dim must be >= 1"), (dict(dims=i3(1291, 1290, 1290)), b"at most 2^31 - 1 cells"),
              (dict(dims=i3(65536, 32768, 1)), b"at most 2^31 - 1 cells"),
              (dict(scratch_bytes=need - 1), b"scratch too small"), (dict(max_per_sample=1 << 21), b"scratch too small"),
              (dict(scratch=None), b"null or unaligned scratch"), (dict(scratch=aligned + 4), b"null or unaligned scratch"),
              (dict(chunk=1000), b"multiple of 1024"), (dict(chunk=-1024), b"multiple of 1024"), (dict(chunk=1), b"multiple of 1024")]
    count_only = [(dict(out_count=None), b"null pointer"), (dict(max_count=-1), b"max_count must be >= 0"),
                  (dict(max_count=2, out_nn_idx=nn_i), b"needs max_count = 0"), (dict(max_count=1, out_nn_dist2=nn_d), b"needs max_count = 0"),
                  (dict(max_count=3, out_nn_idx=nn_i, out_nn_dist2=nn_d), b"needs max_count = 0")]
    filter_only = [(dict(out_points=None), b"null pointer"), (dict(out_offsets=None), b"null pointer"),
                   (dict(min_neighbors=0), b"min_neighbors must be >= 1"), (dict(min_neighbors=-3), b"min_neighbors must be >= 1")]
    for ok, op, post, who, cases in ((count_ok, L.rald_op_radius_count_ragged, L.rald_post_radius_count_ragged, b"radius_count_ragged",
                                      shared + count_only),
                                     (filter_ok, L.rald_op_radius_filter_ragged, L.rald_post_radius_filter_ragged, b"radius_filter_ragged",
                                      shared + filter_only)):
        for change, message in cases:
            a = {**ok, **change}
            assert op(*a.values()) == 1, change
            assert message in L.rald_last_error() and who in L.rald_last_error(), (change, L.rald_last_error())
            if "chunk" not in change:
                del a["chunk"]
                assert post(*a.values()) == 1, change
                assert message in L.rald_last_error(), (change, L.rald_last_error())
    assert not any(cnt) and not any(out) and not any(off) and not any(idx)


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_raise_before_the_library_is_touched(monkeypatch):
    from rald_amd import engine_generation as E, postprocess as PP
    from test_fps_host import _no_library
    _no_library(monkeypatch)
    pts, off = torch.zeros(10, 3), torch.tensor([0, 4, 10])
    grid = PP.voxel_grid((0, 0, 0), (1, 1, 1), 0.5)
    ok = dict(points=pts, offsets=off, radius=0.5, grid=grid, max_per_sample=6)
    bad = [dict(points=torch.zeros(10, 2)), dict(points=torch.zeros(10, 3, dtype=torch.int64)), dict(offsets=torch.tensor([0.0, 4.0, 10.0])),
           dict(offsets=[0, 4, 10]), dict(max_per_sample=0), dict(max_per_sample=(1 << 24) + 1), dict(max_per_sample=True),
           dict(counts=torch.tensor([4, 6])), dict(counts=torch.tensor([4, 6, 1], dtype=torch.int32)), dict(grid=None),
           dict(grid=(grid[0], (0.5, 0.0, 0.5), grid[2])), dict(grid=(grid[0], grid[1], (1291, 1290, 1290))), dict(chunk=1000),
           dict(radius=0), dict(radius=-1.0), dict(radius=float("nan")), dict(radius=float("inf")), dict(radius="wide"), dict(radius=True),
           dict(radius=1e-60), dict(radius=1e60), dict(radius=0.6), dict(grid=(grid[0], (0.5, 0.25, 0.5), grid[2]))]
    for kw in bad:
        with pytest.raises(ValueError):
            PP.radius_neighbor_count_ragged(**{**ok, **kw})
        with pytest.raises(ValueError):
            PP.remove_radius_outliers_ragged(**{**ok, "min_neighbors": 2, **kw})
    for kw in (dict(max_count=-1), dict(max_count=1.5), dict(max_count=True), dict(max_count=2, return_nearest=True)):
        with pytest.raises(ValueError):
            PP.radius_neighbor_count_ragged(**{**ok, **kw})
    for k in (0, -1, 1.5, True, None):
        with pytest.raises((ValueError, TypeError)):
            PP.remove_radius_outliers_ragged(**{**ok, "min_neighbors": k})
    for points, kw in ((torch.zeros(2, 5, 3), {}), (torch.zeros(5, 2), {}), (torch.zeros(5, 3), dict(radius=0)), (torch.zeros(5, 3), dict(min_neighbors=0)),
                       (torch.zeros(5, 3), dict(lo=(0, 0, 0))), (torch.zeros(5, 3, dtype=torch.int32), {}), (torch.zeros(5, 3), dict(radius=float("nan")))):
        with pytest.raises(ValueError):
            PP.remove_radius_outliers(points, **{"radius": 0.5, "min_neighbors": 1, **kw})
    assert PP.remove_radius_outliers(torch.zeros(0, 3), 0.5, 1).shape == (0, 3)
    # a box too large for cells of edge radius: the cells grow, by powers of two, until the grid fits
    g = PP._radius_grid((0, 0, 0), (1e3, 1e3, 1e3), 0.25)
    assert g[1] == (1.0, 1.0, 1.0) and g[2] == (1001,) * 3 and PP._radius_grid((0, 0, 0), (1, 1, 1), 0.25) == PP.voxel_grid((0, 0, 0), (1, 1, 1), 0.25)

    class Vae:
        def __getattr__(self, name):
            raise AssertionError("the autoencoder was touched")
    ns = lambda **kw: type("NS", (), kw)()
    args = ns(dataset=ns(lidar=ns(pc_range=[0, -90, -20, 15.8, 90, 20], view_cone_mode=True)))
    for fn in (E.infer_point_clouds, E.infer_point_clouds_device):
        for denoise in (0.1, (0.1,), (0.1, 2, 3), (0, 2), (-0.1, 2), (float("nan"), 2), (0.1, 0), (0.1, 1.5), (0.1, True), ("r", 2), (1e-3, 2),
                        "fine"):                                                   # 1e-3: (31.6 / 1e-3)^3 cells
            with pytest.raises(ValueError):
                fn(Vae(), torch.zeros(2, 128, 32), args, denoise=denoise)
    assert E._check_denoise(None, args) is None
    assert E._check_denoise((0.5, 3), args) == (0.5, 3, PP.voxel_grid([-15.8] * 3, [15.8] * 3, 0.5))
    args.dataset.lidar.view_cone_mode = False
    assert E._check_denoise((0.5, 3.0), args) == (0.5, 3, PP.voxel_grid([0, -90, -20], [15.8, 90, 20], 0.5))


# ---- the tail ------------------------------------------------------------------------------------------------------------------------------
def _stub_denoise(monkeypatch):
    from test_voxel_downsample_host import _stub_thin
    E, calls, reads, pos, kw, seen = _stub_thin(monkeypatch)

    def denoise(pts, off, radius, min_neighbors, grid, max_per_sample, return_index=False):
        calls.append("remove_radius_outliers_ragged")
        seen.update(d_pts=pts, d_off=off, d_args=(radius, min_neighbors, max_per_sample, return_index), d_grid=grid)
        seen["denoised"] = torch.full((pts.shape[0], 3), 3.0)
        return seen["denoised"], torch.tensor([0, 4, 6]), torch.arange(pts.shape[0]) * 2
    E.PP.remove_radius_outliers_ragged = denoise
    return E, calls, reads, pos, kw, seen


def test_infer_point_clouds_without_denoise_is_what_it_was(monkeypatch):
    from test_cloud_metrics_host import TAIL
    E, calls, reads, pos, kw, seen = _stub_denoise(monkeypatch)
    out = E.infer_point_clouds(*pos, **kw)
    assert calls == TAIL + ["cal_metrics_ragged"] and len(reads) == 1 and set(out) == {"pred", "cd", "n_queries"}
    assert out["cd"] == [1.5, 2.5] and out["n_queries"] == [150, 150] and [p.shape[0] for p in out["pred"]] == [7, 5]
    del calls[:], reads[:]
    out = E.infer_point_clouds(*pos, metric_thresholds=(0.1, 0.2), **kw)
    assert calls == TAIL + ["cloud_metrics_ragged"] and len(reads) == 1 and set(out) == {"pred", "cd", "n_queries", "metrics"}
    del calls[:], reads[:]
    out = E.infer_point_clouds(*pos, thin=4.0, resample=5, **kw)
    assert calls == TAIL + ["cal_metrics_ragged", "voxel_downsample_ragged", "resample_points_ragged"] and len(reads) == 1
    assert set(out) == {"pred", "cd", "n_queries", "thinned", "thin_count", "thin_first", "resampled", "resample_index"}
    assert seen["t_off"].tolist() == [0, 7, 12] and [t.shape[0] for t in out["thinned"]] == [3, 2]
    del calls[:], reads[:]
    assert len(E.infer_point_clouds_device(*pos, **kw)) == 3 and len(E.infer_point_clouds_device(*pos, thin=4.0, resample=5, **kw)) == 9
    assert "remove_radius_outliers_ragged" not in calls and "d_grid" not in seen and not reads


def test_infer_point_clouds_with_denoise(monkeypatch):
    from test_cloud_metrics_host import TAIL
    E, calls, reads, pos, kw, seen = _stub_denoise(monkeypatch)
    base = E.infer_point_clouds(*pos, **kw)
    del calls[:], reads[:]
    out = E.infer_point_clouds(*pos, denoise=(0.5, 2), **kw)
    # the filter after the metric of the full cloud, then the metric of the denoised one; still one host read
    assert calls == TAIL + ["cal_metrics_ragged", "remove_radius_outliers_ragged", "cal_metrics_ragged"] and len(reads) == 1
    assert set(out) == {"pred", "cd", "n_queries", "denoised", "denoise_index", "cd_denoised"}
    assert out["cd"] == base["cd"] and out["n_queries"] == base["n_queries"] and [p.shape[0] for p in out["pred"]] == [7, 5]
    assert [t.shape[0] for t in out["denoised"]] == [4, 2] and out["denoise_index"][1].tolist() == [8, 10] and out["cd_denoised"] == [1.5, 2.5]
    assert seen["d_off"].tolist() == [0, 7, 12] and seen["d_args"] == (0.5, 2, 50, True)
    assert seen["d_grid"] == E.PP.voxel_grid([-15.8] * 3, [15.8] * 3, 0.5)
    # with the metrics in the same host read: each set is unpacked from its own place
    del calls[:], reads[:]
    m = E.infer_point_clouds(*pos, denoise=(0.5, 2), metric_thresholds=(0.1, 0.2), **kw)
    ref = E.infer_point_clouds(*pos, metric_thresholds=(0.1, 0.2), **kw)
    assert calls[:len(TAIL) + 3] == TAIL + ["cloud_metrics_ragged", "remove_radius_outliers_ragged", "cloud_metrics_ragged"] and len(reads) == 2
    assert m["metrics"] == ref["metrics"] and m["metrics_denoised"] == ref["metrics"] and m["cd_denoised"] == ref["cd"] == m["cd"]
    assert [t.shape[0] for t in m["denoised"]] == [4, 2]
    # no surfaces: no metric of either kind, no key for it
    out = E.infer_point_clouds(*pos, denoise=(0.5, 2), **{**kw, "surfaces": None})
    assert out["cd"] is None and "cd_denoised" not in out and [t.shape[0] for t in out["denoised"]] == [4, 2]
    # thin and resample run on the denoised clouds
    del calls[:], reads[:]
    out = E.infer_point_clouds(*pos, denoise=(0.5, 2), thin=4.0, resample=5, metric_thresholds=(0.1,), **kw)
    assert calls == TAIL + ["cloud_metrics_ragged", "remove_radius_outliers_ragged", "cloud_metrics_ragged", "voxel_downsample_ragged",
                            "resample_points_ragged"] and len(reads) == 1
    assert seen["t_pts"] is seen["denoised"] and seen["t_off"].tolist() == [0, 4, 6] and seen["r_pts"] is seen["thinned"]
    assert [t.shape[0] for t in out["thinned"]] == [3, 2] and [t.shape[0] for t in out["denoised"]] == [4, 2]
    assert out["metrics_denoised"][1]["accuracy"] == 2.5 and len(out["metrics_denoised"][0]["f_score"]) == 1
    out = E.infer_point_clouds(*pos, denoise=(0.5, 2), resample=5, **kw)
    assert seen["r_pts"] is seen["denoised"] and seen["r_off"].tolist() == [0, 4, 6]
    del calls[:], reads[:]
    dev = E.infer_point_clouds_device(*pos, denoise=(0.5, 2), thin=4.0, resample=5, **kw)
    assert len(dev) == 13 and dev[3] is seen["denoised"] and dev[4].tolist() == [0, 4, 6] and dev[6].tolist() == [1.5, 2.5]
    assert dev[7] is seen["thinned"] and seen["t_pts"] is seen["denoised"] and not reads
    assert len(E.infer_point_clouds_device(*pos, denoise=(0.5, 2), metric_thresholds=(), **kw)) == 9
