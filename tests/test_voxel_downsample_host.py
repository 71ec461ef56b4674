"""Voxel-grid down-sampling, host side (no GPU): the reference of tests/voxel_ref.py against an independent float64 brute force and on
planted ties and faces; voxel_grid's arithmetic and refusals; the C entries' declarations, scratch sizes and every refusal (through
the built library, before any GPU work); the Python layer's argument errors; and, with the device functions stubbed, that
infer_point_clouds does what it did before when `thin` is left alone, and what it should with it."""
import ctypes as C

import numpy as np
import pytest
import torch

import voxel_ref as REF

F32 = np.float32


# ---- the reference -------------------------------------------------------------------------------------------------------------------------
def _cloud_off_the_faces(seed, n, lo, v, dims):
    """Uniform rows over a box a little larger than the grid, every coordinate at least 1e-4 from every cell face."""
    rs = np.random.RandomState(seed)
    lo, v, dims = np.asarray(lo, np.float64), np.asarray(v, np.float64), np.asarray(dims)
    p = (rs.uniform(-0.1, 1.1, size=(4 * n, 3)) * (v * dims) + lo).astype(F32)
    t = (p.astype(np.float64) - lo) / v
    keep = (np.abs(t - np.round(t)) * v > 1e-4).all(axis=1)
    p = p[keep][:n]
    assert len(p) == n
    return p


@pytest.mark.parametrize("seed,n,lo,v,dims", [(1, 500, (0, 0, 0), (0.5, 0.5, 0.5), (8, 8, 8)), (2, 2000, (-3.2, 1.0, -0.7), (0.05, 0.25, 0.1), (40, 9, 17)),
                                              (3, 300, (-40, -40, -40), (1.0, 2.0, 80.0), (80, 40, 1))])
def test_reference_agrees_with_an_independent_brute_force(seed, n, lo, v, dims):
    p = _cloud_off_the_faces(seed, n, lo, v, dims)
    lo3, v3 = [float(F32(x)) for x in lo], [float(F32(x)) for x in v]
    r = REF.voxel_one(p, lo3, v3, dims)
    cells, cnt, cen, inv = REF.voxel_brute_float64(p, lo3, v3, dims)
    assert 0 < len(cells) < n and (inv == -1).any()                          # some rows share cells, some lie outside
    assert np.array_equal(r["cells"], cells) and np.array_equal(r["count"], cnt) and np.array_equal(r["inverse"], inv)
    assert np.abs(r["points"].astype(np.float64) - cen).max() <= 1e-6 * max(1.0, np.abs(cen).max())
    assert (np.diff(r["keys"]) > 0).all()
    firsts = [int(np.nonzero(inv == k)[0][0]) for k in range(len(cells))]
    assert r["first"].tolist() == firsts


def test_reference_on_planted_ties_and_faces():
    lo3, v3, dims = (0.0, 0.0, 0.0), (0.5, 0.5, 0.5), (4, 4, 4)
    below, above = np.nextafter(F32(0.5), F32(0)), np.nextafter(F32(0.5), F32(1))
    top_in = np.nextafter(F32(2.0), F32(0))
    p = np.array([[0.5, 0, 0], [below, 0, 0], [above, 0, 0], [0, 0, 0], [-0.0, -0.0, -0.0], [2.0, 0, 0], [top_in, 0, 0],
                  [np.nextafter(F32(0), F32(-1)), 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [0.5, 0, 0]], F32)
    r = REF.voxel_one(p, lo3, v3, dims)
    # cells along axis 0: rows 1, 3, 4 in cell 0; rows 0, 2, 11 in cell 1; row 6 in cell 3; the face at 2.0, the float below 0 and the
    # non-finite rows outside
    assert r["inverse"].tolist() == [1, 0, 1, 0, 0, -1, 2, -1, -1, -1, -1, 1]
    assert r["cells"].tolist() == [[0, 0, 0], [1, 0, 0], [3, 0, 0]] and r["count"].tolist() == [3, 3, 1] and r["first"].tolist() == [1, 0, 6]
    assert r["keys"].tolist() == [0, 16, 48]
    # duplicates: the centroid of equal rows is the row
    assert r["points"][2].tolist() == [float(top_in), 0.0, 0.0]
    # the sequential sum's order shows: 1e-30 first is absorbed only at the end
    q = np.array([[1e-30, 0, 0], [0.04, 0, 0], [0.049, 0, 0]], F32)
    s = (np.float64(q[0, 0]) + np.float64(q[1, 0])) + np.float64(q[2, 0])
    assert REF.voxel_one(q, lo3, v3, dims)["points"][0, 0] == F32(s / 3.0)
    # ascending key order whatever the row order
    rs = np.random.RandomState(0)
    cloud = rs.randint(0, 4, size=(200, 3)).astype(F32) * F32(0.5) + F32(0.25)
    a, b = REF.voxel_one(cloud, lo3, v3, dims), REF.voxel_one(cloud[rs.permutation(200)], lo3, v3, dims)
    assert np.array_equal(a["cells"], b["cells"]) and np.array_equal(a["count"], b["count"]) and np.array_equal(a["points"], b["points"])
    # the ragged form: counts, the bound, empty clouds
    off = [0, 50, 50, 200]
    g = REF.voxel_ragged(cloud, off, lo3, v3, dims, 100, counts=[10, 5, 400])
    one = REF.voxel_one(cloud[50:150], lo3, v3, dims)
    m0 = len(REF.voxel_one(cloud[:10], lo3, v3, dims)["count"])
    assert g["offsets"].tolist() == [0, m0, m0, m0 + len(one["count"])] and np.array_equal(g["points"][m0:], one["points"])
    assert g["untouched"][10:50].all() and g["untouched"][150:].all() and not g["untouched"][50:150].any()
    assert [REF.passes(c) for c in (1, 255, 256, 65535, 65536, 2 ** 24 - 1, 2 ** 24, 1290 ** 3, 2 ** 31 - 1)] == [1, 1, 2, 2, 3, 3, 4, 4, 4]


# ---- voxel_grid ----------------------------------------------------------------------------------------------------------------------------
def test_voxel_grid_arithmetic_and_refusals():
    from rald_amd.postprocess import voxel_grid
    lo3, v3, dims3 = voxel_grid((0, -90, -20), (15.8, 90, 20), (0.05, 0.25, 0.5))
    assert lo3 == (0.0, -90.0, -20.0) and v3 == (float(F32(0.05)), 0.25, 0.5)
    assert dims3 == (int(np.floor(15.8 / 0.05)) + 1, 721, 81)
    assert voxel_grid((-10, -10, -10), (10, 10, 10), 1.0) == ((-10.0,) * 3, (1.0,) * 3, (21,) * 3)
    assert voxel_grid((0, 0, 0), (0, 0, 0), 2)[2] == (1, 1, 1)
    assert voxel_grid((0, 0, 0), (1289, 1289, 1289), 1)[2] == (1290,) * 3                       # 1290^3 <= 2^31 - 1
    bad = [((0, 0, 0), (1, 1, 1), 0), ((0, 0, 0), (1, 1, 1), -1.0), ((0, 0, 0), (1, 1, 1), float("nan")), ((0, 0, 0), (1, 1, 1), float("inf")),
           ((0, 0, 0), (1, 1, 1), (1, 1)), ((0, 0, 0), (1, 1, 1), (1, 0, 1)), ((0, 0), (1, 1, 1), 1), ((0, 0, 0), (1, 1), 1),
           ((0, 0, float("nan")), (1, 1, 1), 1), ((0, 0, 0), (1, float("inf"), 1), 1), ((0, 2, 0), (1, 1, 1), 1), ((0, 0, 0), (1, 1, 1), 1e-60),
           ((0, 0, 0), (1, 1, 1), None), ((0, 0, 0), (1290, 1290, 1290), 1), ((0, 0, 0), (1e9, 1e9, 1e9), 0.001), ((0, 0, 0), (1, 1, 1), True)]
    for lo, hi, v in bad:
        with pytest.raises(ValueError):
            voxel_grid(lo, hi, v)


# ---- the C entries -------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entries():
    from rald_amd import _lib
    P, I32, I64 = C.c_void_p, C.c_int32, C.c_int64
    call = [P, P, P, I32, I64, I64, I64, P, P, P, P, P, P, P, P, P, P, I64]
    assert _lib.SIGNATURES["rald_post_voxel_scratch_bytes"] == (I64, [I32, I64, I64])
    assert _lib.SIGNATURES["rald_post_voxel_downsample_ragged"] == (I32, call + [P])
    assert _lib.SIGNATURES["rald_op_voxel_scratch_bytes"] == (I64, [I32, I64, I64, I64])
    assert _lib.SIGNATURES["rald_op_voxel_downsample_ragged"] == (I32, call + [I64, P])
    assert _lib.SIGNATURES["rald_op_voxel_passes"] == (I32, [I64])


def test_scratch_bytes_and_passes():
    from rald_amd._lib import lib
    L = lib()
    q, qo = L.rald_post_voxel_scratch_bytes, L.rald_op_voxel_scratch_bytes
    assert q(1, 1, 1) > 0 and q(1, 0, 1) > 0
    # monotonic in every argument, and 16-byte granular
    sizes = [q(1, 1000, 1000), q(1, 5000, 1000), q(1, 5000, 5000), q(3, 5000, 5000), q(3, 480000, 480000), q(64, 1 << 21, 1 << 21),
             q(64, 1 << 25, 1 << 24)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])) and all(s % 16 == 0 for s in sizes)
    assert qo(2, 70000, 70000, 0) == q(2, 70000, 70000)
    assert qo(2, 70000, 70000, 1024) > qo(2, 70000, 70000, 2048) > qo(2, 70000, 70000, 4096) > qo(2, 70000, 70000, 70 * 1024)
    for args in ((0, 10, 10), (-1, 10, 10), (65536, 10, 10), (1, -1, 10), (1, 1 << 31, 10), (1, 10, 0), (1, 10, -4), (1, 10, (1 << 24) + 1)):
        assert q(*args) == -1, args
        assert b"rald_post_voxel_scratch_bytes" in L.rald_last_error()
    for chunk in (-1024, 1, 1000, 1025):
        assert qo(1, 10, 10, chunk) == -1 and b"rald_op_voxel_scratch_bytes" in L.rald_last_error()
    assert q(1, 10, 1 << 21) > 0 and q(1, 10, 1 << 24) > 0                                          # bounds up to 2^24 are taken
    p = L.rald_op_voxel_passes
    assert [p(c) for c in (1, 255, 256, 65535, 65536, 2 ** 24 - 1, 2 ** 24, 1290 ** 3, 2 ** 31 - 1)] == [1, 1, 2, 2, 3, 3, 4, 4, 4]
    assert p(0) == -1 and p(2 ** 31) == -1 and b"rald_op_voxel_passes" in L.rald_last_error()


def test_every_refusal_comes_before_any_gpu_work():
    """Host buffers stand in for device memory: a refused call touches none of them and launches nothing."""
    from rald_amd._lib import lib
    L = lib()
    pts, out, off = (C.c_float * 64)(), (C.c_float * 64)(), (C.c_int64 * 4)()
    need = L.rald_op_voxel_scratch_bytes(1, 4, 4, 0)
    scratch = (C.c_char * (need + 64))()
    base = C.addressof(scratch)
    aligned = base + (-base) % 16
    f3, i3 = lambda *v: (C.c_float * 3)(*v), lambda *v: (C.c_int32 * 3)(*v)
    ok = dict(points=pts, offsets=None, counts=None, batch=1, n_dense=4, n_total=4, max_per_sample=4, lo=f3(0, 0, 0), v=f3(1, 1, 1), dims=i3(4, 4, 4),
              out_points=out, out_offsets=off, out_count=None, out_first=None, out_cells=None, out_inverse=None, scratch=aligned,
              scratch_bytes=need, chunk=0, stream=None)
    inf, nan = float("inf"), float("nan")
    cases = [(dict(points=None), b"null pointer"), (dict(out_points=None), b"null pointer"), (dict(out_offsets=None), b"null pointer"),
             (dict(lo=None), b"null grid"), (dict(v=None), b"null grid"), (dict(dims=None), b"null grid"),
             (dict(batch=0), b"batch must be 1 .. 65535"), (dict(batch=-2), b"batch must be 1 .. 65535"), (dict(batch=65536), b"batch must be 1 .. 65535"),
             (dict(n_dense=-1), b"n_dense must be >= 0"), (dict(n_total=-1), b"n_total must be"), (dict(n_total=1 << 31), b"n_total must be"),
             (dict(max_per_sample=0), b"max_per_sample must be 1 .. 16777216"), (dict(max_per_sample=-7), b"max_per_sample must be 1 .. 16777216"),
             (dict(max_per_sample=(1 << 24) + 1), b"max_per_sample must be 1 .. 16777216"),
             (dict(dims=i3(4, 0, 4)), b"every dim must be >= 1"), (dict(dims=i3(-1, 4, 4)), b"every dim must be >= 1"),
             (dict(dims=i3(1291, 1290, 1290)), b"at most 2^31 - 1 cells"), (dict(dims=i3(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)), b"at most 2^31 - 1 cells"),
             (dict(dims=i3(65536, 32768, 1)), b"at most 2^31 - 1 cells"),
             (dict(v=f3(1, 0, 1)), b"cell edge must be finite and > 0"), (dict(v=f3(-1, 1, 1)), b"cell edge must be finite and > 0"),
             (dict(v=f3(1, 1, inf)), b"cell edge must be finite and > 0"), (dict(v=f3(nan, 1, 1)), b"cell edge must be finite and > 0"),
             (dict(lo=f3(0, inf, 0)), b"lo must be finite"), (dict(lo=f3(0, 0, nan)), b"lo must be finite"),
             (dict(scratch_bytes=need - 1), b"scratch too small"), (dict(scratch=None), b"null or unaligned scratch"),
             (dict(scratch=aligned + 4), b"null or unaligned scratch"), (dict(max_per_sample=1 << 21), b"scratch too small"),
             (dict(chunk=1000), b"multiple of 1024"), (dict(chunk=-1024), b"multiple of 1024"), (dict(chunk=1), b"multiple of 1024")]
    for change, message in cases:
        a = {**ok, **change}
        assert L.rald_op_voxel_downsample_ragged(*a.values()) == 1, change
        assert message in L.rald_last_error(), (change, L.rald_last_error())
        if "chunk" not in change:
            del a["chunk"]
            assert L.rald_post_voxel_downsample_ragged(*a.values()) == 1, change
            assert message in L.rald_last_error(), (change, L.rald_last_error())


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_raise_before_the_library_is_touched(monkeypatch):
    from rald_amd import engine_generation as E, postprocess as PP
    from test_fps_host import _no_library
    _no_library(monkeypatch)
    pts, off = torch.zeros(10, 3), torch.tensor([0, 4, 10])
    grid = PP.voxel_grid((0, 0, 0), (1, 1, 1), 0.5)
    ok = dict(points=pts, offsets=off, grid=grid, max_per_sample=6)
    bad = [dict(points=torch.zeros(10, 2)), dict(points=torch.zeros(2, 5, 3)), dict(points=torch.zeros(10, 3, dtype=torch.int64)),
           dict(points=[[0.0, 0.0, 0.0]]), dict(offsets=torch.tensor([0.0, 4.0, 10.0])), dict(offsets=torch.tensor([10])), dict(offsets=[0, 4, 10]),
           dict(max_per_sample=0), dict(max_per_sample=(1 << 24) + 1), dict(max_per_sample=2.5), dict(max_per_sample=True),
           dict(counts=torch.tensor([4, 6])), dict(counts=torch.tensor([4, 6, 1], dtype=torch.int32)), dict(counts=[4, 6]),
           dict(grid=None), dict(grid=(grid[0], grid[1])), dict(grid=(grid[0], (0.5, 0.0, 0.5), grid[2])), dict(grid=(grid[0], grid[1], (3, 0, 3))),
           dict(grid=((0.0, float("nan"), 0.0), grid[1], grid[2])), dict(grid=(grid[0], grid[1], (1291, 1290, 1290))),
           dict(grid=(grid[0], grid[1], (3.5, 3, 3))), dict(chunk=1000), dict(chunk=-1024)]
    for kw in bad:
        with pytest.raises(ValueError):
            PP.voxel_downsample_ragged(**{**ok, **kw})
    for points, kw in ((torch.zeros(2, 5, 3), {}), (torch.zeros(5, 2), {}), (torch.zeros(5, 3), dict(voxel=0)), (torch.zeros(5, 3), dict(voxel=(1, 2))),
                       (torch.zeros(5, 3), dict(lo=(0, 0, 0))), (torch.zeros(5, 3), dict(lo=(0, 0, 0), hi=(1e9, 1e9, 1e9), voxel=1e-3)),
                       (torch.zeros(5, 3, dtype=torch.int32), {})):
        with pytest.raises(ValueError):
            PP.voxel_downsample(points, **{"voxel": 0.5, **kw})
    assert PP.voxel_downsample(torch.zeros(0, 3), 0.5).shape == (0, 3)

    class Vae:
        def __getattr__(self, name):
            raise AssertionError("the autoencoder was touched")
    lidar = dict(pc_range=[0, -90, -20, 15.8, 90, 20], view_cone_mode=True)
    ns = lambda **kw: type("NS", (), kw)()
    args = ns(dataset=ns(lidar=ns(**lidar)))
    for fn in (E.infer_point_clouds, E.infer_point_clouds_device):
        for thin in (0, -0.1, float("nan"), (0.1, 0.1), 1e-3, "fine"):               # 1e-3: (31.6 / 1e-3)^3 cells
            with pytest.raises(ValueError):
                fn(Vae(), torch.zeros(2, 128, 32), args, thin=thin)
    # the grid of the tail: the cube of the largest range in view-cone mode, pc_range otherwise
    assert E._thin_grid(0.5, args) == PP.voxel_grid([-15.8] * 3, [15.8] * 3, 0.5) and E._thin_grid(None, args) is None
    args.dataset.lidar.view_cone_mode = False
    assert E._thin_grid((0.5, 1, 2), args) == PP.voxel_grid([0, -90, -20], [15.8, 90, 20], (0.5, 1, 2))


# ---- the tail ------------------------------------------------------------------------------------------------------------------------------
def _stub_thin(monkeypatch):
    from rald_amd import engine_generation as E, postprocess as PP
    from test_cloud_metrics_host import _stub_tail
    real_grid = PP.voxel_grid
    calls, reads, pos, kw, _ = _stub_tail(monkeypatch)
    seen = {}

    def resample(pts, off, k, max_per_sample, return_index=False):
        calls.append("resample_points_ragged")
        seen.update(r_pts=pts, r_off=off, k=k, r_bound=max_per_sample)
        return torch.ones(2, k, 3), torch.zeros(2, k, dtype=torch.int64)

    def thin(pts, off, grid, max_per_sample, return_count=False, return_first=False):
        calls.append("voxel_downsample_ragged")
        seen.update(t_pts=pts, t_off=off, grid=grid, t_bound=max_per_sample, flags=(return_count, return_first))
        seen["thinned"] = torch.full((pts.shape[0], 3), 7.0)
        return seen["thinned"], torch.tensor([0, 3, 5]), torch.ones(pts.shape[0], dtype=torch.int32), torch.arange(pts.shape[0])
    E.PP.resample_points_ragged = resample
    E.PP.voxel_downsample_ragged = thin
    E.PP.voxel_grid = real_grid
    E.PP.FPS_MAX_POINTS = 65536
    return E, calls, reads, pos, kw, seen


def test_infer_point_clouds_without_thin_is_what_it_was(monkeypatch):
    from test_cloud_metrics_host import TAIL
    E, calls, reads, pos, kw, seen = _stub_thin(monkeypatch)
    out = E.infer_point_clouds(*pos, **kw)
    assert calls == TAIL + ["cal_metrics_ragged"] and len(reads) == 1 and set(out) == {"pred", "cd", "n_queries"}
    del calls[:], reads[:]
    out = E.infer_point_clouds(*pos, resample=5, **kw)
    assert calls == TAIL + ["cal_metrics_ragged", "resample_points_ragged"] and len(reads) == 1
    assert set(out) == {"pred", "cd", "n_queries", "resampled", "resample_index"} and seen["r_bound"] == 50 and seen["r_off"].tolist() == [0, 7, 12]
    del calls[:], reads[:]
    assert len(E.infer_point_clouds_device(*pos, **kw)) == 3 and len(E.infer_point_clouds_device(*pos, resample=5, **kw)) == 5 and not reads
    assert "voxel_downsample_ragged" not in calls and "grid" not in seen


def test_infer_point_clouds_with_thin(monkeypatch):
    from test_cloud_metrics_host import TAIL
    E, calls, reads, pos, kw, seen = _stub_thin(monkeypatch)
    out = E.infer_point_clouds(*pos, thin=4.0, **kw)
    assert calls == TAIL + ["cal_metrics_ragged", "voxel_downsample_ragged"] and len(reads) == 1
    assert set(out) == {"pred", "cd", "n_queries", "thinned", "thin_count", "thin_first"} and out["cd"] == [1.5, 2.5]
    assert [t.shape[0] for t in out["thinned"]] == [3, 2] and [t.shape[0] for t in out["thin_count"]] == [3, 2]
    assert out["thin_first"][1].tolist() == [3, 4] and [p.shape[0] for p in out["pred"]] == [7, 5]
    assert seen["t_off"].tolist() == [0, 7, 12] and seen["t_bound"] == 50 and seen["flags"] == (True, True)
    assert seen["grid"] == E.PP.voxel_grid([-15.8] * 3, [15.8] * 3, 4.0) and seen["grid"][2] == (8, 8, 8)
    # with the metrics in the same host read: both are unpacked from their own places
    base = E.infer_point_clouds(*pos, metric_thresholds=(0.1, 0.2), **kw)
    out = E.infer_point_clouds(*pos, thin=4.0, metric_thresholds=(0.1, 0.2), **kw)
    assert out["metrics"] == base["metrics"] and out["cd"] == base["cd"] and [t.shape[0] for t in out["thinned"]] == [3, 2] and len(reads) == 3
    del calls[:], reads[:]
    # with resample: the sampler gets the thinned clouds, their offsets and min(longest, cells, the sampler's limit)
    out = E.infer_point_clouds(*pos, thin=4.0, resample=5, **kw)
    assert calls == TAIL + ["cal_metrics_ragged", "voxel_downsample_ragged", "resample_points_ragged"] and len(reads) == 1
    assert set(out) == {"pred", "cd", "n_queries", "thinned", "thin_count", "thin_first", "resampled", "resample_index"}
    assert seen["r_pts"] is seen["thinned"] and seen["r_off"].tolist() == [0, 3, 5] and seen["r_bound"] == 50 and seen["k"] == 5
    E.infer_point_clouds(*pos, thin=10.0, resample=5, **kw)
    assert seen["grid"][2] == (4, 4, 4) and seen["r_bound"] == 50
    E.infer_point_clouds(*pos, thin=16.0, resample=5, **kw)
    assert seen["grid"][2] == (2, 2, 2) and seen["r_bound"] == 8                  # fewer cells than rows: the cells bound the sampler
    del calls[:], reads[:]
    dev = E.infer_point_clouds_device(*pos, thin=4.0, resample=5, **kw)
    assert len(dev) == 9 and dev[3] is seen["thinned"] and dev[4].tolist() == [0, 3, 5] and dev[7].shape == (2, 5, 3) and not reads
    assert len(E.infer_point_clouds_device(*pos, thin=4.0, **kw)) == 7
