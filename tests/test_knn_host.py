"""k nearest neighbours and statistical outlier removal, host side (no GPU): the brute-force reference of tests/knn_ref.py against an
independent grid walk with the header's termination rule on the constructions the GPU tests use, against scipy's k-d tree in float64
and against numpy's mean and deviation; the reference on planted cases; the C entries' declarations, scratch sizes and every refusal
(through the built library, before any GPU work); the Python layer's argument errors; and, with the device functions stubbed, that
infer_point_clouds does what it did before when `denoise_statistical` is left alone, and what it should with it."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import knn_ref as REF
import radius_ref as RREF

F32 = np.float32


def _same_tables(a, b):
    return (np.array_equal(a["idx"], b["idx"]) and np.array_equal(a["dist2"].view(np.uint32), b["dist2"].view(np.uint32))
            and np.array_equal(a["found"], b["found"]))


# ---- the reference -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(REF.CONSTRUCTIONS))
def test_reference_agrees_with_the_grid_walk(name):
    p, grid = REF.CONSTRUCTIONS[name]()
    p, k = p[:400], 8
    a = REF.knn_one(p, grid, k)
    b, widest = REF.grid_walk_knn(p, grid, k)
    assert a["inside"].all() and (a["found"] == k).all() and _same_tables(a, b)
    if name in ("far_row", "corner_blob"):
        assert widest == max(grid[2])                                         # the far rows' boxes grow to the grid
    if name == "all_equal":
        assert (a["dist2"] == 0).all() and a["idx"][0].tolist() == list(range(1, 9)) and a["idx"][5].tolist() == [0, 1, 2, 3, 4, 6, 7, 8]
    # with a bound between the distances: fewer candidates for some rows, and the walk stops at the bound's range
    r = float(np.sqrt(np.median(a["dist2"][:, 3]))) or 0.5
    c = REF.knn_one(p, grid, k, max_radius=r)
    d, _ = REF.grid_walk_knn(p, grid, k, max_radius=r)
    assert _same_tables(c, d) and (c["found"] <= a["found"]).all()
    r2 = F32(F32(r) * F32(r))
    assert all(np.array_equal(c["idx"][i, :c["found"][i]], a["idx"][i][a["dist2"][i] <= r2]) for i in range(len(p)))


def test_reference_on_planted_cases():
    grid = RREF.cube_grid(0.0, 1.0, 0.125)
    up = np.nextafter(F32(0.25), F32(1))
    p = np.array([[0.25, 0.25, 0.25], [0.375, 0.25, 0.25], [0.25, 0.25, 0.25], [0.375, 0.375, 0.25], [up, 0.25, 0.25], [0.125, 0.25, 0.25],
                  [np.nan, 0.25, 0.25], [0.25, np.inf, 0.25], [2.0, 0.25, 0.25], [-0.01, 0.25, 0.25], [0.9, 0.9, 0.9]], F32)
    a = REF.knn_one(p, grid, 3)
    assert a["found"].tolist() == [3, 3, 3, 3, 3, 3, -1, -1, -1, -1, 3]
    assert a["idx"][0].tolist() == [2, 4, 1]                                  # the duplicate, one ulp up, then rows 1 and 5 at equal d2: 1
    assert a["idx"][5].tolist() == [0, 2, 4] and a["idx"][2].tolist() == [0, 4, 1]
    assert (a["idx"][6:10] == -1).all() and np.isposinf(a["dist2"][6:10]).all() and not np.isin(a["idx"], [6, 7, 8, 9]).any()
    b = REF.knn_one(p, grid, 8)
    assert b["found"].tolist() == [6, 6, 6, 6, 6, 6, -1, -1, -1, -1, 6] and (b["idx"][0, 6:] == -1).all() and np.isposinf(b["dist2"][0, 6:]).all()
    c = REF.knn_one(p, grid, 3, max_radius=0.125)
    assert c["found"].tolist() == [3, 3, 3, 1, 3, 2, -1, -1, -1, -1, 0] and c["idx"][3].tolist() == [1, -1, -1]
    # the filter: means, the fixed sum, the threshold
    s = REF.statistical_one(p, grid, 3, 1.0, max_radius=0.125)
    assert np.isnan(s["mean"][6:10]).all() and np.isposinf(s["mean"][10]) and s["n_f"] == 6
    m = s["mean"][:6]
    want3 = (math.sqrt(float(F32(0.015625))) + 0.0) / 1.0
    assert m[3] == want3 and m[5] == (0.125 + 0.125) / 2 and m[0] == (0.0 + math.sqrt(float(c["dist2"][0, 1])) + 0.125) / 3
    assert abs(s["stats"][0] - m.mean()) < 1e-15 and abs(s["stats"][1] - m.std(ddof=1)) < 1e-15
    assert s["stats"][2] == s["stats"][0] + 1.0 * s["stats"][1] and s["keep"].tolist() == (m <= s["stats"][2]).tolist() + [False] * 5
    f = REF.statistical_ragged(p, [0, 6, 6, 11], grid, 3, 1.0, 4, counts=[5, 3, 9], max_radius=0.125)
    alone = REF.statistical_ragged(p[:4], [0, 4], grid, 3, 1.0, 4, max_radius=0.125)
    assert np.array_equal(f["index"][:f["offsets"][1]], alone["index"]) and np.isnan(f["stats"][1]).all() and f["offsets"][1] == f["offsets"][2]
    assert f["untouched"].tolist() == [False] * 4 + [True] * 2 + [False] * 4 + [True]
    # equal means: kept whole with sigma 0; n_f = 0, 1, 2
    eq = REF.statistical_one(np.tile(p[:1], (5, 1)), grid, 2, 0.0)
    assert eq["keep"].all() and eq["stats"].tolist() == [0.0, 0.0, 0.0]
    assert not REF.statistical_one(p[:1], grid, 2, 1.0)["keep"].any() and np.isnan(REF.statistical_one(p[:1], grid, 2, 1.0)["stats"]).all()
    one = REF.statistical_one(p[[0, 10, 1]], grid, 2, 0.0, max_radius=0.125)
    assert one["n_f"] == 2 and one["keep"].tolist() == [True, False, True] and one["stats"][1] == 0.0
    lone = REF.statistical_one(p[[0, 1, 10, 3]], grid, 1, 0.0, max_radius=0.13)
    assert lone["n_f"] == 3 and lone["found"].tolist() == [1, 1, 0, 1]


def test_fixed_sum_shape():
    """The shape written out once more: blocks of 1024 in row order, a halving tree inside, the blocks left to right."""
    v = np.random.RandomState(3).uniform(0, 1, 2500) * 10.0 ** np.random.RandomState(4).randint(-8, 8, 2500)
    pad = np.concatenate([v, np.zeros(3072 - 2500)])
    blocks = []
    for g in range(3):
        w = list(pad[1024 * g:1024 * g + 1024])
        while len(w) > 1:
            h = len(w) // 2
            w = [w[t] + w[t + h] for t in range(h)]
        blocks.append(w[0])
    assert REF.fixed_sum(v) == ((0.0 + blocks[0]) + blocks[1]) + blocks[2]
    assert REF.fixed_sum(np.zeros(0)) == 0.0 and REF.fixed_sum(np.array([2.5])) == 2.5


SCIPY_CASES = [(257, 16), (1500, 8), (4097, 32)]


@pytest.mark.parametrize("n,k", SCIPY_CASES)
def test_against_scipy_kdtree(n, k):
    """scipy's k-d tree in float64 on the same float32 coordinates: the index lists agree wherever the float32 order is not a matter of
    rounding - rows with two consecutive squared distances among the first k+1 closer than 1e-5 relative are left out, at most 2 %."""
    from scipy.spatial import cKDTree
    p = np.random.RandomState(100 + n).uniform(0, 1, size=(n, 3)).astype(F32)
    a = REF.knn_one(p, RREF.cube_grid(0.0, 1.0, 0.1), k)
    dist, idx = cKDTree(p.astype(np.float64)).query(p.astype(np.float64), k=k + 2)
    assert (idx[:, 0] == np.arange(n)).all()                                  # no duplicates: the row itself comes first
    d2 = dist[:, 1:] ** 2
    close = (np.diff(d2, axis=1) < 1e-5 * d2[:, 1:])[:, :k].any(axis=1)
    print(f"n={n} k={k}: left out {close.mean():.4%}")
    assert close.mean() <= 0.02
    assert np.array_equal(a["idx"][~close], idx[~close, 1:k + 1])


def test_statistics_against_numpy():
    """mu and sigma against numpy.mean / numpy.std(ddof=1).  The fixed-shape sum against math.fsum of the same means, measured on these
    three clouds (n = 257, 1500, 4097): the difference is 0 on all three - the tree sum rounds to the same double as the exact sum, so
    all that the measurement says is "below one ulp", 2^-52 = 2.2e-16 relative.  The tolerance is four times that, 8.9e-16, for mu, and
    the same for sigma, whose sum of squares has the same shape and whose square root halves a relative error.  (Measured against numpy
    itself, mu and sigma also differ by 0 here; numpy's pairwise sum is free to differ by an ulp in another version.)"""
    for n, k in SCIPY_CASES:
        p = np.random.RandomState(100 + n).uniform(0, 1, size=(n, 3)).astype(F32)
        s = REF.statistical_one(p, RREF.cube_grid(0.0, 1.0, 0.1), k, 2.0)
        m = s["mean"]
        assert s["n_f"] == n and np.isfinite(m).all()
        exact = math.fsum(m)
        rel = abs(float(REF.fixed_sum(m)) - exact) / exact
        print(f"n={n}: fixed-shape sum against fsum, relative {rel:.3e}")
        tol = 4 * 2.0 ** -52
        assert rel <= tol
        assert abs(s["stats"][0] - np.mean(m)) <= tol * abs(np.mean(m))
        assert abs(s["stats"][1] - np.std(m, ddof=1)) <= tol * np.std(m, ddof=1)
        assert s["stats"][2] == s["stats"][0] + 2.0 * s["stats"][1] and 0 < s["keep"].sum() < n


# ---- the C entries -------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entries():
    from rald_amd import _lib
    P, I32, I64, F, D = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_double
    head = [P, P, P, I32, I64, I64, I64, P, P, P, I32, F]
    for name in ("knn", "statistical"):
        assert _lib.SIGNATURES[f"rald_post_{name}_scratch_bytes"] == (I64, [I32, I64, I64])
        assert _lib.SIGNATURES[f"rald_op_{name}_scratch_bytes"] == (I64, [I32, I64, I64, I64])
    assert _lib.SIGNATURES["rald_post_knn_ragged"] == (I32, head + [P, P, P, P, I64, P])
    assert _lib.SIGNATURES["rald_op_knn_ragged"] == (I32, head + [P, P, P, P, I64, I64, P])
    assert _lib.SIGNATURES["rald_post_statistical_filter_ragged"] == (I32, head + [D, P, P, P, P, P, P, I64, P])
    assert _lib.SIGNATURES["rald_op_statistical_filter_ragged"] == (I32, head + [D, P, P, P, P, P, P, I64, I64, P])


def test_scratch_bytes():
    from rald_amd._lib import lib
    L = lib()
    qv = L.rald_post_voxel_scratch_bytes
    for q, qo, per_row, name in ((L.rald_post_knn_scratch_bytes, L.rald_op_knn_scratch_bytes, 16, b"knn"),
                                 (L.rald_post_statistical_scratch_bytes, L.rald_op_statistical_scratch_bytes, 28, b"statistical")):
        assert q(1, 1, 1) > 0 and q(1, 0, 1) > 0
        sizes = [q(1, 1000, 1000), q(1, 5000, 1000), q(1, 5000, 5000), q(3, 5000, 5000), q(3, 480000, 480000), q(64, 1 << 21, 1 << 21),
                 q(64, 1 << 25, 1 << 24)]
        assert all(a < b for a, b in zip(sizes, sizes[1:])) and all(s % 16 == 0 for s in sizes)
        assert qv(3, 480000, 480000) + (per_row + 4) * 480000 >= q(3, 480000, 480000) >= qv(3, 480000, 480000) + per_row * 480000 - 4 * 480000
        assert qo(2, 70000, 70000, 0) == q(2, 70000, 70000) and qo(2, 70000, 70000, 1024) > qo(2, 70000, 70000, 4096)
        for args in ((0, 10, 10), (65536, 10, 10), (1, -1, 10), (1, 1 << 31, 10), (1, 10, 0), (1, 10, (1 << 24) + 1)):
            assert q(*args) == -1 and b"rald_post_" + name + b"_scratch_bytes" in L.rald_last_error(), args
        for chunk in (-1024, 1, 1000, 1025):
            assert qo(1, 10, 10, chunk) == -1 and b"rald_op_" + name + b"_scratch_bytes" in L.rald_last_error()
    # the signatures carry no k: the filter's scratch cannot depend on it, and it never holds the [n_total, k] tables
    assert L.rald_post_statistical_scratch_bytes(1, 480000, 480000) < L.rald_post_knn_scratch_bytes(1, 480000, 480000) + 40 * 480000


def test_every_refusal_comes_before_any_gpu_work():
    """Host buffers stand in for device memory: a refused call touches none of them and launches nothing."""
    from rald_amd._lib import lib
    L = lib()
    pts, out, off = (C.c_float * 64)(), (C.c_float * 64)(), (C.c_int64 * 4)()
    o_idx, o_d, o_f, idx = (C.c_int64 * 128)(), (C.c_float * 128)(), (C.c_int32 * 16)(), (C.c_int64 * 16)()
    mean, stats = (C.c_double * 16)(), (C.c_double * 3)()
    need = max(L.rald_op_knn_scratch_bytes(1, 4, 4, 0), L.rald_op_statistical_scratch_bytes(1, 4, 4, 0))
    assert L.rald_op_statistical_scratch_bytes(1, 4, 4, 0) > L.rald_op_knn_scratch_bytes(1, 4, 4, 0)
    scratch = (C.c_char * (need + 64))()
    base = C.addressof(scratch)
    aligned = base + (-base) % 16
    f3, i3 = lambda *v: (C.c_float * 3)(*v), lambda *v: (C.c_int32 * 3)(*v)
    inf, nan = float("inf"), float("nan")
    layout = dict(points=pts, offsets=None, counts=None, batch=1, n_dense=4, n_total=4, max_per_sample=4, lo=f3(0, 0, 0), v=f3(1, 1, 1),
                  dims=i3(4, 4, 4), k=2, max_radius=0.0)
    knn_need, stat_need = L.rald_op_knn_scratch_bytes(1, 4, 4, 0), L.rald_op_statistical_scratch_bytes(1, 4, 4, 0)
    knn_ok = {**layout, **dict(out_idx=o_idx, out_dist2=o_d, out_found=o_f), **dict(scratch=aligned, scratch_bytes=knn_need, chunk=0, stream=None)}
    stat_ok = {**layout, **dict(std_ratio=1.0, out_points=out, out_offsets=off, out_index=idx, out_mean=mean, out_stats=stats),
               **dict(scratch=aligned, scratch_bytes=stat_need, chunk=0, stream=None)}

    def shared(need):
        return [(dict(points=None), b"null pointer"), (dict(lo=None), b"null grid"), (dict(v=None), b"null grid"), (dict(dims=None), b"null grid"),
                (dict(k=0), b"k must be 1 .. 32"), (dict(k=33), b"k must be 1 .. 32"), (dict(k=-1), b"k must be 1 .. 32"),
                (dict(max_radius=-0.5), b"max_radius must be 0 (none) or finite and > 0"), (dict(max_radius=nan), b"max_radius must be"),
                (dict(max_radius=inf), b"max_radius must be"),
                (dict(v=f3(1, 1, inf)), b"cell edge must be finite"), (dict(v=f3(1, nan, 1)), b"cell edge must be finite"),
                (dict(v=f3(0, 1, 1)), b"cell edge must be finite"), (dict(lo=f3(0, nan, 0)), b"lo must be finite"),
                (dict(batch=0), b"batch must be 1 .. 65535"), (dict(batch=65536), b"batch must be 1 .. 65535"),
                (dict(n_dense=-1), b"n_dense must be >= 0"), (dict(n_total=-1), b"n_total must be"), (dict(n_total=1 << 31), b"n_total must be"),
                (dict(max_per_sample=0), b"max_per_sample must be 1 .. 16777216"), (dict(max_per_sample=(1 << 24) + 1), b"max_per_sample must be"),
                (dict(dims=i3(4, 0, 4)), b"every dim must be >= 1"), (dict(dims=i3(1291, 1290, 1290)), b"at most 2^31 - 1 cells"),
                (dict(dims=i3(65536, 32768, 1)), b"at most 2^31 - 1 cells"),
                (dict(scratch_bytes=need - 1), b"scratch too small"), (dict(max_per_sample=1 << 21), b"scratch too small"),
                (dict(scratch=None), b"null or unaligned scratch"), (dict(scratch=aligned + 4), b"null or unaligned scratch"),
                (dict(chunk=1000), b"multiple of 1024"), (dict(chunk=-1024), b"multiple of 1024"), (dict(chunk=1), b"multiple of 1024")]
    knn_only = [(dict(out_idx=None), b"null pointer")]
    stat_only = [(dict(out_points=None), b"null pointer"), (dict(out_offsets=None), b"null pointer"),
                 (dict(std_ratio=-0.1), b"std_ratio must be finite and >= 0"), (dict(std_ratio=nan), b"std_ratio must be finite and >= 0"),
                 (dict(std_ratio=inf), b"std_ratio must be finite and >= 0")]
    for ok, op, post, who, cases in ((knn_ok, L.rald_op_knn_ragged, L.rald_post_knn_ragged, b"knn_ragged", shared(knn_need) + knn_only),
                                     (stat_ok, L.rald_op_statistical_filter_ragged, L.rald_post_statistical_filter_ragged,
                                      b"statistical_filter_ragged", shared(stat_need) + stat_only)):
        for change, message in cases:
            a = {**ok, **change}
            assert op(*a.values()) == 1, change
            assert message in L.rald_last_error() and who in L.rald_last_error(), (change, L.rald_last_error())
            if "chunk" not in change:
                del a["chunk"]
                assert post(*a.values()) == 1, change
                assert message in L.rald_last_error(), (change, L.rald_last_error())
    assert not any(o_idx) and not any(o_d) and not any(o_f) and not any(out) and not any(off) and not any(idx) and not any(mean) and not any(stats)


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_raise_before_the_library_is_touched(monkeypatch):
    from rald_amd import engine_generation as E, postprocess as PP
    from test_fps_host import _no_library
    _no_library(monkeypatch)
    pts, off = torch.zeros(10, 3), torch.tensor([0, 4, 10])
    grid = PP.voxel_grid((0, 0, 0), (1, 1, 1), 0.5)
    ok = dict(points=pts, offsets=off, k=3, grid=grid, max_per_sample=6)
    bad = [dict(points=torch.zeros(10, 2)), dict(points=torch.zeros(10, 3, dtype=torch.int64)), dict(offsets=torch.tensor([0.0, 4.0, 10.0])),
           dict(offsets=[0, 4, 10]), dict(max_per_sample=0), dict(max_per_sample=(1 << 24) + 1), dict(max_per_sample=True),
           dict(counts=torch.tensor([4, 6])), dict(counts=torch.tensor([4, 6, 1], dtype=torch.int32)), dict(grid=None),
           dict(grid=(grid[0], (0.5, 0.0, 0.5), grid[2])), dict(grid=(grid[0], grid[1], (1291, 1290, 1290))), dict(chunk=1000),
           dict(k=0), dict(k=33), dict(k=-1), dict(k=2.5), dict(k=True), dict(k="3"), dict(k=None), dict(k=float("inf")), dict(k=float("nan")),
           dict(max_radius=0), dict(max_radius=-1.0), dict(max_radius=float("nan")), dict(max_radius=float("inf")), dict(max_radius="wide"),
           dict(max_radius=True), dict(max_radius=1e-60), dict(max_radius=1e60)]
    for kw in bad:
        with pytest.raises(ValueError):
            PP.knn_ragged(**{**ok, **kw})
        with pytest.raises(ValueError):
            PP.remove_statistical_outliers_ragged(**{**ok, "std_ratio": 2.0, **kw})
    for ratio in (-0.1, float("nan"), float("inf"), "2", True, None):
        with pytest.raises(ValueError):
            PP.remove_statistical_outliers_ragged(**{**ok, "std_ratio": ratio})
    for points, kw in ((torch.zeros(2, 5, 3), {}), (torch.zeros(5, 2), {}), (torch.zeros(5, 3), dict(k=0)), (torch.zeros(5, 3), dict(k=33)), (torch.zeros(5, 3), dict(k=float("inf"))),
                       (torch.zeros(5, 3), dict(std_ratio=-1)), (torch.zeros(5, 3), dict(lo=(0, 0, 0))), (torch.zeros(5, 3, dtype=torch.int32), {}),
                       (torch.zeros(5, 3), dict(cell=0)), (torch.zeros(5, 3), dict(cell=float("nan"))), (torch.zeros(5, 3), dict(cell=True)),
                       (torch.zeros(5, 3), dict(lo=(0, 0, 0), hi=(1, float("nan"), 1))), (torch.zeros(5, 3), dict(lo=(0, 0, 0), hi=(1, -1, 1)))):
        with pytest.raises(ValueError):
            PP.remove_statistical_outliers(points, **{"k": 4, "std_ratio": 1.0, **kw})
    assert PP.remove_statistical_outliers(torch.zeros(0, 3), 4, 1.0).shape == (0, 3)
    # the automatic edge: half the edge of k rows per cell of the box; a zero-extent box still gives a grid; a huge box still fits 2^31 - 1 cells
    g = PP._knn_grid((0, 0, 0), (1, 1, 1), 8000, 8)
    assert abs(g[1][0] - 0.05) < 1e-6 and g[1][0] == g[1][1] == g[1][2] and g[2][0] in (20, 21) and g[2][0] == g[2][1] == g[2][2]
    assert PP._knn_grid((2, 2, 2), (2, 2, 2), 50, 8)[2] == (1, 1, 1) and PP._knn_grid((0, 0, 0), (0, 0, 0), 50, 8)[2] == (1, 1, 1)
    flat = PP._knn_grid((0, 0, 5), (4, 4, 5), 1600, 4)
    assert flat[2][2] == 1 and abs(flat[1][0] - 0.1) < 1e-6
    big = PP._knn_grid((-1e6, -1e6, -1e6), (1e6, 1e6, 1e6), 1 << 24, 1)
    assert big[2][0] * big[2][1] * big[2][2] <= 2 ** 31 - 1
    thin = PP._knn_grid((0, 0, 0), (1e-30, 1.0, 1e6), 1000, 8)
    assert thin[2][0] * thin[2][1] * thin[2][2] <= 2 ** 31 - 1
    assert PP._knn_grid((0, 0, 0), (1, 1, 1), 100, 8, cell=0.25) == PP.voxel_grid((0, 0, 0), (1, 1, 1), 0.25)
    assert PP._knn_grid((0, 0, 0), (1e3, 1e3, 1e3), 100, 8, cell=0.25)[1] == (1.0, 1.0, 1.0)

    class Vae:
        def __getattr__(self, name):
            raise AssertionError("the autoencoder was touched")
    ns = lambda **kw: type("NS", (), kw)()
    args = ns(dataset=ns(lidar=ns(pc_range=[0, -90, -20, 15.8, 90, 20], view_cone_mode=True)))
    for fn in (E.infer_point_clouds, E.infer_point_clouds_device):
        for stat in (8, (8,), (8, 2.0), (8, 2.0, 0.5, 1.0, 3), (0, 2.0, 0.5), (33, 2.0, 0.5), (float("inf"), 2.0, 0.5), (float("nan"), 2.0, 0.5), (2.5, 2.0, 0.5), (True, 2.0, 0.5), (8, -1.0, 0.5),
                     (8, float("nan"), 0.5), (8, 2.0, 0), (8, 2.0, float("inf")), (8, 2.0, "c"), (8, 2.0, 1e-3), (8, 2.0, 0.5, 0), (8, 2.0, 0.5, -1.0),
                     (8, 2.0, 0.5, float("nan")), "fine"):                   # 1e-3: (31.6 / 1e-3)^3 cells
            with pytest.raises(ValueError):
                fn(Vae(), torch.zeros(2, 128, 32), args, denoise_statistical=stat)
        with pytest.raises(ValueError, match="exclude"):
            fn(Vae(), torch.zeros(2, 128, 32), args, denoise=(0.5, 2), denoise_statistical=(8, 2.0, 0.5))
        with pytest.raises(ValueError):
            fn(Vae(), torch.zeros(2, 128, 32), args, denoise=(0.1, 2, 3))    # `denoise` keeps its refusals
    assert E._check_denoise_statistical(None, None, args) is None and E._check_denoise_statistical(None, (0.5, 2), args) is None
    assert E._check_denoise_statistical((8, 2, 0.5), None, args) == ("statistical", 8, 2.0, PP.voxel_grid([-15.8] * 3, [15.8] * 3, 0.5), None)
    args.dataset.lidar.view_cone_mode = False
    assert E._check_denoise_statistical((8.0, 2.5, 0.5, 1.5), None, args) == ("statistical", 8, 2.5, PP.voxel_grid([0, -90, -20], [15.8, 90, 20], 0.5),
                                                                             1.5)


# ---- the tail ------------------------------------------------------------------------------------------------------------------------------
def _stub_statistical(monkeypatch):
    from rald_amd import postprocess as real
    from test_radius_filter_host import _stub_denoise
    E, calls, reads, pos, kw, seen = _stub_denoise(monkeypatch)

    def statistical(pts, off, k, std_ratio, grid, max_per_sample, max_radius=None, return_index=False, return_stats=False):
        calls.append("remove_statistical_outliers_ragged")
        seen.update(s_pts=pts, s_off=off, s_args=(k, std_ratio, max_per_sample, max_radius, return_index, return_stats), s_grid=grid)
        seen["denoised"] = torch.full((pts.shape[0], 3), 3.0)
        return (seen["denoised"], torch.tensor([0, 4, 6]), torch.arange(pts.shape[0]) * 2,
                torch.tensor([[0.5, 0.25, 1.0], [float("nan")] * 3], dtype=torch.float64))
    E.PP.remove_statistical_outliers_ragged = statistical
    E.PP._knn_k, E.PP._knn_ratio, E.PP._knn_radius = real._knn_k, real._knn_ratio, real._knn_radius
    return E, calls, reads, pos, kw, seen


def test_infer_point_clouds_without_denoise_statistical_is_what_it_was(monkeypatch):
    from test_cloud_metrics_host import TAIL
    E, calls, reads, pos, kw, seen = _stub_statistical(monkeypatch)
    out = E.infer_point_clouds(*pos, **kw)
    assert calls == TAIL + ["cal_metrics_ragged"] and len(reads) == 1 and set(out) == {"pred", "cd", "n_queries"}
    del calls[:], reads[:]
    out = E.infer_point_clouds(*pos, denoise=(0.5, 2), thin=4.0, resample=5, **kw)
    assert calls == TAIL + ["cal_metrics_ragged", "remove_radius_outliers_ragged", "cal_metrics_ragged", "voxel_downsample_ragged",
                            "resample_points_ragged"] and len(reads) == 1
    assert set(out) == {"pred", "cd", "n_queries", "denoised", "denoise_index", "cd_denoised", "thinned", "thin_count", "thin_first", "resampled",
                        "resample_index"}
    del calls[:], reads[:]
    assert len(E.infer_point_clouds_device(*pos, **kw)) == 3 and len(E.infer_point_clouds_device(*pos, denoise=(0.5, 2), thin=4.0, resample=5, **kw)) == 13
    assert "remove_statistical_outliers_ragged" not in calls and "s_grid" not in seen and not reads
    with pytest.raises(ValueError):
        E.infer_point_clouds(*pos, denoise=(0.5, 2), denoise_statistical=(8, 2.0, 0.5), **kw)
    assert "remove_statistical_outliers_ragged" not in calls


def test_infer_point_clouds_with_denoise_statistical(monkeypatch):
    from test_cloud_metrics_host import TAIL
    E, calls, reads, pos, kw, seen = _stub_statistical(monkeypatch)
    base = E.infer_point_clouds(*pos, **kw)
    del calls[:], reads[:]
    out = E.infer_point_clouds(*pos, denoise_statistical=(8, 2.0, 0.5), **kw)
    # the filter after the metric of the full cloud, then the metric of the denoised one; still one host read
    assert calls == TAIL + ["cal_metrics_ragged", "remove_statistical_outliers_ragged", "cal_metrics_ragged"] and len(reads) == 1
    assert set(out) == {"pred", "cd", "n_queries", "denoised", "denoise_index", "cd_denoised", "denoise_stats"}
    assert out["cd"] == base["cd"] and out["n_queries"] == base["n_queries"] and [p.shape[0] for p in out["pred"]] == [7, 5]
    assert [t.shape[0] for t in out["denoised"]] == [4, 2] and out["denoise_index"][1].tolist() == [8, 10] and out["cd_denoised"] == [1.5, 2.5]
    assert out["denoise_stats"][0] == (0.5, 0.25, 1.0) and all(math.isnan(v) for v in out["denoise_stats"][1]) and len(out["denoise_stats"]) == 2
    assert seen["s_off"].tolist() == [0, 7, 12] and seen["s_args"] == (8, 2.0, 50, None, True, True)
    assert seen["s_grid"] == E.PP.voxel_grid([-15.8] * 3, [15.8] * 3, 0.5)
    E.infer_point_clouds(*pos, denoise_statistical=(8, 2.0, 0.5, 1.25), **kw)
    assert seen["s_args"] == (8, 2.0, 50, 1.25, True, True)
    # with the metrics in the same host read: each set is unpacked from its own place, the statistics behind them
    m = E.infer_point_clouds(*pos, denoise_statistical=(8, 2.0, 0.5), metric_thresholds=(0.1, 0.2), **kw)
    ref = E.infer_point_clouds(*pos, metric_thresholds=(0.1, 0.2), **kw)
    assert m["metrics"] == ref["metrics"] and m["metrics_denoised"] == ref["metrics"] and m["cd_denoised"] == ref["cd"] == m["cd"]
    assert m["denoise_stats"][0] == (0.5, 0.25, 1.0)
    out = E.infer_point_clouds(*pos, denoise_statistical=(8, 2.0, 0.5), **{**kw, "surfaces": None})
    assert out["cd"] is None and "cd_denoised" not in out and out["denoise_stats"][0] == (0.5, 0.25, 1.0)
    # thin and resample run on the denoised clouds
    del calls[:], reads[:]
    out = E.infer_point_clouds(*pos, denoise_statistical=(8, 2.0, 0.5), thin=4.0, resample=5, metric_thresholds=(0.1,), **kw)
    assert calls == TAIL + ["cloud_metrics_ragged", "remove_statistical_outliers_ragged", "cloud_metrics_ragged", "voxel_downsample_ragged",
                            "resample_points_ragged"] and len(reads) == 1
    assert seen["t_pts"] is seen["denoised"] and seen["t_off"].tolist() == [0, 4, 6] and seen["r_pts"] is seen["thinned"]
    assert [t.shape[0] for t in out["thinned"]] == [3, 2] and out["denoise_stats"][0] == (0.5, 0.25, 1.0)
    assert out["metrics_denoised"][1]["accuracy"] == 2.5
    del calls[:], reads[:]
    dev = E.infer_point_clouds_device(*pos, denoise_statistical=(8, 2.0, 0.5), thin=4.0, resample=5, **kw)
    assert len(dev) == 14 and dev[3] is seen["denoised"] and dev[4].tolist() == [0, 4, 6] and dev[6].tolist() == [1.5, 2.5]
    assert dev[7].shape == (2, 3) and dev[8] is seen["thinned"] and not reads
    assert len(E.infer_point_clouds_device(*pos, denoise_statistical=(8, 2.0, 0.5), metric_thresholds=(), **kw)) == 10
