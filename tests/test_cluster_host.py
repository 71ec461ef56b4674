"""Density clustering and small-cluster removal, host side (no GPU): the brute-force reference of tests/cluster_ref.py against its
independent route (the grid walk's cells and label propagation) on every construction the GPU tests use; that each construction tells
a wrong kernel from a right one (asserted on the reference alone); the reference on planted cases; the C entries' declarations, scratch
sizes and every refusal (through the built library, before any GPU work); the Python layer's and the tail's argument errors; and,
with the device functions stubbed, that infer_point_clouds does what it did before when `denoise_cluster` is left alone, and what it
should with it."""
import ctypes as C

import numpy as np
import pytest
import torch

import cluster_ref as REF
import radius_ref

F32 = np.float32


# ---- the reference -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,min_points", REF.CASE_IDS)
def test_reference_agrees_with_the_walk_and_propagation(name, min_points):
    a, b = REF.reference(name, min_points), REF.cluster_walk(name, min_points)
    assert 1400 <= len(REF.cloud(name)[0]) <= 3000 or name == "faces"
    assert a["num_clusters"] == b["num_clusters"]
    for k in ("labels", "sizes", "count"):
        assert np.array_equal(a[k], b[k]), k
    lab, C_ = a["labels"], a["num_clusters"]
    assert lab.max() == C_ - 1 and a["sizes"][:C_].sum() == (lab >= 0).sum() and (a["sizes"][:C_] > 0).all() and not a["sizes"][C_:].any()
    first = [int(np.nonzero((lab == c) & a["core"])[0][0]) for c in range(C_)]          # numbered by the smallest core row, ascending
    assert first == sorted(first)


@pytest.mark.parametrize("name", sorted(radius_ref.CONSTRUCTIONS))
def test_radius_constructions_have_clusters_border_and_noise(name):
    a = REF.reference(name, 4)
    lab = a["labels"]
    assert a["num_clusters"] >= 2 and ((lab >= 0) & ~a["core"]).sum() >= 1 and (lab == -1).sum() >= 1


def test_the_new_constructions_are_not_vacuous():
    for order in ("ascending", "descending", "shuffled"):
        a = REF.reference("chain_" + order, 2)
        p = REF.cloud("chain_" + order)[0]
        ends = np.nonzero((p[:, 0] == 0) | (p[:, 0] == p[:, 0].max()))[0]
        assert a["num_clusters"] == 1 and (a["labels"] == 0).all() and len(p) == 2500 > 2 * 1024        # many workgroups, three sort chunks
        assert sorted(np.nonzero(~a["core"])[0].tolist()) == sorted(ends.tolist()) and a["count"].max() == 2
    assert REF.cloud("chain_descending")[0][0, 0] > REF.cloud("chain_descending")[0][1, 0]
    # the two lines stay apart, though one ulp less of a gap would merge them
    a = REF.reference("two_chains", 0)
    p, grid, eps = REF.cloud("two_chains")
    assert a["num_clusters"] == 2 and sorted(a["sizes"][:2].tolist()) == [1250, 1250]
    assert (a["labels"][p[:, 1] == 0] == a["labels"][p[:, 1] == 0][0]).all()
    q = p.copy()
    q[:, 1] = np.where(q[:, 1] > 0, F32(eps), F32(0))
    assert REF.cluster_one(q, grid, eps, 0)["num_clusters"] == 1
    # equal distances to core rows of two clusters: the smaller row index wins, and the other rule gives other labels
    a = REF.reference("border_tie", 4)
    p, grid, eps = REF.cloud("border_tie")
    b = REF.cluster_one(p, grid, eps, 4, tie="largest")
    border = np.nonzero((a["labels"] >= 0) & ~a["core"])[0]
    assert len(border) == 100 and a["num_clusters"] == 200 and (a["labels"][border] != b["labels"][border]).all()
    sizes = a["sizes"][:200]
    assert set(sizes.tolist()) == {7, 8} and not np.array_equal(a["sizes"], b["sizes"])
    # the clique at the cap, and one above it
    assert REF.reference("clique", 1499)["num_clusters"] == 1 and (REF.reference("clique", 1499)["count"] == 1499).all()
    assert REF.reference("clique", 1500)["num_clusters"] == 0 and (REF.reference("clique", 1500)["labels"] == -1).all()
    # more clusters than one block of the numbering scan holds
    assert REF.reference("many", 0)["num_clusters"] > 1024 and REF.reference("many", 0)["sizes"].max() >= 2


def test_reference_on_planted_cases():
    grid = radius_ref.cube_grid(0.0, 2.0, 0.125)
    e = 0.125
    # rows 0 .. 3 on a line (0.25 .. 0.625), row 4 a duplicate of row 1, row 5 far away, rows 6 .. 8 outside, row 9 beside row 3
    p = np.array([[0.25, 0.5, 0.5], [0.375, 0.5, 0.5], [0.5, 0.5, 0.5], [0.625, 0.5, 0.5], [0.375, 0.5, 0.5], [1.5, 1.5, 1.5],
                  [np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [-0.01, 0.5, 0.5], [0.75, 0.5, 0.5]], F32)
    a = REF.cluster_one(p, grid, e, 0)
    assert a["labels"].tolist() == [0, 0, 0, 0, 0, 1, -2, -2, -2, 0] and a["num_clusters"] == 2 and a["sizes"][:3].tolist() == [6, 1, 0]
    assert a["count"].tolist() == [0] * 6 + [-1] * 3 + [0]
    a = REF.cluster_one(p, grid, e, 2)                                        # counts 2 3 3 2 3 0 . . . 1: row 9 is a border row
    assert a["count"].tolist() == [2, 2, 2, 2, 2, 0, -1, -1, -1, 1] and a["core"].tolist() == [True] * 5 + [False] * 5
    assert a["labels"].tolist() == [0, 0, 0, 0, 0, -1, -2, -2, -2, 0] and a["sizes"][:2].tolist() == [6, 0]
    a = REF.cluster_one(p, grid, e, 3)                                        # core: 1, 2, 4; border: 0 (-> 1), 3 (-> 2); 9 is noise
    assert a["core"].tolist() == [False, True, True, False, True] + [False] * 5
    assert a["labels"].tolist() == [0, 0, 0, 0, 0, -1, -2, -2, -2, -1]
    f = REF.filter_ragged(p, [0, 10], grid, e, 0, 2, 100)
    assert f["index"].tolist() == [0, 1, 2, 3, 4, 9] and f["labels"].tolist() == [0] * 6 and f["num_clusters"].tolist() == [2]
    f = REF.filter_ragged(p[::-1].copy(), [0, 10], grid, e, 0, 1, 100, largest_only=True)
    assert f["index"].tolist() == [0, 5, 6, 7, 8, 9] and f["labels"].tolist() == [0] * 6          # row 0 (was 9) names cluster 0 now
    f = REF.filter_ragged(p, [0, 10], grid, e, 0, 7, 100)
    assert f["offsets"].tolist() == [0, 0] and f["num_clusters"].tolist() == [2]
    # equal sizes: the smaller id is the largest cluster
    q = np.array([[1.5, 1.5, 1.5], [0.25, 0.5, 0.5], [1.5, 1.5, 1.625], [0.375, 0.5, 0.5]], F32)
    f = REF.filter_ragged(q, [0, 4], grid, e, 0, 1, 4, largest_only=True)
    assert f["index"].tolist() == [0, 2] and f["labels"].tolist() == [0, 0]
    # ragged: counts and the bound trim, an empty cloud; a cloud equals the same cloud alone
    g = REF.cluster_ragged(p, [0, 6, 6, 10], grid, e, 0, 4, counts=[5, 3, 9])
    alone = REF.cluster_one(p[:4], grid, e, 0)
    assert np.array_equal(g["labels"][:4], alone["labels"]) and g["num_clusters"].tolist() == [1, 0, 1]
    assert g["untouched"].tolist() == [False] * 4 + [True] * 2 + [False] * 4


# ---- the C entries -------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entries():
    from rald_amd import _lib
    P, I32, I64, F = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    head = [P, P, P, I32, I64, I64, I64, P, P, P, F, I32]
    assert _lib.SIGNATURES["rald_post_cluster_scratch_bytes"] == (I64, [I32, I64, I64])
    assert _lib.SIGNATURES["rald_op_cluster_scratch_bytes"] == (I64, [I32, I64, I64, I64])
    assert _lib.SIGNATURES["rald_post_cluster_labels_ragged"] == (I32, head + [P, P, P, P, P, I64, P])
    assert _lib.SIGNATURES["rald_op_cluster_labels_ragged"] == (I32, head + [P, P, P, P, P, I64, I64, P])
    assert _lib.SIGNATURES["rald_post_cluster_filter_ragged"] == (I32, head + [I32, I32, P, P, P, P, P, P, I64, P])
    assert _lib.SIGNATURES["rald_op_cluster_filter_ragged"] == (I32, head + [I32, I32, P, P, P, P, P, P, I64, I64, P])


def test_scratch_bytes():
    from rald_amd._lib import lib
    L = lib()
    q, qo, qr = L.rald_post_cluster_scratch_bytes, L.rald_op_cluster_scratch_bytes, L.rald_post_radius_scratch_bytes
    assert q(1, 1, 1) > 0 and q(1, 0, 1) > 0
    sizes = [q(1, 1000, 1000), q(1, 5000, 1000), q(1, 5000, 5000), q(3, 5000, 5000), q(3, 480000, 480000), q(64, 1 << 21, 1 << 21),
             q(64, 1 << 25, 1 << 24)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])) and all(s % 16 == 0 for s in sizes)
    assert q(3, 480000, 480000) >= qr(3, 480000, 480000) + 20 * 480000                  # the parents, the roots, the labels, the sizes ...
    assert qo(2, 70000, 70000, 0) == q(2, 70000, 70000) and qo(2, 70000, 70000, 1024) > qo(2, 70000, 70000, 4096)
    for args in ((0, 10, 10), (65536, 10, 10), (1, -1, 10), (1, 1 << 31, 10), (1, 10, 0), (1, 10, (1 << 24) + 1)):
        assert q(*args) == -1 and b"rald_post_cluster_scratch_bytes" in L.rald_last_error(), args
    for chunk in (-1024, 1, 1000, 1025):
        assert qo(1, 10, 10, chunk) == -1 and b"rald_op_cluster_scratch_bytes" in L.rald_last_error()


def test_every_refusal_comes_before_any_gpu_work():
    """Host buffers stand in for device memory: a refused call touches none of them and launches nothing."""
    from rald_amd._lib import lib
    L = lib()
    pts, out, off = (C.c_float * 64)(), (C.c_float * 64)(), (C.c_int64 * 4)()
    lab, num, sizes, cnt, idx = (C.c_int32 * 16)(), (C.c_int32 * 4)(), (C.c_int32 * 16)(), (C.c_int32 * 16)(), (C.c_int64 * 16)()
    need = L.rald_op_cluster_scratch_bytes(1, 4, 4, 0)
    scratch = (C.c_char * (need + 64))()
    base = C.addressof(scratch)
    aligned = base + (-base) % 16
    f3, i3 = lambda *v: (C.c_float * 3)(*v), lambda *v: (C.c_int32 * 3)(*v)
    inf, nan = float("inf"), float("nan")
    layout = dict(points=pts, offsets=None, counts=None, batch=1, n_dense=4, n_total=4, max_per_sample=4, lo=f3(0, 0, 0), v=f3(1, 1, 1),
                  dims=i3(4, 4, 4), eps=0.5, min_points=2)
    tail = dict(scratch=aligned, scratch_bytes=need, chunk=0, stream=None)
    labels_ok = {**layout, **dict(out_labels=lab, out_num_clusters=num, out_sizes=sizes, out_count=cnt), **tail}
    filter_ok = {**layout, **dict(min_cluster_size=2, largest_only=0, out_points=out, out_offsets=off, out_index=idx, out_labels=lab,
                                  out_num_clusters=num), **tail}
    shared = [(dict(points=None), b"null pointer"), (dict(out_labels=None), b"null pointer"), (dict(out_num_clusters=None), b"null pointer"),
              (dict(min_points=-1), b"min_points must be >= 0"),
              (dict(lo=None), b"null grid"), (dict(v=None), b"null grid"), (dict(dims=None), b"null grid"),
              (dict(eps=0.0), b"eps must be finite and > 0"), (dict(eps=-0.5), b"eps must be finite and > 0"),
              (dict(eps=nan), b"eps must be finite and > 0"), (dict(eps=inf), b"eps must be finite and > 0"),
              (dict(eps=nan, dims=i3(4, 0, 4)), b"eps must be finite and > 0"),                          # eps first, then the grid
              (dict(v=f3(0.4, 1, 1)), b"cell edge must be >= eps"), (dict(v=f3(1, 0.4, 1)), b"cell edge must be >= eps"),
              (dict(v=f3(1, 1, 0.4999)), b"cell edge must be >= eps"), (dict(v=f3(1, nan, 1)), b"cell edge must be >= eps"),
              (dict(v=f3(1, 1, inf)), b"cell edge must be finite"), (dict(lo=f3(0, nan, 0)), b"lo must be finite"),
              (dict(batch=0), b"batch must be 1 .. 65535"), (dict(batch=65536), b"batch must be 1 .. 65535"),
              (dict(n_dense=-1), b"n_dense must be >= 0"), (dict(n_total=-1), b"n_total must be"), (dict(n_total=1 << 31), b"n_total must be"),
              (dict(max_per_sample=0), b"max_per_sample must be 1 .. 16777216"), (dict(max_per_sample=(1 << 24) + 1), b"max_per_sample must be"),
              (dict(dims=i3(4, 0, 4)), b"every dim must be >= 1"), (dict(dims=i3(1291, 1290, 1290)), b"at most 2^31 - 1 cells"),
              (dict(scratch_bytes=need - 1), b"scratch too small"), (dict(max_per_sample=1 << 21), b"scratch too small"),
              (dict(scratch=None), b"null or unaligned scratch"), (dict(scratch=aligned + 4), b"null or unaligned scratch"),
              (dict(chunk=1000), b"multiple of 1024"), (dict(chunk=-1024), b"multiple of 1024"), (dict(chunk=1), b"multiple of 1024")]
    filter_only = [(dict(out_points=None), b"null pointer"), (dict(out_offsets=None), b"null pointer"),
                   (dict(min_cluster_size=0), b"min_cluster_size must be >= 1"), (dict(min_cluster_size=-3), b"min_cluster_size must be >= 1")]
    for ok, op, post, who, cases in ((labels_ok, L.rald_op_cluster_labels_ragged, L.rald_post_cluster_labels_ragged, b"cluster_labels_ragged",
                                      shared),
                                     (filter_ok, L.rald_op_cluster_filter_ragged, L.rald_post_cluster_filter_ragged, b"cluster_filter_ragged",
                                      shared + filter_only)):
        for change, message in cases:
            a = {**ok, **change}
            assert op(*a.values()) == 1, change
            assert message in L.rald_last_error() and who in L.rald_last_error(), (change, L.rald_last_error())
            if "chunk" not in change:
                del a["chunk"]
                assert post(*a.values()) == 1, change
                assert message in L.rald_last_error(), (change, L.rald_last_error())
    assert not any(lab) and not any(num) and not any(sizes) and not any(cnt) and not any(out) and not any(off) and not any(idx)


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_raise_before_the_library_is_touched(monkeypatch):
    from rald_amd import engine_generation as E, postprocess as PP
    from test_fps_host import _no_library
    _no_library(monkeypatch)
    pts, off = torch.zeros(10, 3), torch.tensor([0, 4, 10])
    grid = PP.voxel_grid((0, 0, 0), (1, 1, 1), 0.5)
    ok = dict(points=pts, offsets=off, eps=0.5, min_points=2, grid=grid, max_per_sample=6)
    bad = [dict(points=torch.zeros(10, 2)), dict(points=torch.zeros(10, 3, dtype=torch.int64)), dict(offsets=torch.tensor([0.0, 4.0, 10.0])),
           dict(offsets=[0, 4, 10]), dict(max_per_sample=0), dict(max_per_sample=(1 << 24) + 1), dict(max_per_sample=True),
           dict(counts=torch.tensor([4, 6])), dict(counts=torch.tensor([4, 6, 1], dtype=torch.int32)), dict(grid=None),
           dict(grid=(grid[0], (0.5, 0.0, 0.5), grid[2])), dict(grid=(grid[0], grid[1], (1291, 1290, 1290))), dict(chunk=1000),
           dict(eps=0), dict(eps=-1.0), dict(eps=float("nan")), dict(eps=float("inf")), dict(eps="wide"), dict(eps=True),
           dict(eps=1e-60), dict(eps=1e60), dict(eps=0.6), dict(grid=(grid[0], (0.5, 0.25, 0.5), grid[2])),
           dict(min_points=-1), dict(min_points=1.5), dict(min_points=True), dict(min_points=1 << 31)]
    for kw in bad:
        with pytest.raises(ValueError):
            PP.cluster_dbscan_ragged(**{**ok, **kw})
        with pytest.raises(ValueError):
            PP.remove_small_clusters_ragged(**{**ok, "min_cluster_size": 2, **kw})
    for k in (0, -1, 1.5, True, None, "big", 1 << 31):
        with pytest.raises(ValueError):
            PP.remove_small_clusters_ragged(**{**ok, "min_cluster_size": k})
    one = dict(eps=0.5, min_points=1)
    for points, kw in ((torch.zeros(2, 5, 3), {}), (torch.zeros(5, 2), {}), (torch.zeros(5, 3), dict(eps=0)), (torch.zeros(5, 3), dict(min_points=-1)),
                       (torch.zeros(5, 3), dict(min_points=0.5)), (torch.zeros(5, 3), dict(lo=(0, 0, 0))), (torch.zeros(5, 3, dtype=torch.int32), {}),
                       (torch.zeros(5, 3), dict(eps=float("nan"))), (torch.zeros(5, 3), dict(hi=(1, 1, 1)))):
        with pytest.raises(ValueError):
            PP.cluster_dbscan(points, **{**one, **kw})
        with pytest.raises(ValueError):
            PP.remove_small_clusters(points, **{**one, "min_cluster_size": 1, **kw})
    with pytest.raises(ValueError):
        PP.remove_small_clusters(torch.zeros(5, 3), 0.5, 1, 0)
    assert PP.remove_small_clusters(torch.zeros(0, 3), 0.5, 1, 1).shape == (0, 3)
    assert PP.cluster_dbscan(torch.zeros(0, 3), 0.5, 1).shape == (0,) and PP.cluster_dbscan(torch.zeros(0, 3), 0.5, 1).dtype == torch.int32

    class Vae:
        def __getattr__(self, name):
            raise AssertionError("the autoencoder was touched")
    ns = lambda **kw: type("NS", (), kw)()
    args = ns(dataset=ns(lidar=ns(pc_range=[0, -90, -20, 15.8, 90, 20], view_cone_mode=True)))
    for fn in (E.infer_point_clouds, E.infer_point_clouds_device):
        for clu in (0.1, (0.1,), (0.1, 2), (0.1, 2, 3, True, 5), (0, 2, 3), (-0.1, 2, 3), (float("nan"), 2, 3), (0.1, -1, 3), (0.1, 1.5, 3),
                    (0.1, True, 3), (0.1, 2, 0), (0.1, 2, 1.5), (0.1, 2, True), (0.1, 2, 3, "yes"), ("r", 2, 3), (1e-3, 2, 3), "fine"):
            with pytest.raises(ValueError):
                fn(Vae(), torch.zeros(2, 128, 32), args, denoise_cluster=clu)
        with pytest.raises(ValueError, match="excludes"):
            fn(Vae(), torch.zeros(2, 128, 32), args, denoise_cluster=(0.5, 2, 3), denoise=(0.5, 2))
        with pytest.raises(ValueError, match="excludes"):
            fn(Vae(), torch.zeros(2, 128, 32), args, denoise_cluster=(0.5, 2, 3), denoise_statistical=(8, 1.0, 0.5))
    assert E._check_denoise_cluster(None, None, None, args) is None
    g = PP.voxel_grid([-15.8] * 3, [15.8] * 3, 0.5)
    assert E._check_denoise_cluster((0.5, 0, 3), None, None, args) == ("cluster", 0.5, 0, 3, False, g)
    assert E._check_denoise_cluster((0.5, 4.0, 30, True), None, None, args) == ("cluster", 0.5, 4, 30, True, g)


# ---- the tail ------------------------------------------------------------------------------------------------------------------------------
def _stub_cluster(monkeypatch):
    from rald_amd import postprocess as PP
    from test_radius_filter_host import _stub_denoise
    real_size = PP._cluster_size
    E, calls, reads, pos, kw, seen = _stub_denoise(monkeypatch)
    E.PP._cluster_size = real_size

    def cluster(pts, off, eps, min_points, min_cluster_size, grid, max_per_sample, largest_only=False, return_index=False,
                return_labels=False):
        calls.append("remove_small_clusters_ragged")
        seen.update(c_pts=pts, c_off=off, c_args=(eps, min_points, min_cluster_size, max_per_sample, largest_only, return_index, return_labels),
                    c_grid=grid)
        seen["denoised"] = torch.full((pts.shape[0], 3), 3.0)
        seen["c_labels"] = torch.arange(pts.shape[0], dtype=torch.int32) % 3
        return seen["denoised"], torch.tensor([0, 4, 6]), torch.arange(pts.shape[0]) * 2, seen["c_labels"], torch.tensor([5, 9], dtype=torch.int32)
    E.PP.remove_small_clusters_ragged = cluster
    return E, calls, reads, pos, kw, seen


def test_infer_point_clouds_without_denoise_cluster_is_what_it_was(monkeypatch):
    from test_cloud_metrics_host import TAIL
    E, calls, reads, pos, kw, seen = _stub_cluster(monkeypatch)
    out = E.infer_point_clouds(*pos, **kw)
    assert calls == TAIL + ["cal_metrics_ragged"] and len(reads) == 1 and set(out) == {"pred", "cd", "n_queries"}
    del calls[:], reads[:]
    out = E.infer_point_clouds(*pos, denoise=(0.5, 2), **kw)
    assert calls == TAIL + ["cal_metrics_ragged", "remove_radius_outliers_ragged", "cal_metrics_ragged"] and len(reads) == 1
    assert set(out) == {"pred", "cd", "n_queries", "denoised", "denoise_index", "cd_denoised"}
    assert len(E.infer_point_clouds_device(*pos, **kw)) == 3 and len(E.infer_point_clouds_device(*pos, denoise=(0.5, 2), **kw)) == 7
    assert "remove_small_clusters_ragged" not in calls and "c_grid" not in seen


def test_infer_point_clouds_with_denoise_cluster(monkeypatch):
    from test_cloud_metrics_host import TAIL
    E, calls, reads, pos, kw, seen = _stub_cluster(monkeypatch)
    base = E.infer_point_clouds(*pos, **kw)
    del calls[:], reads[:]
    out = E.infer_point_clouds(*pos, denoise_cluster=(0.5, 2, 30), **kw)
    # the filter after the metric of the full cloud, then the metric of the denoised one; still one host read
    assert calls == TAIL + ["cal_metrics_ragged", "remove_small_clusters_ragged", "cal_metrics_ragged"] and len(reads) == 1
    assert set(out) == {"pred", "cd", "n_queries", "denoised", "denoise_index", "cd_denoised", "denoise_labels", "n_clusters"}
    assert out["cd"] == base["cd"] and out["n_queries"] == base["n_queries"] and [p.shape[0] for p in out["pred"]] == [7, 5]
    assert [t.shape[0] for t in out["denoised"]] == [4, 2] and out["denoise_index"][1].tolist() == [8, 10] and out["cd_denoised"] == [1.5, 2.5]
    assert out["n_clusters"] == [5, 9] and [t.tolist() for t in out["denoise_labels"]] == [[0, 1, 2, 0], [1, 2]]
    assert out["denoise_labels"][0].dtype == torch.int32
    assert seen["c_off"].tolist() == [0, 7, 12] and seen["c_args"] == (0.5, 2, 30, 50, False, True, True)
    assert seen["c_grid"] == E.PP.voxel_grid([-15.8] * 3, [15.8] * 3, 0.5)
    E.infer_point_clouds(*pos, denoise_cluster=(0.5, 0, 1, True), **kw)
    assert seen["c_args"] == (0.5, 0, 1, 50, True, True, True)
    # with the metrics in the same host read: each set is unpacked from its own place
    m = E.infer_point_clouds(*pos, denoise_cluster=(0.5, 2, 30), metric_thresholds=(0.1, 0.2), **kw)
    ref = E.infer_point_clouds(*pos, metric_thresholds=(0.1, 0.2), **kw)
    assert m["metrics"] == ref["metrics"] and m["metrics_denoised"] == ref["metrics"] and m["cd_denoised"] == ref["cd"] == m["cd"]
    assert m["n_clusters"] == [5, 9] and [t.shape[0] for t in m["denoised"]] == [4, 2]
    # no surfaces: no metric of either kind, no key for it
    out = E.infer_point_clouds(*pos, denoise_cluster=(0.5, 2, 30), **{**kw, "surfaces": None})
    assert out["cd"] is None and "cd_denoised" not in out and out["n_clusters"] == [5, 9]
    # thin and resample run on the denoised clouds
    del calls[:], reads[:]
    out = E.infer_point_clouds(*pos, denoise_cluster=(0.5, 2, 30), thin=4.0, resample=5, metric_thresholds=(0.1,), **kw)
    assert calls == TAIL + ["cloud_metrics_ragged", "remove_small_clusters_ragged", "cloud_metrics_ragged", "voxel_downsample_ragged",
                            "resample_points_ragged"] and len(reads) == 1
    assert seen["t_pts"] is seen["denoised"] and seen["t_off"].tolist() == [0, 4, 6] and seen["r_pts"] is seen["thinned"]
    assert [t.shape[0] for t in out["thinned"]] == [3, 2] and out["n_clusters"] == [5, 9]
    del calls[:], reads[:]
    dev = E.infer_point_clouds_device(*pos, denoise_cluster=(0.5, 2, 30), thin=4.0, resample=5, **kw)
    assert len(dev) == 15 and dev[3] is seen["denoised"] and dev[4].tolist() == [0, 4, 6] and dev[6].tolist() == [1.5, 2.5]
    assert dev[7] is seen["c_labels"] and dev[8].tolist() == [5, 9] and dev[9] is seen["thinned"] and not reads
