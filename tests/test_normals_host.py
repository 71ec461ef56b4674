"""PCA normals and normal consistency, host side (no GPU): the reference of tests/normals_ref.py against numpy.linalg.eigh in float64,
its neighbourhoods against scipy's k-d tree, the reference on planted cases, the consistency against a direct loop; the C entries'
declarations, scratch sizes and every refusal (through the built library, before any GPU work); the Python layer's argument errors;
and, with the device functions stubbed, that infer_point_clouds does what it did before when `normal_consistency` is left alone, and
what it should with it."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import knn_ref as KREF
import normals_ref as REF
import radius_ref as RREF

F32 = np.float32
F64 = np.float64


# ---- the reference against eigh ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(REF.HOST_CLOUDS))
def test_reference_against_eigh(name):
    """Six fixed sweeps against numpy.linalg.eigh on the reference's own float64 moments, k = 16: rows with (l1 - l0) / l2 >= 1e-3 (the
    rest, where the smallest eigenvector is not determined, at most 2 %): the fp32 normal within sin(angle) <= 1e-6 (fp32 rounding of a
    unit vector is about 1.1e-7), every eigenvalue within 2^-23 |l| + 1e-12 l2, and the off-diagonals left are exactly 0."""
    p = REF.HOST_CLOUDS[name]()
    assert len(p) == (288 if name == "lattice_slab" else 1500)
    r = REF.normals_one(p, REF.box_grid(p, 1.0), 16)
    assert r["defined"].all() and (r["found"] == 16).all() and (r["off"] == 0.0).all()
    m = r["moments"]
    A = np.zeros((len(p), 3, 3), F64)
    A[:, 0, 0], A[:, 0, 1], A[:, 0, 2], A[:, 1, 1], A[:, 1, 2], A[:, 2, 2] = (m[:, e] for e in range(6))
    A = A + np.triu(A, 1).transpose(0, 2, 1)
    w, v = np.linalg.eigh(A)
    take = (w[:, 1] - w[:, 0]) / w[:, 2] >= 1e-3
    sin64 = np.linalg.norm(np.cross(r["vec"], v[:, :, 0]), axis=1)[take].max()
    sin32 = np.linalg.norm(np.cross(r["normals"].astype(F64), v[:, :, 0]), axis=1)[take].max()
    lam_err = (np.abs(r["eigenvalues"].astype(F64) - w) - (2.0 ** -23 * np.abs(w) + 1e-12 * w[:, 2:])).max()
    print(f"{name}: excluded {1 - take.mean():.4%}, sin float64 {sin64:.2e}, sin fp32 {sin32:.2e}, eigenvalues over their bound by {lam_err:.2e}")
    assert 1 - take.mean() <= 0.02 and sin32 <= 1e-6 and lam_err <= 0
    assert (np.diff(r["lam"], axis=1) >= 0).all() and np.abs(np.linalg.norm(r["normals"].astype(F64), axis=1) - 1).max() < 2e-7
    cv = r["lam"][:, 0] / r["lam"].sum(axis=1)
    assert np.allclose(r["curvature"], cv, rtol=1e-6, atol=0) and (r["curvature"] >= 0).all() and (r["curvature"] <= F32(1 / 3) * F32(1.000001)).all()
    # the mean and the moments themselves against numpy on the gathered neighbourhoods
    t = KREF.knn_one(p, REF.box_grid(p, 1.0), 16)
    nb = np.concatenate([p[:, None, :], p[t["idx"]]], axis=1).astype(F64)
    cov = np.einsum("nki,nkj->nij", nb - nb.mean(axis=1, keepdims=True), nb - nb.mean(axis=1, keepdims=True)) / 17.0
    assert np.abs(A - cov).max() <= 1e-12 * max(np.abs(cov).max(), 1.0)


def test_neighbourhoods_against_scipy_kdtree():
    """The neighbourhood of the normals is knn_ref's: scipy's k-d tree in float64 on the same coordinates gives the same index lists
    wherever the fp32 order is not a matter of rounding (section 23's rule: two consecutive squared distances among the first k + 1
    closer than 1e-5 relative leave the row out, at most 2 %)."""
    from scipy.spatial import cKDTree
    p = REF.sphere_shell()
    k = 16
    a = KREF.knn_one(p, REF.box_grid(p, 1.0), k)
    dist, idx = cKDTree(p.astype(F64)).query(p.astype(F64), k=k + 2)
    d2 = dist[:, 1:] ** 2
    close = (np.diff(d2, axis=1) < 1e-5 * d2[:, 1:])[:, :k].any(axis=1)
    assert close.mean() <= 0.02 and np.array_equal(a["idx"][~close], idx[~close, 1:k + 1])


# ---- planted cases ---------------------------------------------------------------------------------------------------------------------------
def _plane():
    g = np.stack(np.meshgrid(np.arange(9), np.arange(9), indexing="ij"), -1).reshape(-1, 2)
    return np.concatenate([g, np.zeros((81, 1))], 1).astype(F32), ((-0.5, -0.5, -0.5), (1.0, 1.0, 1.0), (10, 10, 2))


def test_the_exact_plane_and_its_three_views():
    p, grid = _plane()
    for view, z in (((4.0, 4.0, 5.0), 1.0), ((4.0, 4.0, -5.0), -1.0), ((100.0, -3.0, 0.0), 1.0), (None, 1.0)):
        r = REF.normals_one(p, grid, 8, view=view)
        assert (r["normals"] == np.array([0.0, 0.0, z], F32)).all() and (r["curvature"] == 0).all() and (r["eigenvalues"][:, 0] == 0).all()
        assert not np.signbit(r["normals"][:, :2]).any() or z < 0
    r = REF.normals_one(p, grid, 8, view=(4.0, 4.0, -5.0))
    assert np.signbit(r["normals"][:, 2]).all()


def test_degenerate_neighbourhoods():
    grid = RREF.cube_grid(0.0, 1.0, 0.25)
    same = np.tile(np.array([[0.3, 0.6, 0.9]], F32), (20, 1))
    r = REF.normals_one(same, grid, 5)
    # all rows equal: the moments are 0, no rotation happens, the three eigenvalues tie and the lowest column wins: (1, 0, 0); the sum is 0
    assert (r["normals"] == np.array([1.0, 0.0, 0.0], F32)).all() and (r["curvature"] == 0).all() and (r["eigenvalues"] == 0).all()
    # collinear rows along x: l0 = l1 = 0 with the vectors (0, 1, 0) and (0, 0, 1) in column order; the lower column is the normal
    line = np.zeros((10, 3), F32)
    line[:, 0] = np.arange(10) * 0.0625 + 0.125
    line[:, 1:] = 0.5
    r = REF.normals_one(line, grid, 4)
    assert (r["normals"] == np.array([0.0, 1.0, 0.0], F32)).all() and (r["curvature"] == 0).all() and (r["eigenvalues"][:, 2] > 0).all()
    r = REF.normals_one(line, grid, 4, view=(0.5, -3.0, 0.5))
    assert (r["normals"] == np.array([0.0, -1.0, 0.0], F32)).all()
    # found = 0, 1 and 2, and rows outside: 0 and 1 are undefined, 2 is the smallest defined neighbourhood
    p = np.array([[0.1, 0.1, 0.1], [0.9, 0.9, 0.9], [0.12, 0.1, 0.1], [0.1, 0.13, 0.1], [np.nan, 0.1, 0.1], [2.0, 0.1, 0.1], [0.9, 0.9, 0.88]], F32)
    r = REF.normals_one(p, grid, 4, max_radius=0.05)
    assert r["found"].tolist() == [2, 1, 2, 2, -1, -1, 1]
    und = np.array([False, True, False, False, True, True, True])
    assert (r["normals"][und] == 0).all() and np.isnan(r["curvature"][und]).all() and np.isnan(r["eigenvalues"][und]).all()
    assert (r["normals"][~und] == np.array([0.0, 0.0, 1.0], F32)).all() and (r["curvature"][~und] == 0).all()
    assert REF.normals_one(p[:1], grid, 4)["found"].tolist() == [0] and REF.normals_one(p[:0], grid, 4)["normals"].shape == (0, 3)
    rag = REF.normals_ragged(p, [0, 4, 4, 7], grid, 4, 3, counts=[9, 2, 2], max_radius=0.05)
    assert rag["untouched"].tolist() == [False] * 3 + [True] + [False] * 2 + [True] and rag["found"][:3].tolist() == [1, 0, 1]


def test_sign_rule_without_a_view():
    """The component of the largest magnitude is made positive, the lowest axis on equal magnitudes."""
    p, grid = _plane()
    rot = np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]], F32)                     # the plane y = 0 reached through z -> -y
    q = (p @ rot.T).astype(F32) + np.array([0, 0.25, 0], F32)
    g = ((-0.5, -0.5, -0.5), (1.0, 1.0, 1.0), (10, 2, 10))
    assert (REF.normals_one(q, g, 8)["normals"] == np.array([0.0, 1.0, 0.0], F32)).all()
    diag = np.stack([p[:, 0], p[:, 1], p[:, 0]], 1).astype(F32)                  # the plane x = z: the normal is (1, 0, -1) / sqrt 2 up to sign
    r = REF.normals_one(diag, ((-0.5, -0.5, -0.5), (1.0, 1.0, 1.0), (10, 10, 10)), 8)
    n, vec = r["normals"], r["vec"]
    assert (np.abs(n[:, 0]) == np.abs(n[:, 2])).all() and (n[:, 0] * n[:, 2] < 0).all() and (np.abs(n[:, 1]) < 1e-15).all()
    # the two magnitudes are equal in fp32 but decided in float64, where they may differ in the last place: the first of the largest wins
    big = np.abs(vec).argmax(axis=1)
    assert (vec[np.arange(len(vec)), big] > 0).all() and set(big.tolist()) <= {0, 2}


# ---- normal consistency ----------------------------------------------------------------------------------------------------------------------
def test_consistency_against_a_direct_loop():
    rs = np.random.RandomState(41)
    a, b = rs.uniform(0, 1, (700, 3)).astype(F32), rs.uniform(0, 1, (1300, 3)).astype(F32)
    unit = lambda v: (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)
    na, nb = unit(rs.normal(size=(700, 3))), unit(rs.normal(size=(1300, 3)))
    na[5], nb[7], na[9, 1], nb[11, 0] = 0, 0, np.nan, np.inf
    nc, cnt = REF.consistency_ragged(a, na, [0, 700], b, nb, [0, 1300])

    def loop(x, nx, y, ny):
        total, rows = 0.0, 0
        for i in range(len(x)):
            j = int(((y.astype(F64) - x[i].astype(F64)) ** 2).sum(axis=1).argmin())
            if REF.usable(nx[i:i + 1])[0] and REF.usable(ny[j:j + 1])[0]:
                total += abs(float(np.dot(nx[i].astype(F64), ny[j].astype(F64))))
                rows += 1
        return total / rows, rows
    fwd, bwd = loop(a, na, b, nb), loop(b, nb, a, na)
    assert cnt.tolist() == [[fwd[1], bwd[1]]] and fwd[1] < 700 and bwd[1] < 1300
    assert abs(nc[0, 0] - fwd[0]) <= 1e-13 and abs(nc[0, 1] - bwd[0]) <= 1e-13 and nc[0, 2] == (nc[0, 0] + nc[0, 1]) / 2
    # a cloud against itself: every term is n . n of a unit vector rounded to fp32, within 2^-22 of 1
    same, cs = REF.consistency_ragged(b, unit(rs.normal(size=(1300, 3))), [0, 1300], b, unit(rs.normal(size=(1300, 3))), [0, 1300])
    assert cs.tolist() == [[1300, 1300]] and 0.4 < same[0, 0] < 0.6                              # independent normals: the mean of |cos| is 1/2
    un = unit(rs.normal(size=(1300, 3)))
    one, _ = REF.consistency_ragged(b, un, [0, 1300], b, -un, [0, 1300])
    assert abs(one[0, 0] - 1.0) <= 2.0 ** -22 and abs(one[0, 2] - 1.0) <= 2.0 ** -22
    # a planted pair with known dots: 1, 0, 0.5 -> 0.5; the other direction sees rows 0 and 1 of a twice... each b row its nearest a row
    pa = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], F32)
    pb = np.array([[0, 0.1, 0], [1, 0.1, 0], [2, 0.1, 0], [2, 0.2, 0]], F32)
    qa = np.array([[0, 0, 1], [0, 1, 0], [0.5, 0, 0]], F32)
    qb = np.array([[0, 0, -1], [1, 0, 0], [1, 0, 0], [0, 0, 0]], F32)
    planted, pc = REF.consistency_ragged(pa, qa, [0, 3], pb, qb, [0, 4])
    assert planted[0].tolist() == [0.5, 0.5, 0.5] and pc.tolist() == [[3, 3]]
    # frames without rows on a side, and without a counting row
    e, ec = REF.consistency_ragged(pa, qa, [0, 0, 3], pb, qb, [0, 4, 4])
    assert np.isnan(e).all() and ec.tolist() == [[0, 0], [0, 0]]
    z, zc = REF.consistency_ragged(pa, qa * 0, [0, 3], pb, qb, [0, 4])
    assert np.isnan(z).all() and zc.tolist() == [[0, 0]]


# ---- the C entries -------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entries():
    from rald_amd import _lib
    P, I32, I64, F = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    head = [P, P, P, I32, I64, I64, I64, P, P, P, I32, F, P]
    assert _lib.SIGNATURES["rald_post_normals_scratch_bytes"] == (I64, [I32, I64, I64])
    assert _lib.SIGNATURES["rald_op_normals_scratch_bytes"] == (I64, [I32, I64, I64, I64])
    assert _lib.SIGNATURES["rald_post_normals_ragged"] == (I32, head + [P, P, P, P, P, I64, P])
    assert _lib.SIGNATURES["rald_op_normals_ragged"] == (I32, head + [P, P, P, P, P, I64, I64, P])
    assert _lib.SIGNATURES["rald_post_normal_consistency_scratch_bytes"] == (I64, [I32, I64, I64, I64, I64])
    assert _lib.SIGNATURES["rald_post_normal_consistency_ragged"] == (I32, [P, P, P, I64, P, P, P, I64, I32, I64, I64, P, P, P, I64, P])


def test_scratch_bytes():
    from rald_amd._lib import lib
    L = lib()
    q, qo, qk = L.rald_post_normals_scratch_bytes, L.rald_op_normals_scratch_bytes, L.rald_post_knn_scratch_bytes
    assert q(1, 1, 1) > 0 and q(1, 0, 1) > 0
    sizes = [q(1, 1000, 1000), q(1, 5000, 1000), q(1, 5000, 5000), q(3, 5000, 5000), q(3, 480000, 480000), q(64, 1 << 21, 1 << 21)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])) and all(s % 16 == 0 for s in sizes)
    # the index, then 6 doubles and found per row: the signature carries no k, and no [n_total, k] table fits in 52 bytes a row
    assert qk(3, 480000, 480000) + 52 * 480000 <= q(3, 480000, 480000) <= qk(3, 480000, 480000) + 52 * 480000 + 64
    assert qo(2, 70000, 70000, 0) == q(2, 70000, 70000) and qo(2, 70000, 70000, 1024) > qo(2, 70000, 70000, 4096)
    for args in ((0, 10, 10), (65536, 10, 10), (1, -1, 10), (1, 1 << 31, 10), (1, 10, 0), (1, 10, (1 << 24) + 1)):
        assert q(*args) == -1 and b"rald_post_normals_scratch_bytes" in L.rald_last_error(), args
    for chunk in (-1024, 1, 1000, 1025):
        assert qo(1, 10, 10, chunk) == -1 and b"rald_op_normals_scratch_bytes" in L.rald_last_error()
    c = L.rald_post_normal_consistency_scratch_bytes
    assert c(1, 0, 0, 0, 0) >= 0 and c(2, 5000, 3000, 2500, 1500) > L.rald_post_cloud_metrics_scratch_bytes(2, 2500, 1500) + 8 * 5000
    assert c(2, 5000, 3000, 2500, 1500) % 16 == 0 and c(2, 5000, 3000, 2500, 1500) < c(2, 9000, 3000, 2500, 1500) < c(2, 9000, 3000, 4500, 1500)
    for args in ((0, 1, 1, 1, 1), (65536, 1, 1, 1, 1), (1, -1, 1, 1, 1), (1, 1, 1 << 31, 1, 1), (1, 1, 1, -1, 1), (1, 1, 1, 1, 1 << 31)):
        assert c(*args) == -1 and b"rald_post_normal_consistency_scratch_bytes" in L.rald_last_error(), args


def test_every_refusal_comes_before_any_gpu_work():
    """Host buffers stand in for device memory: a refused call touches none of them and launches nothing."""
    from rald_amd._lib import lib
    L = lib()
    pts, o_n, o_c, o_e, o_f = (C.c_float * 64)(), (C.c_float * 64)(), (C.c_float * 16)(), (C.c_float * 64)(), (C.c_int32 * 16)()
    need = L.rald_op_normals_scratch_bytes(1, 4, 4, 0)
    scratch = (C.c_char * (max(need, L.rald_post_normal_consistency_scratch_bytes(1, 4, 4, 4, 4)) + 64))()
    base = C.addressof(scratch)
    aligned = base + (-base) % 16
    f3, i3 = lambda *v: (C.c_float * 3)(*v), lambda *v: (C.c_int32 * 3)(*v)
    inf, nan = float("inf"), float("nan")
    ok = dict(points=pts, offsets=None, counts=None, batch=1, n_dense=4, n_total=4, max_per_sample=4, lo=f3(0, 0, 0), v=f3(1, 1, 1),
              dims=i3(4, 4, 4), k=2, max_radius=0.0, view=f3(0, 0, 0), out_normals=o_n, out_curvature=o_c, out_eigenvalues=o_e, out_found=o_f,
              scratch=aligned, scratch_bytes=need, chunk=0, stream=None)
    cases = [(dict(points=None), b"null pointer"), (dict(out_normals=None), b"null pointer"), (dict(lo=None), b"null grid"),
             (dict(v=None), b"null grid"), (dict(dims=None), b"null grid"),
             (dict(k=0), b"k must be 1 .. 32"), (dict(k=33), b"k must be 1 .. 32"), (dict(k=-1), b"k must be 1 .. 32"),
             (dict(max_radius=-0.5), b"max_radius must be 0 (none) or finite and > 0"), (dict(max_radius=nan), b"max_radius must be"),
             (dict(max_radius=inf), b"max_radius must be"),
             (dict(view=f3(0, nan, 0)), b"view must be finite"), (dict(view=f3(inf, 0, 0)), b"view must be finite"),
             (dict(view=f3(0, 0, -inf)), b"view must be finite"),
             (dict(v=f3(1, 1, inf)), b"cell edge must be finite"), (dict(v=f3(0, 1, 1)), b"cell edge must be finite"),
             (dict(lo=f3(0, nan, 0)), b"lo must be finite"),
             (dict(batch=0), b"batch must be 1 .. 65535"), (dict(batch=65536), b"batch must be 1 .. 65535"),
             (dict(n_dense=-1), b"n_dense must be >= 0"), (dict(n_total=-1), b"n_total must be"), (dict(n_total=1 << 31), b"n_total must be"),
             (dict(max_per_sample=0), b"max_per_sample must be 1 .. 16777216"), (dict(max_per_sample=(1 << 24) + 1), b"max_per_sample must be"),
             (dict(dims=i3(4, 0, 4)), b"every dim must be >= 1"), (dict(dims=i3(1291, 1290, 1290)), b"at most 2^31 - 1 cells"),
             (dict(scratch_bytes=need - 1), b"scratch too small"), (dict(max_per_sample=1 << 21), b"scratch too small"),
             (dict(scratch=None), b"null or unaligned scratch"), (dict(scratch=aligned + 4), b"null or unaligned scratch"),
             (dict(chunk=1000), b"multiple of 1024"), (dict(chunk=-1024), b"multiple of 1024"), (dict(chunk=1), b"multiple of 1024")]
    for change, message in cases:
        a = {**ok, **change}
        assert L.rald_op_normals_ragged(*a.values()) == 1, change
        assert message in L.rald_last_error() and b"normals_ragged" in L.rald_last_error(), (change, L.rald_last_error())
        if "chunk" not in change:
            del a["chunk"]
            assert L.rald_post_normals_ragged(*a.values()) == 1, change
            assert message in L.rald_last_error(), (change, L.rald_last_error())
    off, o_nc, o_cnt = (C.c_int64 * 2)(0, 4), (C.c_double * 3)(), (C.c_int64 * 2)()
    cneed = L.rald_post_normal_consistency_scratch_bytes(1, 4, 4, 4, 4)
    cok = dict(pred=pts, pred_normals=o_n, pred_offsets=off, n_pred=4, gt=pts, gt_normals=o_n, gt_offsets=off, n_gt=4, batch=1, max_pred=4, max_gt=4,
               out_nc=o_nc, out_counts=o_cnt, scratch=aligned, scratch_bytes=cneed, stream=None)
    ccases = [(dict(**{key: None}), b"null pointer") for key in ("pred", "pred_normals", "pred_offsets", "gt", "gt_normals", "gt_offsets", "out_nc",
                                                               "out_counts")]
    ccases += [(dict(batch=0), b"batch 1 .. 65535"), (dict(batch=65536), b"batch 1 .. 65535"), (dict(n_pred=-1), b"the totals and the bounds"),
               (dict(n_gt=1 << 31), b"the totals and the bounds"), (dict(max_pred=-1), b"the totals and the bounds"),
               (dict(max_gt=1 << 31), b"the totals and the bounds"), (dict(scratch_bytes=cneed - 1), b"scratch too small"),
               (dict(max_pred=1 << 20), b"scratch too small"), (dict(scratch=None), b"null or unaligned scratch"),
               (dict(scratch=aligned + 8), b"null or unaligned scratch")]
    for change, message in ccases:
        assert L.rald_post_normal_consistency_ragged(*{**cok, **change}.values()) == 1, change
        assert message in L.rald_last_error() and b"normal_consistency_ragged" in L.rald_last_error(), (change, L.rald_last_error())
    assert not any(o_n) and not any(o_c) and not any(o_e) and not any(o_f) and not any(o_nc) and not any(o_cnt) and not any(scratch.raw)


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
           dict(max_radius=True), dict(max_radius=1e-60), dict(max_radius=1e60),
           dict(view=(0, 0)), dict(view=(0, 0, 0, 0)), dict(view=(0, float("nan"), 0)), dict(view=(float("inf"), 0, 0)), dict(view=5.0),
           dict(view="abc"), dict(view=(0, 0, 1e60))]
    for kw in bad:
        with pytest.raises(ValueError):
            PP.estimate_normals_ragged(**{**ok, **kw})
    for points, kw in ((torch.zeros(2, 5, 3), {}), (torch.zeros(5, 2), {}), (torch.zeros(5, 3), dict(k=0)), (torch.zeros(5, 3), dict(k=33)),
                       (torch.zeros(5, 3), dict(lo=(0, 0, 0))), (torch.zeros(5, 3, dtype=torch.int32), {}), (torch.zeros(5, 3), dict(cell=0)),
                       (torch.zeros(5, 3), dict(cell=True)), (torch.zeros(5, 3), dict(view=(0, 0))), (torch.zeros(5, 3), dict(view=(0, 0, float("nan")))),
                       (torch.zeros(5, 3), dict(lo=(0, 0, 0), hi=(1, -1, 1)))):
        with pytest.raises(ValueError):
            PP.estimate_normals(points, **{"k": 4, **kw})
    assert PP.estimate_normals(torch.zeros(0, 3), 4).shape == (0, 3)
    n3, off3 = torch.zeros(10, 3), torch.tensor([0, 4, 10])
    cok = dict(y_pred=pts, pred_normals=n3, pred_offsets=off3, y_gt=pts, gt_normals=n3, gt_offsets=off3, max_pred=6, max_gt=6)
    for kw in (dict(y_pred=torch.zeros(10, 2)), dict(y_gt=torch.zeros(3)), dict(pred_normals=torch.zeros(9, 3)), dict(gt_normals=torch.zeros(10, 2)),
               dict(pred_normals=None), dict(pred_offsets=[0, 4, 10]), dict(gt_offsets=torch.tensor([0, 10])), dict(max_pred=-1), dict(max_gt=2.5)):
        with pytest.raises(ValueError):
            PP.normal_consistency_ragged(**{**cok, **kw})
    with pytest.raises(ValueError):
        PP.normal_consistency(torch.zeros(4, 2), torch.zeros(4, 3), pts, n3)

    class Vae:
        def __getattr__(self, name):
            raise AssertionError("the autoencoder was touched")
    ns = lambda **kw: type("NS", (), kw)()
    args = ns(dataset=ns(lidar=ns(pc_range=[0, -90, -20, 15.8, 90, 20], view_cone_mode=True)))
    surf = torch.zeros(2, 20, 3)
    for fn in (E.infer_point_clouds, E.infer_point_clouds_device):
        for nc in (8, (8,), (8, 0.5, 1), (0, 0.5), (33, 0.5), (2.5, 0.5), (True, 0.5), (8, 0), (8, float("inf")), (8, "c"), (8, 1e-3), "ab"):
            with pytest.raises(ValueError):
                fn(Vae(), torch.zeros(2, 128, 32), args, surfaces=surf, normals=True, normal_consistency=nc)
        with pytest.raises(ValueError, match="surfaces"):
            fn(Vae(), torch.zeros(2, 128, 32), args, normals=True, normal_consistency=(8, 0.5))
        with pytest.raises(ValueError, match="normals"):
            fn(Vae(), torch.zeros(2, 128, 32), args, surfaces=surf, normal_consistency=(8, 0.5))
    assert E._check_normal_consistency(None, args, None, False, 0) is None
    assert E._check_normal_consistency((8.0, 0.5), args, surf, False, 2) == (8, PP.voxel_grid([-15.8] * 3, [15.8] * 3, 0.5))


# ---- the tail ------------------------------------------------------------------------------------------------------------------------------
def _stub_normals(monkeypatch):
    from rald_amd import postprocess as real
    from test_knn_host import _stub_statistical
    E, calls, reads, pos, kw, seen = _stub_statistical(monkeypatch)

    def estimate(pts, off, k, grid, max_per_sample, view=None):
        calls.append("estimate_normals_ragged")
        seen.update(n_pts=pts, n_off=off, n_args=(k, max_per_sample, view), n_grid=grid)
        seen["surface_normals"] = torch.arange(pts.shape[0] * 3, dtype=torch.float32).reshape(-1, 3)
        return seen["surface_normals"]

    def consistency(pred, pred_n, pred_off, gt, gt_n, gt_off, max_pred, max_gt):
        calls.append("normal_consistency_ragged")
        seen.update(c_pred=pred, c_pred_n=pred_n, c_pred_off=pred_off, c_gt_n=gt_n, c_gt_off=gt_off, c_bounds=(max_pred, max_gt))
        return torch.tensor([[0.75, 0.5, 0.625], [float("nan")] * 3], dtype=torch.float64), torch.tensor([[7, 20], [0, 0]])

    def oriented(kept, grad, off, *a, **k):
        calls.append("oriented_points_ragged")
        seen["pred_normals"] = torch.full((kept.shape[0], 3), 0.5)
        return kept, seen["pred_normals"]
    E.PP.estimate_normals_ragged, E.PP.normal_consistency_ragged, E.PP.oriented_points_ragged = estimate, consistency, oriented
    E.QP.project_to_surface_ragged = lambda vae, z, kept, off, longest, steps, max_step: (calls.append("project_to_surface_ragged"), (kept, None, kept))[1]
    return E, calls, reads, pos, kw, seen


def _with_index(E, calls):
    """occupied_points_ragged with the kept rows' indices, which the oriented tail gathers by."""
    def occupied(logits, queries, offsets, *a, return_index=False, **k):
        calls.append("occupied_points_ragged")
        return torch.zeros(queries.shape[0], 3), torch.tensor([0, 7, 12]), torch.zeros(queries.shape[0], dtype=torch.int64) if return_index else None
    E.PP.occupied_points_ragged = occupied


def test_infer_point_clouds_without_normal_consistency_is_what_it_was(monkeypatch):
    from test_cloud_metrics_host import TAIL
    E, calls, reads, pos, kw, seen = _stub_normals(monkeypatch)
    out = E.infer_point_clouds(*pos, **kw)
    assert calls == TAIL + ["cal_metrics_ragged"] and len(reads) == 1 and set(out) == {"pred", "cd", "n_queries"}
    assert out["cd"] == [1.5, 2.5] and out["n_queries"] == [150, 150] and [p.shape[0] for p in out["pred"]] == [7, 5]
    del calls[:], reads[:]
    out = E.infer_point_clouds(*pos, denoise_statistical=(8, 2.0, 0.5), thin=4.0, resample=5, metric_thresholds=(0.1,), **kw)
    assert calls == TAIL + ["cloud_metrics_ragged", "remove_statistical_outliers_ragged", "cloud_metrics_ragged", "voxel_downsample_ragged",
                            "resample_points_ragged"] and len(reads) == 1
    assert set(out) == {"pred", "cd", "n_queries", "metrics", "denoised", "denoise_index", "cd_denoised", "metrics_denoised", "denoise_stats",
                        "thinned", "thin_count", "thin_first", "resampled", "resample_index"}
    del calls[:], reads[:]
    assert len(E.infer_point_clouds_device(*pos, **kw)) == 3 and len(E.infer_point_clouds_device(*pos, denoise=(0.5, 2), thin=4.0, resample=5, **kw)) == 13
    assert "estimate_normals_ragged" not in calls and "normal_consistency_ragged" not in calls and "n_grid" not in seen and not reads
    for bad in (dict(normal_consistency=(8, 0.5)), dict(normal_consistency=(8, 0.5), normals=True, surfaces=None)):
        with pytest.raises(ValueError):
            E.infer_point_clouds(*pos, **{**kw, **bad})
    assert "estimate_normals_ragged" not in calls and not reads


def test_infer_point_clouds_with_normal_consistency(monkeypatch):
    from test_cloud_metrics_host import TAIL
    E, calls, reads, pos, kw, seen = _stub_normals(monkeypatch)
    _with_index(E, calls)
    oriented_tail = TAIL[:6] + ["project_to_surface_ragged", "oriented_points_ragged"] + TAIL[7:]
    base = E.infer_point_clouds(*pos, normals=True, **kw)
    assert calls == oriented_tail + ["cal_metrics_ragged"] and set(base) == {"pred", "cd", "n_queries", "normals"}
    del calls[:], reads[:]
    out = E.infer_point_clouds(*pos, normals=True, normal_consistency=(8, 0.5), **kw)
    # the surfaces' normals and the comparison after the surfaces are in the final frame, before the metric; still one host read
    assert calls == oriented_tail + ["estimate_normals_ragged", "normal_consistency_ragged", "cal_metrics_ragged"] and len(reads) == 1
    assert set(out) == set(base) | {"normal_consistency", "surface_normals"}
    assert out["cd"] == base["cd"] and out["n_queries"] == base["n_queries"] and [p.shape[0] for p in out["pred"]] == [7, 5]
    assert out["normal_consistency"][0] == (0.75, 0.5, 0.625) and all(math.isnan(v) for v in out["normal_consistency"][1])
    assert [t.shape for t in out["surface_normals"]] == [(20, 3), (20, 3)] and out["surface_normals"][1][0].tolist() == [60.0, 61.0, 62.0]
    assert seen["n_args"] == (8, 20, (0.0, 0.0, 0.0)) and seen["n_off"].tolist() == [0, 20, 40] and seen["n_pts"].shape == (40, 3)
    assert seen["n_grid"] == E.PP.voxel_grid([-15.8] * 3, [15.8] * 3, 0.5)
    assert seen["c_pred_n"] is seen["pred_normals"] and seen["c_gt_n"] is seen["surface_normals"] and seen["c_pred_off"].tolist() == [0, 7, 12]
    assert seen["c_gt_off"].tolist() == [0, 20, 40] and seen["c_bounds"] == (50, 20)
    # surface_steps alone gives the predicted normals too; skip_eval_metric keeps the consistency and drops the metric
    del calls[:], reads[:]
    out = E.infer_point_clouds(*pos, surface_steps=2, normal_consistency=(8, 0.5), **kw)
    assert out["normal_consistency"][0] == (0.75, 0.5, 0.625) and len(reads) == 1
    pos[2].eval.skip_eval_metric = True
    del calls[:], reads[:]
    out = E.infer_point_clouds(*pos, normals=True, normal_consistency=(8, 0.5), **kw)
    assert out["cd"] is None and out["normal_consistency"][0] == (0.75, 0.5, 0.625) and "cal_metrics_ragged" not in calls and len(reads) == 1
    pos[2].eval.skip_eval_metric = False
    # with everything else in the same host read: each set is unpacked from its own place
    del calls[:], reads[:]
    more = dict(normals=True, denoise_statistical=(8, 2.0, 0.5), resample=5, metric_thresholds=(0.1, 0.2))
    ref = E.infer_point_clouds(*pos, **more, **kw)
    del calls[:], reads[:]
    out = E.infer_point_clouds(*pos, normal_consistency=(8, 0.5), **more, **kw)
    assert len(reads) == 1 and set(out) == set(ref) | {"normal_consistency", "surface_normals"}
    assert out["normal_consistency"][0] == (0.75, 0.5, 0.625) and out["metrics"] == ref["metrics"] and out["metrics_denoised"] == ref["metrics_denoised"]
    assert out["denoise_stats"][0] == ref["denoise_stats"][0] and out["cd"] == ref["cd"] and out["cd_denoised"] == ref["cd_denoised"]
    more = dict(normals=True, thin=4.0, resample=5, metric_thresholds=(0.1, 0.2))                # the thinned offsets stay the last of the read
    ref = E.infer_point_clouds(*pos, **more, **kw)
    out = E.infer_point_clouds(*pos, normal_consistency=(8, 0.5), **more, **kw)
    assert out["normal_consistency"][0] == (0.75, 0.5, 0.625) and out["metrics"] == ref["metrics"] and [t.shape[0] for t in out["thinned"]] == [3, 2]
    assert [t.tolist() for t in out["thin_first"]] == [t.tolist() for t in ref["thin_first"]]
    del calls[:], reads[:]
    dev = E.infer_point_clouds_device(*pos, normals=True, normal_consistency=(8, 0.5), **kw)
    assert len(dev) == 6 and dev[3] is seen["pred_normals"] and dev[4].shape == (2, 3) and dev[5] is seen["surface_normals"] and not reads
