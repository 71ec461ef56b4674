"""PCA normals and normal consistency on the GPU (rald_amd/csrc/cloud_normals.hip) against tests/normals_ref.py, by equality: integers
as integers, floats and doubles by bit pattern (a NaN the definition asks for: any NaN but the poison).  Every call goes through
_run: the outputs are pre-filled with poison and followed by guard rows, the input rows the kernels must not read (behind counts,
behind the bound, behind offsets[B]) are NaN, and the checks assert that everything the definition does not write still holds its
poison.  Every case runs the sort's three routes - chunks of 1024, one workgroup, automatic - and compares the three."""
import ctypes as C

import numpy as np
import pytest
import torch

import knn_ref as KREF
import normals_ref as REF
import radius_ref as RREF
from test_gpu_radius_filter import GUARD, POISON_F, POISON_I, _bits, _offsets, _one_chunk, _spans

gpu = pytest.mark.gpu
F32 = np.float32
F64 = np.float64
POISON_D = np.array([0x7FF8000012345678], np.uint64).view(F64)[0]
KEYS = ("normals", "curvature", "eigenvalues", "found")


def _run(points, offsets, grid, k, bound, counts=None, chunk=0, post=False, max_radius=None, view=None, dense=False, absent=()):
    """The C entries on poisoned, guarded buffers -> dict of numpy arrays, whole buffers (guards included).  dense: offsets describe equal
    clouds, passed as n_dense with a NULL offsets pointer.  absent: the optional outputs passed as NULL."""
    from rald_amd._handles import _stream
    from rald_amd._lib import check, lib
    p = np.array(points, F32).reshape(-1, 3)
    T, B = len(p), len(offsets) - 1
    dev_p = np.concatenate([p, np.zeros((GUARD, 3), F32)])
    dev_p[_spans(T, offsets, bound, counts)] = np.nan
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    t = dict(points=cu(dev_p), offsets=None if dense else cu(np.array(offsets, np.int64)),
             counts=None if counts is None else cu(np.array(counts, np.int32)))
    n_dense = offsets[1] - offsets[0] if dense else 0
    L = lib()
    nbytes = L.rald_post_normals_scratch_bytes(B, T, bound) if post else L.rald_op_normals_scratch_bytes(B, T, bound, chunk)
    assert nbytes > 0
    scratch = torch.empty(nbytes + 16 * GUARD, dtype=torch.uint8, device="cuda")
    scratch[nbytes:] = 0xA5
    lo3, v3, dims3 = (C.c_float * 3)(*grid[0]), (C.c_float * 3)(*grid[1]), (C.c_int32 * 3)(*grid[2])
    view3 = None if view is None else (C.c_float * 3)(*view)
    t.update(normals=cu(np.full((T + GUARD, 3), POISON_F, F32)), curvature=cu(np.full(T + GUARD, POISON_F, F32)),
             eigenvalues=cu(np.full((T + GUARD, 3), POISON_F, F32)), found=cu(np.full(T + GUARD, POISON_I, np.int32)))
    ptr = lambda key: None if t.get(key) is None or key in absent else t[key].data_ptr()
    head = (ptr("points"), ptr("offsets"), ptr("counts"), B, n_dense, T, bound, lo3, v3, dims3, k, 0.0 if max_radius is None else float(max_radius),
            view3, ptr("normals"), ptr("curvature"), ptr("eigenvalues"), ptr("found"))
    tail = (scratch.data_ptr(), nbytes) + (() if post else (chunk,)) + (_stream(),)
    check((L.rald_post_normals_ragged if post else L.rald_op_normals_ragged)(*head, *tail))
    torch.cuda.synchronize()
    assert bool((scratch[nbytes:] == 0xA5).all()), "the scratch's guard was written"
    return {key: t[key].cpu().numpy() for key in KEYS}


def _raw(a):
    return a.view(np.uint32) if a.dtype == F32 else a.view(np.uint64) if a.dtype == F64 else a


def _same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(_raw(a[key]), _raw(b[key])) for key in a)


def _routes(points, offsets, grid, k, bound, **kw):
    """The call by chunks of 1024, by one workgroup and by the automatic rule -> the first result; the three must be the same bits."""
    runs = [_run(points, offsets, grid, k, bound, chunk=c, **kw) for c in (1024, _one_chunk(bound), 0)]
    for other in runs[1:]:
        assert _same(runs[0], other)
    return runs[0]


def _eq32(got, want, untouched):
    """fp32 by bits; where the definition asks for NaN any NaN but the poison; untouched rows hold the poison."""
    un = untouched.reshape((-1,) + (1,) * (got.ndim - 1))
    g, w = _bits(got), _bits(want)
    nan_ok = np.isnan(got) & np.isnan(want) & (g != _bits(POISON_F))
    return np.where(un, g == _bits(POISON_F), (g == w) | nan_ok)


def _check(got, ref, absent=()):
    T = len(ref["found"])
    un = ref["untouched"]
    for key in ("normals", "curvature", "eigenvalues"):
        if key in absent:
            assert (_bits(got[key]) == _bits(POISON_F)).all(), key
            continue
        ok = _eq32(got[key][:T], ref[key], un)
        bad = np.nonzero(~(ok if ok.ndim == 1 else ok.all(axis=1)))[0]
        assert bad.size == 0, (key, bad[:5], got[key][bad[:3]], ref[key][bad[:3]], ref["found"][bad[:3]])
        assert (_bits(got[key][T:]) == _bits(POISON_F)).all(), key
    if "found" in absent:
        assert (got["found"] == POISON_I).all()
    else:
        assert np.array_equal(got["found"][:T], np.where(un, POISON_I, ref["found"])) and (got["found"][T:] == POISON_I).all()


def _both(p, off, grid, k, bound, counts=None, max_radius=None, view=None, dense=False):
    ref = REF.normals_ragged(p, off, grid, k, bound, counts, max_radius, view)
    _check(_routes(p, off, grid, k, bound, counts=counts, max_radius=max_radius, view=view, dense=dense), ref)
    return ref


# ---- 1. sizes ------------------------------------------------------------------------------------------------------------------------------
K0 = 8
LENGTHS = [0, 1, 2, 3, 4, 63, 64, 65, 129, 1025]
VIEW = (0.4, 0.5, 3.0)


def _sizes_cloud():
    """Rows uniform in [-0.03, 1.03)^3, so some lie outside the box [0, 1]^3 of the grid."""
    off = _offsets(LENGTHS)
    return off, np.random.RandomState(5).uniform(-0.03, 1.03, size=(off[-1], 3)).astype(F32), RREF.cube_grid(0.0, 1.0, 0.125)


@gpu
def test_sizes_in_one_ragged_batch():
    """Clouds of 0 .. 1025 rows around found = 2, the wave (64), the search's workgroup (128) and the eigen kernel's (256) in one batch."""
    off, p, grid = _sizes_cloud()
    ref = _both(p, off, grid, K0, max(LENGTHS), view=VIEW)
    assert 0 < (ref["found"] == -1).sum() < 0.3 * len(p) and (ref["found"] == K0).sum() > 0.5 * len(p)
    assert (ref["normals"][off[1]:off[3]] == 0).all() and np.isnan(ref["curvature"][off[1]:off[3]]).all()   # 1 and 2 rows: found < 2
    assert np.abs(ref["normals"][off[3]:off[4]]).max() > 0                                                    # 3 rows: found = 2


@gpu
@pytest.mark.parametrize("b", range(len(LENGTHS)))
def test_sizes_alone(b):
    """Every cloud of the batch alone (the 0-row cloud included: n_total = 0), its length as the bound: the sort's three routes and the
    rald_post_ entry; the result equals the cloud's rows of the batch run (the reference computes it from the cloud alone)."""
    off, p, grid = _sizes_cloud()
    n = LENGTHS[b]
    q = p[off[b]:off[b + 1]]
    one = _both(q, [0, n], grid, K0, max(n, 1), view=VIEW)
    _check(_run(q, [0, n], grid, K0, max(n, 1), post=True, view=VIEW), one)


# ---- 2. every k on the lattice ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("k", [1, 2, 3, 8, 17, 32])
def test_k_on_the_integer_lattice_with_duplicates(k):
    """Integer coordinates with duplicates: ties in the neighbour order go by row index, equal eigenvalues by column; k = 1 leaves every
    row undefined (found = 1 < 2)."""
    p, grid = KREF.lattice(n=700)
    ref = _both(p, [0, len(p)], grid, k, len(p), view=(3.5, 3.5, 20.0))
    assert (ref["found"] == k).all()
    if k == 1:
        assert (ref["normals"] == 0).all() and np.isnan(ref["eigenvalues"]).all()
    else:
        assert (np.abs(np.linalg.norm(ref["normals"].astype(F64), axis=1) - 1) < 2e-7).all()


@gpu
@pytest.mark.parametrize("name", ["lattice_ulp", "all_equal", "far_row", "faces"])
def test_constructions(name):
    """The +-1 ulp lattice, all rows equal, one row far from a dense blob (its box grows to the grid), rows on cell faces."""
    p, grid = KREF.CONSTRUCTIONS[name]()
    p = p[:700]
    if name == "far_row":
        p[350] = (60.3, 61.7, 59.1)
    ref = _both(p, [0, len(p)], grid, 8, len(p), view=(0.5, 0.5, 9.0))
    assert (ref["found"] == 8).all()
    if name == "all_equal":
        assert (ref["normals"] == np.array([1, 0, 0], F32)).all() and (ref["curvature"] == 0).all() and (ref["eigenvalues"] == 0).all()


@gpu
def test_the_exact_plane_and_its_three_views():
    """The lattice plane z = 0: the normal is exactly (0, 0, 1) with the view above, (0, 0, -1) below, (0, 0, 1) with the view in the plane
    (s == 0) and without a view; the curvature is exactly 0."""
    g = np.stack(np.meshgrid(np.arange(9), np.arange(9), indexing="ij"), -1).reshape(-1, 2)
    p = np.concatenate([g, np.zeros((81, 1))], 1).astype(F32)
    grid = ((-0.5, -0.5, -0.5), (1.0, 1.0, 1.0), (10, 10, 2))
    for view, z in (((4.0, 4.0, 5.0), 1.0), ((4.0, 4.0, -5.0), -1.0), ((100.0, -3.0, 0.0), 1.0), (None, 1.0)):
        ref = _both(p, [0, 81], grid, 8, 81, view=view)
        assert (ref["normals"] == np.array([0, 0, z], F32)).all() and (ref["curvature"] == 0).all()


@gpu
def test_rows_outside_with_nan_and_inf():
    p = np.random.RandomState(12).uniform(0, 1, size=(300, 3)).astype(F32)
    p[[3, 50, 51, 170, 299]] = [[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf], [1.7, 0.5, 0.5], [-0.001, 0.2, 0.2]]
    ref = _both(p, [0, 300], RREF.cube_grid(0.0, 1.0, 0.2), 6, 300, view=(0.0, 0.0, 0.0))
    assert (ref["found"][[3, 50, 51, 170, 299]] == -1).all() and (ref["normals"][[3, 50, 51, 170, 299]] == 0).all()
    assert (ref["found"][np.setdiff1d(np.arange(300), [3, 50, 51, 170, 299])] == 6).all()


# ---- 3. the layout -----------------------------------------------------------------------------------------------------------------------------
@gpu
def test_counts_bounds_and_the_dense_layout():
    rs = np.random.RandomState(13)
    p = rs.uniform(0, 1, size=(900, 3)).astype(F32)
    grid = RREF.cube_grid(0.0, 1.0, 0.2)
    off = [0, 200, 200, 650, 900]
    _both(p, off, grid, 5, 300, counts=[150, 7, 450, 0], view=VIEW)               # counts below, above the segment, above the bound, 0
    _both(p, off, grid, 5, 100, view=VIEW)                                        # the bound cuts three clouds
    _both(p, [0, 300, 600, 900], grid, 5, 300, dense=True)
    _both(p, [0, 300, 600, 900], grid, 5, 300, counts=[300, 2, 120], dense=True, view=VIEW)


@gpu
def test_max_radius_leaving_one_two_and_three_neighbours():
    """Pairs, triples and quadruples 0.01 apart, the groups 0.2 apart: max_radius 0.05 leaves found = 1, 2 and 3 (k = 8)."""
    rs = np.random.RandomState(14)
    groups, sizes = [], rs.randint(2, 5, size=120)
    centres = np.stack(np.meshgrid(np.arange(5), np.arange(5), np.arange(5), indexing="ij"), -1).reshape(-1, 3)[:120] * 0.2 + 0.1
    for c, s in zip(centres, sizes):
        groups.append(c + rs.uniform(-0.01, 0.01, size=(s, 3)))
    p = np.concatenate(groups).astype(F32)
    ref = _both(p, [0, len(p)], RREF.cube_grid(0.0, 1.2, 0.07), 8, len(p), max_radius=0.05, view=VIEW)
    assert set(ref["found"].tolist()) == {1, 2, 3} and (ref["normals"][ref["found"] == 1] == 0).all()
    assert (np.abs(ref["normals"][ref["found"] >= 2]).max(axis=1) > 0.5).all()
    assert (ref["eigenvalues"][ref["found"] == 2, 0] <= 1e-12).all()                # three points: a plane


# ---- 4. the grid and stale state ---------------------------------------------------------------------------------------------------------------
@gpu
def test_grid_independence():
    """One cloud over five grids of the same box, from one cell to cells far smaller than the spacing of the rows: equal outputs."""
    p = np.random.RandomState(9).uniform(0.0, 1.6, size=(1200, 3)).astype(F32)
    off = [0, len(p)]
    grids = [((0.0,) * 3, (2.0,) * 3, (1, 1, 1)), ((0.0,) * 3, (0.25,) * 3, (8, 8, 8)), ((0.0,) * 3, (0.5, 0.125, 2.0), (4, 16, 1)),
             ((0.0,) * 3, (0.0078125,) * 3, (256, 256, 256)), ((0.0,) * 3, (0.001953125,) * 3, (1024, 1024, 1024))]
    ref = REF.normals_ragged(p, off, grids[1], 9, len(p), view=VIEW)
    for grid in grids:
        _check(_routes(p, off, grid, 9, len(p), view=VIEW), ref)


@gpu
def test_stale_scratch_a_large_call_then_a_small_one():
    """The same scratch buffer serves a call of 2100 rows and then one of 40 rows whose rows mostly have found < 2: nothing of the first
    call's moments or found shows."""
    from rald_amd._handles import _stream
    from rald_amd._lib import check, lib
    L = lib()
    rs = np.random.RandomState(15)
    big, small = rs.uniform(0, 1, size=(2100, 3)).astype(F32), rs.uniform(0, 1, size=(40, 3)).astype(F32)
    grid = RREF.cube_grid(0.0, 1.0, 0.1)
    nbytes = L.rald_post_normals_scratch_bytes(1, 2100, 2100)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    lo3, v3, dims3 = (C.c_float * 3)(*grid[0]), (C.c_float * 3)(*grid[1]), (C.c_int32 * 3)(*grid[2])

    def call(p, max_radius):
        n = len(p)
        t = dict(points=torch.from_numpy(p).cuda(), off=torch.tensor([0, n], device="cuda"), normals=torch.zeros(n, 3, device="cuda"),
                 curvature=torch.zeros(n, device="cuda"), eigenvalues=torch.zeros(n, 3, device="cuda"),
                 found=torch.zeros(n, dtype=torch.int32, device="cuda"))
        check(L.rald_post_normals_ragged(t["points"].data_ptr(), t["off"].data_ptr(), None, 1, 0, n, n, lo3, v3, dims3, 8, max_radius, None,
                                         t["normals"].data_ptr(), t["curvature"].data_ptr(), t["eigenvalues"].data_ptr(), t["found"].data_ptr(),
                                         scratch.data_ptr(), nbytes, _stream()))
        torch.cuda.synchronize()
        return {key: t[key].cpu().numpy() for key in KEYS}
    got_big = call(big, 0.0)
    got_small = call(small, 0.25)
    for got, p, r in ((got_big, big, None), (got_small, small, 0.25)):
        ref = REF.normals_ragged(p, [0, len(p)], grid, 8, len(p), max_radius=r)
        for key in ("normals", "curvature", "eigenvalues"):
            assert _eq32(got[key], ref[key], ref["untouched"]).all(), key
        assert np.array_equal(got["found"], ref["found"])
    assert (got_small["found"] < 2).sum() > 10 and (got_small["found"] >= 2).sum() > 3


@gpu
def test_nullable_outputs_absent_and_present():
    p = np.random.RandomState(16).uniform(0, 1, size=(500, 3)).astype(F32)
    grid = RREF.cube_grid(0.0, 1.0, 0.2)
    ref = REF.normals_ragged(p, [0, 200, 500], grid, 7, 300, view=VIEW)
    for absent in ((), ("curvature",), ("eigenvalues",), ("found",), ("curvature", "eigenvalues", "found")):
        _check(_run(p, [0, 200, 500], grid, 7, 300, view=VIEW, absent=absent), ref, absent)
        _check(_run(p, [0, 200, 500], grid, 7, 300, view=VIEW, absent=absent, post=True), ref, absent)


# ---- 5. normal consistency ---------------------------------------------------------------------------------------------------------------------
def _unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


def _consistency(pred, pn, poff, gt, gn, goff, max_pred=None, max_gt=None):
    from rald_amd._handles import _stream
    from rald_amd._lib import check, lib
    L = lib()
    B = len(poff) - 1
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    pad = lambda a: np.concatenate([a, np.full((GUARD, 3), np.nan, F32)])           # rows behind offsets[B] must not be read
    max_pred = max(np.diff(poff).max(), 0) if max_pred is None else max_pred
    max_gt = max(np.diff(goff).max(), 0) if max_gt is None else max_gt
    Tp, Tg = len(pred), len(gt)
    nbytes = L.rald_post_normal_consistency_scratch_bytes(B, Tp, Tg, int(max_pred), int(max_gt))
    assert nbytes >= 0
    scratch = torch.empty(nbytes + 16 * GUARD, dtype=torch.uint8, device="cuda")
    scratch[nbytes:] = 0xA5
    t = [cu(pad(pred)), cu(pad(pn)), cu(np.array(poff, np.int64)), cu(pad(gt)), cu(pad(gn)), cu(np.array(goff, np.int64))]
    nc, cnt = cu(np.full((B + GUARD, 3), POISON_D, F64)), cu(np.full((B + GUARD, 2), POISON_I, np.int64))
    check(L.rald_post_normal_consistency_ragged(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), Tp, t[3].data_ptr(), t[4].data_ptr(),
                                                t[5].data_ptr(), Tg, B, int(max_pred), int(max_gt), nc.data_ptr(), cnt.data_ptr(),
                                                scratch.data_ptr(), nbytes, _stream()))
    torch.cuda.synchronize()
    assert bool((scratch[nbytes:] == 0xA5).all()), "the scratch's guard was written"
    nc, cnt = nc.cpu().numpy(), cnt.cpu().numpy()
    assert (nc[B:].view(np.uint64) == np.array(POISON_D).view(np.uint64)).all() and (cnt[B:] == POISON_I).all()
    return nc[:B], cnt[:B]


def _eq64(got, want):
    g, w = np.ascontiguousarray(got).view(np.uint64), np.ascontiguousarray(want).view(np.uint64)
    return ((g == w) | (np.isnan(got) & np.isnan(want) & (g != np.array(POISON_D).view(np.uint64)))).all()


@gpu
def test_normal_consistency_batch():
    """Frames of 1025 against 2049 rows (two and three blocks of the fixed sum), 300 against 0, 0 against 70, 5 against 5 with only zero
    normals on one side, and 64 against 64; zero, NaN and inf normals on either side of the first frame."""
    rs = np.random.RandomState(17)
    np_, ng = [1025, 300, 0, 5, 64], [2049, 0, 70, 5, 64]
    poff, goff = _offsets(np_), _offsets(ng)
    pred, gt = rs.uniform(0, 1, (poff[-1], 3)).astype(F32), rs.uniform(0, 1, (goff[-1], 3)).astype(F32)
    pn, gn = _unit(rs.normal(size=(poff[-1], 3))), _unit(rs.normal(size=(goff[-1], 3)))
    pn[[3, 1024]], gn[[0, 2048]] = 0, 0
    pn[7, 1], pn[9, 2], gn[5, 0], gn[1500] = np.nan, np.inf, -np.inf, np.nan
    pn[poff[3]:poff[4]] = 0
    gt[goff[4]:goff[5]] = pred[poff[4]:poff[5]]                                       # the last frame: the same cloud, the same normals
    gn[goff[4]:goff[5]] = -pn[poff[4]:poff[5]]
    want_nc, want_cnt = REF.consistency_ragged(pred, pn, poff, gt, gn, goff)
    nc, cnt = _consistency(pred, pn, poff, gt, gn, goff)
    assert np.array_equal(cnt, want_cnt), (cnt, want_cnt)
    assert _eq64(nc, want_nc), (nc, want_nc)
    assert 1000 < cnt[0, 0] < 1025 and 2000 < cnt[0, 1] < 2049 and cnt[1:4].tolist() == [[0, 0]] * 3 and np.isnan(nc[1:4]).all()
    assert abs(nc[4, 0] - 1.0) <= 2.0 ** -22 and abs(nc[4, 2] - 1.0) <= 2.0 ** -22
    # every frame alone: the same bits
    for f in range(5):
        a, c = _consistency(pred[poff[f]:poff[f + 1]], pn[poff[f]:poff[f + 1]], [0, np_[f]], gt[goff[f]:goff[f + 1]], gn[goff[f]:goff[f + 1]],
                            [0, ng[f]])
        assert _eq64(a, want_nc[f:f + 1]) and np.array_equal(c, want_cnt[f:f + 1]), f
    # bounds above the segments change nothing
    b, c = _consistency(pred, pn, poff, gt, gn, goff, max_pred=4000, max_gt=2500)
    assert _eq64(b, want_nc) and np.array_equal(c, want_cnt)


# ---- 6. the Python layer -------------------------------------------------------------------------------------------------------------------------
@gpu
def test_python_layer():
    from rald_amd import postprocess as PP
    rs = np.random.RandomState(18)
    p = rs.uniform(0, 0.5, size=(1500, 3)).astype(F32)
    off = [0, 700, 700, 1500]
    grid = PP.voxel_grid((0, 0, 0), (0.5, 0.5, 0.5), 0.06)
    dp, doff = torch.from_numpy(p).cuda(), torch.tensor(off, device="cuda")
    ref = REF.normals_ragged(p, off, grid, 6, 800, view=VIEW)
    n, c, e, f = PP.estimate_normals_ragged(dp, doff, 6, grid, 800, view=VIEW, return_curvature=True, return_eigenvalues=True, return_found=True)
    for got, key in ((n, "normals"), (c, "curvature"), (e, "eigenvalues")):
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(ref[key])), key
    assert np.array_equal(f.cpu().numpy(), ref["found"]) and f.dtype == torch.int32
    only = PP.estimate_normals_ragged(dp, doff, 6, grid, 800, view=VIEW, chunk=1024)
    assert torch.equal(only, n)
    empty = PP.estimate_normals_ragged(dp[:0], torch.zeros(3, dtype=torch.int64, device="cuda"), 6, grid, 8, return_found=True)
    assert empty[0].shape == (0, 3) and empty[1].shape == (0,)
    q = p[:700]
    one = PP.estimate_normals(dp[:700], 6, view=VIEW, lo=(0, 0, 0), hi=(0.5, 0.5, 0.5), cell=0.06)
    assert np.array_equal(_bits(one.cpu().numpy()), _bits(ref["normals"][:700]))
    own = PP.estimate_normals(dp[:700], 6)
    box = PP.voxel_grid(q.min(axis=0).tolist(), q.max(axis=0).tolist(), 0.1)
    assert np.array_equal(_bits(own.cpu().numpy()), _bits(REF.normals_ragged(q, [0, 700], box, 6, 700)["normals"]))
    # the consistency of the estimated normals of two samplings of one sphere: high, and equal to the reference on the device's normals
    a, b = REF.sphere_shell(seed=51, n=900), REF.sphere_shell(seed=52, n=1100)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    na, nb = PP.estimate_normals(da, 12, view=(40.0, 5.0, 1.0)), PP.estimate_normals(db, 12, view=(40.0, 5.0, 1.0))
    offs = torch.tensor([[0, 900], [0, 1100]], device="cuda")
    nc, cnt = PP.normal_consistency_ragged(da, na, offs[0], db, nb, offs[1], 900, 1100)
    want_nc, want_cnt = REF.consistency_ragged(a, na.cpu().numpy(), [0, 900], b, nb.cpu().numpy(), [0, 1100])
    assert _eq64(nc.cpu().numpy(), want_nc) and np.array_equal(cnt.cpu().numpy(), want_cnt) and nc[0, 2] > 0.97
    host = PP.normal_consistency(da, na, db, nb)
    assert host == {"pred_to_gt": want_nc[0, 0], "gt_to_pred": want_nc[0, 1], "mean": want_nc[0, 2]}
    # the inward view turns every normal of the sphere towards the centre
    centre = np.array([40.0, 5.0, 1.0])
    assert ((na.cpu().numpy().astype(F64) * (centre - a)).sum(axis=1) > 0).all()
    e_nc, e_cnt = PP.normal_consistency_ragged(da[:0], na[:0], torch.zeros(2, dtype=torch.int64, device="cuda"), db, nb, offs[1], 0, 1100)
    assert torch.isnan(e_nc).all() and e_cnt.tolist() == [[0, 0]]
    with pytest.raises(RuntimeError):
        PP.estimate_normals_ragged(torch.from_numpy(p), doff, 6, grid, 800)


# ---- 7. the tail -------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_infer_point_clouds_normal_consistency():
    """infer_point_clouds(..., normals=True, surfaces=..., normal_consistency=(8, 1.0)) on the 4-frame setup of
    tests/test_gpu_infer_batch.py: the new keys equal the reference applied to the 'pred', 'normals' and surfaces of the call, every other
    key equals the call without the argument; then with denoise_statistical and thin on top, which leave the new keys as they are."""
    from rald_amd import engine_generation as E, postprocess as PP, query_points as QP, synth
    from test_gpu_infer_batch import _small_vae, _tail_args
    vae, z9 = _small_vae()
    z = z9[:4].contiguous()
    n, aug = 3000, 2048
    args = _tail_args(n, aug)
    lidar = args.dataset.lidar
    helpers = [synth.queries(1, max(h, 1), seed=100 + h)[0][:h].cuda() for h in (0, 1, 500, 1100)]
    surfaces = synth.point_cloud(4, 1000, seed=62).cuda()
    draws = QP.draw_tail_randoms(4, n, aug, 10, torch.Generator("cuda").manual_seed(23))
    kw = dict(helper_points=helpers, surfaces=surfaces, draws=draws, normals=True)
    grid = PP.voxel_grid([-15.8] * 3, [15.8] * 3, 1.0)
    base = E.infer_point_clouds(vae, z, args, **kw)
    res = E.infer_point_clouds(vae, z, args, normal_consistency=(8, 1.0), **kw)
    assert set(res) == set(base) | {"normal_consistency", "surface_normals"} and res["n_queries"] == base["n_queries"]
    print("cd with and without:", res["cd"], base["cd"])
    assert all(a == b or abs(a - b) <= 1e-9 * abs(b) for a, b in zip(res["cd"], base["cd"]))   # Chamfer's sums are atomic: equal to rounding
    assert all(torch.equal(a, b) for a, b in zip(res["pred"], base["pred"])) and all(torch.equal(a, b) for a, b in zip(res["normals"], base["normals"]))

    def check(r):
        for b in range(4):
            gt = PP.polar2cartesian(PP.inverse_norm_points(surfaces[b], lidar.pc_range, lidar.norm_anisotropy, lidar.norm_isotropy)).cpu().numpy()
            want_n = REF.normals_ragged(gt, [0, 1000], grid, 8, 1000, view=(0.0, 0.0, 0.0))["normals"]
            assert np.array_equal(_bits(r["surface_normals"][b].cpu().numpy()), _bits(want_n)), b
            want, _ = REF.consistency_ragged(r["pred"][b].cpu().numpy(), r["normals"][b].cpu().numpy(), [0, r["pred"][b].shape[0]], gt, want_n, [0, 1000])
            assert _eq64(np.array(r["normal_consistency"][b]), want[0]), (b, r["normal_consistency"][b], want[0])
    check(res)
    print("normal consistency per frame:", res["normal_consistency"])
    assert any(np.isfinite(v[2]) for v in res["normal_consistency"])
    more = dict(denoise_statistical=(8, 1.0, 0.5), thin=1.0)
    ref2 = E.infer_point_clouds(vae, z, args, **more, **kw)
    res2 = E.infer_point_clouds(vae, z, args, normal_consistency=(8, 1.0), **more, **kw)
    assert set(res2) == set(ref2) | {"normal_consistency", "surface_normals"}
    check(res2)
    for b in range(4):
        assert _eq64(np.array(res2["normal_consistency"][b]), np.array(res["normal_consistency"][b]))
        assert torch.equal(res2["thinned"][b], ref2["thinned"][b]) and torch.equal(res2["denoised"][b], ref2["denoised"][b])
    assert res2["denoise_stats"] == ref2["denoise_stats"] or all(_eq64(np.array(a), np.array(b)) for a, b in zip(res2["denoise_stats"], ref2["denoise_stats"]))
    dev = E.infer_point_clouds_device(vae, z, args, normal_consistency=(8, 1.0), **kw)
    assert len(dev) == 6 and _eq64(dev[4].cpu().numpy(), np.array(res["normal_consistency"])) and dev[5].shape == (4000, 3)
    with pytest.raises(ValueError):
        E.infer_point_clouds(vae, z, args, normal_consistency=(8, 1.0), **{**kw, "normals": False})
