"""The k nearest other rows and the statistical outlier filter on the GPU (rald_amd/csrc/knn_search.hip) against tests/knn_ref.py, by
equality: integers as integers, floats and doubles by bit pattern (a NaN the definition asks for: any NaN).  Every call goes through
_run: the outputs are pre-filled with poison and followed by guard rows, the input rows the kernels must not read (behind counts,
behind the bound, behind offsets[B]) are NaN, and the checks assert that everything the definition does not write still holds its
poison.  Every case runs the sort's three routes - chunks of 1024, one workgroup, automatic - and compares the three."""
import ctypes as C

import numpy as np
import pytest
import torch

import knn_ref as REF
import radius_ref as RREF
from test_gpu_radius_filter import GUARD, POISON_F, POISON_I, _bits, _offsets, _one_chunk, _spans

gpu = pytest.mark.gpu
F32 = np.float32
F64 = np.float64
POISON_D = np.array([0x7FF8000012345678], np.uint64).view(F64)[0]


def _bits64(a):
    return np.ascontiguousarray(a, dtype=F64).view(np.uint64)


def _run(points, offsets, grid, k, bound, counts=None, chunk=0, post=False, max_radius=None, std_ratio=None, dense=False):
    """The C entries on poisoned, guarded buffers -> dict of numpy arrays, whole buffers (guards included): the search or, with
    std_ratio, the filter.  dense: offsets describe equal clouds, passed as n_dense with a NULL offsets pointer."""
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
    name = "knn" if std_ratio is None else "statistical"
    nbytes = getattr(L, f"rald_post_{name}_scratch_bytes")(B, T, bound) if post else getattr(L, f"rald_op_{name}_scratch_bytes")(B, T, bound, chunk)
    assert nbytes > 0
    scratch = torch.empty(nbytes + 16 * GUARD, dtype=torch.uint8, device="cuda")
    scratch[nbytes:] = 0xA5
    lo3, v3, dims3 = (C.c_float * 3)(*grid[0]), (C.c_float * 3)(*grid[1]), (C.c_int32 * 3)(*grid[2])
    ptr = lambda key: None if t.get(key) is None else t[key].data_ptr()
    head = (ptr("points"), ptr("offsets"), ptr("counts"), B, n_dense, T, bound, lo3, v3, dims3, k, 0.0 if max_radius is None else float(max_radius))
    tail = (scratch.data_ptr(), nbytes) + (() if post else (chunk,)) + (_stream(),)
    if std_ratio is None:
        t.update(idx=cu(np.full((T + GUARD, k), POISON_I, np.int64)), dist2=cu(np.full((T + GUARD, k), POISON_F, F32)),
                 found=cu(np.full(T + GUARD, POISON_I, np.int32)))
        fn = L.rald_post_knn_ragged if post else L.rald_op_knn_ragged
        check(fn(*head, ptr("idx"), ptr("dist2"), ptr("found"), *tail))
        keys = ("idx", "dist2", "found")
    else:
        t.update(out=cu(np.full((T + GUARD, 3), POISON_F, F32)), out_offsets=cu(np.full(B + 1 + GUARD, POISON_I, np.int64)),
                 index=cu(np.full(T + GUARD, POISON_I, np.int64)), mean=cu(np.full(T + GUARD, POISON_D, F64)),
                 stats=cu(np.full((B + GUARD, 3), POISON_D, F64)))
        fn = L.rald_post_statistical_filter_ragged if post else L.rald_op_statistical_filter_ragged
        check(fn(*head, float(std_ratio), ptr("out"), ptr("out_offsets"), ptr("index"), ptr("mean"), ptr("stats"), *tail))
        keys = ("out", "out_offsets", "index", "mean", "stats")
    torch.cuda.synchronize()
    assert bool((scratch[nbytes:] == 0xA5).all()), "the scratch's guard was written"
    return {key: t[key].cpu().numpy() for key in keys}


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


def _eq64(got, want):
    """Doubles by bits, except that a NaN the definition asks for is any NaN."""
    return ((_bits64(got) == _bits64(want)) | (np.isnan(got) & np.isnan(want) & (_bits64(got) != _bits64(POISON_D)))).all()


def _check_knn(got, ref):
    T = len(ref["found"])
    un = ref["untouched"]
    want = np.where(un[:, None], POISON_I, ref["idx"])
    bad = np.nonzero((got["idx"][:T] != want).any(axis=1))[0]
    assert bad.size == 0, (bad[:5], got["idx"][bad[:3]], want[bad[:3]])
    want = np.where(un[:, None], _bits(POISON_F), _bits(ref["dist2"]))
    bad = np.nonzero((_bits(got["dist2"][:T]) != want).any(axis=1))[0]
    assert bad.size == 0, (bad[:5], got["dist2"][bad[:3]], ref["dist2"][bad[:3]])
    assert np.array_equal(got["found"][:T], np.where(un, POISON_I, ref["found"]))
    assert (got["idx"][T:] == POISON_I).all() and (_bits(got["dist2"][T:]) == _bits(POISON_F)).all() and (got["found"][T:] == POISON_I).all()


def _check_filter(got, ref, B):
    M = int(ref["offsets"][-1])
    T = len(ref["mean"])
    assert _eq64(got["mean"][:T], np.where(ref["untouched"], POISON_D, ref["mean"])), np.nonzero(_bits64(got["mean"][:T]) != _bits64(ref["mean"]))[0][:5]
    assert (_bits64(got["mean"][T:]) == _bits64(POISON_D)).all()
    assert _eq64(got["stats"][:B], ref["stats"]), (got["stats"][:B], ref["stats"])
    assert (_bits64(got["stats"][B:]) == _bits64(POISON_D)).all()
    assert got["out_offsets"][:B + 1].tolist() == ref["offsets"].tolist() and (got["out_offsets"][B + 1:] == POISON_I).all()
    assert np.array_equal(got["index"][:M], ref["index"]) and (got["index"][M:] == POISON_I).all()
    assert np.array_equal(_bits(got["out"][:M]), _bits(ref["points"])) and (_bits(got["out"][M:]) == _bits(POISON_F)).all()


def _search_and_filter(p, off, grid, k, bound, counts=None, max_radius=None, ratios=(0.0, 1.0, 2.5), dense=False):
    """The whole surface on one batch, every route: the search with all three tables, the filter with every std_ratio."""
    B = len(off) - 1
    ref = REF.knn_ragged(p, off, grid, k, bound, counts, max_radius)
    _check_knn(_routes(p, off, grid, k, bound, counts=counts, max_radius=max_radius, dense=dense), ref)
    for ratio in ratios:
        _check_filter(_routes(p, off, grid, k, bound, counts=counts, max_radius=max_radius, std_ratio=ratio, dense=dense),
                      REF.statistical_ragged(p, off, grid, k, ratio, bound, counts, max_radius, knn=ref), B)
    return ref


# ---- 1. sizes ------------------------------------------------------------------------------------------------------------------------------
K0 = 8
LENGTHS = [0, 1, 2, K0, K0 + 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097]


def _sizes_cloud():
    """Rows uniform in [-0.03, 1.03)^3, so some lie outside the box [0, 1]^3 of the grid."""
    off = _offsets(LENGTHS)
    return off, np.random.RandomState(5).uniform(-0.03, 1.03, size=(off[-1], 3)).astype(F32), RREF.cube_grid(0.0, 1.0, 0.125)


@gpu
def test_sizes_in_one_ragged_batch():
    """Clouds of 0 .. 4097 rows around k, the wave (64), the search's workgroup (128) and the blocks of the sums (1024) in one batch."""
    off, p, grid = _sizes_cloud()
    ref = _search_and_filter(p, off, grid, K0, max(LENGTHS))
    assert 0 < (ref["found"] == -1).sum() < 0.3 * len(p) and (ref["found"] == K0).sum() > 0.5 * len(p)
    assert ref["found"][off[2]:off[3]].max() == 1 and 0 < ref["found"][off[3]:off[4]].max() < K0         # 2 and k rows: fewer than k others


@gpu
@pytest.mark.parametrize("b", range(len(LENGTHS)))
def test_sizes_alone(b):
    """Every cloud of the batch alone (the 0-row cloud included: n_total = 0), its length as the bound: the sort's three routes and
    the rald_post_ entries, the filter with every std_ratio."""
    off, p, grid = _sizes_cloud()
    n = LENGTHS[b]
    q = p[off[b]:off[b + 1]]
    one = _search_and_filter(q, [0, n], grid, K0, max(n, 1))
    _check_knn(_run(q, [0, n], grid, K0, max(n, 1), post=True), one)
    for ratio in (0.0, 1.0, 2.5):
        _check_filter(_run(q, [0, n], grid, K0, max(n, 1), post=True, std_ratio=ratio),
                      REF.statistical_ragged(q, [0, n], grid, K0, ratio, max(n, 1), knn=one), 1)


# ---- 2. every k on the lattice ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("k", [1, 2, 7, 8, 9, 16, 17, 32])
def test_k_on_the_integer_lattice_with_duplicates(k):
    """Integer coordinates with duplicates: shells of many equal distances, cut by k anywhere - ties go by row index."""
    p, grid = REF.lattice()
    ref = _search_and_filter(p, [0, len(p)], grid, k, len(p))
    assert (ref["found"] == k).all()
    d = ref["dist2"]
    ties = (d[:, 1:] == d[:, :-1])
    assert ties.size == 0 or (ref["idx"][:, 1:][ties] > ref["idx"][:, :-1][ties]).all()
    if k >= 7:
        assert ties.mean() > 0.5 and (d[:, 0] == 0).mean() > 0.5                # duplicates first, at distance 0


@gpu
@pytest.mark.parametrize("name", ["lattice_ulp", "one_cell", "all_equal", "far_row", "corner_blob", "faces", "uniform"])
def test_constructions(name):
    """The +-1 ulp lattice, all rows in one cell, all rows equal, one row far from a dense blob (its box grows to the grid), a blob in
    one corner of a grid 1290 cells wide, rows on cell faces (tests/test_knn_host.py holds the reference against an independent walk
    on the same clouds)."""
    p, grid = REF.CONSTRUCTIONS[name]()
    ref = _search_and_filter(p, [0, len(p)], grid, 8, len(p))
    assert (ref["found"] == 8).all()
    if name == "all_equal":
        assert (ref["dist2"] == 0).all() and ref["idx"][0].tolist() == list(range(1, 9)) and ref["idx"][20].tolist() == list(range(8))
    if name == "far_row":
        assert ref["dist2"][len(p) // 2].min() > 10000.0


# ---- 3. the grid does not show -------------------------------------------------------------------------------------------------------------
@gpu
def test_grid_independence():
    """One cloud over five grids of the same box, from one cell to cells far smaller than the spacing of the rows: equal outputs."""
    p = np.random.RandomState(9).uniform(0.0, 1.6, size=(2000, 3)).astype(F32)
    p[1000:] = (p[:1000] + np.random.RandomState(10).uniform(-0.01, 0.01, size=(1000, 3))).clip(0, 1.6).astype(F32)
    off = [0, len(p)]
    grids = [((0.0,) * 3, (2.0,) * 3, (1, 1, 1)), ((0.0,) * 3, (0.25,) * 3, (8, 8, 8)), ((0.0,) * 3, (0.5, 0.125, 2.0), (4, 16, 1)),
             ((0.0,) * 3, (0.0078125,) * 3, (256, 256, 256)), ((0.0,) * 3, (0.001953125,) * 3, (1024, 1024, 1024))]
    ref = REF.knn_ragged(p, off, grids[1], 9, len(p))
    frefs = {ratio: REF.statistical_ragged(p, off, grids[1], 9, ratio, len(p), knn=ref) for ratio in (0.0, 1.0, 2.5)}
    assert (ref["found"] == 9).all() and 0 < len(frefs[0.0]["index"]) < len(frefs[1.0]["index"]) < len(frefs[2.5]["index"]) < len(p)
    bounded = REF.knn_ragged(p, off, grids[1], 9, len(p), max_radius=0.15)
    assert 0 < (bounded["found"] < 9).mean() < 1
    for grid in grids:
        assert RREF.inside_of(p, *[grid[i] for i in (0, 2, 1)]).all()
        _check_knn(_routes(p, off, grid, 9, len(p)), ref)
        for ratio, fref in frefs.items():
            _check_filter(_routes(p, off, grid, 9, len(p), std_ratio=ratio), fref, 1)
        _check_knn(_run(p, off, grid, 9, len(p), max_radius=0.15), bounded)


# ---- 4. ragged batches -----------------------------------------------------------------------------------------------------------------------
@gpu
def test_ragged_batch_counts_and_dense():
    """B = 5 with an empty cloud, a one-row cloud and a `counts` that trims; a loose and a tight host bound; the dense layout."""
    lengths = [700, 0, 1, 1500, 1100]
    off = _offsets(lengths)
    p = np.random.RandomState(12).uniform(0.0, 0.6, size=(off[-1], 3)).astype(F32)
    grid = RREF.cube_grid(0.0, 0.6, 0.1)
    ref = _search_and_filter(p, off, grid, 7, 1500)
    for b in range(5):
        alone = REF.knn_ragged(p[off[b]:off[b + 1]], [0, lengths[b]], grid, 7, max(lengths[b], 1))
        assert np.array_equal(alone["idx"], ref["idx"][off[b]:off[b + 1]])
    assert _same(_run(p, off, grid, 7, 1500), _run(p, off, grid, 7, 10 ** 6))                     # a loose host bound does not show
    for counts, bound in (([650, 5, 1, 1024, 0], 1500), ([-5, 1 << 30, 7, 1, 1025], 1500), ([700, 0, 1, 1500, 1100], 1000)):
        _search_and_filter(p, off, grid, 7, bound, counts=counts)
    dense_off = _offsets([800] * 4)
    _search_and_filter(p[:3200], dense_off, grid, 7, 800, dense=True)
    _search_and_filter(p[:3200], dense_off, grid, 7, 800, counts=[800, 0, 13, 799], dense=True)


# ---- 5. rows outside -------------------------------------------------------------------------------------------------------------------------
@gpu
def test_outside_rows_take_no_part():
    rs = np.random.RandomState(14)
    p = rs.uniform(0.0, 0.5, size=(2000, 3)).astype(F32)
    grid = RREF.cube_grid(0.0, 0.5, 0.05)
    bad = rs.choice(2000, size=300, replace=False)
    p[bad[:60], rs.randint(0, 3, 60)] = np.nan
    p[bad[60:120], rs.randint(0, 3, 60)] = np.inf
    p[bad[120:180], rs.randint(0, 3, 60)] = -np.inf
    p[bad[180:240], 0] = F32(-0.001)                                                                # just below the box, beside inside rows
    p[bad[240:], 2] = F32(0.56)                                                                     # the cells end at 0.55
    ref = _search_and_filter(p, [0, 2000], grid, 8, 2000)
    assert (ref["found"][bad] == -1).all() and (ref["idx"][bad] == -1).all() and np.isposinf(ref["dist2"][bad]).all()
    good = np.setdiff1d(np.arange(2000), bad)
    assert (ref["found"][good] == 8).all() and not np.isin(ref["idx"][good], bad).any()
    assert np.array_equal(REF.knn_one(p[good], grid, 8)["dist2"], ref["dist2"][good])               # as if the outside rows were not there


# ---- 6. max_radius ---------------------------------------------------------------------------------------------------------------------------
@gpu
def test_max_radius():
    """A bound below every distance (all -1), one between the k-th and the (k+1)-th distance of a row, and one exactly on a pair's
    distance (d2 <= r2max holds with equality)."""
    p, grid = REF.uniform()
    off = [0, len(p)]
    free = REF.knn_one(p, grid, 9)
    tiny = 0.5 * float(np.sqrt(free["dist2"][:, 0].min()))
    ref = _search_and_filter(p, off, grid, 8, len(p), max_radius=tiny)
    assert (ref["found"] == 0).all() and (ref["idx"] == -1).all()
    d8, d9 = float(free["dist2"][0, 7]), float(free["dist2"][0, 8])
    between = float(np.sqrt((d8 + d9) / 2))
    assert d8 < F32(between) * F32(between) < d9
    ref = _search_and_filter(p, off, grid, 8, len(p), max_radius=between)
    assert ref["found"][0] == 8 and 0 < (ref["found"] < 8).sum() and (ref["found"] == 0).sum() < len(p)
    assert REF.knn_one(p, grid, 9, max_radius=between)["found"][0] == 8                             # the ninth is beyond the bound
    # the lattice: face neighbours at exactly fl(1.0)^2
    q, qgrid = REF.lattice()
    ref = _search_and_filter(q, [0, len(q)], qgrid, 32, len(q), max_radius=1.0)
    sel = ref["dist2"][ref["idx"] >= 0]
    assert (sel <= 1).all() and (sel == 1).any() and (ref["found"] < 32).any()
    assert (REF.knn_one(q, qgrid, 32, max_radius=float(np.nextafter(F32(1), F32(0))))["dist2"] == 1).sum() == 0


# ---- 7. the filter's own cases -----------------------------------------------------------------------------------------------------------------
@gpu
def test_filter_edges():
    """Equal means (kept whole, sigma 0), clouds with 0, 1 and 2 rows that count, and 1025 / 2049 rows across the blocks of the sums."""
    grid = RREF.cube_grid(0.0, 4.0, 0.5)
    cube = np.array([[x, y, z] for x in (1, 2) for y in (1, 2) for z in (1, 2)], F32)              # every corner: three neighbours at 1
    lone = np.array([[0.5, 0.5, 0.5]], F32)
    pair_far = np.array([[0.5, 0.5, 0.5], [3.5, 3.5, 3.5], [0.75, 0.5, 0.5]], F32)
    batch = np.concatenate([cube, lone, pair_far, np.full((2, 3), np.nan, F32)])
    off = _offsets([8, 1, 3, 2])
    for ratio in (0.0, 1.0, 2.5):
        ref = REF.statistical_ragged(batch, off, grid, 3, ratio, 8, max_radius=1.0)
        _check_filter(_routes(batch, off, grid, 3, 8, max_radius=1.0, std_ratio=ratio), ref, 4)
    assert ref["offsets"].tolist() == [0, 8, 8, 10, 10] and ref["stats"][0].tolist() == [1.0, 0.0, 1.0]
    assert np.isnan(ref["stats"][[1, 3]]).all() and ref["stats"][2].tolist() == [0.25, 0.0, 0.25] and np.isposinf(ref["mean"][[8, 10]]).all()
    one = REF.statistical_ragged(batch[:4], [0, 4], grid, 1, 0.0, 4, max_radius=1.0)
    _check_filter(_routes(batch[:4], [0, 4], grid, 1, 4, max_radius=1.0, std_ratio=0.0), one, 1)
    rs = np.random.RandomState(31)
    for n in (1025, 2049):
        p = rs.uniform(0.0, 4.0, size=(n, 3)).astype(F32)
        p[n - 1] = p[0]                                                                              # the last block's one row counts
        for ratio in (0.0, 1.0, 2.5):
            ref = REF.statistical_ragged(p, [0, n], grid, 5, ratio, n)
            _check_filter(_routes(p, [0, n], grid, 5, n, std_ratio=ratio), ref, 1)
        assert 0 < ref["offsets"][1] < n


# ---- 8. stale state ------------------------------------------------------------------------------------------------------------------------
@gpu
def test_results_do_not_depend_on_stale_state():
    """A large call, then a small one on the same (cached) scratch; the same bits on a second call and after a launch that fills every
    CU's LDS with NaN patterns."""
    from rald_amd import postprocess as PP
    from rald_amd._handles import _stream
    from rald_amd._lib import check, lib
    big = np.random.RandomState(15).uniform(0.0, 0.5, size=(6000, 3)).astype(F32)
    grid = RREF.cube_grid(0.0, 0.5, 0.05)
    lengths = [1025, 0, 2049, 65]
    off = _offsets(lengths)
    p = np.random.RandomState(16).uniform(0.0, 0.5, size=(off[-1], 3)).astype(F32)
    dp, doff = torch.from_numpy(p).cuda(), torch.tensor(off, device="cuda")
    db, dboff = torch.from_numpy(big).cuda(), torch.tensor([0, 6000], device="cuda")
    ref = REF.statistical_ragged(p, off, grid, 32, 1.0, 2049)
    for _ in range(2):
        PP.remove_statistical_outliers_ragged(db, dboff, 32, 1.0, grid, 6000)
        out, o, idx, mean, stats = PP.remove_statistical_outliers_ragged(dp, doff, 5, 1.0, grid, 2049, return_index=True, return_mean=True,
                                                                         return_stats=True)
        small = REF.statistical_ragged(p, off, grid, 5, 1.0, 2049)
        assert o.tolist() == small["offsets"].tolist() and _eq64(mean.cpu().numpy(), small["mean"]) and _eq64(stats.cpu().numpy(), small["stats"])
        assert np.array_equal(idx[:int(o[-1])].cpu().numpy(), small["index"])
    for kw in (dict(), dict(max_radius=0.04), dict(std_ratio=0.0), dict(std_ratio=2.5), dict(std_ratio=1.0)):
        for chunk in (1024, 0):
            first = _run(p, off, grid, 32, 2049, chunk=chunk, **kw)
            assert _same(first, _run(p, off, grid, 32, 2049, chunk=chunk, **kw))
            check(lib().rald_debug_poison_lds(_stream()))
            assert _same(first, _run(p, off, grid, 32, 2049, chunk=chunk, **kw))
    _check_filter(first, ref, 4)


# ---- 9. past the scans' 256 lanes --------------------------------------------------------------------------------------------------------------
@gpu
def test_257_clouds_cross_the_batch_scan():
    """257 clouds are one more than the 256 lanes of the scan that makes out_offsets over the batch: its second turn starts from the
    first one's carry.  Lengths cycle 0, 1, 2, 3, 5 rows; the down-sampler, the radius filter and the statistical filter, every output
    against its reference."""
    import test_gpu_radius_filter as RAD
    import test_gpu_voxel_downsample as VOX
    import voxel_ref as VREF
    B = 257
    off = _offsets([(0, 1, 2, 3, 5)[b % 5] for b in range(B)])
    p = np.random.RandomState(41).uniform(0.02, 0.98, size=(off[-1], 3)).astype(F32)
    grid = RREF.cube_grid(0.0, 1.0, 0.5)
    vox = VREF.voxel_ragged(p, off, *grid, 5)
    assert vox["offsets"][B] == vox["offsets"][B - 1] + 1 > 256             # the last cloud's one row: a voxel behind the carry
    VOX._check(VOX._run(p, off, grid, 5), vox, B)
    rad = RREF.filter_ragged(p, off, grid, 0.5, 1, 5)
    assert 256 < rad["offsets"][B - 1] == rad["offsets"][B] < off[-1]       # the last cloud's one row has no neighbour: not kept
    RAD._check_filter(RAD._run(p, off, grid, 0.5, 5, min_neighbors=1), rad, B)
    stat = REF.statistical_ragged(p, off, grid, 2, 0.5, 5)
    assert 256 < stat["offsets"][B - 1] == stat["offsets"][B] < off[-1]
    _check_filter(_run(p, off, grid, 2, 5, std_ratio=0.5), stat, B)


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------------
@gpu
def test_python_layer():
    from rald_amd import postprocess as PP
    off = _offsets([700, 0, 2100])
    p = np.random.RandomState(17).uniform(-0.02, 0.52, size=(off[-1], 3)).astype(F32)
    grid = PP.voxel_grid((0, 0, 0), (0.5, 0.5, 0.5), 0.06)
    ref = REF.knn_ragged(p, off, grid, 6, 2100)
    dp, doff = torch.from_numpy(p).cuda(), torch.tensor(off, device="cuda")
    idx, d2 = PP.knn_ragged(dp, doff, 6, grid, 2100)
    assert idx.dtype == torch.int64 and idx.shape == (2800, 6) and np.array_equal(idx.cpu().numpy(), ref["idx"])
    assert d2.dtype == torch.float32 and np.array_equal(_bits(d2.cpu().numpy()), _bits(ref["dist2"]))
    only = PP.knn_ragged(dp, doff, 6, grid, 2100, return_dist2=False, chunk=1024)
    assert isinstance(only, torch.Tensor) and torch.equal(only, idx)
    idx2, found = PP.knn_ragged(dp, doff, 6, grid, 2100, return_dist2=False, return_found=True)
    assert found.dtype == torch.int32 and np.array_equal(found.cpu().numpy(), ref["found"]) and torch.equal(idx2, idx)
    bounded = REF.knn_ragged(p, off, grid, 6, 2100, max_radius=0.03)
    got = PP.knn_ragged(dp, doff, 6, grid, 2100, max_radius=0.03, return_found=True)
    assert len(got) == 3 and np.array_equal(got[0].cpu().numpy(), bounded["idx"]) and np.array_equal(got[2].cpu().numpy(), bounded["found"])
    fref = REF.statistical_ragged(p, off, grid, 6, 1.5, 2100, knn=ref)
    M = int(fref["offsets"][-1])
    out = PP.remove_statistical_outliers_ragged(dp, doff, 6, 1.5, grid, 2100, return_index=True, return_mean=True, return_stats=True)
    assert len(out) == 5 and out[1].tolist() == fref["offsets"].tolist() and 0 < M < len(p)
    assert np.array_equal(_bits(out[0][:M].cpu().numpy()), _bits(fref["points"])) and np.array_equal(out[2][:M].cpu().numpy(), fref["index"])
    assert out[3].dtype == torch.float64 and _eq64(out[3].cpu().numpy(), fref["mean"]) and _eq64(out[4].cpu().numpy(), fref["stats"])
    assert len(PP.remove_statistical_outliers_ragged(dp, doff, 6, 1.5, grid, 2100)) == 2
    for ratio in (0.0, 1.0, 2.5):
        want = REF.statistical_ragged(p, off, grid, 6, ratio, 2100, knn=ref)
        got = PP.remove_statistical_outliers_ragged(dp, doff, 6, ratio, grid, 2100, return_index=True, return_stats=True, chunk=1024)
        assert got[1].tolist() == want["offsets"].tolist() and np.array_equal(got[2][:int(want["offsets"][-1])].cpu().numpy(), want["index"])
        assert _eq64(got[3].cpu().numpy(), want["stats"])
    empty = PP.remove_statistical_outliers_ragged(dp[:0], torch.zeros(3, dtype=torch.int64, device="cuda"), 6, 1.0, grid, 5, return_stats=True)
    assert empty[0].shape == (0, 3) and empty[1].tolist() == [0, 0, 0] and torch.isnan(empty[2]).all() and empty[2].shape == (2, 3)
    none = PP.knn_ragged(dp[:0], torch.zeros(3, dtype=torch.int64, device="cuda"), 6, grid, 5, return_found=True)
    assert none[0].shape == (0, 6) and none[1].shape == (0, 6) and none[2].shape == (0,)
    # one cloud, with bounds and with its own extent; the edge does not show
    one = PP.remove_statistical_outliers(dp[:700], 6, 1.5, lo=(0, 0, 0), hi=(0.5, 0.5, 0.5), cell=0.06)
    assert np.array_equal(_bits(one.cpu().numpy()), _bits(fref["points"][:int(fref["offsets"][1])]))
    inner = np.clip(p[:700], 0.0, 0.5)                                                              # every row within lo .. hi
    want = REF.statistical_ragged(inner, [0, 700], grid, 6, 1.5, 700)["points"]
    for cell in (None, 0.06, 0.5, 1e-4):
        one = PP.remove_statistical_outliers(torch.from_numpy(inner).cuda(), 6, 1.5, lo=(0, 0, 0), hi=(0.5, 0.5, 0.5), cell=cell)
        assert np.array_equal(_bits(one.cpu().numpy()), _bits(want)) and 0 < len(want) < 700, cell
    q = p[:700]
    own = PP.remove_statistical_outliers(dp[:700], 6, 1.5)
    box = PP.voxel_grid(q.min(axis=0).tolist(), q.max(axis=0).tolist(), 0.1)
    assert np.array_equal(_bits(own.cpu().numpy()), _bits(REF.statistical_ragged(q, [0, 700], box, 6, 1.5, 700)["points"]))
    flat = torch.zeros(50, 3, device="cuda")
    assert torch.equal(PP.remove_statistical_outliers(flat, 4, 1.0), flat)                        # a box of no extent; equal means
    with pytest.raises(RuntimeError):
        PP.knn_ragged(torch.from_numpy(p), doff, 6, grid, 2100)


# ---- the tail ------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_infer_point_clouds_denoise_statistical():
    """infer_point_clouds(..., denoise_statistical=(8, 1.0, 0.5)) on the 4-frame setup of tests/test_gpu_infer_batch.py: the new keys
    equal the reference applied to the 'pred' it returned, every other key equals the call without the argument; then with thin and
    resample on top, whose indices count rows of 'denoised'."""
    import fps_ref
    import voxel_ref
    from rald_amd import engine_generation as E, postprocess as PP, query_points as QP, synth
    from test_gpu_infer_batch import _small_vae, _tail_args
    vae, z9 = _small_vae()
    z = z9[:4].contiguous()
    n, aug, k = 3000, 2048, 100
    stat = (8, 1.0, 0.5)
    args = _tail_args(n, aug)
    helpers = [synth.queries(1, max(h, 1), seed=100 + h)[0][:h].cuda() for h in (0, 1, 500, 1100)]
    surfaces = synth.point_cloud(4, 1000, seed=62).cuda()
    draws = QP.draw_tail_randoms(4, n, aug, 10, torch.Generator("cuda").manual_seed(23))
    kw = dict(helper_points=helpers, surfaces=surfaces, draws=draws)
    grid = PP.voxel_grid([-15.8] * 3, [15.8] * 3, 0.5)
    base = E.infer_point_clouds(vae, z, args, **kw)
    res = E.infer_point_clouds(vae, z, args, denoise_statistical=stat, **kw)
    assert set(res) == set(base) | {"denoised", "denoise_index", "cd_denoised", "denoise_stats"} and res["n_queries"] == base["n_queries"]
    assert all(torch.equal(a, b) for a, b in zip(res["pred"], base["pred"]))

    def check_denoise(r, max_radius=None):
        refs = []
        for b in range(4):
            pred = r["pred"][b]
            ref = REF.statistical_ragged(pred.cpu().numpy(), [0, pred.shape[0]], grid, stat[0], stat[1], max(pred.shape[0], 1),
                                         max_radius=max_radius)
            assert np.array_equal(r["denoise_index"][b].cpu().numpy(), ref["index"]) and r["denoise_index"][b].dtype == torch.int64, b
            assert np.array_equal(_bits(r["denoised"][b].cpu().numpy()), _bits(ref["points"])), b
            assert torch.equal(r["denoised"][b], pred[r["denoise_index"][b]])
            assert _eq64(np.array(r["denoise_stats"][b]), ref["stats"][0]), (b, r["denoise_stats"][b], ref["stats"][0])
            refs.append(ref)
        return refs
    refs = check_denoise(res)
    sizes = [(p.shape[0], len(r["index"])) for p, r in zip(res["pred"], refs)]
    print("final clouds and their denoised rows:", sizes)
    assert any(0 < m < n_ for n_, m in sizes)
    for b in range(4):                                                                             # the metric of the denoised cloud
        want = PP.cal_metrics(res["denoised"][b], PP.polar2cartesian(PP.inverse_norm_points(surfaces[b], args.dataset.lidar.pc_range,
                                                                                            args.dataset.lidar.norm_anisotropy,
                                                                                            args.dataset.lidar.norm_isotropy)))
        got = res["cd_denoised"][b]
        assert got == want or abs(got - want) <= 1e-9 * abs(want), (b, got, want)
    check_denoise(E.infer_point_clouds(vae, z, args, denoise_statistical=stat + (0.4,), **kw), max_radius=0.4)
    with_n = E.infer_point_clouds(vae, z, args, denoise_statistical=stat, normals=True, metric_thresholds=(0.1, 0.5), **kw)
    check_denoise(with_n)
    assert set(with_n) == set(res) | {"normals", "denoised_normals", "metrics", "metrics_denoised"}
    for b in range(4):
        assert torch.equal(with_n["denoised_normals"][b], with_n["normals"][b][with_n["denoise_index"][b]])
        assert with_n["metrics_denoised"][b]["cd"] == with_n["cd_denoised"][b] and with_n["metrics"][b]["cd"] == with_n["cd"][b]
    # thin and resample on top: both run on the denoised clouds
    both = E.infer_point_clouds(vae, z, args, denoise_statistical=stat, thin=1.0, resample=k, **kw)
    assert set(both) == set(res) | {"thinned", "thin_count", "thin_first", "resampled", "resample_index"}
    refs = check_denoise(both)
    tgrid = PP.voxel_grid([-15.8] * 3, [15.8] * 3, 1.0)
    thin_refs = [voxel_ref.voxel_one(r["points"], *tgrid) for r in refs]
    for b in range(4):
        assert np.array_equal(_bits(both["thinned"][b].cpu().numpy()), _bits(thin_refs[b]["points"]))
        assert np.array_equal(both["thin_first"][b].cpu().numpy(), thin_refs[b]["first"])                       # rows of 'denoised'
    lengths = [len(t["count"]) for t in thin_refs]
    want_pts, want_idx = fps_ref.resample_ref(np.concatenate([t["points"] for t in thin_refs]), _offsets(lengths), k, max(max(lengths), 1))
    assert np.array_equal(both["resample_index"].cpu().numpy(), want_idx) and np.array_equal(_bits(both["resampled"].cpu().numpy()), _bits(want_pts))
    dev = E.infer_point_clouds_device(vae, z, args, denoise_statistical=stat, thin=1.0, resample=k, **kw)
    assert len(dev) == 14 and dev[4].tolist() == _offsets([len(r["index"]) for r in refs]) and torch.equal(dev[-1], both["resample_index"])
    assert _eq64(dev[7].cpu().numpy(), np.stack([r["stats"][0] for r in refs]))
    with pytest.raises(ValueError):
        E.infer_point_clouds(vae, z, args, denoise=(0.5, 3), denoise_statistical=stat, **kw)
