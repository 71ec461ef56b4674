"""Fixed-radius neighbour counts, the nearest other row and the radius outlier filter on the GPU (rald_amd/csrc/radius_search.hip)
against tests/radius_ref.py, by equality: integers as integers, floats by bit pattern.  Every call goes through _run: the outputs are
pre-filled with poison (NaN with a payload, -7) and followed by guard rows, the input rows the kernels must not read (behind counts,
behind the bound, behind offsets[B]) are NaN, and _check asserts that everything the definition does not write still holds its
poison.  Every case runs the sort's three routes - chunks of 1024, one workgroup, automatic - and compares the three."""
import ctypes as C

import numpy as np
import pytest
import torch

import radius_ref as REF

gpu = pytest.mark.gpu
F32 = np.float32
GUARD = 64
POISON_F = np.array([0x7FC12345], np.uint32).view(F32)[0]          # a NaN with a payload: compared by bits
POISON_I = -7


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _offsets(lengths):
    return [0] + np.cumsum(lengths).tolist()


def _spans(T, offsets, bound, counts):
    hidden = np.ones(T + GUARD, bool)
    for b in range(len(offsets) - 1):
        n = offsets[b + 1] - offsets[b]
        if counts is not None:
            n = min(n, max(int(counts[b]), 0))
        hidden[offsets[b]:offsets[b] + max(min(n, bound), 0)] = False
    return hidden


def _run(points, offsets, grid, radius, bound, counts=None, chunk=0, post=False, max_count=0, nearest=True, min_neighbors=None, dense=False):
    """The C entries on poisoned, guarded buffers -> dict of numpy arrays, whole buffers (guards included): the count call (with the
    nearest outputs unless a cap forbids them) or, with min_neighbors, the filter.  dense: offsets describe equal clouds, passed as
    n_dense with a NULL offsets pointer."""
    from rald_amd._handles import _stream
    from rald_amd._lib import check, lib
    p = np.array(points, F32).reshape(-1, 3)
    T, B = len(p), len(offsets) - 1
    dev_p = np.concatenate([p, np.zeros((GUARD, 3), F32)])
    dev_p[_spans(T, offsets, bound, counts)] = np.nan
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    t = dict(points=cu(dev_p), offsets=None if dense else cu(np.array(offsets, np.int64)),
             counts=None if counts is None else cu(np.array(counts, np.int32)), count=cu(np.full(T + GUARD, POISON_I, np.int32)))
    n_dense = offsets[1] - offsets[0] if dense else 0
    L = lib()
    nbytes = L.rald_post_radius_scratch_bytes(B, T, bound) if post else L.rald_op_radius_scratch_bytes(B, T, bound, chunk)
    assert nbytes > 0
    scratch = torch.empty(nbytes + 16 * GUARD, dtype=torch.uint8, device="cuda")
    scratch[nbytes:] = 0xA5
    lo3, v3, dims3 = (C.c_float * 3)(*grid[0]), (C.c_float * 3)(*grid[1]), (C.c_int32 * 3)(*grid[2])
    ptr = lambda k: None if t.get(k) is None else t[k].data_ptr()
    head = (ptr("points"), ptr("offsets"), ptr("counts"), B, n_dense, T, bound, lo3, v3, dims3, float(radius))
    tail = (scratch.data_ptr(), nbytes) + (() if post else (chunk,)) + (_stream(),)
    if min_neighbors is None:
        if nearest and not max_count:
            t.update(nn_idx=cu(np.full(T + GUARD, POISON_I, np.int64)), nn_dist2=cu(np.full(T + GUARD, POISON_F, F32)))
        fn = L.rald_post_radius_count_ragged if post else L.rald_op_radius_count_ragged
        check(fn(*head, max_count, ptr("count"), ptr("nn_idx"), ptr("nn_dist2"), *tail))
        keys = ("count", "nn_idx", "nn_dist2")
    else:
        t.update(out=cu(np.full((T + GUARD, 3), POISON_F, F32)), out_offsets=cu(np.full(B + 1 + GUARD, POISON_I, np.int64)),
                 index=cu(np.full(T + GUARD, POISON_I, np.int64)))
        fn = L.rald_post_radius_filter_ragged if post else L.rald_op_radius_filter_ragged
        check(fn(*head, min_neighbors, ptr("out"), ptr("out_offsets"), ptr("index"), ptr("count"), *tail))
        keys = ("count", "out", "out_offsets", "index")
    torch.cuda.synchronize()
    assert bool((scratch[nbytes:] == 0xA5).all()), "the scratch's guard was written"
    return {k: t[k].cpu().numpy() for k in keys if k in t}


def _one_chunk(bound):
    return -(-bound // 1024) * 1024                                   # >= the bound: the one-workgroup sort


def _routes(points, offsets, grid, radius, bound, **kw):
    """The call by chunks of 1024, by one workgroup and by the automatic rule -> the first result; the three must be the same bits."""
    runs = [_run(points, offsets, grid, radius, bound, chunk=c, **kw) for c in (1024, _one_chunk(bound), 0)]
    for other in runs[1:]:
        assert _same(runs[0], other)
    return runs[0]


def _same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k].view(np.uint32) if a[k].dtype == F32 else a[k],
                                                       b[k].view(np.uint32) if b[k].dtype == F32 else b[k]) for k in a)


def _check_count(got, ref):
    """Everything the count call writes equals the reference; everything else still holds its poison."""
    T = len(ref["count"])
    un = ref["untouched"]
    want = np.where(un, POISON_I, ref["count"])
    bad = np.nonzero(got["count"][:T] != want)[0]
    assert bad.size == 0, (bad[:5], got["count"][bad[:5]], want[bad[:5]])
    assert (got["count"][T:] == POISON_I).all()
    if "nn_idx" in got:
        want = np.where(un, POISON_I, ref["nn_idx"])
        bad = np.nonzero(got["nn_idx"][:T] != want)[0]
        assert bad.size == 0, (bad[:5], got["nn_idx"][bad[:5]], want[bad[:5]])
        want = np.where(un, _bits(POISON_F), _bits(ref["nn_dist2"]))
        bad = np.nonzero(_bits(got["nn_dist2"][:T]) != want)[0]
        assert bad.size == 0, (bad[:5], got["nn_dist2"][bad[:5]], ref["nn_dist2"][bad[:5]])
        assert (got["nn_idx"][T:] == POISON_I).all() and (_bits(got["nn_dist2"][T:]) == _bits(POISON_F)).all()


def _check_filter(got, ref, B):
    M = int(ref["offsets"][-1])
    T = len(ref["count"])
    assert got["out_offsets"][:B + 1].tolist() == ref["offsets"].tolist() and (got["out_offsets"][B + 1:] == POISON_I).all()
    assert np.array_equal(got["index"][:M], ref["index"]) and (got["index"][M:] == POISON_I).all()
    assert np.array_equal(_bits(got["out"][:M]), _bits(ref["points"])) and (_bits(got["out"][M:]) == _bits(POISON_F)).all()
    assert np.array_equal(got["count"][:T], np.where(ref["untouched"], POISON_I, ref["count"])) and (got["count"][T:] == POISON_I).all()


def _count_and_filter(p, off, grid, radius, bound, counts=None, caps=(1, 3), mins=(1, 2, 5), dense=False):
    """The whole surface on one batch, every route: the uncapped count with the nearest row, capped counts, the filter."""
    B = len(off) - 1
    ref = REF.radius_ragged(p, off, grid, radius, bound, counts)
    _check_count(_routes(p, off, grid, radius, bound, counts=counts, dense=dense), ref)
    for cap in caps:
        capped = dict(ref, count=np.where(ref["count"] < 0, -1, np.minimum(ref["count"], cap)).astype(np.int32))
        _check_count(_routes(p, off, grid, radius, bound, counts=counts, max_count=cap, dense=dense), capped)
    for m in mins:
        _check_filter(_routes(p, off, grid, radius, bound, counts=counts, min_neighbors=m, dense=dense),
                      REF.filter_ragged(p, off, grid, radius, m, bound, counts, uncapped=ref), B)
    return ref


# ---- 1. sizes ------------------------------------------------------------------------------------------------------------------------------
LENGTHS = [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 4097]


@gpu
def test_sizes_in_one_ragged_batch():
    """Clouds of 0 .. 4097 rows around the wave (64) and the blocks (256, 1024) in one batch; with chunks of 1024 the longest spans 5.
    Rows are uniform in [-0.03, 1.03)^3, so some lie outside the box [0, 1]^3 of the grid (cell edge = radius = 0.1)."""
    off = _offsets(LENGTHS)
    p = np.random.RandomState(5).uniform(-0.03, 1.03, size=(off[-1], 3)).astype(F32)
    grid = REF.cube_grid(0.0, 1.0, 0.1)
    assert -(-4097 // 1024) == 5
    ref = _count_and_filter(p, off, grid, 0.1, max(LENGTHS), caps=(3,), mins=(2,))
    assert 0 < (ref["count"] == -1).sum() < 0.3 * len(p) and ref["count"].max() > 10
    # every cloud alone, its length as the bound, through the rald_post_ entries as well
    for b in (1, 2, 5, 8, 10):
        n = LENGTHS[b]
        one = REF.radius_ragged(p[off[b]:off[b + 1]], [0, n], grid, 0.1, n)
        assert np.array_equal(one["count"], ref["count"][off[b]:off[b + 1]]) and np.array_equal(one["nn_idx"], ref["nn_idx"][off[b]:off[b + 1]])
        _check_count(_run(p[off[b]:off[b + 1]], [0, n], grid, 0.1, n, post=True), one)
        _check_filter(_run(p[off[b]:off[b + 1]], [0, n], grid, 0.1, n, post=True, min_neighbors=2),
                      REF.filter_ragged(p[off[b]:off[b + 1]], [0, n], grid, 0.1, 2, n), 1)


# ---- 2. the lattice and the boundary constructions -----------------------------------------------------------------------------------------
@gpu
def test_lattice_with_duplicates():
    """Coordinates k * 2^-3, radius 2^-3: face neighbours lie at exactly r2 and count, diagonals do not, duplicates count each other,
    the nearest of equal distances is the smallest row."""
    p, grid, radius = REF.lattice_cloud()
    assert radius == 0.125 and len(p) == 1500
    ref = _count_and_filter(p, [0, len(p)], grid, radius, len(p))
    sites = {}
    for i, s in enumerate(map(tuple, np.round(p / F32(radius)).astype(int))):
        sites.setdefault(s, []).append(i)
    want = np.array([sum(len(sites.get((s[0] + d[0], s[1] + d[1], s[2] + d[2]), ())) for d in
                         ((0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))) - 1
                     for s in map(tuple, np.round(p / F32(radius)).astype(int))])
    assert np.array_equal(ref["count"], want) and max(len(v) for v in sites.values()) >= 3
    dup = [v for v in sites.values() if len(v) >= 2]
    assert all(ref["nn_idx"][v[0]] == v[1] and ref["nn_dist2"][v[0]] == 0 for v in dup)          # the duplicate; of several, the smallest
    assert all(ref["nn_idx"][i] == v[0] for v in dup for i in v[1:])
    r2 = F32(radius) * F32(radius)
    lone = [i for i in range(len(p)) if ref["count"][i] > 0 and ref["nn_dist2"][i] == r2]
    assert lone and all(ref["nn_idx"][i] == min(j for j in range(len(p)) if j != i and np.abs(p[j] - p[i]).sum() == F32(radius)) for i in lone[:20])


@gpu
@pytest.mark.parametrize("name", ["lattice_ulp", "pairs", "faces", "far_box", "uniform"])
def test_boundary_constructions(name):
    """The clouds on which a scan that is too narrow loses neighbours (tests/test_radius_filter_host.py holds the reference against an
    independent walk on the same clouds)."""
    p, grid, radius = REF.CONSTRUCTIONS[name]()
    ref = _count_and_filter(p, [0, len(p)], grid, radius, len(p), caps=(1,), mins=(1, 2))
    assert (ref["count"] > 0).any() and (ref["count"] >= 0).all()


# ---- 3. the grid does not show -------------------------------------------------------------------------------------------------------------
@gpu
def test_grid_independence():
    """The same cloud with cells of (r, r, r), (r, 2r, 1.5r) and (64r, r, r) - one cell on an axis - and with a shifted lo that keeps
    every row inside: equal outputs."""
    r = 0.05
    p = np.random.RandomState(9).uniform(0.2, 1.4, size=(3000, 3)).astype(F32)
    p[1500:] = p[:1500] + np.random.RandomState(10).uniform(-0.04, 0.04, size=(1500, 3)).astype(F32)
    off = [0, len(p)]
    ref = REF.radius_ragged(p, off, REF.cube_grid(0.0, 1.6, r), r, len(p))
    assert (ref["count"] >= 1).mean() > 0.5 and (ref["count"] >= 0).all() and REF.cube_grid(0.0, 1.6, (64 * r, r, r))[2][0] == 1
    fref = REF.filter_ragged(p, off, REF.cube_grid(0.0, 1.6, r), r, 3, len(p), uncapped=ref)
    assert 0 < len(fref["index"]) < len(p)
    for grid in (REF.cube_grid(0.0, 1.6, r), REF.cube_grid(0.0, 1.6, (r, 2 * r, 1.5 * r)), REF.cube_grid(0.0, 1.6, (64 * r, r, r)),
                 REF.cube_grid(-0.0137, 1.6, r), REF.cube_grid(-7.3, 1.6, (r, 1.25 * r, r))):
        _check_count(_routes(p, off, grid, r, len(p)), ref)
        _check_filter(_routes(p, off, grid, r, len(p), min_neighbors=3), fref, 1)


# ---- 4. ragged batches -----------------------------------------------------------------------------------------------------------------------
@gpu
def test_ragged_batch_counts_and_dense():
    """B = 5 with an empty cloud, a one-row cloud and a `counts` that trims; a loose and a tight host bound; the dense layout.  Every
    cloud equals the same cloud alone."""
    lengths = [700, 0, 1, 1500, 1100]
    off = _offsets(lengths)
    p = np.random.RandomState(12).uniform(0.0, 0.6, size=(off[-1], 3)).astype(F32)
    grid, r = REF.cube_grid(0.0, 0.6, 0.05), 0.05
    ref = _count_and_filter(p, off, grid, r, 1500, caps=(3,), mins=(2,))
    for b in range(5):
        alone = REF.radius_ragged(p[off[b]:off[b + 1]], [0, lengths[b]], grid, r, max(lengths[b], 1))
        assert np.array_equal(alone["count"], ref["count"][off[b]:off[b + 1]])
    assert _same(_run(p, off, grid, r, 1500), _run(p, off, grid, r, 10 ** 6))                     # a loose host bound does not show
    for counts, bound in (([650, 5, 1, 1024, 0], 1500), ([-5, 1 << 30, 7, 1, 1025], 1500), ([700, 0, 1, 1500, 1100], 1000)):
        _count_and_filter(p, off, grid, r, bound, counts=counts, caps=(), mins=(2,))
    dense_off = _offsets([800] * 4)
    ref = _count_and_filter(p[:3200], dense_off, grid, r, 800, caps=(3,), mins=(2,), dense=True)
    _count_and_filter(p[:3200], dense_off, grid, r, 800, counts=[800, 0, 13, 799], caps=(), mins=(1,), dense=True)
    assert np.array_equal(ref["count"][:800], REF.radius_one(p[:800], grid, r)["count"])


# ---- 5. rows outside -------------------------------------------------------------------------------------------------------------------------
@gpu
def test_outside_rows_take_no_part():
    """NaN, +-inf and rows outside the box among 2000 others, some of them right beside inside rows: count -1, nearest -1 / +inf, never
    anybody's neighbour, dropped by the filter."""
    rs = np.random.RandomState(14)
    p = rs.uniform(0.0, 0.5, size=(2000, 3)).astype(F32)
    grid, r = REF.cube_grid(0.0, 0.5, 0.05), 0.05
    bad = rs.choice(2000, size=300, replace=False)
    p[bad[:60], rs.randint(0, 3, 60)] = np.nan
    p[bad[60:120], rs.randint(0, 3, 60)] = np.inf
    p[bad[120:180], rs.randint(0, 3, 60)] = -np.inf
    p[bad[180:240], 0] = F32(-0.001)                                                                # just below the box, within r of inside rows
    p[bad[240:], 2] = F32(0.56)                                                                     # the cells end at 0.55
    ref = _count_and_filter(p, [0, 2000], grid, r, 2000, caps=(2,), mins=(1, 3))
    assert (ref["count"][bad] == -1).all() and (ref["nn_idx"][bad] == -1).all() and np.isposinf(ref["nn_dist2"][bad]).all()
    good = np.setdiff1d(np.arange(2000), bad)
    assert (ref["count"][good] >= 0).all() and not np.isin(ref["nn_idx"][good], bad).any()
    clean = REF.radius_one(p[good], grid, r)
    assert np.array_equal(clean["count"], ref["count"][good])                                       # as if the outside rows were not there


# ---- 6. degenerate clouds ------------------------------------------------------------------------------------------------------------------
@gpu
def test_degenerate_clouds():
    """300 duplicates of one point and 300 rows in one cell: every count n - 1; the nearest of a duplicate is row 0 (row 1 for row 0)."""
    grid, r = REF.cube_grid(0.0, 1.0, 0.25), 0.25
    dup = np.tile(np.array([[0.3, 0.6, 0.9]], F32), (300, 1))
    ref = _count_and_filter(dup, [0, 300], grid, r, 300, caps=(1, 299, 300), mins=(1, 299, 300))
    assert (ref["count"] == 299).all() and ref["nn_idx"].tolist() == [1] + [0] * 299 and (ref["nn_dist2"] == 0).all()
    cell = (np.random.RandomState(15).uniform(0.26, 0.3, size=(300, 3))).astype(F32)
    ref = _count_and_filter(cell, [0, 300], grid, r, 300, caps=(7,), mins=(299, 300))
    assert (ref["count"] == 299).all()
    both = np.concatenate([dup, cell, dup[:1]])
    _count_and_filter(both, [0, 300, 600, 601], grid, r, 300, caps=(), mins=(1,))


# ---- 7. stale state ------------------------------------------------------------------------------------------------------------------------
@gpu
def test_results_do_not_depend_on_stale_state():
    """The same bits on a second call and after a launch that fills every CU's LDS with NaN patterns."""
    from rald_amd._handles import _stream
    from rald_amd._lib import check, lib
    lengths = [1025, 0, 2049, 65]
    off = _offsets(lengths)
    p = np.random.RandomState(16).uniform(0.0, 0.5, size=(off[-1], 3)).astype(F32)
    grid, r = REF.cube_grid(0.0, 0.5, 0.05), 0.05
    for kw in (dict(), dict(max_count=2), dict(min_neighbors=3)):
        for chunk in (1024, 0):
            first = _run(p, off, grid, r, 2049, chunk=chunk, **kw)
            assert _same(first, _run(p, off, grid, r, 2049, chunk=chunk, **kw))
            check(lib().rald_debug_poison_lds(_stream()))
            assert _same(first, _run(p, off, grid, r, 2049, chunk=chunk, **kw))


# ---- 8. past the scans' 256 lanes --------------------------------------------------------------------------------------------------------------
@gpu
def test_filter_one_cloud_of_257_row_blocks():
    """262 145 rows are 257 blocks of 1024 rows, one more than the 256 lanes of the per-cloud scan of the block counts: its second turn
    starts from the first one's carry.  The reference is by construction (the brute force is quadratic): every row has its own integer
    x in 0 .. 262144 (exact in float32), z = 0, and y = 0 except for a seeded set of lifted rows - single ones and short runs in x - at
    y = 10, so with radius 1 a row's neighbours are the rows at x - 1 and x + 1 on its own level, at d2 = 1 = r2 exactly.  The rows
    come in a seeded random order."""
    from rald_amd.postprocess import voxel_grid
    n = 256 * 1024 + 1
    rs = np.random.RandomState(33)
    lifted = np.zeros(n, bool)
    lifted[rs.randint(0, n, size=3000)] = True                       # single rows (where two meet, a run)
    for start, length in zip(rs.randint(0, n - 8, size=2000), rs.randint(2, 8, size=2000)):
        lifted[start:start + length] = True
    same = lifted[1:] == lifted[:-1]                                  # x and x + 1 on one level
    by_x = np.concatenate([[False], same]).astype(np.int32) + np.concatenate([same, [False]])
    x = rs.permutation(n)
    p = np.stack([x, np.where(lifted[x], 10.0, 0.0), np.zeros(n)], axis=1).astype(F32)
    assert np.array_equal(p[:, 0].astype(np.int64), x)
    count = by_x[x].astype(np.int32)
    kept = np.nonzero(count >= 2)[0]
    assert (count == 0).sum() > 500 and (count == 1).sum() > 4000 and 0.9 * n < len(kept) < n - 5000
    ref = dict(points=p[kept], offsets=np.array([0, len(kept)], np.int64), index=kept.astype(np.int64), count=count, untouched=np.zeros(n, bool))
    grid = voxel_grid((0, -1, -1), (262144, 11, 1), 1.0)
    assert grid[2] == (262145, 13, 3)
    _check_filter(_run(p, [0, n], grid, 1.0, n, min_neighbors=2), ref, 1)


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------------
@gpu
def test_python_layer():
    from rald_amd import postprocess as PP
    off = _offsets([700, 0, 2100])
    p = np.random.RandomState(17).uniform(-0.02, 0.52, size=(off[-1], 3)).astype(F32)
    r = 0.05
    grid = PP.voxel_grid((0, 0, 0), (0.5, 0.5, 0.5), r)
    ref = REF.radius_ragged(p, off, grid, r, 2100)
    dp, doff = torch.from_numpy(p).cuda(), torch.tensor(off, device="cuda")
    cnt = PP.radius_neighbor_count_ragged(dp, doff, r, grid, 2100)
    assert cnt.dtype == torch.int32 and np.array_equal(cnt.cpu().numpy(), ref["count"])
    cnt, nn_idx, nn_d = PP.radius_neighbor_count_ragged(dp, doff, r, grid, 2100, return_nearest=True, chunk=1024)
    assert np.array_equal(cnt.cpu().numpy(), ref["count"]) and np.array_equal(nn_idx.cpu().numpy(), ref["nn_idx"])
    assert nn_idx.dtype == torch.int64 and np.array_equal(_bits(nn_d.cpu().numpy()), _bits(ref["nn_dist2"]))
    capped = PP.radius_neighbor_count_ragged(dp, doff, r, grid, 2100, max_count=2)
    assert np.array_equal(capped.cpu().numpy(), np.where(ref["count"] < 0, -1, np.minimum(ref["count"], 2)))
    fref = REF.filter_ragged(p, off, grid, r, 3, 2100)
    M = int(fref["offsets"][-1])
    out = PP.remove_radius_outliers_ragged(dp, doff, r, 3, grid, 2100, return_index=True, return_count=True)
    assert len(out) == 4 and out[1].tolist() == fref["offsets"].tolist() and 0 < M < len(p)
    assert np.array_equal(_bits(out[0][:M].cpu().numpy()), _bits(fref["points"])) and np.array_equal(out[2][:M].cpu().numpy(), fref["index"])
    assert np.array_equal(out[3].cpu().numpy(), fref["count"]) and out[2].dtype == torch.int64 and out[3].dtype == torch.int32
    assert len(PP.remove_radius_outliers_ragged(dp, doff, r, 3, grid, 2100)) == 2
    # one cloud, with bounds and with its own extent
    one = PP.remove_radius_outliers(dp[:700], r, 3, lo=(0, 0, 0), hi=(0.5, 0.5, 0.5))
    assert np.array_equal(_bits(one.cpu().numpy()), _bits(fref["points"][:int(fref["offsets"][1])]))
    q = p[:700]
    own = PP.remove_radius_outliers(dp[:700], r, 2)
    want = REF.filter_ragged(q, [0, 700], PP.voxel_grid(q.min(axis=0).tolist(), q.max(axis=0).tolist(), r), r, 2, 700)
    assert np.array_equal(_bits(own.cpu().numpy()), _bits(want["points"])) and (want["count"] >= 0).all()
    with pytest.raises(RuntimeError):
        PP.radius_neighbor_count_ragged(torch.from_numpy(p), doff, r, grid, 2100)


# ---- the tail ------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_infer_point_clouds_denoise():
    """infer_point_clouds(..., denoise=(0.5, 3)) on the 4-frame setup of tests/test_gpu_infer_batch.py: the new keys equal
    remove_radius_outliers and the reference applied to the 'pred' it returned, every other key equals the call without the argument;
    then with thin and resample on top, whose indices count rows of 'denoised'."""
    import fps_ref
    import voxel_ref
    from rald_amd import engine_generation as E, postprocess as PP, query_points as QP, synth
    from test_gpu_infer_batch import _small_vae, _tail_args
    vae, z9 = _small_vae()
    z = z9[:4].contiguous()
    n, aug, k = 3000, 2048, 100
    radius, need = 0.5, 3
    args = _tail_args(n, aug)
    helpers = [synth.queries(1, max(h, 1), seed=100 + h)[0][:h].cuda() for h in (0, 1, 500, 1100)]
    surfaces = synth.point_cloud(4, 1000, seed=62).cuda()
    draws = QP.draw_tail_randoms(4, n, aug, 10, torch.Generator("cuda").manual_seed(23))
    kw = dict(helper_points=helpers, surfaces=surfaces, draws=draws)
    grid = PP.voxel_grid([-15.8] * 3, [15.8] * 3, radius)
    base = E.infer_point_clouds(vae, z, args, **kw)
    res = E.infer_point_clouds(vae, z, args, denoise=(radius, need), **kw)
    assert set(res) == set(base) | {"denoised", "denoise_index", "cd_denoised"} and res["n_queries"] == base["n_queries"]
    assert all(torch.equal(a, b) for a, b in zip(res["pred"], base["pred"]))
    assert all(a == b or abs(a - b) <= 1e-9 * abs(b) for a, b in zip(res["cd"], base["cd"]))      # cal_metrics_ragged's double atomics

    def check_denoise(r):
        refs = []
        for b in range(4):
            pred = r["pred"][b]
            ref = REF.filter_ragged(pred.cpu().numpy(), [0, pred.shape[0]], grid, radius, need, max(pred.shape[0], 1))
            assert np.array_equal(r["denoise_index"][b].cpu().numpy(), ref["index"]) and r["denoise_index"][b].dtype == torch.int64, b
            assert np.array_equal(_bits(r["denoised"][b].cpu().numpy()), _bits(ref["points"])), b
            assert torch.equal(r["denoised"][b], PP.remove_radius_outliers(pred, radius, need, lo=[-15.8] * 3, hi=[15.8] * 3))
            assert torch.equal(r["denoised"][b], pred[r["denoise_index"][b]])
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
    with_n = E.infer_point_clouds(vae, z, args, denoise=(radius, need), normals=True, metric_thresholds=(0.1, 0.5), **kw)
    check_denoise(with_n)
    assert set(with_n) == set(res) | {"normals", "denoised_normals", "metrics", "metrics_denoised"}
    for b in range(4):
        assert torch.equal(with_n["denoised_normals"][b], with_n["normals"][b][with_n["denoise_index"][b]])
        assert with_n["metrics_denoised"][b]["cd"] == with_n["cd_denoised"][b] and with_n["metrics"][b]["cd"] == with_n["cd"][b]
    # thin and resample on top: both run on the denoised clouds
    both = E.infer_point_clouds(vae, z, args, denoise=(radius, need), thin=1.0, resample=k, **kw)
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
    only = E.infer_point_clouds(vae, z, args, denoise=(radius, need), resample=k, **kw)
    lengths = [len(r["index"]) for r in refs]
    want_pts, want_idx = fps_ref.resample_ref(np.concatenate([r["points"] for r in refs]), _offsets(lengths), k, max(max(lengths), 1))
    assert np.array_equal(only["resample_index"].cpu().numpy(), want_idx) and np.array_equal(_bits(only["resampled"].cpu().numpy()), _bits(want_pts))
    dev = E.infer_point_clouds_device(vae, z, args, denoise=(radius, need), thin=1.0, resample=k, **kw)
    assert len(dev) == 13 and dev[4].tolist() == _offsets([len(r["index"]) for r in refs]) and torch.equal(dev[-1], both["resample_index"])
    with pytest.raises(ValueError):
        E.infer_point_clouds(vae, z, args, denoise=(0.01, 2), **kw)
