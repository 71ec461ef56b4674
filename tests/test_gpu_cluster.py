"""Density clustering and small-cluster removal on the GPU (rald_amd/csrc/cloud_cluster.hip) against tests/cluster_ref.py, by
equality: integers as integers, floats by bit pattern.  Every call goes through _run: the outputs are pre-filled with poison (NaN with
a payload, -7) and followed by guard rows, the input rows the kernels must not read (behind counts, behind the bound, behind
offsets[B]) are NaN, the scratch is followed by a guard, and the checks assert that everything the definition does not write still
holds its poison.  Every case runs the sort's three routes - chunks of 1024, one workgroup, automatic - and compares the three."""
import ctypes as C

import numpy as np
import pytest
import torch

import cluster_ref as REF
import radius_ref
from test_gpu_radius_filter import F32, GUARD, POISON_F, POISON_I, _bits, _offsets, _one_chunk, _same, _spans

gpu = pytest.mark.gpu


def _run(points, offsets, grid, eps, min_points, bound, counts=None, chunk=0, post=False, keep=None, dense=False, optional=True):
    """The C entries on poisoned, guarded buffers -> dict of numpy arrays, whole buffers (guards included): the labels call (with sizes
    and count unless optional is False) or, with keep = (min_cluster_size, largest_only), the filter.  dense: offsets describe equal
    clouds, passed as n_dense with a NULL offsets pointer."""
    from rald_amd._handles import _stream
    from rald_amd._lib import check, lib
    p = np.array(points, F32).reshape(-1, 3)
    T, B = len(p), len(offsets) - 1
    dev_p = np.concatenate([p, np.zeros((GUARD, 3), F32)])
    dev_p[_spans(T, offsets, bound, counts)] = np.nan
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    t = dict(points=cu(dev_p), offsets=None if dense else cu(np.array(offsets, np.int64)),
             counts=None if counts is None else cu(np.array(counts, np.int32)), labels=cu(np.full(T + GUARD, POISON_I, np.int32)),
             num=cu(np.full(B + GUARD, POISON_I, np.int32)))
    n_dense = offsets[1] - offsets[0] if dense else 0
    L = lib()
    nbytes = L.rald_post_cluster_scratch_bytes(B, T, bound) if post else L.rald_op_cluster_scratch_bytes(B, T, bound, chunk)
    assert nbytes > 0
    scratch = torch.empty(nbytes + 16 * GUARD, dtype=torch.uint8, device="cuda")
    scratch[nbytes:] = 0xA5
    lo3, v3, dims3 = (C.c_float * 3)(*grid[0]), (C.c_float * 3)(*grid[1]), (C.c_int32 * 3)(*grid[2])
    ptr = lambda k: None if t.get(k) is None else t[k].data_ptr()
    head = (ptr("points"), ptr("offsets"), ptr("counts"), B, n_dense, T, bound, lo3, v3, dims3, float(eps), int(min_points))
    tail = (scratch.data_ptr(), nbytes) + (() if post else (chunk,)) + (_stream(),)
    if keep is None:
        if optional:
            t.update(sizes=cu(np.full(T + GUARD, POISON_I, np.int32)), count=cu(np.full(T + GUARD, POISON_I, np.int32)))
        fn = L.rald_post_cluster_labels_ragged if post else L.rald_op_cluster_labels_ragged
        check(fn(*head, ptr("labels"), ptr("num"), ptr("sizes"), ptr("count"), *tail))
        keys = ("labels", "num", "sizes", "count")
    else:
        t.update(out=cu(np.full((T + GUARD, 3), POISON_F, F32)), out_offsets=cu(np.full(B + 1 + GUARD, POISON_I, np.int64)))
        if optional:
            t.update(index=cu(np.full(T + GUARD, POISON_I, np.int64)))
        fn = L.rald_post_cluster_filter_ragged if post else L.rald_op_cluster_filter_ragged
        check(fn(*head, int(keep[0]), int(keep[1]), ptr("out"), ptr("out_offsets"), ptr("index"), ptr("labels"), ptr("num"), *tail))
        keys = ("labels", "num", "out", "out_offsets", "index")
    torch.cuda.synchronize()
    assert bool((scratch[nbytes:] == 0xA5).all()), "the scratch's guard was written"
    return {k: t[k].cpu().numpy() for k in keys if k in t}


def _routes(points, offsets, grid, eps, min_points, bound, **kw):
    """The call by chunks of 1024, by one workgroup and by the automatic rule -> the first result; the three must be the same bits."""
    runs = [_run(points, offsets, grid, eps, min_points, bound, chunk=c, **kw) for c in (1024, _one_chunk(bound), 0)]
    for other in runs[1:]:
        assert _same(runs[0], other)
    return runs[0]


def _check_labels(got, ref):
    """Everything the labels call writes equals the reference; everything else still holds its poison."""
    T, B = len(ref["labels"]), len(ref["num_clusters"])
    un = ref["untouched"]
    for k in ("labels", "sizes", "count"):
        if k in got:
            want = np.where(un, POISON_I, ref[k])
            bad = np.nonzero(got[k][:T] != want)[0]
            assert bad.size == 0, (k, bad[:5], got[k][bad[:5]], want[bad[:5]])
            assert (got[k][T:] == POISON_I).all(), k
    assert got["num"][:B].tolist() == ref["num_clusters"].tolist() and (got["num"][B:] == POISON_I).all()


def _check_filter(got, ref, B):
    M = int(ref["offsets"][-1])
    assert got["out_offsets"][:B + 1].tolist() == ref["offsets"].tolist() and (got["out_offsets"][B + 1:] == POISON_I).all()
    if "index" in got:
        assert np.array_equal(got["index"][:M], ref["index"]) and (got["index"][M:] == POISON_I).all()
    assert np.array_equal(_bits(got["out"][:M]), _bits(ref["points"])) and (_bits(got["out"][M:]) == _bits(POISON_F)).all()
    bad = np.nonzero(got["labels"][:M] != ref["labels"])[0]
    assert bad.size == 0, (bad[:5], got["labels"][bad[:5]], ref["labels"][bad[:5]])
    assert (got["labels"][M:] == POISON_I).all()
    assert got["num"][:B].tolist() == ref["num_clusters"].tolist() and (got["num"][B:] == POISON_I).all()


def _labelled(name, min_points):
    """cluster_ref.reference as the one-cloud result of cluster_ragged."""
    one = REF.reference(name, min_points)
    return dict(labels=one["labels"], sizes=one["sizes"], count=one["count"], num_clusters=np.array([one["num_clusters"]], np.int32),
                untouched=np.zeros(len(one["labels"]), bool))


def _labels_and_filter(p, off, grid, eps, min_points, bound, keeps, counts=None, dense=False, ref=None):
    """The whole surface on one batch, every route: the labels with sizes and count, then the filter for every (size, largest_only)."""
    B = len(off) - 1
    ref = REF.cluster_ragged(p, off, grid, eps, min_points, bound, counts) if ref is None else ref
    _check_labels(_routes(p, off, grid, eps, min_points, bound, counts=counts, dense=dense), ref)
    kept = []
    for keep in keeps:
        want = REF.filter_ragged(p, off, grid, eps, min_points, keep[0], bound, counts, largest_only=keep[1], labelled=ref)
        _check_filter(_routes(p, off, grid, eps, min_points, bound, counts=counts, keep=keep, dense=dense), want, B)
        kept.append(int(want["offsets"][-1]))
    return ref, kept


# ---- 1. the constructions ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name,min_points", REF.CASE_IDS)
def test_constructions(name, min_points):
    """Labels, num_clusters, sizes and count on every cloud of tests/cluster_ref.py (tests/test_cluster_host.py holds the reference
    against an independent route on the same clouds and shows what each is for), then the filter: every cluster, the clusters above a
    middle size, the largest one, and a size above every cluster, which leaves an empty cloud."""
    p, grid, eps = REF.cloud(name)
    ref = _labelled(name, min_points)
    sizes = ref["sizes"][:int(ref["num_clusters"][0])]
    top = int(sizes.max()) if len(sizes) else 0
    middle = max(2, int(np.sort(sizes)[len(sizes) // 2])) if len(sizes) else 2
    _, kept = _labels_and_filter(p, [0, len(p)], grid, eps, min_points, len(p), [(1, 0), (middle, 0), (1, 1), (top + 1, 0)], ref=ref)
    assert kept[0] == (ref["labels"] >= 0).sum() and kept[2] == top and kept[3] == 0 and kept[1] <= kept[0]
    if name == "two_chains":                                         # a size tie of two clusters: the smaller id is the largest
        assert sizes.tolist() == [1250, 1250] and kept[2] == 1250


# ---- 2. ragged batches ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_ragged_batch_counts_and_dense():
    """B = 5 with an empty cloud, a one-row cloud, a cloud entirely outside the box and a `counts` that trims; a loose and a tight host
    bound; the dense layout; the rald_post_ entries; without the optional outputs.  Every cloud equals the same cloud alone."""
    lengths = [700, 0, 1, 1500, 1100]
    off = _offsets(lengths)
    p = np.random.RandomState(21).uniform(0.0, 0.6, size=(off[-1], 3)).astype(F32)
    p[off[3]:off[4]] += F32(10.0)
    grid, e = radius_ref.cube_grid(0.0, 0.6, 0.05), 0.05
    keeps = [(3, 0), (1, 1)]
    ref, _ = _labels_and_filter(p, off, grid, e, 3, 1500, keeps)
    assert ref["num_clusters"][[1, 3]].tolist() == [0, 0] and (ref["labels"][off[3]:off[4]] == -2).all() and ref["num_clusters"][0] >= 2
    assert (ref["labels"][:700] == -1).any() and ((ref["labels"][:700] >= 0) & (ref["count"][:700] < 3)).any()      # noise and border rows
    for b in range(5):
        n = lengths[b]
        alone = REF.cluster_ragged(p[off[b]:off[b + 1]], [0, n], grid, e, 3, max(n, 1))
        assert np.array_equal(alone["labels"], ref["labels"][off[b]:off[b + 1]]) and alone["num_clusters"][0] == ref["num_clusters"][b]
        if n:
            _check_labels(_run(p[off[b]:off[b + 1]], [0, n], grid, e, 3, n, post=True), alone)
            want = REF.filter_ragged(p[off[b]:off[b + 1]], [0, n], grid, e, 3, 3, n, labelled=alone)
            _check_filter(_run(p[off[b]:off[b + 1]], [0, n], grid, e, 3, n, post=True, keep=(3, 0)), want, 1)
    assert _same(_run(p, off, grid, e, 3, 1500), _run(p, off, grid, e, 3, 10 ** 6))                   # a loose host bound does not show
    assert _same(_run(p, off, grid, e, 3, 1500, chunk=0), _run(p, off, grid, e, 3, 1500, post=True))  # rald_post_* is rald_op_* at chunk 0
    assert _same(_run(p, off, grid, e, 3, 1500, keep=(3, 0)), _run(p, off, grid, e, 3, 1500, keep=(3, 0), post=True))
    bare = _run(p, off, grid, e, 3, 1500, optional=False)
    assert set(bare) == {"labels", "num"}
    _check_labels(bare, ref)
    _check_filter(_run(p, off, grid, e, 3, 1500, keep=(3, 0), optional=False),
                  REF.filter_ragged(p, off, grid, e, 3, 3, 1500, labelled=ref), 5)
    for counts, bound in (([650, 5, 1, 1024, 0], 1500), ([-5, 1 << 30, 7, 1, 1025], 1500), ([700, 0, 1, 1500, 1100], 1000)):
        _labels_and_filter(p, off, grid, e, 3, bound, keeps[:1], counts=counts)
    for mp in (0, 1):
        _labels_and_filter(p, off, grid, e, mp, 1500, [(2, 0)])
    dense_off = _offsets([800] * 4)
    ref, _ = _labels_and_filter(p[:3200], dense_off, grid, e, 3, 800, keeps, dense=True)
    _labels_and_filter(p[:3200], dense_off, grid, e, 3, 800, keeps[:1], counts=[800, 0, 13, 799], dense=True)
    assert np.array_equal(ref["labels"][:800], REF.cluster_one(p[:800], grid, e, 3)["labels"])


# ---- 3. rows outside -----------------------------------------------------------------------------------------------------------------------
@gpu
def test_outside_rows_take_no_part():
    """NaN, +-inf and rows outside the box among 2000 others, some right beside inside rows: label -2, count -1, never anybody's
    neighbour, dropped by the filter - the labels of the others are those of the cloud without them."""
    rs = np.random.RandomState(22)
    p = rs.uniform(0.0, 0.5, size=(2000, 3)).astype(F32)
    grid, e = radius_ref.cube_grid(0.0, 0.5, 0.05), 0.05
    bad = rs.choice(2000, size=300, replace=False)
    p[bad[:60], rs.randint(0, 3, 60)] = np.nan
    p[bad[60:120], rs.randint(0, 3, 60)] = np.inf
    p[bad[120:180], rs.randint(0, 3, 60)] = -np.inf
    p[bad[180:240], 0] = F32(-0.001)
    p[bad[240:], 2] = F32(0.56)
    for mp in (0, 4):
        ref, _ = _labels_and_filter(p, [0, 2000], grid, e, mp, 2000, [(2, 0), (1, 1)])
        good = np.setdiff1d(np.arange(2000), bad)
        assert (ref["labels"][bad] == -2).all() and (ref["count"][bad] == -1).all() and (ref["labels"][good] >= -1).all()
        clean = REF.cluster_one(p[good], grid, e, mp)
        assert np.array_equal(clean["labels"], ref["labels"][good]) and clean["num_clusters"] == ref["num_clusters"][0]


# ---- 4. the grid does not show -------------------------------------------------------------------------------------------------------------
@gpu
def test_grid_independence():
    """The same cloud with cells of (e, e, e), (e, 2e, 1.5e) and (64e, e, e) - one cell on an axis - and with a shifted lo that keeps
    every row inside: equal outputs."""
    e = 0.05
    p = np.random.RandomState(23).uniform(0.2, 1.4, size=(2000, 3)).astype(F32)
    p[1000:] = p[:1000] + np.random.RandomState(24).uniform(-0.04, 0.04, size=(1000, 3)).astype(F32)
    off = [0, len(p)]
    ref = REF.cluster_ragged(p, off, radius_ref.cube_grid(0.0, 1.6, e), e, 2, len(p))
    assert ref["num_clusters"][0] > 10 and (ref["labels"] == -1).any() and (ref["labels"] > -2).all()
    fref = REF.filter_ragged(p, off, radius_ref.cube_grid(0.0, 1.6, e), e, 2, 4, len(p), labelled=ref)
    assert 0 < len(fref["index"]) < (ref["labels"] >= 0).sum()
    for grid in (radius_ref.cube_grid(0.0, 1.6, e), radius_ref.cube_grid(0.0, 1.6, (e, 2 * e, 1.5 * e)),
                 radius_ref.cube_grid(0.0, 1.6, (64 * e, e, e)), radius_ref.cube_grid(-0.0137, 1.6, e)):
        _check_labels(_routes(p, off, grid, e, 2, len(p)), ref)
        _check_filter(_routes(p, off, grid, e, 2, len(p), keep=(4, 0)), fref, 1)


# ---- 5. stale state ------------------------------------------------------------------------------------------------------------------------
@gpu
def test_results_do_not_depend_on_stale_state():
    """The same bits on a second call and after a launch that fills every CU's LDS with NaN patterns."""
    from rald_amd._handles import _stream
    from rald_amd._lib import check, lib
    lengths = [1025, 0, 2049, 65]
    off = _offsets(lengths)
    p = np.random.RandomState(25).uniform(0.0, 0.5, size=(off[-1], 3)).astype(F32)
    grid, e = radius_ref.cube_grid(0.0, 0.5, 0.05), 0.05
    for kw in (dict(min_points=0), dict(min_points=3), dict(min_points=3, keep=(3, 0)), dict(min_points=1, keep=(1, 1))):
        for chunk in (1024, 0):
            first = _run(p, off, grid, e, bound=2049, chunk=chunk, **kw)
            assert _same(first, _run(p, off, grid, e, bound=2049, chunk=chunk, **kw))
            check(lib().rald_debug_poison_lds(_stream()))
            assert _same(first, _run(p, off, grid, e, bound=2049, chunk=chunk, **kw))


# ---- 6. one walk, one early stop -------------------------------------------------------------------------------------------------------------
@gpu
def test_capped_count_equals_the_radius_count():
    """rad_count and clu_count run the same radius_walk (cloud_index.h) and must stop it at the same cap: for caps 1 and 3 the capped
    count of radius_neighbor_count_ragged, cluster_dbscan_ragged's count and the brute-force reference are equal, on one ragged batch
    of 0, 257 and 1025 rows (one past rad_count's workgroup of 256 positions, one past a CLOUD_SEG of 1024): a lattice of 11^3 sites of
    edge = cell = radius (face neighbours at exactly r2, duplicates) with a few rows outside the box, NaN and inf included."""
    from rald_amd import postprocess as PP
    e, side = 0.125, 11
    off = _offsets([0, 257, 1025])
    rs = np.random.RandomState(27)
    p = (rs.randint(0, side, size=(off[-1], 3)).astype(F32) * F32(e)).astype(F32)
    bad = np.concatenate([rs.choice(257, 8, replace=False), 257 + rs.choice(1025, 8, replace=False)])
    for rows, value in ((bad[0::4], np.nan), (bad[1::4], np.inf), (bad[2::4], -e), (bad[3::4], (side + 1) * e)):
        p[rows, rs.randint(0, 3, len(rows))] = F32(value)
    grid = radius_ref.cube_grid(0.0, side * e, e)
    free = radius_ref.radius_ragged(p, off, grid, e, 1025)["count"]
    sites = {tuple(s) for s in np.round(np.delete(p, bad, axis=0) / F32(e)).astype(int).tolist()}
    assert (free[bad] == -1).all() and (np.delete(free, bad) >= 0).all() and len(sites) < len(p) - len(bad)          # duplicates
    dp, doff = torch.from_numpy(p).cuda(), torch.tensor(off, device="cuda")
    for cap in (1, 3):
        ref = radius_ref.radius_ragged(p, off, grid, e, 1025, max_count=cap)["count"]
        for lo, hi in zip(off[1:], off[2:]):                                  # in each cloud the cap bites for some rows and not for others
            assert (free[lo:hi] > cap).any() and ((free[lo:hi] >= 0) & (free[lo:hi] < cap)).any()
        rad = PP.radius_neighbor_count_ragged(dp, doff, e, grid, 1025, max_count=cap).cpu().numpy()
        clu = PP.cluster_dbscan_ragged(dp, doff, e, cap, grid, 1025, return_count=True)[2].cpu().numpy()
        assert rad.dtype == clu.dtype == ref.dtype == np.int32
        assert np.array_equal(rad, ref) and np.array_equal(clu, ref) and np.array_equal(rad, clu)


# ---- 7. the largest cluster: ties past the argmax's 256 threads ------------------------------------------------------------------------------
def _pairs_cloud(triples):
    """300 groups of rows, group i at x = i, its rows 2^-6 apart: pairs, and triples for the groups named.  Group i is cluster i: the
    clusters are numbered by their smallest row, and the groups stand in row order."""
    step = F32(2.0 ** -6)
    rows = []
    for i in range(300):
        rows += [(i, 0, 0), (i + step, 0, 0)] + ([(i, step, 0)] if i in triples else [])
    return np.array(rows, F32)


@gpu
def test_largest_cluster_ties_beyond_one_stride_of_the_argmax():
    """clu_argmax gives thread t the clusters t, t + 256, ..: cluster 260 is thread 4's second.  All 300 clusters of size 2: cluster 0
    (every comparison of block_argmax's tree is a tie).  Cluster 260 alone of size 3: it wins from the second stride.  Clusters 4 and
    260 of size 3: thread 4 must keep the earlier one.  The properties are asserted of the reference first, then kept rows, index and
    labels are compared with it by equality."""
    from rald_amd.postprocess import voxel_grid
    eps = 2.0 ** -4
    grid = voxel_grid((-1, -1, -1), (301, 1, 1), eps)
    for triples, winner, first_row in (((), 0, 0), ((260,), 260, 520), ((4, 260), 4, 8)):
        p = _pairs_cloud(triples)
        n, size = len(p), 3 if triples else 2
        assert n == 600 + len(triples)
        ref = REF.cluster_ragged(p, [0, n], grid, eps, 1, n)
        sizes = ref["sizes"][:300].tolist()
        assert ref["num_clusters"].tolist() == [300] and sizes == [3 if i in triples else 2 for i in range(300)]
        assert ref["labels"][first_row] == winner and (ref["labels"][first_row:first_row + size] == winner).all()
        want = REF.filter_ragged(p, [0, n], grid, eps, 1, 1, n, largest_only=True, labelled=ref)
        assert want["index"].tolist() == list(range(first_row, first_row + size)) and want["labels"].tolist() == [winner] * size
        _check_filter(_routes(p, [0, n], grid, eps, 1, n, keep=(1, 1)), want, 1)


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------------
@gpu
def test_python_layer():
    from rald_amd import postprocess as PP
    off = _offsets([700, 0, 2100])
    p = np.random.RandomState(26).uniform(-0.02, 0.52, size=(off[-1], 3)).astype(F32)
    e = 0.05
    grid = PP.voxel_grid((0, 0, 0), (0.5, 0.5, 0.5), e)
    ref = REF.cluster_ragged(p, off, grid, e, 3, 2100)
    dp, doff = torch.from_numpy(p).cuda(), torch.tensor(off, device="cuda")
    out = PP.cluster_dbscan_ragged(dp, doff, e, 3, grid, 2100)
    assert len(out) == 2 and out[0].dtype == out[1].dtype == torch.int32
    assert np.array_equal(out[0].cpu().numpy(), ref["labels"]) and out[1].tolist() == ref["num_clusters"].tolist()
    out = PP.cluster_dbscan_ragged(dp, doff, e, 3, grid, 2100, return_sizes=True, return_count=True, chunk=1024)
    assert len(out) == 4 and all(np.array_equal(t.cpu().numpy(), ref[k]) for t, k in zip(out, ("labels", "num_clusters", "sizes", "count")))
    only = PP.cluster_dbscan_ragged(dp, doff, e, 3, grid, 2100, return_count=True)
    assert len(only) == 3 and np.array_equal(only[2].cpu().numpy(), ref["count"])
    fref = REF.filter_ragged(p, off, grid, e, 3, 5, 2100, labelled=ref)
    M = int(fref["offsets"][-1])
    out = PP.remove_small_clusters_ragged(dp, doff, e, 3, 5, grid, 2100, return_index=True, return_labels=True)
    assert len(out) == 5 and out[1].tolist() == fref["offsets"].tolist() and 0 < M < (ref["labels"] >= 0).sum()
    assert np.array_equal(_bits(out[0][:M].cpu().numpy()), _bits(fref["points"])) and np.array_equal(out[2][:M].cpu().numpy(), fref["index"])
    assert np.array_equal(out[3][:M].cpu().numpy(), fref["labels"]) and out[4].tolist() == ref["num_clusters"].tolist()
    assert out[2].dtype == torch.int64 and out[3].dtype == torch.int32
    assert len(PP.remove_small_clusters_ragged(dp, doff, e, 3, 5, grid, 2100)) == 2
    big = REF.filter_ragged(p, off, grid, e, 3, 1, 2100, largest_only=True, labelled=ref)
    out = PP.remove_small_clusters_ragged(dp, doff, e, 3, 1, grid, 2100, largest_only=True)
    assert out[1].tolist() == big["offsets"].tolist() and np.array_equal(_bits(out[0][:int(big["offsets"][-1])].cpu().numpy()), _bits(big["points"]))
    # one cloud, with bounds and with its own extent
    one = PP.cluster_dbscan(dp[:700], e, 3, lo=(0, 0, 0), hi=(0.5, 0.5, 0.5))
    assert one.dtype == torch.int32 and np.array_equal(one.cpu().numpy(), ref["labels"][:700])
    kept = PP.remove_small_clusters(dp[:700], e, 3, 5, lo=(0, 0, 0), hi=(0.5, 0.5, 0.5))
    assert np.array_equal(_bits(kept.cpu().numpy()), _bits(fref["points"][:int(fref["offsets"][1])]))
    q = p[:700]
    own = PP.cluster_dbscan(dp[:700], e, 2)
    want = REF.cluster_one(q, PP.voxel_grid(q.min(axis=0).tolist(), q.max(axis=0).tolist(), e), e, 2)
    assert np.array_equal(own.cpu().numpy(), want["labels"]) and (want["labels"] > -2).all()
    with pytest.raises(RuntimeError):
        PP.cluster_dbscan_ragged(torch.from_numpy(p), doff, e, 3, grid, 2100)


# ---- the tail ------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_infer_point_clouds_denoise_cluster(monkeypatch):
    """infer_point_clouds(..., denoise_cluster=(0.5, 3, 20)) on the 4-frame setup of tests/test_gpu_infer_batch.py: the new keys equal
    remove_small_clusters_ragged and the reference applied to the 'pred' it returned, 'pred' and 'cd' equal the call without the
    argument, and the number of host reads is the same (one)."""
    from rald_amd import engine_generation as E, postprocess as PP, query_points as QP, synth
    from test_gpu_infer_batch import _small_vae, _tail_args
    vae, z9 = _small_vae()
    z = z9[:4].contiguous()
    n, aug = 3000, 2048
    eps, mp, size = 0.5, 3, 20
    args = _tail_args(n, aug)
    helpers = [synth.queries(1, max(h, 1), seed=100 + h)[0][:h].cuda() for h in (0, 1, 500, 1100)]
    surfaces = synth.point_cloud(4, 1000, seed=62).cuda()
    draws = QP.draw_tail_randoms(4, n, aug, 10, torch.Generator("cuda").manual_seed(23))
    kw = dict(helper_points=helpers, surfaces=surfaces, draws=draws)
    grid = PP.voxel_grid([-15.8] * 3, [15.8] * 3, eps)

    def counted(**more):
        calls = []
        real_cpu = torch.Tensor.cpu
        with monkeypatch.context() as m:
            m.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (calls.append(1), real_cpu(self, *a, **k))[1])
            for name in ("item", "tolist", "numpy"):
                real = getattr(torch.Tensor, name)
                m.setattr(torch.Tensor, name, (lambda real: lambda self, *a, **k: (calls.append(1) if self.is_cuda else None, real(self, *a, **k))[1])(real))
            out = E.infer_point_clouds(vae, z, args, **kw, **more)
        return out, len(calls)
    base, base_reads = counted()
    res, reads = counted(denoise_cluster=(eps, mp, size))
    assert reads == base_reads == 1
    assert set(res) == set(base) | {"denoised", "denoise_index", "cd_denoised", "denoise_labels", "n_clusters"}
    assert res["n_queries"] == base["n_queries"] and all(torch.equal(a, b) for a, b in zip(res["pred"], base["pred"]))
    assert all(a == b or abs(a - b) <= 1e-9 * abs(b) for a, b in zip(res["cd"], base["cd"]))      # cal_metrics_ragged's double atomics
    stats = []
    for b in range(4):
        pred = res["pred"][b]
        m = pred.shape[0]
        ref = REF.filter_ragged(pred.cpu().numpy(), [0, m], grid, eps, mp, size, max(m, 1))
        assert np.array_equal(res["denoise_index"][b].cpu().numpy(), ref["index"]) and res["denoise_index"][b].dtype == torch.int64, b
        assert np.array_equal(_bits(res["denoised"][b].cpu().numpy()), _bits(ref["points"])), b
        assert np.array_equal(res["denoise_labels"][b].cpu().numpy(), ref["labels"]) and res["denoise_labels"][b].dtype == torch.int32, b
        assert res["n_clusters"][b] == int(ref["num_clusters"][0]) and torch.equal(res["denoised"][b], pred[res["denoise_index"][b]])
        off = torch.tensor([0, m], device="cuda")
        direct = PP.remove_small_clusters_ragged(pred, off, eps, mp, size, grid, max(m, 1), return_labels=True)
        k = int(direct[1][1].item())
        assert torch.equal(direct[0][:k], res["denoised"][b]) and torch.equal(direct[2][:k], res["denoise_labels"][b])
        want = PP.cal_metrics(res["denoised"][b], PP.polar2cartesian(PP.inverse_norm_points(surfaces[b], args.dataset.lidar.pc_range,
                                                                                            args.dataset.lidar.norm_anisotropy,
                                                                                            args.dataset.lidar.norm_isotropy)))
        got = res["cd_denoised"][b]
        assert got == want or abs(got - want) <= 1e-9 * abs(want), (b, got, want)
        stats.append((m, len(ref["index"]), int(ref["num_clusters"][0])))
    print("final clouds, their kept rows and clusters:", stats)
    assert any(0 < k < m for m, k, _ in stats) and any(c >= 2 for _, _, c in stats)
    largest, _ = counted(denoise_cluster=(eps, mp, 1, True), thin=1.0, resample=50)
    assert set(largest) == set(res) | {"thinned", "thin_count", "thin_first", "resampled", "resample_index"}
    for b in range(4):
        pred = largest["pred"][b]
        ref = REF.filter_ragged(pred.cpu().numpy(), [0, pred.shape[0]], grid, eps, mp, 1, max(pred.shape[0], 1), largest_only=True)
        assert np.array_equal(largest["denoise_index"][b].cpu().numpy(), ref["index"]) and len(set(ref["labels"].tolist())) <= 1
    dev = E.infer_point_clouds_device(vae, z, args, denoise_cluster=(eps, mp, size), **kw)
    assert len(dev) == 9 and dev[4].tolist() == _offsets([k for _, k, _ in stats]) and dev[8].tolist() == [c for _, _, c in stats]
    with pytest.raises(ValueError):
        E.infer_point_clouds(vae, z, args, denoise_cluster=(0.001, 2, 3), **kw)
