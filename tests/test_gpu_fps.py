"""Farthest-point sampling on the GPU against tests/fps_ref.py, the definition in numpy float32.  Everything is
compared by equality: idx as integers, dist2 by bit pattern; there is no tolerance anywhere.  Outputs are pre-filled with a poison value
and followed by guard rows that must survive; NaN rows sit behind every input row the kernel must not read (past counts[b], past
max_per_sample, past the last cloud).  Every case runs under both kernel forms unless it says otherwise."""
import numpy as np
import pytest
import torch

import fps_ref as REF

gpu = pytest.mark.gpu

FORMS = (1, 2)                                   # resident, streaming
POISON_I, POISON_D, GUARD = -987654321, -12345.5, 5
SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 4097)
RESIDENT_MAX = 16384
_CACHE = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _offsets(lengths):
    return np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)


def uniform_cloud(n, seed):
    key = ("uniform", n, seed)
    if key not in _CACHE:
        _CACHE[key] = np.random.RandomState(seed).uniform(-10, 10, size=(n, 3)).astype(np.float32)
    return _CACHE[key]


def ref_one(key, points, k, start=0, scale=None):
    """fps_ref.fps_one, computed once per key and never modified."""
    if key not in _CACHE:
        idx, dist = REF.fps_one(points, k, start, scale)
        idx.setflags(write=False)
        dist.setflags(write=False)
        _CACHE[key] = (idx, dist)
    return _CACHE[key]


def raw_call(points, offsets, k, max_per_sample, counts=None, start=None, scale=None, form=0, n_dense=0, want_dist=True, tail_rows=7):
    """rald_post_fps_ragged on poisoned outputs with GUARD rows behind them and `tail_rows` NaN rows behind the points
    -> (idx [B,k], dist2 [B,k] or None) as numpy; asserts that the guard rows kept their poison."""
    import ctypes as C
    from rald_amd._handles import _stream
    from rald_amd._lib import check, lib
    pts = np.concatenate((np.asarray(points, np.float32).reshape(-1, 3), np.full((tail_rows, 3), np.nan, np.float32)))
    B = len(offsets) - 1 if offsets is not None else (len(pts) - tail_rows) // max(n_dense, 1)
    p = torch.from_numpy(pts).cuda()
    od = torch.from_numpy(np.asarray(offsets, np.int64)).cuda() if offsets is not None else None
    cd = torch.from_numpy(np.asarray(counts, np.int32)).cuda() if counts is not None else None
    sd = torch.from_numpy(np.asarray(start, np.int64)).cuda() if start is not None else None
    idx = torch.full((B + GUARD, k), POISON_I, device="cuda", dtype=torch.int64)
    dist = torch.full((B + GUARD, k), POISON_D, device="cuda", dtype=torch.float32) if want_dist else None
    nbytes = lib().rald_post_fps_scratch_bytes(B, max_per_sample, form)
    assert nbytes >= 0
    scratch = torch.full((max(nbytes, 16),), 0xFF, device="cuda", dtype=torch.uint8)           # NaN patterns: nothing stale may matter
    s3 = (C.c_float * 3)(*scale) if scale is not None else None
    opt = lambda t: t.data_ptr() if t is not None else None
    check(lib().rald_post_fps_ragged(p.data_ptr(), opt(od), opt(cd), B, n_dense, max_per_sample, k, opt(sd), s3, idx.data_ptr(), opt(dist),
                                     scratch.data_ptr(), nbytes, form, _stream()))
    assert bool((idx[B:] == POISON_I).all()), "guard rows of idx"
    if want_dist:
        assert bool((dist[B:] == POISON_D).all()), "guard rows of dist2"
    return idx[:B].cpu().numpy(), dist[:B].cpu().numpy() if want_dist else None


def assert_same(got, want, what=""):
    gi, gd = got
    wi, wd = want
    assert np.array_equal(gi, wi), (what, "idx", np.nonzero(gi != wi), gi[gi != wi][:4], wi[gi != wi][:4])
    if gd is not None:
        assert np.array_equal(_bits(gd), _bits(wd)), (what, "dist2", np.nonzero(_bits(gd) != _bits(wd)))


# ---- 1. sizes ----------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n", SIZES)
def test_sizes_around_the_wave_and_the_workgroup(n):
    """One cloud of n uniform points, k in {1, 2, n - 1, n, n + 3}: the choices for a smaller k are a prefix of those for a larger one,
    so the reference is computed once, for k = n + 3 (its last three slots are -1 / NaN).  Without dist2 once per size."""
    pts = uniform_cloud(n, 100 + n)
    wi, wd = ref_one(("sizes", n), pts, n + 3)
    for k in sorted({k for k in (1, 2, n - 1, n, n + 3) if k >= 1}):
        want = (wi[None, :k], wd[None, :k])
        for form in FORMS:
            assert_same(raw_call(pts, _offsets([n]), k, n, form=form), want, (n, k, form))
    assert_same(raw_call(pts, _offsets([n]), n, n, want_dist=False), (wi[None, :n], None), (n, "no dist2"))


@gpu
def test_resident_limit_and_the_streaming_thresholds():
    """Every size at which the host picks another kernel: the resident form's steps in points per thread and threads (256 / 257, 1024
    / 1025 are in SIZES, 2048 / 2049, 4096 / 4097, 8192 / 8193), the largest cloud it takes (16384) under the resident form and under
    auto, one point more under auto (streaming), the step between the streaming form's two kernels (8192 / 8193) and the largest cloud
    of all (65536); the resident form refuses 16385.  k is small: the cost of an iteration, not their number, is what grows."""
    from rald_amd._lib import lib
    cases = [(n, 24, (1,)) for n in (256, 257, 2048, 2049, 4096)] + [(8192, 24, (1, 2)), (8193, 24, (1, 2))]
    cases += [(RESIDENT_MAX, 40, (1, 0, 2)), (RESIDENT_MAX + 1, 40, (0, 2)), (65536, 12, (0,))]
    for n, k, forms in cases:
        pts = uniform_cloud(n, 7)
        wi, wd = ref_one(("limit", n), pts, k, start=n - 3)
        for form in forms:
            assert_same(raw_call(pts, _offsets([n]), k, n, start=[n - 3], form=form), (wi[None], wd[None]), (n, form))
    assert lib().rald_post_fps_scratch_bytes(1, RESIDENT_MAX, 0) == 0 and lib().rald_post_fps_scratch_bytes(1, RESIDENT_MAX + 1, 0) > 0
    assert lib().rald_post_fps_scratch_bytes(1, RESIDENT_MAX + 1, 1) == -1


# ---- 2. batches --------------------------------------------------------------------------------------------------------------------------
def _ragged_case(B):
    """B clouds of mixed lengths (an empty one and one shorter than k among them when B > 1), packed; -> (points, lengths)."""
    key = ("ragged", B)
    if key not in _CACHE:
        rng = np.random.RandomState(500 + B)
        lengths = [300] if B == 1 else [int(v) for v in rng.randint(1, 700, size=B)]
        if B > 1:
            lengths[1], lengths[2] = 0, 17
        if B > 3:
            lengths[-1], lengths[5] = 1100, 64
        _CACHE[key] = (rng.uniform(-5, 5, size=(sum(lengths), 3)).astype(np.float32), lengths)
    return _CACHE[key]


@gpu
@pytest.mark.parametrize("B", (1, 3, 65))
def test_ragged_batches_and_batch_invariance(B):
    """Mixed lengths in one batch, an empty cloud (all -1 / NaN) and a cloud shorter than k (its n choices, then -1 / NaN), per-cloud
    starts; every cloud's rows equal the reference of that cloud alone, and cloud 0 and the last cloud run alone give the same bits."""
    pts, lengths = _ragged_case(B)
    off, k = _offsets(lengths), 40
    start = [(37 * b) % 1000 - 20 for b in range(B)]
    key = ("ragged_ref", B)
    if key not in _CACHE:
        _CACHE[key] = REF.fps_ragged(pts, off, k, max(lengths), start=start)
    want = _CACHE[key]
    if B > 1:
        assert (want[0][1] == -1).all() and np.isnan(want[1][1]).all() and (want[0][2][17:] == -1).all() and (want[0][2][:17] >= 0).all()
    for form in FORMS:
        got = raw_call(pts, off, k, max(lengths), start=start, form=form)
        assert_same(got, want, (B, form))
        for b in (0, B - 1):
            alone = raw_call(pts[off[b]:off[b + 1]], _offsets([lengths[b]]), k, max(lengths), start=[start[b]], form=form)
            assert_same(alone, (got[0][b:b + 1], got[1][b:b + 1]), (B, form, "alone", b))


@gpu
def test_counts_dense_layout_and_the_bound():
    """The cropped layout (counts[b] valid rows at offsets[b], NaN rows behind them), a count above its segment (capped), the dense
    layout without offsets, and a bound below a cloud's length: that cloud is sampled from its first max_per_sample rows, the rows
    behind the bound are NaN here."""
    rng = np.random.RandomState(77)
    seg, counts = [400, 130, 64, 90], [250, 130, 0, 500]
    off = _offsets(seg)
    pts = rng.uniform(-3, 3, size=(sum(seg), 3)).astype(np.float32)
    valid = [min(s, c) for s, c in zip(seg, counts)]
    for b in range(4):
        pts[off[b] + valid[b]:off[b + 1]] = np.nan
    want = REF.fps_ragged(pts, off, 70, 400, counts=counts, start=[5, 6, 7, 8])
    assert (want[0][2] == -1).all() and want[0][3].max() < 90
    for form in FORMS:
        assert_same(raw_call(pts, off, 70, 400, counts=counts, start=[5, 6, 7, 8], form=form), want, ("counts", form))
    dense = rng.uniform(-3, 3, size=(5, 333, 3)).astype(np.float32)
    want = REF.fps_dense(dense, 50, start=[0, 1, 2, 3, 4])
    for form in FORMS:
        assert_same(raw_call(dense, None, 50, 333, start=[0, 1, 2, 3, 4], form=form, n_dense=333), want, ("dense", form))
    long = rng.uniform(-3, 3, size=(900, 3)).astype(np.float32)
    cut = long.copy()
    cut[200:700] = np.nan                                            # cloud 0 holds rows 0 .. 699, the bound is 200
    off = _offsets([700, 200])
    want = REF.fps_ragged(cut, off, 30, 200, start=[699, 3])         # start mod the bounded length
    assert want[0].max() < 200
    for form in FORMS:
        assert_same(raw_call(cut, off, 30, 200, start=[699, 3], form=form), want, ("bound", form))


# ---- 3. data -----------------------------------------------------------------------------------------------------------------------------
def _data_cases():
    rng = np.random.RandomState(11)
    n = 700
    lattice = rng.randint(-3, 4, size=(n, 3)).astype(np.float32)                 # 343 distinct points: exact ties everywhere, then repeats
    two = np.where((np.arange(n) % 3 == 0)[:, None], np.float32([1.5, -2, 0.25]), np.float32([-7, 3, 3])).astype(np.float32)
    mixed = rng.uniform(-1, 1, size=(n, 3)).astype(np.float32)
    mixed[::2] *= np.float32(2.0 ** -30)
    mixed[1::2] *= np.float32(2.0 ** 10)
    return {"identical": np.tile(np.float32([[0.1, -0.2, 0.3]]), (n, 1)), "two points": two, "lattice": lattice, "mixed scales": mixed,
            "uniform": uniform_cloud(n, 3)}


@gpu
@pytest.mark.parametrize("name", ["identical", "two points", "lattice", "mixed scales", "uniform"])
def test_data_ties_repeats_scales_and_starts(name):
    """All-identical points (index 0 repeats at distance 0 from the second choice on), two distinct points repeated, a lattice with
    many exact ties (the smallest index must win each), coordinates at 2^-30 and 2^10 in one cloud, uniform points; each with and
    without a per-axis scale that is no power of two, and with the starts 0, n - 1, n, -1 and 2^40 + 5."""
    pts = _data_cases()[name]
    n, k = len(pts), 400
    scale = (0.3, 1.7, 0.011)
    starts = (0, n - 1, n, -1, 2 ** 40 + 5)
    for sc in (None, scale):
        want_i, want_d = zip(*(ref_one(("data", name, s, sc), pts, k, s, sc) for s in starts))
        want = (np.stack(want_i), np.stack(want_d))
        assert [int(w[0]) for w in want_i] == [0, n - 1, 0, n - 1, (2 ** 40 + 5) % n]
        if name == "identical":
            assert (want[0][:, 1:] == 0).all() and (want[1][:, 1:] == 0).all()
        if name == "lattice" and sc is None:
            assert (want[1][:, 1:] == np.round(want[1][:, 1:])).all() and (want[1][:, -1] == 0).all()     # exact integers; repeats at the end
        batch = np.concatenate([pts] * len(starts))
        for form in FORMS:
            got = raw_call(batch, _offsets([n] * len(starts)), k, n, start=starts, scale=sc, form=form)
            assert_same(got, want, (name, sc, form))


# ---- 4. stale state ----------------------------------------------------------------------------------------------------------------------
@gpu
def test_results_do_not_depend_on_stale_lds():
    """The same bits before and after a launch that fills every CU's LDS with NaN patterns: the slots of waves that do not exist (64
    points: one wave of 16) and the double-buffered slots are written before they are read."""
    from rald_amd._handles import _stream
    from rald_amd._lib import check, lib
    pts, lengths = _ragged_case(3)
    off = _offsets(lengths)
    small = uniform_cloud(64, 164)
    for form in FORMS:
        before = raw_call(pts, off, 40, max(lengths), form=form), raw_call(small, _offsets([64]), 64, 64, form=form)
        check(lib().rald_debug_poison_lds(_stream()))
        after = raw_call(pts, off, 40, max(lengths), form=form), raw_call(small, _offsets([64]), 64, 64, form=form)
        for a, b in zip(before, after):
            assert_same(a, b, ("stale", form))
        assert_same(after[1], tuple(v[None, :64] for v in ref_one(("sizes", 64), small, 67)), ("stale ref", form))


# ---- 5. the Python layer -------------------------------------------------------------------------------------------------------------------
@gpu
def test_python_wrappers_and_resample_padding():
    """farthest_point_sample(_ragged) return what the C entry returns; resample_points_ragged gathers by idx, fills slot j >= n of a
    short cloud with slot j mod n (pad='repeat') or NaN (pad='nan'), and gives NaN rows for an empty cloud."""
    from rald_amd import postprocess as PP
    lengths = [90, 0, 7, 1, 40]
    off = _offsets(lengths)
    pts = np.random.RandomState(5).uniform(-2, 2, size=(sum(lengths), 3)).astype(np.float32)
    start = [3, 0, 11, 5, 39]
    scale = (1.0, 0.5, 3.0)
    p, o, s = torch.from_numpy(pts).cuda(), torch.from_numpy(off).cuda(), torch.tensor(start, device="cuda")
    want = REF.fps_ragged(pts, off, 20, 90, start=start, scale=scale)
    for form in (None, "resident", "streaming"):
        idx, dist = PP.farthest_point_sample_ragged(p, o, 20, 90, start=s, scale=scale, return_dist=True, form=form)
        assert idx.dtype == torch.int64 and dist.dtype == torch.float32 and idx.is_cuda
        assert_same((idx.cpu().numpy(), dist.cpu().numpy()), want, form)
    assert torch.equal(PP.farthest_point_sample_ragged(p, o, 20, 90, start=s, scale=scale), idx)
    counts = torch.tensor([50, 0, 7, 1, 2], dtype=torch.int32, device="cuda")
    got = PP.farthest_point_sample_ragged(p, o, 20, 90, counts=counts)
    assert np.array_equal(got.cpu().numpy(), REF.fps_ragged(pts, off, 20, 90, counts=[50, 0, 7, 1, 2])[0])
    dense = np.random.RandomState(6).uniform(-2, 2, size=(3, 129, 3)).astype(np.float32)
    di, dd = PP.farthest_point_sample(torch.from_numpy(dense).cuda(), 130, start=torch.tensor([1, 2, 128], device="cuda"), return_dist=True)
    assert_same((di.cpu().numpy(), dd.cpu().numpy()), REF.fps_dense(dense, 130, start=[1, 2, 128]), "dense")
    # the resampler
    want_pts, want_idx = REF.resample_ref(pts, off, 20, 90, start=start, scale=scale)
    out, ridx = PP.resample_points_ragged(p, o, 20, 90, start=s, scale=scale, return_index=True)
    assert out.shape == (5, 20, 3) and np.array_equal(ridx.cpu().numpy(), want_idx)
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(want_pts))
    assert np.isnan(want_pts[1]).all() and not np.isnan(want_pts[[0, 2, 3, 4]]).any()
    assert np.array_equal(want_pts[2, 7:14], want_pts[2, :7]) and (want_pts[3] == want_pts[3, 0]).all()
    nan_pad = PP.resample_points_ragged(p, o, 20, 90, start=s, scale=scale, pad="nan").cpu().numpy()
    assert np.array_equal(_bits(nan_pad[[0, 4]]), _bits(want_pts[[0, 4]])) and np.array_equal(_bits(nan_pad[2, :7]), _bits(want_pts[2, :7]))
    assert np.isnan(nan_pad[2, 7:]).all() and np.isnan(nan_pad[3, 1:]).all() and np.isnan(nan_pad[1]).all()


class _SplitRng(np.random.Generator):
    """A numpy Generator whose point-selection draws (choice without replacement, integers) come from a stream of their own, so the
    'random' and the 'fps' mode of LidarFrames.batch see the same draws for everything else."""

    def __init__(self, seed):
        super().__init__(np.random.PCG64(seed))
        self.selection = np.random.default_rng(seed + 1)

    def choice(self, a, size=None, replace=True, **kw):
        if not replace:
            return self.selection.choice(a, size, replace=False, **kw)
        return super().choice(a, size, replace=True, **kw)

    def integers(self, *a, **kw):
        if "size" in kw or len(a) > 2:                # numpy's own choice(replace=True) draws through integers(..., size=...)
            return super().integers(*a, **kw)
        return self.selection.integers(*a, **kw)      # batch's start index: integers(0, N)


@gpu
@pytest.mark.parametrize("loader", ["train", "test"])
def test_lidar_batch_with_farthest_point_sampling(loader):
    """LidarFrames.batch(point_sampling='fps') on polar rows (used as they are): lidar_points are the rows the reference chooses -
    from the start the rng draws, with the normalisation's scale - normalised as the loader normalises them; queries and labels equal
    the random mode's under the same other draws; too few points raise as before."""
    import lidar_ref
    from rald_amd.lidar import LidarFrames, fps_scale, load_lidar_config
    S = 256
    cfg = load_lidar_config({"dataset": {"lidar": dict(pc_range=[0, -90, -20, 15.8, 90, 20], num_point_features=3, voxel_size=[0.05, 0.25, 0.5],
                                                        max_points_per_voxel=10, max_number_of_voxels=50000, sampling=True, num_samples=S,
                                                        query_ratio=0.0625, norm_isotropy=False, norm_anisotropy=True, cache_voxel=False,
                                                        view_cone_mode=True)}})
    rng = np.random.default_rng(31)
    frames = [np.stack([rng.uniform(1, 15, n), rng.uniform(-80, 80, n), rng.uniform(-15, 15, n)], axis=1).astype(np.float32)
              for n in (1500, 257, 2100)]
    h = LidarFrames(cfg)
    torch.manual_seed(9)
    d_fps = h.batch(frames, loader, rng=_SplitRng(40), polar=True, point_sampling="fps")
    torch.manual_seed(9)
    d_rnd = h.batch(frames, loader, rng=_SplitRng(40), polar=True)
    for key in ("query_points", "query_labels", "in_voxel_num"):
        assert torch.equal(d_fps[key].cpu(), d_rnd[key].cpu()), key
    assert not torch.equal(d_fps["lidar_points"], d_rnd["lidar_points"])
    sel = np.random.default_rng(41)
    scale = fps_scale(cfg)
    assert np.allclose(scale, [1 / 7.9, 1 / 90, 1 / 20], rtol=1e-6)
    for b, f in enumerate(frames):
        idx, _ = REF.fps_one(f, S, int(sel.integers(0, len(f))), scale)
        want = torch.from_numpy(f[idx].copy())
        lidar_ref.norm_points(want, None, cfg.pc_range, True, False)
        assert np.array_equal(_bits(d_fps["lidar_points"][b].cpu().numpy()), _bits(want.numpy())), b
    with pytest.raises(ValueError, match="Error sampling points from 255 points"):
        h.batch([frames[0][:255]], loader, rng=_SplitRng(1), polar=True, point_sampling="fps")
    with pytest.raises(ValueError):
        h.batch(frames, loader, polar=True, point_sampling="grid")


@gpu
def test_lidar_batch_fps_on_cropped_raw_scans_with_a_device_generator():
    """crop=True: the sampler runs over the cropped layout (counts[b] rows at offsets[b]) of the polar rows; the indices it returns
    are the reference's on those rows, from the start the device generator draws."""
    from rald_amd import postprocess as PP, synth
    from rald_amd.lidar import LidarFrames, fps_scale, load_lidar_config
    S = 512
    cfg = load_lidar_config({"dataset": {"lidar": dict(pc_range=[0, -90, -20, 15.8, 90, 20], num_point_features=3, voxel_size=[0.05, 0.25, 0.5],
                                                        max_points_per_voxel=10, max_number_of_voxels=50000, sampling=True, num_samples=S,
                                                        query_ratio=0.0625, norm_isotropy=False, norm_anisotropy=True, cache_voxel=False,
                                                        view_cone_mode=True)}})
    h = LidarFrames(cfg)
    scans = synth.lidar_scan(2, 77, 4096)
    seen = {}
    real = PP.farthest_point_sample_ragged

    def spy(points, offsets, k, max_per_sample, **kw):
        seen.update(points=points, offsets=offsets, k=k, max_per_sample=max_per_sample, **kw)
        seen["idx"] = real(points, offsets, k, max_per_sample, **kw)
        return seen["idx"]
    PP.farthest_point_sample_ragged = spy
    try:
        d = h.batch(scans, "test", rng=torch.Generator("cuda").manual_seed(3), crop=True, point_sampling="fps")
    finally:
        PP.farthest_point_sample_ragged = real
    counts = seen["counts"].cpu().numpy()
    assert seen["counts"].dtype == torch.int32 and seen["k"] == S and seen["max_per_sample"] == counts.max() and seen["scale"] == fps_scale(cfg)
    start = seen["start"].cpu().numpy()
    assert ((0 <= start) & (start < counts)).all()
    want, _ = REF.fps_ragged(seen["points"].cpu().numpy(), seen["offsets"].cpu().numpy(), S, int(counts.max()), counts=counts, start=start,
                             scale=seen["scale"])
    assert np.array_equal(seen["idx"].cpu().numpy(), want) and (want >= 0).all()
    assert d["lidar_points"].shape == (2, S, 3) and torch.isfinite(d["lidar_points"]).all()


@gpu
def test_infer_point_clouds_resample():
    """infer_point_clouds(..., resample=k) on the small autoencoder of tests/test_gpu_infer_batch.py: 'resampled' and 'resample_index'
    equal the reference on the returned clouds (a frame with fewer than k points repeats them, an empty one is NaN), every other key
    equals the call without the argument, and the device form returns the same two tensors last."""
    from rald_amd import engine_generation as E, query_points as QP, synth
    from test_gpu_infer_batch import _small_vae, _tail_args
    vae, z9 = _small_vae()
    z = z9[:4].contiguous()
    n, aug, k = 3000, 2048, 300
    args = _tail_args(n, aug)
    helpers = [synth.queries(1, max(h, 1), seed=100 + h)[0][:h].cuda() for h in (0, 1, 500, 1100)]
    surfaces = synth.point_cloud(4, 1000, seed=62).cuda()
    draws = QP.draw_tail_randoms(4, n, aug, 10, torch.Generator("cuda").manual_seed(23))
    kw = dict(helper_points=helpers, surfaces=surfaces, draws=draws)
    base = E.infer_point_clouds(vae, z, args, **kw)
    res = E.infer_point_clouds(vae, z, args, resample=k, **kw)
    assert set(res) == set(base) | {"resampled", "resample_index"}
    # cd comes from cal_metrics_ragged, whose double atomics add a frame's <= 1e6 distances in an order that changes from call to call:
    # two calls differ by at most ~1e6 * 2^-53 ~ 1e-10 relative (the bound tests/test_gpu_infer_batch.py uses for the same value is 1e-9)
    assert res["n_queries"] == base["n_queries"] and len(res["cd"]) == 4
    assert all(a == b or abs(a - b) <= 1e-9 * abs(b) for a, b in zip(res["cd"], base["cd"]))
    assert all(torch.equal(a, b) for a, b in zip(res["pred"], base["pred"]))
    assert res["resampled"].shape == (4, k, 3) and res["resample_index"].shape == (4, k) and res["resampled"].is_cuda
    lengths = [p.shape[0] for p in res["pred"]]
    print("final clouds:", lengths)
    assert max(lengths) > k
    flat = np.concatenate([p.cpu().numpy() for p in res["pred"]])
    want_pts, want_idx = REF.resample_ref(flat, _offsets(lengths), k, max(max(lengths), 1))
    assert np.array_equal(res["resample_index"].cpu().numpy(), want_idx)
    assert np.array_equal(_bits(res["resampled"].cpu().numpy()), _bits(want_pts))
    dev = E.infer_point_clouds_device(vae, z, args, resample=k, **kw)
    assert len(dev) == 5 and torch.equal(dev[-1], res["resample_index"])
    assert np.array_equal(_bits(dev[-2].cpu().numpy()), _bits(res["resampled"].cpu().numpy()))
    assert len(E.infer_point_clouds_device(vae, z, args, **kw)) == 3
