"""Farthest-point sampling, host side (no GPU): the reference of tests/fps_ref.py against a brute-force float64 choice and its own
properties; the C entries' declarations, scratch sizes and every refusal (through the built library, before any GPU work); the Python
layer's argument errors; and, with the device functions stubbed, that LidarFrames.batch and infer_point_clouds do what they did before
when the new arguments are left alone."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import fps_ref as REF


# ---- the reference -------------------------------------------------------------------------------------------------------------------------
def _integer_cloud(seed, n, planted=True):
    """Integer coordinates with |c| <= 64 (every float32 operation of the distance is exact), with planted exact ties: rows 3 and 40
    are the same point, rows 7 and 8 mirror each other through row 0."""
    p = np.random.RandomState(seed).randint(-64, 65, size=(n, 3)).astype(np.float32)
    if planted:
        p[0] = (0, 0, 0)
        p[40] = p[3]
        p[7], p[8] = (60, -61, 62), (-60, 61, -62)
    return p


@pytest.mark.parametrize("seed,n,k,start", [(1, 50, 50, 0), (2, 97, 60, 96), (3, 64, 70, 1000003), (4, 41, 41, -1)])
def test_reference_agrees_with_a_brute_force_float64_choice(seed, n, k, start):
    p = _integer_cloud(seed, n)
    idx, dist = REF.fps_one(p, k, start)
    want_idx, want_dist = REF.fps_brute_float64(p, k, start)
    m = min(n, k)
    assert idx[:m].tolist() == want_idx and dist[:m].astype(np.float64).tolist() == want_dist
    assert (idx[m:] == -1).all() and np.isnan(dist[m:]).all()


def test_reference_breaks_ties_towards_the_smallest_index():
    # rows 7 and 8 are equally far from row 0 (and farther than any other row): the smaller index goes first, the larger follows
    p = _integer_cloud(5, 50)
    idx, dist = REF.fps_one(p, 3, 0)
    far = np.float32(60 * 60 + 61 * 61 + 62 * 62)
    assert idx.tolist() == [0, 7, 8] and dist[1] == far and dist[2] == far
    # the centre of a square and its four corners: from the centre all four are tied at 32, and stay tied whichever is taken
    sq = np.float32([[0, 0, 0], [4, 4, 0], [-4, 4, 0], [4, -4, 0], [-4, -4, 0]])
    idx, dist = REF.fps_one(sq, 5, 0)
    assert idx.tolist() == [0, 1, 2, 3, 4] and dist.tolist() == [np.inf, 32.0, 32.0, 32.0, 32.0]
    # the same corners in another order: the rows chosen change, the rule (the smallest index of the tied) does not
    idx, _ = REF.fps_one(sq[[0, 4, 3, 2, 1]], 5, 0)
    assert idx.tolist() == [0, 1, 2, 3, 4]
    idx, _ = REF.fps_one(sq, 5, 3)
    assert idx.tolist() == [3, 2, 1, 4, 0]                            # farthest from a corner: the opposite one; then a tie of 1 and 4
    # duplicates: of a point and its copy only the smaller index is ever chosen; with nothing distinct left, row 0 at distance 0
    idx, dist = REF.fps_one(p, 50, 0)
    assert 3 in idx.tolist() and 40 not in idx.tolist() and idx[49] == 0 and dist[49] == 0 and (dist[1:49] > 0).all()


def test_reference_properties():
    p = np.random.RandomState(8).uniform(-1, 1, size=(300, 3)).astype(np.float32)
    p[200:] = p[:100]                                                 # 200 distinct points
    idx, dist = REF.fps_one(p, 260, 17, scale=(0.3, 1.7, 0.011))
    assert idx[0] == 17 and dist[0] == np.inf
    assert (np.diff(dist[1:]) <= 0).all()                             # non-increasing
    assert len(set(idx[:200].tolist())) == 200 and (dist[1:200] > 0).all()       # distinct while distinct points remain
    assert (idx[200:] == 0).all() and (dist[200:] == 0).all()         # then the smallest index, at distance 0
    # the start modulo, counts, the bound and the padding
    assert REF.fps_one(p, 1, 300)[0][0] == 0 and REF.fps_one(p, 1, -1)[0][0] == 299 and REF.fps_one(p, 1, 2 ** 40 + 5)[0][0] == (2 ** 40 + 5) % 300
    off = np.array([0, 100, 100, 300])
    ri, rd = REF.fps_ragged(p, off, 8, 50, counts=[3, 5, 400], start=[4, 0, 51])
    assert ri[0].tolist()[:3] != [-1] * 3 and (ri[0][3:] == -1).all() and np.isnan(rd[0][3:]).all() and ri[0][0] == 1
    assert (ri[1] == -1).all() and np.isnan(rd[1]).all()
    assert ri[2][0] == 1 and ri[2].max() < 50                         # 200 rows, count 400: capped at the segment, then at the bound
    one = REF.fps_one(p[100:150], 8, 51)
    assert np.array_equal(ri[2], one[0]) and np.array_equal(rd[2], one[1])
    pts, idx = REF.resample_ref(p, off, 8, 50, counts=[3, 5, 400])
    assert np.array_equal(pts[0, 3:6], pts[0, :3]) and np.isnan(pts[1]).all() and np.array_equal(pts[2], p[100 + idx[2]])


# ---- the C entries -------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entries():
    from rald_amd import _lib
    P, I32, I64 = C.c_void_p, C.c_int32, C.c_int64
    assert _lib.SIGNATURES["rald_post_fps_scratch_bytes"] == (I64, [I32, I64, I32])
    assert _lib.SIGNATURES["rald_post_fps_ragged"] == (I32, [P, P, P, I32, I64, I64, I32, P, P, P, P, P, I64, I32, P])


def test_scratch_bytes():
    from rald_amd._lib import lib
    L = lib()
    q = L.rald_post_fps_scratch_bytes
    # the resident form needs none; the streaming form keeps x, y, z of every slot of its kernel: 8 or 64 points for each of 1024 threads
    assert q(1, 1, 0) == 0 and q(64, 16384, 0) == 0 and q(7, 2048, 1) == 0
    assert q(1, 1, 2) == 3 * 8 * 1024 * 4 and q(5, 8192, 2) == 5 * 3 * 8 * 1024 * 4
    assert q(1, 8193, 2) == 3 * 64 * 1024 * 4 and q(64, 65536, 0) == 64 * 3 * 65536 * 4 and q(3, 16385, 0) == q(3, 65536, 2)
    for args in ((0, 100, 0), (-1, 100, 0), (1, 0, 0), (1, -5, 2), (1, 65537, 0), (1, 65537, 2), (1, 16385, 1), (1, 100, 3), (1, 100, -1)):
        assert q(*args) == -1, args
        assert b"rald_post_fps_scratch_bytes" in L.rald_last_error()


def test_every_refusal_comes_before_any_gpu_work():
    """Host buffers stand in for device memory: a refused call touches none of them and launches nothing."""
    from rald_amd._lib import lib
    L = lib()
    pts, out = (C.c_float * 64)(), (C.c_int64 * 64)()
    scratch = (C.c_char * (3 * 8 * 1024 * 4 + 64))()
    base = C.addressof(scratch)
    aligned = base + (-base) % 16
    big = 3 * 8 * 1024 * 4
    ok = dict(points=pts, offsets=None, counts=None, batch=1, n_dense=4, max_per_sample=4, k=2, start=None, scale=None, out_idx=out, out_dist2=None,
              scratch=aligned, scratch_bytes=big, form=2, stream=None)
    cases = [(dict(points=None), b"null pointer"), (dict(out_idx=None), b"null pointer"), (dict(batch=0), b"batch must be >= 1"),
             (dict(batch=-3), b"batch must be >= 1"), (dict(k=0), b"k must be >= 1"), (dict(k=-1), b"k must be >= 1"),
             (dict(n_dense=-1), b"n_dense must be >= 0"), (dict(max_per_sample=0), b"max_per_sample must be 1 .. 65536"),
             (dict(max_per_sample=65537), b"max_per_sample must be 1 .. 65536"), (dict(form=3), b"form must be 0"),
             (dict(form=-1), b"form must be 0"), (dict(form=1, max_per_sample=16385), b"resident form takes max_per_sample up to 16384"),
             (dict(scratch_bytes=big - 1), b"scratch too small"), (dict(scratch=None), b"null or unaligned scratch"),
             (dict(scratch=aligned + 4), b"null or unaligned scratch"), (dict(form=0, max_per_sample=16385, scratch_bytes=big), b"scratch too small")]
    for change, message in cases:
        a = {**ok, **change}
        assert L.rald_post_fps_ragged(*a.values()) == 1, change
        assert message in L.rald_last_error(), (change, L.rald_last_error())


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------------
def _no_library(monkeypatch):
    from rald_amd import _lib

    def no_library():
        raise AssertionError("the library was touched")
    # import first, patch second: a module imported while _lib.lib is patched would bind the stub for good
    mods = [__import__("rald_amd." + mod, fromlist=["x"]) for mod in ("engine_generation", "postprocess", "query_points", "_handles", "lidar")]
    monkeypatch.setattr(_lib, "lib", no_library)
    for m in mods:
        if hasattr(m, "lib"):
            monkeypatch.setattr(m, "lib", no_library)


def test_argument_errors_raise_before_the_library_is_touched(monkeypatch):
    from rald_amd import engine_generation as E, postprocess as PP
    _no_library(monkeypatch)
    pts, off = torch.zeros(10, 3), torch.tensor([0, 4, 10])
    ok = dict(points=pts, offsets=off, k=4, max_per_sample=6)
    bad = [dict(points=torch.zeros(10, 2)), dict(points=torch.zeros(2, 5, 3)), dict(points=torch.zeros(10, 3, dtype=torch.int64)),
           dict(points=[[0.0, 0.0, 0.0]]), dict(offsets=torch.tensor([0.0, 4.0, 10.0])), dict(offsets=torch.tensor([10])), dict(offsets=[0, 4, 10]),
           dict(k=0), dict(k=-2), dict(k=1.5), dict(k=True), dict(max_per_sample=0), dict(max_per_sample=65537), dict(max_per_sample=2.5),
           dict(counts=torch.tensor([4, 6])), dict(counts=torch.tensor([4, 6, 1], dtype=torch.int32)), dict(counts=[4, 6]),
           dict(start=torch.tensor([0, 1], dtype=torch.int32)), dict(start=torch.tensor([0])), dict(start=[0, 1]),
           dict(scale=(1.0, 2.0)), dict(scale=(1.0, float("inf"), 1.0)), dict(scale=(1.0, float("nan"), 1.0)), dict(form="fast"), dict(form=1)]
    for kw in bad:
        with pytest.raises(ValueError):
            PP.farthest_point_sample_ragged(**{**ok, **kw})
        with pytest.raises(ValueError):
            PP.resample_points_ragged(**{**ok, **{k: v for k, v in kw.items() if k != "form"}, **({"pad": "zero"} if "form" in kw else {})})
    for points, kw in ((torch.zeros(10, 3), {}), (torch.zeros(2, 0, 3), {}), (torch.zeros(0, 5, 3), {}), (torch.zeros(1, 65537, 3), {}),
                       (torch.zeros(2, 5, 2), {}), (torch.zeros(2, 5, 3), dict(k=0)), (torch.zeros(2, 5, 3), dict(start=torch.tensor([1]))),
                       (torch.zeros(2, 5, 3), dict(scale=(1, 2)))):
        with pytest.raises(ValueError):
            PP.farthest_point_sample(points, **{"k": 3, **kw})

    class Vae:
        def __getattr__(self, name):
            raise AssertionError("the autoencoder was touched")
    for fn in (E.infer_point_clouds, E.infer_point_clouds_device):
        for k in (0, -4, 2.5, True):
            with pytest.raises(ValueError):
                fn(Vae(), torch.zeros(2, 128, 32), None, resample=k)


# ---- what stays as it was --------------------------------------------------------------------------------------------------------------------
def _stub_frames(monkeypatch, n_rows, voxels):
    """A LidarFrames whose three device stages are recorders on CPU tensors (a CPU torch.Generator puts the whole batch on the CPU)."""
    from rald_amd import postprocess as PP
    from rald_amd.lidar import LidarFrames, load_lidar_config
    cfg = load_lidar_config({"dataset": {"lidar": dict(pc_range=[0, -90, -20, 15.8, 90, 20], num_point_features=3, voxel_size=[0.05, 0.25, 0.5],
                                                        max_points_per_voxel=10, max_number_of_voxels=50000, sampling=True, num_samples=32,
                                                        query_ratio=0.25, norm_isotropy=False, norm_anisotropy=True, cache_voxel=False,
                                                        view_cone_mode=True)}})
    h = LidarFrames(cfg)
    seen = {}
    B = len(n_rows)

    def voxelize(x, offs, counts, to_polar=False, with_voxels=True):
        return dict(polar=None, coords=None, kept_keys=None, voxel_counts=torch.tensor(voxels, dtype=torch.int32))

    def queries(points, offsets, num_samples, in_num, sample_idx, u_in, voxel_idx, u_out, empty_rank, vox):
        seen.update(sample_idx=sample_idx, u_in=u_in, voxel_idx=voxel_idx, u_out=u_out, empty_rank=empty_rank, points=points)
        return torch.zeros(B, num_samples, 3), torch.zeros(B, num_samples, 3), torch.zeros(B, num_samples)

    def fps(points, offsets, k, max_per_sample, **kw):
        seen.update(fps=dict(points=points, offsets=offsets, k=k, max_per_sample=max_per_sample, **kw))
        return torch.arange(k).repeat(B, 1)
    monkeypatch.setattr(h, "voxelize", voxelize)
    monkeypatch.setattr(h, "queries", queries)
    monkeypatch.setattr(PP, "farthest_point_sample_ragged", fps)
    frames = [np.random.RandomState(b).uniform(1, 10, size=(n, 3)).astype(np.float32) for b, n in enumerate(n_rows)]
    return h, cfg, frames, seen


def _replay_draws(gen, n_rows, voxels, cells, S, in_num, out_num, vsize, first):
    """The draws of LidarFrames.batch with a torch generator, frame by frame in its order; `first` makes a frame's selection draw."""
    lo = torch.tensor(-np.array(vsize) / 2)
    out = dict(sample_idx=[], u_in=[], u_out=[], voxel_idx=[], empty_rank=[])
    for N, V in zip(n_rows, voxels):
        out["sample_idx"].append(first(N, gen))
        out["u_in"].append(torch.rand((in_num, 3), dtype=torch.float64, generator=gen) * (2 * -lo) + lo)
        out["u_out"].append(torch.rand((out_num, 3), dtype=torch.float64, generator=gen) * (2 * -lo) + lo)
        out["voxel_idx"].append(torch.randint(0, V, (in_num,), generator=gen))
        out["empty_rank"].append(torch.randint(0, cells - V, (out_num,), generator=gen))
    return {k: torch.stack(v) for k, v in out.items()}


def test_lidar_batch_consumes_its_rng_as_before_and_fps_replaces_one_draw(monkeypatch):
    """Without point_sampling: every draw, in order and in value, is what the loop drew before (replayed here from a generator of the
    same seed), the generator ends in the same state, and the sampler is not called.  With 'fps': one start index per frame in place
    of the permutation, the other draws in their order; the sampler gets the rows, the bound, the starts and the normalisation's
    scale, and its indices go to the query stage."""
    n_rows, voxels = [100, 57, 32], [40, 9, 31]
    h, cfg, frames, seen = _stub_frames(monkeypatch, n_rows, voxels)
    S, in_num = 32, 8
    gen = torch.Generator().manual_seed(77)
    d = h.batch(frames, "train", rng=gen, polar=True)
    assert "fps" not in seen and set(d) == {"lidar_points", "query_points", "query_labels", "in_voxel_num", "raw_query_points"}
    replay = torch.Generator().manual_seed(77)
    want = _replay_draws(replay, n_rows, voxels, h.cells, S, in_num, S - in_num, cfg.voxel_size, lambda N, g: torch.randperm(N, generator=g)[:S])
    for key, w in want.items():
        assert torch.equal(seen[key], w), key
    assert torch.equal(gen.get_state(), replay.get_state())
    assert torch.equal(h.batch(frames, "train", rng=torch.Generator().manual_seed(77), polar=True, point_sampling="random")["lidar_points"],
                       d["lidar_points"]) and "fps" not in seen

    gen = torch.Generator().manual_seed(77)
    h.batch(frames, "train", rng=gen, polar=True, point_sampling="fps")
    replay = torch.Generator().manual_seed(77)
    want = _replay_draws(replay, n_rows, voxels, h.cells, S, in_num, S - in_num, cfg.voxel_size, lambda N, g: torch.randint(0, N, (1,), generator=g)[0])
    call = seen["fps"]
    assert torch.equal(call["start"], want.pop("sample_idx")) and call["start"].dtype == torch.int64 and call["start"].shape == (3,)
    assert all(0 <= int(s) < n for s, n in zip(call["start"], n_rows))
    for key, w in want.items():
        assert torch.equal(seen[key], w), key
    assert torch.equal(gen.get_state(), replay.get_state())
    assert call["k"] == S and call["max_per_sample"] == 100 and call["counts"] is None and call["offsets"].tolist() == [0, 100, 157, 189]
    assert call["points"] is seen["points"] and np.allclose(call["scale"], [1 / 7.9, 1 / 90, 1 / 20], rtol=1e-6)
    assert torch.equal(seen["sample_idx"], torch.arange(S).repeat(3, 1))
    with pytest.raises(ValueError, match="Error sampling points from 31 points"):
        h.batch([frames[0][:31]], "train", rng=torch.Generator().manual_seed(1), polar=True, point_sampling="fps")
    with pytest.raises(ValueError, match="point_sampling"):
        h.batch(frames, "train", rng=gen, polar=True, point_sampling="farthest")


def test_fps_scale_follows_the_normalisation():
    from rald_amd.lidar import fps_scale
    cfg = {"pc_range": [0, -90, -20, 15.8, 90, 20]}
    ns = lambda **kw: types.SimpleNamespace(get=lambda k, d=None: {**cfg, **kw}.get(k, d), pc_range=cfg["pc_range"])
    assert fps_scale(ns()) is None
    half = np.array([7.9, 90.0, 20.0])
    assert fps_scale(ns(norm_anisotropy=True)) == [float(v) for v in (1 / half).astype(np.float32)]
    assert fps_scale(ns(norm_isotropy=True)) == [float(np.float32(1 / 90.0))] * 3
    assert fps_scale(ns(norm_anisotropy=True, norm_isotropy=True)) == [float(v) for v in (1 / half / 90.0).astype(np.float32)]


def test_infer_point_clouds_without_resample_is_what_it_was(monkeypatch):
    """The stubbed tail of tests/test_cloud_metrics_host.py: without `resample` the same calls, one host read and the same keys; with
    it one more call, after the metric, on the final clouds and their host bound, and still one host read."""
    from rald_amd import engine_generation as E
    from test_cloud_metrics_host import TAIL, _stub_tail
    calls, reads, pos, kw, _ = _stub_tail(monkeypatch)
    seen = {}

    def resample(pts, off, k, max_per_sample, return_index=False):
        calls.append("resample_points_ragged")
        seen.update(pts=pts, off=off, k=k, max_per_sample=max_per_sample, return_index=return_index)
        return torch.ones(2, k, 3), torch.zeros(2, k, dtype=torch.int64)
    E.PP.resample_points_ragged = resample
    E.PP.FPS_MAX_POINTS = 65536
    out = E.infer_point_clouds(*pos, **kw)
    assert calls == TAIL + ["cal_metrics_ragged"] and len(reads) == 1 and set(out) == {"pred", "cd", "n_queries"}
    del calls[:], reads[:]
    assert len(E.infer_point_clouds_device(*pos, **kw)) == 3 and calls == TAIL + ["cal_metrics_ragged"] and len(reads) == 0
    del calls[:]
    out = E.infer_point_clouds(*pos, resample=5, **kw)
    assert calls == TAIL + ["cal_metrics_ragged", "resample_points_ragged"] and len(reads) == 1
    assert set(out) == {"pred", "cd", "n_queries", "resampled", "resample_index"}
    assert out["resampled"].shape == (2, 5, 3) and out["resample_index"].shape == (2, 5) and out["cd"] == [1.5, 2.5]
    assert seen["k"] == 5 and seen["max_per_sample"] == 50 and seen["return_index"] and seen["off"].tolist() == [0, 7, 12]
    del calls[:]
    dev = E.infer_point_clouds_device(*pos, resample=5, **kw)
    assert len(dev) == 5 and dev[3].shape == (2, 5, 3) and dev[4].shape == (2, 5) and calls[-1] == "resample_points_ragged"
