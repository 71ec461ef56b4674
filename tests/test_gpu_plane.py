"""RANSAC plane segmentation and plane removal on the GPU (rald_amd/csrc/cloud_plane.hip) against tests/plane_ref.py, by equality:
integers as integers, floats and doubles by bit pattern - no tolerance anywhere.  Every call goes through _run: the outputs are
pre-filled with poison (NaNs with a payload, -7) and followed by guard rows, the input rows the kernels must not read (behind counts,
behind the bound, behind offsets[B]) are NaN, the scratch is followed by a guard, and the checks assert that everything the definition
does not write still holds its poison.  tests/test_plane_host.py holds the reference against an independent route on the same
constructions and shows on the reference alone what each is for."""
import numpy as np
import pytest
import torch

import plane_ref as REF
from test_gpu_radius_filter import F32, GUARD, POISON_F, POISON_I, _bits, _offsets, _same, _spans

gpu = pytest.mark.gpu
POISON_D = np.array([0x7FF8000000012345], np.uint64).view(np.float64)[0]
_bits64 = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _run(points, offsets, bound, t, H, K=1, min_inliers=3, refine=True, seed=0, view=None, counts=None, keep=None, dense=False, optional=True):
    """The C entries on poisoned, guarded buffers -> dict of numpy arrays, whole buffers (guards included): the segment call (with
    inliers and best unless optional is False) or, with keep = keep_planes (0 / 1), the filter (with the index unless optional is False).  dense:
    offsets describe equal clouds, passed as n_dense with a NULL offsets pointer."""
    import ctypes as C
    from rald_amd._handles import _stream
    from rald_amd._lib import check, lib
    p = np.array(points, F32).reshape(-1, 3)
    T, B = len(p), len(offsets) - 1
    dev_p = np.concatenate([p, np.zeros((GUARD, 3), F32)])
    dev_p[_spans(T, offsets, bound, counts)] = np.nan
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    t_ = dict(points=cu(dev_p), offsets=None if dense else cu(np.array(offsets, np.int64)),
              counts=None if counts is None else cu(np.array(counts, np.int32)), labels=cu(np.full(T + GUARD, POISON_I, np.int32)),
              planes=cu(np.full((B + GUARD, max(K, 1), 4), POISON_D, np.float64)), num=cu(np.full(B + GUARD, POISON_I, np.int32)))
    n_dense = offsets[1] - offsets[0] if dense else 0
    L = lib()
    nbytes = L.rald_post_plane_scratch_bytes(B, T, bound, H, K)
    if nbytes < 0:                                                     # sizes the call refuses too: it must say so itself
        assert not (1 <= H <= 65536 and 1 <= K <= 8)
        nbytes = 1 << 16
    assert nbytes > 0
    scratch = torch.empty(nbytes + 16 * GUARD, dtype=torch.uint8, device="cuda")
    scratch[:nbytes] = 0xFF                                            # -1 / NaN everywhere: nothing may rest on a zeroed scratch
    scratch[nbytes:] = 0xA5
    ptr = lambda k: None if t_.get(k) is None else t_[k].data_ptr()
    view3 = None if view is None else (C.c_float * 3)(*view)
    head = (ptr("points"), ptr("offsets"), ptr("counts"), B, n_dense, T, bound, float(t), H, K, int(min_inliers), int(refine), int(seed), view3)
    tail = (scratch.data_ptr(), nbytes, _stream())
    if keep is None:
        if optional:
            t_.update(inliers=cu(np.full((B + GUARD, K), POISON_I, np.int32)), best=cu(np.full((B + GUARD, K), POISON_I, np.int32)))
        check(L.rald_post_plane_segment_ragged(*head, ptr("labels"), ptr("planes"), ptr("num"), ptr("inliers"), ptr("best"), *tail))
        keys = ("labels", "planes", "num", "inliers", "best")
    else:
        t_.update(out=cu(np.full((T + GUARD, 3), POISON_F, F32)), out_offsets=cu(np.full(B + 1 + GUARD, POISON_I, np.int64)))
        if optional:
            t_.update(index=cu(np.full(T + GUARD, POISON_I, np.int64)))
        check(L.rald_post_plane_filter_ragged(*head, int(keep), ptr("out"), ptr("out_offsets"), ptr("index"), ptr("labels"), ptr("planes"),
                                              ptr("num"), *tail))
        keys = ("labels", "planes", "num", "out", "out_offsets", "index")
    torch.cuda.synchronize()
    assert bool((scratch[nbytes:] == 0xA5).all()), "the scratch's guard was written"
    return {k: t_[k].cpu().numpy() for k in keys if k in t_}


def _same_all(a, b):
    return _same({k: v for k, v in a.items() if k != "planes"}, {k: v for k, v in b.items() if k != "planes"}) and \
        np.array_equal(_bits64(a["planes"]), _bits64(b["planes"]))


def _check_planes(got, ref, B):
    assert got["num"][:B].tolist() == ref["num_planes"].tolist() and (got["num"][B:] == POISON_I).all()
    bad = np.nonzero(_bits64(got["planes"][:B]) != _bits64(ref["planes"]))
    assert bad[0].size == 0, (bad, got["planes"][:B][bad][:4], ref["planes"][bad][:4])
    assert (_bits64(got["planes"][B:]) == _bits64(POISON_D)).all()


def _check_segment(got, ref):
    """Everything the segment call writes equals the reference; everything else still holds its poison."""
    T, B = len(ref["labels"]), len(ref["num_planes"])
    want = np.where(ref["untouched"], POISON_I, ref["labels"])
    bad = np.nonzero(got["labels"][:T] != want)[0]
    assert bad.size == 0, (bad[:5], got["labels"][bad[:5]], want[bad[:5]])
    assert (got["labels"][T:] == POISON_I).all()
    _check_planes(got, ref, B)
    for k in ("inliers", "best"):
        if k in got:
            assert got[k][:B].tolist() == ref[k].tolist() and (got[k][B:] == POISON_I).all(), (k, got[k][:B], ref[k])


def _check_filter(got, ref, B):
    M = int(ref["offsets"][-1])
    assert got["out_offsets"][:B + 1].tolist() == ref["offsets"].tolist() and (got["out_offsets"][B + 1:] == POISON_I).all()
    if "index" in got:
        assert np.array_equal(got["index"][:M], ref["index"]) and (got["index"][M:] == POISON_I).all()
    assert np.array_equal(_bits(got["out"][:M]), _bits(ref["points"])) and (_bits(got["out"][M:]) == _bits(POISON_F)).all()
    assert np.array_equal(got["labels"][:M], ref["labels"]) and (got["labels"][M:] == POISON_I).all()
    _check_planes(got, ref, B)


def _segment_and_filter(p, off, bound, kw, counts=None, dense=False, keeps=(0, 1), ref=None):
    """The whole surface on one batch: the segment call, then the filter in the senses given -> (the reference, the kept rows)."""
    B = len(off) - 1
    ref = REF.segment_ragged(p, off, max_per_sample=bound, counts=counts, **kw) if ref is None else ref
    _check_segment(_run(p, off, bound, counts=counts, dense=dense, **kw), ref)
    kept = []
    for keep in keeps:
        want = REF.filter_ragged(p, off, max_per_sample=bound, counts=counts, keep_planes=bool(keep), labelled=ref, **kw)
        _check_filter(_run(p, off, bound, counts=counts, dense=dense, keep=keep, **kw), want, B)
        kept.append(int(want["offsets"][-1]))
    return ref, kept


# ---- the constructions ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_tiny():
    """Clouds of 0, 1, 2 and 3 rows, 3 collinear rows, 3 rows of which two are equal, in one batch: a plane only in the cloud of three
    rows in general position, through all three; NaN planes, best -1 and labels -1 everywhere else."""
    p, off = REF.tiny_clouds()
    for refine in (False, True):
        ref, kept = _segment_and_filter(p, off, 3, dict(REF.TINY, refine=refine))
        assert ref["num_planes"].tolist() == [0, 0, 0, 1, 0, 0] and ref["labels"].tolist() == [-1] * 3 + [0] * 3 + [-1] * 6
        assert kept == [9, 3]


@gpu
@pytest.mark.parametrize("n", REF.SLAB_SIZES)
def test_slab(n):
    """The lattice slab at 257, 1025 and 2049 rows (a partial wave, one past pln_score's tile and the 1024-block of the sums, two tiles
    and one row): without refine the rows at exactly +-t are inliers and those at +-t (1 + 2^-22) are not; with refine the float64
    re-mark of the same rows."""
    p, far = REF.slab_cloud(n)
    ref, kept = _segment_and_filter(p, [0, n], n, REF.SLAB)
    z = np.abs(p[:, 2])
    assert (ref["labels"][z <= F32(REF.T_SLAB)] == 0).all() and (ref["labels"][z == far] == -1).all() and (z == far).sum() > 10
    assert kept == [int((z == far).sum()), int((z != far).sum())]
    _segment_and_filter(p, [0, n], n, dict(REF.SLAB, refine=True), keeps=(0,))


@gpu
def test_tie():
    """Two parallel planes of 300 rows each: hypotheses inside either score exactly 300 (tests/test_plane_host.py shows both kinds
    occur); the smallest h wins, and out_best shows it."""
    p = REF.tie_cloud()
    ref, _ = _segment_and_filter(p, [0, len(p)], len(p), REF.TIE, keeps=(1,))
    assert ref["inliers"].tolist() == [[300]] and ref["best"].tolist() == [[0]]


def _late_tie_cloud(seed=45):
    """40 distinct sites of the lattice (0 .. 31)^2 * 2^-3 in z = 0 and 300 rows uniform in [0, 4]^3 with z >= 0.5, in random order:
    only a hypothesis drawn wholly inside the plane scores 40, about 2048 (40 / 340)^3 = 3 of 2048."""
    rs = np.random.RandomState(seed)
    sites = rs.choice(32 * 32, 40, replace=False)
    plane = np.stack([sites // 32, sites % 32, np.zeros(40)], 1).astype(F32) * F32(0.125)
    rest = rs.uniform(0.0, 4.0, size=(300, 3))
    rest[:, 2] = rs.uniform(0.5, 4.0, size=300)
    p = np.concatenate([plane, rest.astype(F32)]).astype(F32)
    return p[rs.permutation(len(p))]


@gpu
def test_tie_with_the_winner_beyond_the_first_stride_of_the_argmax():
    """pln_argmax gives thread t the hypotheses t, t + 256, ..  With seed 0 the reference's scores tie at 40 in the hypotheses 650, 1486
    and 1566: the winner is thread 138's third, and the tie 1566 stands at thread 30, which the tree of block_argmax meets first.
    Both properties are asserted of the reference, then labels, planes (by bits), inliers and best are compared with it."""
    p = _late_tie_cloud()
    kw = dict(t=REF.T_SLAB, H=2048, K=1, min_inliers=30, refine=False, seed=0)
    score = REF.scores_of(p, REF.hypotheses(p, 0, kw["H"], kw["seed"], kw["t"]))          # every row is usable: the live rows are p
    tied = np.nonzero(score == score.max())[0]
    ref = REF.segment_ragged(p, [0, len(p)], max_per_sample=len(p), **kw)
    assert score.max() == 40 and ref["best"].tolist() == [[int(tied[0])]] and ref["inliers"].tolist() == [[40]]
    assert tied[0] >= 256 and len(tied) >= 2 and (tied[1:] % 256 < tied[0] % 256).any()
    assert (ref["labels"] == np.where(p[:, 2] == 0, 0, -1)).all()
    _check_segment(_run(p, [0, len(p)], len(p), **kw), ref)


@gpu
@pytest.mark.parametrize("order", ("built", "reversed", "shuffled"))
def test_faces(order):
    """Three orthogonal faces of 576, 400 and 256 rows and 100 scattered rows, max_planes = 4, min_inliers = 256, in three row orders:
    labels 0, 1, 2 by size, the fourth plane not found; both filters with index and labels."""
    p, truth = REF.faces_cloud(order)
    ref, kept = _segment_and_filter(p, [0, len(p)], len(p), REF.FACES)
    assert ref["num_planes"].tolist() == [3] and np.array_equal(ref["labels"], truth) and ref["inliers"].tolist() == [[576, 400, 256, 0]]
    assert kept == [100, 1232] and np.isnan(ref["planes"][0, 3]).all() and ref["best"][0, 3] == -1


@gpu
@pytest.mark.parametrize("refine", (False, True))
def test_noisy(refine):
    """normals_ref.noisy_plane with 40 % outliers and NaN / inf rows, the view on either side of the plane (the sign rule), both
    filters; H = 1, 63, 64, 65 and 1000 around pln_score's chunk of 64 hypotheses; a seed >= 2^32 gives the result of its low word."""
    p, nrm, centre = REF.noisy_cloud()
    n = len(p)
    for side in (1.0, -1.0):
        kw = dict(REF.NOISY, refine=refine, view=(centre + side * 5.0 * nrm).astype(F32).tolist())
        ref, kept = _segment_and_filter(p, [0, n], n, kw)
        assert ref["num_planes"][0] == 1 and side * float(ref["planes"][0, 0, :3] @ nrm) > 0.99 and kept[0] + kept[1] == n - 12
        assert (ref["labels"][~np.isfinite(p).all(axis=1)] == -2).all()
    for H in (1, 63, 64, 65, 1000):
        _segment_and_filter(p, [0, n], n, dict(REF.NOISY, refine=refine, H=H, min_inliers=3), keeps=())
    low = _run(p, [0, n], n, **dict(REF.NOISY, refine=refine, seed=5))
    assert _same_all(low, _run(p, [0, n], n, **dict(REF.NOISY, refine=refine, seed=(7 << 32) + 5)))
    assert not np.array_equal(low["best"], _run(p, [0, n], n, **dict(REF.NOISY, refine=refine, seed=6))["best"])


# ---- ragged batches ------------------------------------------------------------------------------------------------------------------------
@gpu
def test_ragged_batch_counts_and_dense():
    """B = 5 with two empty clouds; `counts` that trim, a bound shorter than a cloud, the dense layout, without the optional outputs.
    Every cloud's result equals its one-cloud result, at every batch position (the cloud's index is not in the Philox counter)."""
    faces, _ = REF.faces_cloud("shuffled")
    noisy, _, _ = REF.noisy_cloud()
    slab, _ = REF.slab_cloud(1025)
    clouds = [faces, np.zeros((0, 3), F32), noisy[:1400], np.zeros((0, 3), F32), slab]
    off = _offsets([len(c) for c in clouds])
    p = np.concatenate(clouds)
    kw = dict(t=0.05, H=128, K=3, min_inliers=200, refine=True, seed=11)
    ref, _ = _segment_and_filter(p, off, 1500, kw)
    assert ref["num_planes"].tolist() == [3, 0, 1, 0, 1]
    for b in (0, 2, 4):
        alone = REF.segment_ragged(clouds[b], [0, len(clouds[b])], max_per_sample=len(clouds[b]), **kw)
        _check_segment(_run(clouds[b], [0, len(clouds[b])], len(clouds[b]), **kw), alone)
        assert np.array_equal(alone["labels"], ref["labels"][off[b]:off[b + 1]]) and \
            np.array_equal(_bits64(alone["planes"][0]), _bits64(ref["planes"][b])) and alone["best"][0].tolist() == ref["best"][b].tolist()
    order = [4, 3, 0, 1, 2]                                            # the same clouds at other batch positions
    moved = _run(np.concatenate([clouds[b] for b in order]), _offsets([len(clouds[b]) for b in order]), 1500, **kw)
    assert all(np.array_equal(_bits64(moved["planes"][i]), _bits64(ref["planes"][b])) and moved["best"][i].tolist() == ref["best"][b].tolist()
               for i, b in enumerate(order))
    first = _run(p, off, 1500, **kw)
    assert _same_all(first, _run(p, off, 1500, **kw)) and _same_all(first, _run(p, off, 10 ** 6, **kw))   # again; a loose host bound
    bare = _run(p, off, 1500, optional=False, **kw)
    assert set(bare) == {"labels", "planes", "num"}
    _check_segment(bare, ref)
    _check_filter(_run(p, off, 1500, keep=0, optional=False, **kw),
                  REF.filter_ragged(p, off, max_per_sample=1500, keep_planes=False, labelled=ref, **kw), 5)
    for counts, bound in (([1000, 5, 1024, 0, 1025], 1500), ([-5, 1 << 30, 2, 1, 1024], 1500), (None, 1000)):
        _segment_and_filter(p, off, bound, kw, counts=counts, keeps=(0,))
    dense_off = _offsets([700] * 4)
    dense = np.concatenate([faces[:700], noisy[:700], slab[:700], faces[500:1200]])
    ref, _ = _segment_and_filter(dense, dense_off, 700, kw, dense=True)
    _segment_and_filter(dense, dense_off, 700, kw, counts=[700, 0, 13, 699], dense=True, keeps=(1,))
    assert ref["num_planes"].min() >= 1


@gpu
def test_results_do_not_depend_on_stale_state():
    """The same bits after a launch that fills every CU's LDS with NaN patterns."""
    from rald_amd._handles import _stream
    from rald_amd._lib import check, lib
    p, _ = REF.faces_cloud("built")
    for keep in (None, 0):
        first = _run(p, [0, len(p)], len(p), keep=keep, **REF.FACES)
        check(lib().rald_debug_poison_lds(_stream()))
        assert _same_all(first, _run(p, [0, len(p)], len(p), keep=keep, **REF.FACES))


@gpu
def test_refused_arguments():
    """Every invalid argument is refused with a status before any GPU work: the outputs keep their poison."""
    p, _ = REF.slab_cloud(257)
    for bad in (dict(t=0.0), dict(t=float("nan")), dict(H=0), dict(H=65537), dict(K=0), dict(K=9), dict(min_inliers=2), dict(refine=2),
                dict(view=(0.0, float("inf"), 0.0))):
        with pytest.raises(RuntimeError):
            _run(p, [0, 257], 257, **dict(REF.SLAB, **bad))
        with pytest.raises(RuntimeError):
            _run(p, [0, 257], 257, keep=0, **dict(REF.SLAB, **bad))
    from rald_amd._lib import lib
    assert lib().rald_post_plane_scratch_bytes(1, 257, 257, 65537, 1) == -1 and lib().rald_post_plane_scratch_bytes(1, 257, 257, 64, 9) == -1


# ---- the Python layer ----------------------------------------------------------------------------------------------------------------------
@gpu
def test_python_layer():
    from rald_amd import postprocess as PP
    faces, _ = REF.faces_cloud("shuffled")
    noisy, _, centre = REF.noisy_cloud()
    off = _offsets([len(faces), 0, len(noisy)])
    p = np.concatenate([faces, noisy])
    kw = dict(t=0.03125, H=256, K=4, min_inliers=256, refine=True, seed=3)
    ref = REF.segment_ragged(p, off, max_per_sample=len(noisy), **kw)
    dp, doff = torch.from_numpy(p).cuda(), torch.tensor(off, device="cuda")
    args = dict(num_hypotheses=256, max_planes=4, min_inliers=256, refine=True, seed=3)
    out = PP.segment_planes_ragged(dp, doff, 0.03125, len(noisy), **args)
    assert len(out) == 4 and [t.dtype for t in out] == [torch.int32, torch.float64, torch.int32, torch.int32]
    assert np.array_equal(out[0].cpu().numpy(), ref["labels"]) and np.array_equal(_bits64(out[1].cpu().numpy()), _bits64(ref["planes"]))
    assert out[2].tolist() == ref["num_planes"].tolist() and out[3].tolist() == ref["inliers"].tolist()
    best = PP.segment_planes_ragged(dp, doff, 0.03125, len(noisy), return_best=True, **args)[4]
    assert best.tolist() == ref["best"].tolist()
    for keep in (False, True):
        fref = REF.filter_ragged(p, off, max_per_sample=len(noisy), keep_planes=keep, labelled=ref, **kw)
        M = int(fref["offsets"][-1])
        out = PP.remove_planes_ragged(dp, doff, 0.03125, len(noisy), keep_planes=keep, return_index=True, return_labels=True, **args)
        assert len(out) == 6 and out[1].tolist() == fref["offsets"].tolist() and 0 < M < len(p)
        assert np.array_equal(_bits(out[0][:M].cpu().numpy()), _bits(fref["points"])) and np.array_equal(out[2][:M].cpu().numpy(), fref["index"])
        assert np.array_equal(out[3][:M].cpu().numpy(), fref["labels"]) and out[5].tolist() == ref["num_planes"].tolist()
        assert np.array_equal(_bits64(out[4].cpu().numpy()), _bits64(ref["planes"]))
    assert len(PP.remove_planes_ragged(dp, doff, 0.03125, len(noisy), **args)) == 2
    empty = PP.segment_planes_ragged(dp[:0], torch.tensor([0, 0], device="cuda"), 0.1, 1)
    assert empty[2].tolist() == [0] and bool(torch.isnan(empty[1]).all())
    # one cloud: Open3D's shape of result
    one = REF.segment_one(noisy, 0.03, 256, min_inliers=500, view=centre.astype(F32).tolist())
    plane, idx = PP.segment_plane(torch.from_numpy(noisy).cuda(), 0.03, num_hypotheses=256, min_inliers=500, view=centre.astype(F32).tolist())
    assert plane.dtype == torch.float64 and idx.dtype == torch.int64 and np.array_equal(_bits64(plane.cpu().numpy()), _bits64(one["planes"][0]))
    assert np.array_equal(idx.cpu().numpy(), np.nonzero(one["labels"] == 0)[0])
    rest = PP.remove_planes(torch.from_numpy(noisy).cuda(), 0.03, num_hypotheses=256, min_inliers=500, view=centre.astype(F32).tolist())
    assert np.array_equal(_bits(rest.cpu().numpy()), _bits(noisy[one["labels"] == -1]))
    none = PP.segment_plane(torch.from_numpy(noisy[:2]).cuda(), 0.03)
    assert bool(torch.isnan(none[0]).all()) and none[1].numel() == 0
    with pytest.raises(RuntimeError):
        PP.segment_planes_ragged(torch.from_numpy(p), doff, 0.03125, len(noisy))


# ---- the tail ------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_infer_point_clouds_remove_planes(monkeypatch):
    """infer_point_clouds(..., remove_planes=(0.5, 64, 2)) on the 4-frame setup of tests/test_gpu_infer_batch.py: the new keys equal
    remove_planes_ragged and the reference applied to the 'pred' it returned, 'pred' and 'cd' equal the call without the argument, and
    the number of host reads is the same (one).  The seed is the generator's; thin and resample run on the result."""
    from rald_amd import engine_generation as E, postprocess as PP, query_points as QP, synth
    from test_gpu_infer_batch import _small_vae, _tail_args
    vae, z9 = _small_vae()
    z = z9[:4].contiguous()
    n, aug = 3000, 2048
    t, H, K = 0.5, 64, 2
    args = _tail_args(n, aug)
    helpers = [synth.queries(1, max(h, 1), seed=100 + h)[0][:h].cuda() for h in (0, 1, 500, 1100)]
    surfaces = synth.point_cloud(4, 1000, seed=62).cuda()
    draws = QP.draw_tail_randoms(4, n, aug, 10, torch.Generator("cuda").manual_seed(23))
    kw = dict(helper_points=helpers, surfaces=surfaces, draws=draws)

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
    for keep, seed, rng in ((False, 0, None), (True, 77, torch.Generator("cuda").manual_seed((5 << 32) + 77))):
        res, reads = counted(remove_planes=(t, H, K, keep), rng=rng)
        assert reads == base_reads == 1
        assert set(res) == set(base) | {"denoised", "denoise_index", "cd_denoised", "denoise_labels", "planes", "num_planes"}
        assert res["n_queries"] == base["n_queries"] and all(torch.equal(a, b) for a, b in zip(res["pred"], base["pred"]))
        stats = []
        for b in range(4):
            pred = res["pred"][b]
            m = pred.shape[0]
            ref = REF.filter_ragged(pred.cpu().numpy(), [0, m], t, H, max(m, 1), keep_planes=keep, K=K, seed=seed, view=(0.0, 0.0, 0.0))
            M = int(ref["offsets"][-1])
            assert np.array_equal(res["denoise_index"][b].cpu().numpy(), ref["index"]) and res["denoise_index"][b].dtype == torch.int64, b
            assert np.array_equal(_bits(res["denoised"][b].cpu().numpy()), _bits(ref["points"])), b
            assert np.array_equal(res["denoise_labels"][b].cpu().numpy(), ref["labels"]) and res["denoise_labels"][b].dtype == torch.int32, b
            assert res["num_planes"][b] == int(ref["num_planes"][0]) and len(res["planes"][b]) == res["num_planes"][b]
            assert np.array_equal(_bits64(np.array(res["planes"][b], np.float64).reshape(-1, 4)), _bits64(ref["planes"][0, :res["num_planes"][b]]))
            assert torch.equal(res["denoised"][b], pred[res["denoise_index"][b]])
            off = torch.tensor([0, m], device="cuda")
            direct = PP.remove_planes_ragged(pred, off, t, max(m, 1), H, K, seed=seed, keep_planes=keep, return_labels=True)
            assert torch.equal(direct[0][:M], res["denoised"][b]) and torch.equal(direct[2][:M], res["denoise_labels"][b])
            stats.append((m, M, int(ref["num_planes"][0])))
        print("final clouds, their kept rows and planes:", stats)
        assert any(0 < k < m for m, k, _ in stats)
    chained, _ = counted(remove_planes=(t, H), thin=1.0, resample=50)
    assert set(chained) == set(base) | {"denoised", "denoise_index", "cd_denoised", "denoise_labels", "planes", "num_planes", "thinned",
                                        "thin_count", "thin_first", "resampled", "resample_index"}
    dev = E.infer_point_clouds_device(vae, z, args, remove_planes=(t, H, K, True), rng=torch.Generator("cuda").manual_seed(77), **kw)
    assert len(dev) == 10 and dev[4].tolist() == _offsets([k for _, k, _ in stats]) and dev[9].tolist() == [c for _, _, c in stats]
    with pytest.raises(ValueError):
        E.infer_point_clouds(vae, z, args, remove_planes=(t, H), denoise=(0.5, 2), **kw)
