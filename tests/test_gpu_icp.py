"""ICP registration and the rigid transform of ragged clouds on the GPU (rald_amd/csrc/cloud_icp.hip) against tests/icp_ref.py, by
equality: integers as integers, floats and doubles by bit pattern - no tolerance anywhere.  Every call goes through _run: the outputs
are pre-filled with poison (NaNs with a payload, -7) and followed by guard rows, the input rows the kernels must not read (behind
counts, behind the bound, behind offsets[B]; points and normals alike) are NaN, the scratch is filled with 0xFF and followed by a
guard, and the checks assert that everything the definition does not write still holds its poison.  tests/test_icp_host.py holds the
reference against an independent route on the same cases and shows on the reference alone what each is for."""
import numpy as np
import pytest
import torch

import icp_ref as REF
from test_gpu_radius_filter import F32, GUARD, POISON_F, POISON_I, _bits, _offsets, _spans

gpu = pytest.mark.gpu
F64 = np.float64
POISON_D = np.array([0x7FF8000000012345], np.uint64).view(F64)[0]
_bits64 = lambda a: np.ascontiguousarray(a, dtype=F64).view(np.uint64)
KEYS = ("transform", "stats", "info", "corr", "moved")


def _hide(rows, T, offsets, bound, counts):
    dev = np.concatenate([np.array(rows, F32).reshape(-1, 3), np.zeros((GUARD, 3), F32)])
    dev[_spans(T, offsets, bound, counts)] = np.nan
    return dev


def _run(src, so, tgt, to, grid, max_dist, max_src, max_tgt, mode=0, normals=None, init=None, max_iterations=30, tolerance=1e-6,
         min_correspondences=6, src_counts=None, tgt_counts=None, chunk=0, post=False, dense=False, optional=True):
    """The C entries on poisoned, guarded buffers -> dict of numpy arrays, whole buffers (guards included).  post: rald_post_icp_ragged
    (no chunk); dense: both offsets describe equal clouds, passed as n_dense with NULL offsets; optional: with out_corr and out_moved."""
    import ctypes as C
    from rald_amd._handles import _stream
    from rald_amd._lib import check, lib
    Ts, Tt, B = len(src), len(tgt), len(so) - 1
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    t = dict(src=cu(_hide(src, Ts, so, max_src, src_counts)), tgt=cu(_hide(tgt, Tt, to, max_tgt, tgt_counts)),
             so=None if dense else cu(np.array(so, np.int64)), to=None if dense else cu(np.array(to, np.int64)),
             sc=None if src_counts is None else cu(np.array(src_counts, np.int32)),
             tc=None if tgt_counts is None else cu(np.array(tgt_counts, np.int32)),
             normals=None if normals is None else cu(_hide(normals, Tt, to, max_tgt, tgt_counts)),
             init=None if init is None else cu(np.concatenate([np.array(init, F64).reshape(B, 12), np.full((GUARD, 12), np.nan)])),
             transform=cu(np.full((B + GUARD, 16), POISON_D, F64)), stats=cu(np.full((B + GUARD, 4), POISON_D, F64)),
             info=cu(np.full((B + GUARD, 3), POISON_I, np.int32)))
    if optional:
        t.update(corr=cu(np.full(Ts + GUARD, POISON_I, np.int64)), moved=cu(np.full((Ts + GUARD, 3), POISON_F, F32)))
    L = lib()
    nbytes = L.rald_post_icp_scratch_bytes(B, Ts, max_src, Tt, max_tgt) if post else L.rald_op_icp_scratch_bytes(B, Ts, max_src, Tt, max_tgt, chunk)
    if nbytes < 0:                                                     # sizes the call refuses too: it must say so itself
        nbytes = 1 << 16
    scratch = torch.empty(nbytes + 16 * GUARD, dtype=torch.uint8, device="cuda")
    scratch[:nbytes] = 0xFF                                            # -1 / NaN everywhere: nothing may rest on a zeroed scratch
    scratch[nbytes:] = 0xA5
    ptr = lambda k: None if t.get(k) is None else t[k].data_ptr()
    lo3, v3, dims3 = grid
    args = (ptr("src"), ptr("so"), ptr("sc"), so[1] - so[0] if dense else 0, Ts, max_src,
            ptr("tgt"), ptr("to"), ptr("tc"), to[1] - to[0] if dense else 0, Tt, max_tgt, ptr("normals"), B,
            (C.c_float * 3)(*lo3), (C.c_float * 3)(*v3), (C.c_int32 * 3)(*dims3), int(mode), float(max_dist), int(max_iterations),
            float(tolerance), int(min_correspondences), ptr("init"), ptr("transform"), ptr("stats"), ptr("info"), ptr("corr"), ptr("moved"),
            scratch.data_ptr(), nbytes)
    check(L.rald_post_icp_ragged(*args, _stream()) if post else L.rald_op_icp_ragged(*args, chunk, _stream()))
    torch.cuda.synchronize()
    assert bool((scratch[nbytes:] == 0xA5).all()), "the scratch's guard was written"
    return {k: t[k].cpu().numpy() for k in KEYS if k in t}


def _check(got, ref):
    """Everything the call writes equals the reference; everything else still holds its poison."""
    B, Ts = len(ref["info"]), len(ref["corr"])
    assert np.array_equal(got["info"][:B], ref["info"]) and (got["info"][B:] == POISON_I).all(), (got["info"][:B], ref["info"])
    for k, width in (("transform", 16), ("stats", 4)):
        bad = np.nonzero(_bits64(got[k][:B]) != _bits64(ref[k]))
        assert bad[0].size == 0, (k, bad, got[k][:B][bad][:4], ref[k][bad][:4])
        assert (_bits64(got[k][B:]) == _bits64(POISON_D)).all()
    if "corr" in got:
        un = ref["untouched"]
        want = np.where(un, POISON_I, ref["corr"])
        bad = np.nonzero(got["corr"][:Ts] != want)[0]
        assert bad.size == 0, (bad[:5], got["corr"][bad[:5]], want[bad[:5]])
        assert (got["corr"][Ts:] == POISON_I).all()
        want = np.where(un[:, None], _bits(POISON_F), _bits(ref["moved"]))
        bad = np.nonzero((_bits(got["moved"][:Ts]) != want).any(axis=1))[0]
        assert bad.size == 0, (bad[:5], got["moved"][bad[:5]], ref["moved"][bad[:5]])
        assert (_bits(got["moved"][Ts:]) == _bits(POISON_F)).all()


def _same(a, b):
    view = lambda v: v.view(np.uint64) if v.dtype == F64 else (v.view(np.uint32) if v.dtype == F32 else v)
    return a.keys() == b.keys() and all(np.array_equal(view(a[k]), view(b[k])) for k in a)


def _as_ragged(one, n_src):
    """icp_one's result as icp_ragged's for a batch of one."""
    return dict(transform=one["transform"][None], stats=one["stats"][None], info=one["info"][None], corr=one["corr"], moved=one["moved"],
                untouched=np.zeros(n_src, bool))


def _case(name, **how):
    """A case of icp_ref.CASES alone in a batch of one -> (the pair, the reference's result)."""
    pair, kw, ref = REF.case(name)
    n, m = len(pair["src"]), len(pair["tgt"])
    got = _run(pair["src"], [0, n], pair["tgt"], [0, m], pair["grid"], pair["max_dist"], max(n, 1), max(m, 1), normals=pair["normals"],
               **kw, **how)
    _check(got, _as_ragged(ref, n))
    return pair, ref


# ---- the constructions ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("motion", list(REF.MOTIONS))
@pytest.mark.parametrize("mode", ("plane", "point"))
def test_faces(motion, mode):
    """Three orthogonal faces, the source 1000 of the 3000 target rows after a known motion: converged within 30 iterations, the
    motion recovered (shown on the reference in tests/test_icp_host.py), every output the reference's bits; by the automatic chunk, by
    chunks of 1024 (three of them) and through rald_post_icp_ragged."""
    pair, ref = _case(f"faces_{motion}_{mode}")
    assert ref["info"][0] == 1 and ref["info"][1] < 30 and ref["stats"][0] == 1.0
    _case(f"faces_{motion}_{mode}", chunk=1024)
    _case(f"faces_{motion}_{mode}", post=True)


@gpu
@pytest.mark.parametrize("mode", ("plane", "point"))
def test_overlap(mode):
    """300 further source rows far from every target row: fitness is exactly 1000 / 1300 and their correspondence -1."""
    _, ref = _case(f"overlap_{mode}")
    assert ref["stats"][0] == 1000 / 1300 and (ref["corr"][1000:] == -1).all() and (ref["corr"][:1000] >= 0).all()


@gpu
def test_tie_and_edge():
    """Source rows exactly midway between two and between eight rows of a lattice take the lowest target row; rows at exactly d2 ==
    fl(max_dist^2) count, rows one float farther do not - in the evaluation at the identity, and in the sums of one step."""
    _, ref = _case("tie_eval")
    assert ref["info"].tolist() == [2, 0, 120]
    for name in ("tie_step_point", "tie_step_plane", "edge_step"):
        _case(name)
        _case(name, chunk=1024)
    _, ref = _case("edge_eval")
    assert ref["corr"].tolist() == [0, -1, 1, -1, 2, -1, 3, -1, 4, -1, 5, -1, 6, -1]


@gpu
def test_planar_and_line():
    """A target on one exact plane: plane mode is refused at iteration 0 by the pivot rule (status 3, the transform unchanged), point
    mode converges.  Rows along a line: point mode is refused by the pivot FLOOR (the pivot is positive)."""
    _, ref = _case("planar_plane")
    assert ref["info"].tolist() == [3, 0, 600] and ref["transform"].tolist() == np.eye(4).reshape(-1).tolist()
    _, ref = _case("planar_point")
    assert ref["info"][0] == 1
    _, ref = _case("line_point")
    assert ref["info"].tolist() == [3, 0, 400]


@gpu
def test_few_and_bad_rows():
    """0, 1, 5 and 6 counting rows against min_correspondences = 6 (status 2 below it); NaN / inf rows on both sides, target rows
    outside the grid, zero and NaN target normals."""
    for n, status in ((0, 2), (1, 2), (5, 2), (6, 1)):
        _, ref = _case(f"few_{n}")
        assert ref["info"][0] == status and ref["info"][2] == n
    for mode in ("plane", "point"):
        _, ref = _case(f"bad_rows_{mode}")
        assert ref["info"][0] == 1
        assert (ref["corr"][[3, 500, 999]] == -1).all()


@gpu
@pytest.mark.parametrize("n", (1023, 1024, 1025, 2049))
def test_sum_shape_boundaries(n):
    """Source lengths around CLOUD_SEG = 1024, the block of the fixed sum shape, against a target that needs three sort chunks of 1024.
    icp_sums and icp_solve are the hand-scheduled instance of that shape (two tree levels in registers, sixteen block sums in flight);
    every other user calls block_tree_sum and fold_blocks of cloud_index.h.  This test pins the hand-scheduled one to the same bits."""
    _case(f"length_{n}", chunk=1024)
    _case(f"length_{n}")


@gpu
def test_iteration_counts():
    """tolerance 0 runs all iterations (status 0); max_iterations 1 and 64."""
    _, ref = _case("tolerance_0")
    assert ref["info"].tolist() == [0, 6, 300]
    _, ref = _case("iterations_64")
    assert ref["info"].tolist() == [0, 64, 300]
    _, ref = _case("iterations_1")
    assert ref["info"].tolist() == [0, 1, 300]


# ---- ragged batches ------------------------------------------------------------------------------------------------------------------------
def _batch():
    names = ["faces_small_plane", "few_0", "length_1025", "planar_plane", "faces_large_plane"]
    pairs = [dict(REF.case(n)[0]) for n in names]
    pairs[1] = dict(pairs[1], src=np.zeros((0, 3), F32))                                  # an empty source
    pairs[3] = dict(pairs[3], tgt=np.zeros((0, 3), F32), normals=np.zeros((0, 3), F32))   # an empty target
    return names, pairs


def _ragged(pairs, order=None):
    order = range(len(pairs)) if order is None else order
    cat = lambda key: np.concatenate([pairs[b][key] for b in order])
    return (cat("src"), _offsets([len(pairs[b]["src"]) for b in order]), cat("tgt"), _offsets([len(pairs[b]["tgt"]) for b in order]),
            cat("normals"))


@gpu
def test_ragged_batch_counts_and_dense():
    """B = 5 with an empty source and an empty target; every pair's result equals its one-pair result, at every batch position and for
    every chunk; `counts` that trim, bounds shorter than a cloud, the dense layout, an initial transform, without the optional outputs."""
    names, pairs = _batch()
    src, so, tgt, to, nrm = _ragged(pairs)
    kw = dict(grid=REF.FACES_GRID, max_dist=REF.FACES_DIST, max_src=1025, max_tgt=3000, mode=1)
    ref = REF.icp_ragged(src, so, tgt, to, normals=nrm, **kw)
    assert ref["info"][:, 0].tolist() == [1, 2, 1, 2, 1] and ref["info"][1].tolist() == [2, 0, 0] and ref["info"][3].tolist() == [2, 0, 0]
    first = _run(src, so, tgt, to, normals=nrm, **kw)
    _check(first, ref)
    for b in (0, 2, 4):                                                # the batch's pair is the pair alone, by bits
        alone = REF.case(names[b])[2]
        assert np.array_equal(_bits64(alone["transform"]), _bits64(ref["transform"][b])) and \
            np.array_equal(_bits64(alone["stats"]), _bits64(ref["stats"][b])) and np.array_equal(alone["corr"], ref["corr"][so[b]:so[b + 1]])
    assert _same(first, _run(src, so, tgt, to, normals=nrm, **kw)) and _same(first, _run(src, so, tgt, to, normals=nrm, chunk=1024, **kw))
    assert _same(first, _run(src, so, tgt, to, normals=nrm, **dict(kw, max_src=10 ** 6, max_tgt=10 ** 6)))        # loose host bounds
    order = [4, 3, 0, 1, 2]                                            # the same pairs at other batch positions
    moved = _run(*_ragged(pairs, order)[:4], normals=_ragged(pairs, order)[4], chunk=2048, **kw)
    for i, b in enumerate(order):
        for k in ("transform", "stats", "info"):
            assert _same({k: moved[k][i]}, {k: first[k][b]}), (k, i, b)
    bare = _run(src, so, tgt, to, normals=nrm, optional=False, **kw)
    assert set(bare) == {"transform", "stats", "info"}
    _check(bare, ref)
    for sc, tc, bs, bt in (([1000, 5, 1024, 600, 7], [3000, 3000, 2999, 0, 1500], 1025, 3000), ([-5, 1 << 30, 2, 1, 1000], None, 1025, 3000),
                           (None, [3000, 0, 3000, 5, 2000], 800, 2500)):
        kw2 = dict(kw, max_src=bs, max_tgt=bt)
        _check(_run(src, so, tgt, to, normals=nrm, src_counts=sc, tgt_counts=tc, **kw2),
               REF.icp_ragged(src, so, tgt, to, normals=nrm, src_counts=sc, tgt_counts=tc, **kw2))
    # an initial transform: the inverse motion of pair 4 brings every pair that has its motion home in fewer steps
    f = pairs[4]
    init = np.tile(np.concatenate([f["Rm"].T.reshape(9), -f["Rm"].T @ f["tm"]]), (5, 1))
    init[0] = REF.IDENTITY
    got = _run(src, so, tgt, to, normals=nrm, init=init, mode=0, **{k: v for k, v in kw.items() if k != "mode"})
    want = REF.icp_ragged(src, so, tgt, to, normals=nrm, init=init, **dict(kw, mode=0))
    _check(got, want)
    assert want["info"][4, 1] < REF.case("faces_large_point")[2]["info"][1] and np.array_equal(want["transform"][3].reshape(4, 4)[:3, :3],
                                                                                                 f["Rm"].T)
    # the dense layout: four pairs of 700 source and 1500 target rows
    dsrc = np.concatenate([pairs[b]["src"][:700] for b in (0, 2, 4, 0)])
    dtgt = np.concatenate([pairs[b]["tgt"][:1500] for b in (0, 2, 4, 2)])
    dnrm = np.concatenate([pairs[b]["normals"][:1500] for b in (0, 2, 4, 2)])
    dso, dto = _offsets([700] * 4), _offsets([1500] * 4)
    kw3 = dict(kw, max_src=700, max_tgt=1500)
    _check(_run(dsrc, dso, dtgt, dto, normals=dnrm, dense=True, **kw3), REF.icp_ragged(dsrc, dso, dtgt, dto, normals=dnrm, **kw3))
    _check(_run(dsrc, dso, dtgt, dto, normals=dnrm, dense=True, src_counts=[700, 0, 13, 699], **kw3),
           REF.icp_ragged(dsrc, dso, dtgt, dto, normals=dnrm, src_counts=[700, 0, 13, 699], **kw3))


@gpu
def test_results_do_not_depend_on_stale_state():
    """The same bits after a launch that fills every CU's LDS with NaN patterns."""
    from rald_amd._handles import _stream
    from rald_amd._lib import check, lib
    pair, kw, _ = REF.case("length_2049")
    n, m = len(pair["src"]), len(pair["tgt"])
    run = lambda: _run(pair["src"], [0, n], pair["tgt"], [0, m], pair["grid"], pair["max_dist"], n, m, normals=pair["normals"], **kw)
    first = run()
    check(lib().rald_debug_poison_lds(_stream()))
    assert _same(first, run())


@gpu
def test_refused_arguments():
    """Every invalid argument is refused with a status before any GPU work."""
    pair, kw, _ = REF.case("few_6")
    n, m = len(pair["src"]), len(pair["tgt"])
    base = dict(grid=pair["grid"], max_dist=pair["max_dist"], max_src=n, max_tgt=m, mode=1, normals=pair["normals"])
    small = ((-1.0,) * 3, (0.25,) * 3, (25,) * 3)
    for bad in (dict(mode=2), dict(mode=1, normals=None), dict(max_dist=0.0), dict(max_dist=float("nan")), dict(max_iterations=0),
                dict(max_iterations=65), dict(tolerance=-1.0), dict(tolerance=float("nan")), dict(min_correspondences=0), dict(grid=small),
                dict(max_src=0), dict(max_tgt=(1 << 24) + 1), dict(chunk=1000)):
        with pytest.raises(RuntimeError):
            _run(pair["src"], [0, n], pair["tgt"], [0, m], **dict(base, **bad))
    from rald_amd._lib import lib
    L = lib()
    assert L.rald_post_icp_scratch_bytes(0, n, n, m, m) == -1 and L.rald_post_icp_scratch_bytes(1, n, 0, m, m) == -1
    assert L.rald_post_icp_scratch_bytes(1, n, n, 1 << 31, m) == -1 and L.rald_op_icp_scratch_bytes(1, n, n, m, m, 1000) == -1
    assert L.rald_post_icp_scratch_bytes(1, n, n, m, m) > 0


# ---- the rigid transform -------------------------------------------------------------------------------------------------------------------
@gpu
def test_rigid_transform():
    """Points and normals of a ragged batch with an empty cloud, counts and a short bound, by [B,12] and by [B,16] transforms; the
    points are the ICP's out_moved for its out_transform."""
    from rald_amd._handles import _stream
    from rald_amd._lib import check, lib
    rs = np.random.RandomState(41)
    lengths = [300, 0, 1025, 77]
    off = _offsets(lengths)
    T = off[-1]
    p = rs.uniform(-5, 5, size=(T, 3)).astype(F32)
    nrm = rs.normal(size=(T, 3)).astype(F32)
    p[[5, 400]] = [[np.nan, 1, 1], [1, np.inf, 1]]
    M16 = np.zeros((4, 16), F64)
    for b in range(4):
        M = np.eye(4)
        M[:3, :3] = REF.rotation(rs.normal(size=3), rs.uniform(0, 180))
        M[:3, 3] = rs.normal(size=3)
        M16[b] = M.reshape(-1)
    M12 = np.concatenate([M16.reshape(4, 4, 4)[:, :3, :3].reshape(4, 9), M16.reshape(4, 4, 4)[:, :3, 3]], axis=1)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for M, counts, bound, with_normals in ((M12, None, 1025, True), (M16, None, 1025, True), (M16, [300, 5, 1000, 0], 900, True),
                                           (M12, None, 1025, False)):
        want_p, want_n, un = REF.transform_ragged(p, off, M, bound, nrm if with_normals else None, counts)
        dp, dn = cu(_hide(p, T, off, bound, counts)), cu(_hide(nrm, T, off, bound, counts))
        out = cu(np.full((T + GUARD, 3), POISON_F, F32))
        outn = cu(np.full((T + GUARD, 3), POISON_F, F32))
        dM = cu(np.concatenate([M, np.full((GUARD, M.shape[1]), np.nan)]))
        doff, dcounts = cu(np.array(off, np.int64)), None if counts is None else cu(np.array(counts, np.int32))
        check(lib().rald_post_rigid_transform_ragged(dp.data_ptr(), doff.data_ptr(), None if counts is None else dcounts.data_ptr(), 4, 0, T, bound,
                                                     dM.data_ptr(), M.shape[1], dn.data_ptr() if with_normals else None, out.data_ptr(),
                                                     outn.data_ptr() if with_normals else None, _stream()))
        torch.cuda.synchronize()
        got, gotn = out.cpu().numpy(), outn.cpu().numpy()
        assert np.array_equal(_bits(got[:T]), np.where(un[:, None], _bits(POISON_F), _bits(want_p))) and (_bits(got[T:]) == _bits(POISON_F)).all()
        if with_normals:
            assert np.array_equal(_bits(gotn[:T]), np.where(un[:, None], _bits(POISON_F), _bits(want_n)))
        assert (_bits(gotn[T:]) == _bits(POISON_F)).all() and (with_normals or (_bits(gotn) == _bits(POISON_F)).all())
    for bad in (dict(stride=13), dict(bound=0)):
        rc = lib().rald_post_rigid_transform_ragged(dp.data_ptr(), doff.data_ptr(), None, 4, 0, T, bad.get("bound", 1025),
                                                    dM.data_ptr(), bad.get("stride", 12), None, out.data_ptr(), None, _stream())
        assert rc != 0


# ---- the Python layer ----------------------------------------------------------------------------------------------------------------------
@gpu
def test_python_layer():
    from rald_amd import postprocess as PP
    names, pairs = _batch()
    src, so, tgt, to, nrm = _ragged(pairs)
    kw = dict(grid=REF.FACES_GRID, max_dist=REF.FACES_DIST, max_src=1025, max_tgt=3000)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dsrc, dso, dtgt, dto, dnrm = cu(src), cu(np.array(so, np.int64)), cu(tgt), cu(np.array(to, np.int64)), cu(nrm)
    for mode, normals in ((1, dnrm), (0, None)):
        ref = REF.icp_ragged(src, so, tgt, to, normals=nrm, mode=mode, **kw)
        out = PP.register_icp_ragged(dsrc, dso, dtgt, dto, REF.FACES_DIST, REF.FACES_GRID, 1025, 3000, target_normals=normals,
                                     return_correspondences=True, return_moved=True)
        assert set(out) == {"transform", "fitness", "inlier_rmse", "step", "residual", "status", "iterations", "count", "correspondences", "moved"}
        assert out["transform"].shape == (5, 4, 4) and out["transform"].dtype == torch.float64 and out["status"].dtype == torch.int32
        assert np.array_equal(_bits64(out["transform"].cpu().numpy().reshape(5, 16)), _bits64(ref["transform"]))
        for i, k in enumerate(("fitness", "inlier_rmse", "step", "residual")):
            assert np.array_equal(_bits64(out[k].cpu().numpy()), _bits64(ref["stats"][:, i])), k
        for i, k in enumerate(("status", "iterations", "count")):
            assert out[k].tolist() == ref["info"][:, i].tolist(), k
        assert np.array_equal(out["correspondences"].cpu().numpy(), ref["corr"]) and np.array_equal(_bits(out["moved"].cpu().numpy()), _bits(ref["moved"]))
        # the transform entry applies the result: its points are the call's `moved`
        again = PP.transform_points_ragged(dsrc, dso, out["transform"], 1025)
        assert torch.equal(again.view(torch.int32), out["moved"].view(torch.int32))
    assert set(PP.register_icp_ragged(dsrc, dso, dtgt, dto, REF.FACES_DIST, REF.FACES_GRID, 1025, 3000)) == \
        {"transform", "fitness", "inlier_rmse", "step", "residual", "status", "iterations", "count"}
    # one pair: the grid from the target's own box (its edge doubles until the cells fit; the result does not depend on it)
    f, fkw, fref = REF.case("faces_large_plane")
    one = PP.register_icp(cu(f["src"]), cu(f["tgt"]), REF.FACES_DIST, target_normals=cu(f["normals"]), return_moved=True)
    assert one["transform"].shape == (4, 4) and one["status"].item() == 1
    assert np.array_equal(_bits64(one["transform"].cpu().numpy().reshape(16)), _bits64(fref["transform"]))
    assert np.array_equal(_bits(one["moved"].cpu().numpy()), _bits(fref["moved"]))
    pts, rot = PP.transform_points(cu(f["src"]), one["transform"], normals=cu(f["normals"][:1000]))
    want_p, want_n, _ = REF.transform_ragged(f["src"], [0, 1000], fref["transform"][None], 1000, f["normals"][:1000])
    assert np.array_equal(_bits(pts.cpu().numpy()), _bits(want_p)) and np.array_equal(_bits(rot.cpu().numpy()), _bits(want_n))
    init = torch.from_numpy(fref["transform"].reshape(4, 4)).cuda()
    warm = PP.register_icp(cu(f["src"]), cu(f["tgt"]), REF.FACES_DIST, target_normals=cu(f["normals"]), init=init)
    assert warm["status"].item() == 1 and warm["iterations"].item() == 1
    empty = PP.register_icp(cu(f["src"]), cu(f["tgt"][:0]), REF.FACES_DIST, init=init)
    assert empty["status"].item() == 2 and torch.equal(empty["transform"], init) and empty["fitness"].item() == 0.0
    empty = PP.register_icp(cu(f["src"][:0]), cu(f["tgt"]), REF.FACES_DIST)
    assert empty["status"].item() == 2 and torch.equal(empty["transform"], torch.eye(4, dtype=torch.float64, device="cuda"))
    with pytest.raises(RuntimeError):
        PP.register_icp_ragged(torch.from_numpy(src), dso, dtgt, dto, REF.FACES_DIST, REF.FACES_GRID, 1025, 3000)


# ---- the tail ------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_infer_point_clouds_align(monkeypatch):
    """infer_point_clouds(..., align=...) on the 4-frame setup of tests/test_gpu_infer_batch.py: every key of the call without `align`
    is bit-identical, the number of host reads is the same (one), and the new keys equal register_icp_ragged and the reference applied
    to the 'pred' it returned and the surfaces in the final frame - point mode, and plane mode with normal_consistency's (k, cell) or
    its own."""
    from rald_amd import engine_generation as E, postprocess as PP, query_points as QP, synth
    from test_gpu_infer_batch import PC_RANGE, _small_vae, _tail_args
    vae, z9 = _small_vae()
    z = z9[:4].contiguous()
    n, aug = 3000, 2048
    args = _tail_args(n, aug)
    helpers = [synth.queries(1, max(h, 1), seed=100 + h)[0][:h].cuda() for h in (0, 1, 500, 1100)]
    surfaces = synth.point_cloud(4, 1000, seed=62).cuda()
    draws = QP.draw_tail_randoms(4, n, aug, 10, torch.Generator("cuda").manual_seed(23))
    kw = dict(helper_points=helpers, surfaces=surfaces, draws=draws, metric_thresholds=(0.5, 1.0))

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

    def identical(a, b):
        if isinstance(a, torch.Tensor):
            return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))
        if isinstance(a, (list, tuple)):
            return len(a) == len(b) and all(identical(x, y) for x, y in zip(a, b))
        if isinstance(a, dict):
            return a.keys() == b.keys() and all(identical(a[k], b[k]) for k in a)
        return a == b or (isinstance(a, float) and a != a and b != b)
    new = {"align_transform", "align_fitness", "align_rmse", "align_status", "aligned", "cd_aligned", "metrics_aligned"}
    gt = PP.polar2cartesian(PP.inverse_norm_points(surfaces.reshape(-1, 3), PC_RANGE, True, False)).cpu().numpy().reshape(4, 1000, 3)
    grid = PP.voxel_grid([-PC_RANGE[3]] * 3, [PC_RANGE[3]] * 3, 2.0)
    for more, align in ((dict(), ("point", 2.0)), (dict(normals=True, normal_consistency=(8, 1.0)), ("plane", 2.0, 12)),
                        (dict(), ("plane", 2.0, 12, 8, 1.0))):
        base, base_reads = counted(**more)
        res, reads = counted(align=align, **more)
        assert reads == base_reads == 1 and set(res) == set(base) | new
        assert all(identical(res[k], base[k]) for k in base), [k for k in base if not identical(res[k], base[k])]
        mode = PP.ICP_MODES[align[0]]
        iters = align[2] if len(align) > 2 else 30
        stats = []
        for b in range(4):
            pred = res["pred"][b]
            m = pred.shape[0]
            nrm = None
            if mode == 1:
                nrm = PP.estimate_normals_ragged(torch.from_numpy(gt[b]).cuda(), torch.tensor([0, 1000], device="cuda"), 8,
                                                 PP.voxel_grid([-PC_RANGE[3]] * 3, [PC_RANGE[3]] * 3, 1.0), 1000, view=(0.0, 0.0, 0.0)).cpu().numpy()
            ref = REF.icp_one(pred.cpu().numpy(), gt[b], grid, 2.0, mode, nrm, max_iterations=iters)
            assert np.array_equal(_bits64(np.array(res["align_transform"][b], F64).reshape(16)), _bits64(ref["transform"])), b
            assert _bits64(res["align_fitness"][b]) == _bits64(ref["stats"][0]) and _bits64(res["align_rmse"][b]) == _bits64(ref["stats"][1])
            assert res["align_status"][b] == int(ref["info"][0]) and isinstance(res["align_status"][b], int)
            assert np.array_equal(_bits(res["aligned"][b].cpu().numpy()), _bits(ref["moved"])) and res["aligned"][b].shape == (m, 3)
            moved = PP.transform_points(pred, torch.tensor(res["align_transform"][b], dtype=torch.float64, device="cuda")) if m else pred
            assert torch.equal(moved.view(torch.int32), res["aligned"][b].view(torch.int32))
            if m:
                direct = PP.cloud_metrics(res["aligned"][b], torch.from_numpy(gt[b]).cuda(), (0.5, 1.0))
                # the one-frame call may add its float64 terms in another order than the batch: n * 2^-53 with n <= 4096 rows a side
                assert res["cd_aligned"][b] == res["metrics_aligned"][b]["cd"] and direct["cd"] == pytest.approx(res["cd_aligned"][b], rel=1e-12)
            stats.append((m, int(ref["info"][0]), int(ref["info"][1]), round(float(ref["stats"][0]), 3), res["cd"][b], res["cd_aligned"][b]))
        print("align", align, "rows, status, iterations, fitness, cd, cd_aligned:", stats)
        assert any(s[1] in (0, 1) and s[2] > 0 for s in stats)
    bare, _ = counted(align=("point", 2.0, 5))
    assert len(bare["align_transform"]) == 4 and len(bare["align_transform"][0]) == 4 and len(bare["align_transform"][0][0]) == 4
    for bad in (("plane", 2.0), ("point",), ("point", 0.0), ("point", 2.0, 65), ("spline", 2.0), ("plane", 2.0, 5, 0, 1.0), ("point", 1e-9)):
        with pytest.raises(ValueError):
            E.infer_point_clouds(vae, z, args, align=bad, **kw)
    with pytest.raises(ValueError):
        E.infer_point_clouds(vae, z, args, align=("point", 2.0), helper_points=helpers, draws=draws)        # no surfaces
