"""Point-cloud metrics on the GPU: exact nearest neighbours per point, their reductions per frame and the
metrics derived from them.  The reference is the float64 oracle in this file - a brute-force numpy replay of the kernels' operations in
their order, cross-checked against scipy.spatial.cKDTree - and the existing Chamfer path; never the code under test."""
import ctypes as C

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

# (n_pred, n_gt) per frame: single points, around the 16-candidate group, the 256-lane row stride, the 1024-row block / 1024-point tile,
# three chunks of 1024 candidates, and an empty side each way
FRAMES = ((1, 1), (1, 1025), (1025, 1), (63, 64), (64, 65), (255, 1023), (256, 1024), (257, 1025), (1023, 255), (2049, 2500), (0, 7), (7, 0))
N_PRED, N_GT = [f[0] for f in FRAMES], [f[1] for f in FRAMES]
LATTICE_TAUS = (5.0, 5.000001, 1.0, 50.0, 50.5)
RANDOM_TAUS = (0.002, 0.3, 0.7, 1.5)
RANDOM_SEEDS = (1234, 4321)                    # pred, gt; test_oracle_* checks on the CPU that they give no near-tie


def _offsets(lengths):
    return np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)


PO, GO = _offsets(N_PRED), _offsets(N_GT)


# ---- the float64 oracle -------------------------------------------------------------------------------------------------------------------
def oracle_nn(a, b):
    """a [na,3], b [nb,3] float32 -> (d2 float64 [na], idx int64 [na], next float64 [na], ties int64 [na]): the nearest squared
    distance as dx*dx + dy*dy + dz*dz in float64, left to right, every operation rounded; the LOWEST index that reaches it; the
    smallest squared distance that is larger (inf if none) and the number of rows that reach the minimum, for the near-tie checks."""
    A, Bm = a.astype(np.float64), b.astype(np.float64)
    d2, nxt = np.empty(len(A)), np.empty(len(A))
    idx, ties = np.empty(len(A), np.int64), np.empty(len(A), np.int64)
    for i0 in range(0, len(A), 512):
        s = slice(i0, i0 + 512)
        dx, dy, dz = (A[s, None, k] - Bm[None, :, k] for k in range(3))
        m = dx * dx + dy * dy + dz * dz
        idx[s] = m.argmin(axis=1)                              # the first occurrence: the lowest index
        d2[s] = m[np.arange(m.shape[0]), idx[s]]
        ties[s] = (m == d2[s, None]).sum(axis=1)
        nxt[s] = np.where(m > d2[s, None], m, np.inf).min(axis=1)
    return d2, idx, nxt, ties


def apart(dist, nxt, rel):
    """Rows whose nearest and next distinct distance differ by more than rel, relatively (or that have no other distance)."""
    with np.errstate(invalid="ignore"):
        return np.isinf(nxt) | (nxt - dist > rel * nxt)


def replay_sum(v):
    """The order the kernels add a frame's rows in: blocks of 1024 rows; lane t of 256 adds its rows t, 256 + t, 512 + t, 768 + t in
    that order; a butterfly (offsets 32 .. 1) over every 64 lanes; the four wave sums in order; the blocks in order."""
    total = 0.0
    lanes = np.arange(64)
    for x0 in range(0, len(v), 1024):
        blk = np.zeros(1024)
        blk[:len(v[x0:x0 + 1024])] = v[x0:x0 + 1024]
        lane = np.zeros(256)
        for r in range(4):
            lane = lane + blk[r * 256:(r + 1) * 256]
        w = lane.reshape(4, 64)
        for o in (32, 16, 8, 4, 2, 1):
            w = w + w[:, lanes ^ o]
        t = w[0, 0]
        for k in range(1, 4):
            t = t + w[k, 0]
        total = total + t
    return total


def oracle_frame(pred, gt, taus):
    """-> raw [2, 3 + K], (dist, idx, next distinct dist, ties) of pred -> gt and of gt -> pred (None for a frame with an empty side)."""
    raw = np.zeros((2, 3 + len(taus)))
    per = [None, None]
    if len(pred) and len(gt):
        for d, (a, b) in enumerate(((pred, gt), (gt, pred))):
            d2, idx, nxt, ties = oracle_nn(a, b)
            dist = np.sqrt(d2)
            raw[d, 0], raw[d, 1], raw[d, 2] = replay_sum(dist), replay_sum(d2), dist.max()
            raw[d, 3:] = [(dist < np.float64(t)).sum() for t in taus]          # strict, float64, on d
            per[d] = (dist, idx, np.sqrt(nxt), ties)
    return raw, per


def derive(raw, n_pred, n_gt):
    """The metric definitions, from raw [2, 3 + K] of one frame."""
    K = raw.shape[1] - 3
    if n_pred == 0 or n_gt == 0:
        out = {k: float("inf") for k in ("accuracy", "completeness", "cd", "cd_l2", "hausdorff", "mhd")}
        out.update(precision=[0.0] * K, recall=[0.0] * K, f_score=[0.0] * K)
        return out
    acc, comp = raw[0, 0] / n_pred, raw[1, 0] / n_gt
    p, r = raw[0, 3:] / n_pred, raw[1, 3:] / n_gt
    return {"accuracy": acc, "completeness": comp, "cd": 0.5 * acc + 0.5 * comp, "cd_l2": raw[0, 1] / n_pred + raw[1, 1] / n_gt,
            "hausdorff": max(raw[0, 2], raw[1, 2]), "mhd": max(acc, comp), "precision": list(p), "recall": list(r),
            "f_score": [2 * a * b / (a + b) if a + b > 0 else 0.0 for a, b in zip(p, r)]}


# ---- the inputs (built once, never modified) ------------------------------------------------------------------------------------------------
_CACHE = {}


def lattice_clouds():
    """Integer coordinates in [-40, 40] as float32: every product, sum and comparison of the distance is exact."""
    if "lattice" not in _CACHE:
        rng = np.random.RandomState(7)
        pred = rng.randint(-40, 41, size=(PO[-1], 3)).astype(np.float32)
        gt = rng.randint(-40, 41, size=(GO[-1], 3)).astype(np.float32)
        # frame 0 (1, 1): a 3-4-5 pair - d is exactly 5.0, which the strict d < 5.0 does not count and d < 5.000001 does
        pred[PO[0]] = (0, 0, 0)
        gt[GO[0]] = (3, 4, 0)
        # frame 4 (64, 65): gt on a line, pred one step beside it (every d is 1 or sqrt 2), and one outlier at exactly 50
        gt[GO[4]:GO[5]] = [(0, 0, j - 32) for j in range(65)]
        pred[PO[4]:PO[5]] = [(1, 0, i - 32) for i in range(64)]
        pred[PO[4] + 10] = (30, 40, -22)
        # frame 9 (2049, 2500): the same point at rows of different chunks of 1024, of different tiles and inside one 16-candidate group
        g9, p9 = gt[GO[9]:GO[10]], pred[PO[9]:PO[10]]
        g9[[5, 6, 1030, 2100, 2499]] = (17, -23, 31)
        p9[0] = (17, -23, 31)
        p9[[3, 1500, 2047, 2048]] = (-29, 8, -14)
        g9[0] = (-29, 8, -14)
        g9[1] = (-29, 8, -13)                                     # nearest at distance 1, four times
        _CACHE["lattice"] = (pred, gt)
    return _CACHE["lattice"]


def random_clouds():
    """Uniform fp32 coordinates in [-10, 10]^3; frame 7 (257, 1025) sits near 100 on a 1e-3 grid (fp32 spacing there: 7.6e-6)."""
    if "random" not in _CACHE:
        pred = np.random.RandomState(RANDOM_SEEDS[0]).uniform(-10, 10, size=(PO[-1], 3)).astype(np.float32)
        gt = np.random.RandomState(RANDOM_SEEDS[1]).uniform(-10, 10, size=(GO[-1], 3)).astype(np.float32)
        rng = np.random.RandomState(99)
        pred[PO[7]:PO[8]] = (100.0 + 1e-3 * rng.randint(0, 50, size=(N_PRED[7], 3))).astype(np.float32)
        gt[GO[7]:GO[8]] = (100.0 + 1e-3 * rng.randint(0, 50, size=(N_GT[7], 3))).astype(np.float32)
        _CACHE["random"] = (pred, gt)
    return _CACHE["random"]


def oracle_batch(name, taus):
    key = ("oracle", name)
    if key not in _CACHE:
        pred, gt = lattice_clouds() if name == "lattice" else random_clouds()
        _CACHE[key] = [oracle_frame(pred[PO[f]:PO[f + 1]], gt[GO[f]:GO[f + 1]], taus) for f in range(len(FRAMES))]
    return _CACHE[key]


# ---- the calls --------------------------------------------------------------------------------------------------------------------------
POISON_D, POISON_I, GUARD = -12345.5, -987654321, 300


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def raw_call(pred, po, gt, go, max_pred, max_gt, taus, per_point=True):
    """rald_post_cloud_metrics_ragged on poisoned outputs that are GUARD rows longer than the clouds (raw: one row longer) ->
    (raw [B,2,3+K], dist_pred, idx_pred, dist_gt, idx_gt) as device tensors, the guard rows included."""
    from rald_amd._handles import _stream
    from rald_amd._lib import check, lib
    B, K = len(po) - 1, len(taus)
    p, g, pod, god = _dev(pred), _dev(gt), _dev(po), _dev(go)
    raw = torch.full((B + 1, 2, 3 + K), POISON_D, device="cuda", dtype=torch.float64)
    outs = [None] * 4
    if per_point:
        outs = [torch.full((len(pred) + GUARD,), POISON_D, device="cuda", dtype=torch.float64),
                torch.full((len(pred) + GUARD,), POISON_I, device="cuda", dtype=torch.int64),
                torch.full((len(gt) + GUARD,), POISON_D, device="cuda", dtype=torch.float64),
                torch.full((len(gt) + GUARD,), POISON_I, device="cuda", dtype=torch.int64)]
    nbytes = lib().rald_post_cloud_metrics_scratch_bytes(B, max_pred, max_gt)
    assert nbytes > 0
    scratch = torch.empty(nbytes, device="cuda", dtype=torch.uint8)
    tau = (C.c_double * max(K, 1))(*taus)
    check(lib().rald_post_cloud_metrics_ragged(p.data_ptr(), pod.data_ptr(), g.data_ptr(), god.data_ptr(), B, max_pred, max_gt, tau, K,
                                               raw.data_ptr(), *[t.data_ptr() if t is not None else None for t in outs],
                                               scratch.data_ptr(), _stream()))
    return (raw, *outs)


def assert_guards(res, n_pred_rows, n_gt_rows):
    raw, dp, ip, dg, ig = res
    assert bool((raw[-1] == POISON_D).all())
    assert bool((dp[n_pred_rows:] == POISON_D).all()) and bool((ip[n_pred_rows:] == POISON_I).all())
    assert bool((dg[n_gt_rows:] == POISON_D).all()) and bool((ig[n_gt_rows:] == POISON_I).all())


def oracle_rows(oracle, d, which):
    """The frames' per-row oracle values of direction d concatenated (inf / -1 where the other side is empty)."""
    rows = []
    for f, (_, per) in enumerate(oracle):
        n = (N_PRED, N_GT)[d][f]
        if per[d] is None:
            rows.append(np.full(n, np.inf) if which != 1 else np.full(n, -1, np.int64))
        else:
            rows.append(per[d][which])
    return np.concatenate(rows)


# ---- 0. the oracle itself (CPU) -------------------------------------------------------------------------------------------------------------
def test_oracle_agrees_with_ckdtree_and_the_random_clouds_have_no_near_tie():
    """The brute-force replay against scipy's cKDTree on both input sets (distances within 1e-12 relative; indices wherever the
    nearest distance is reached once), and the properties the GPU tests rely on: in the random clouds no row's nearest and next
    distinct distance are within 1e-12 relative, and no distance is within 1e-9 relative of a threshold."""
    from scipy.spatial import cKDTree
    for name, taus in (("lattice", LATTICE_TAUS), ("random", RANDOM_TAUS)):
        pred, gt = lattice_clouds() if name == "lattice" else random_clouds()
        for f, (raw, per) in enumerate(oracle_batch(name, taus)):
            sides = (pred[PO[f]:PO[f + 1]], gt[GO[f]:GO[f + 1]])
            if per[0] is None:
                assert not raw.any()
                continue
            for d in range(2):
                dist, idx, nxt, ties = per[d]
                dd, ii = cKDTree(sides[1 - d].astype(np.float64)).query(sides[d].astype(np.float64))
                assert np.all(np.abs(dd - dist) <= 1e-12 * dist), (name, f, d)
                once = (ties == 1) & apart(dist, nxt, 1e-9)
                assert np.array_equal(ii[once], idx[once]), (name, f, d)
                if name == "random":
                    assert np.all(apart(dist, nxt, 1e-12)), (f, d, "near-tie: choose other seeds")
                    for t in taus:
                        assert np.all(np.abs(dist - t) > 1e-9 * t), (f, d, t)
    # the planted lattice cases, on the oracle
    lat = oracle_batch("lattice", LATTICE_TAUS)
    assert lat[0][1][0][0][0] == 5.0 and list(lat[0][0][0, 3:5]) == [0.0, 1.0]
    d4 = np.sort(lat[4][1][0][0])
    assert d4[-1] == 50.0 and d4[-2] <= np.sqrt(2.0) and lat[4][0][1, 2] == np.sqrt(2.0)
    assert lat[9][1][0][1][0] == 5 and lat[9][1][0][0][0] == 0.0 and lat[9][1][1][1][0] == 3 and lat[9][1][1][1][1] == 3


# ---- 1. integer lattice, bit-exact -----------------------------------------------------------------------------------------------------------
@gpu
def test_integer_lattice_is_bit_exact():
    """Integer coordinates in [-40, 40]: d^2 is an exact integer, so per-row distances, indices (equal distances abound on a lattice:
    the lowest index must win everywhere) and raw are torch.equal to the oracle - with the automatic chunking and with chunks of 1024
    (2500 rows: 3 chunks), 2048 and 3072 candidates.  Planted: one point at b rows 5, 6, 1030, 2100 and 2499 (index 5 wins); a 3-4-5 pair against the
    thresholds 5.0 (not counted) and 5.000001 (counted); an outlier at exactly 50 that alone sets hausdorff; pred identical to gt."""
    from rald_amd import postprocess as PP
    pred, gt = lattice_clouds()
    oracle = oracle_batch("lattice", LATTICE_TAUS)
    res = raw_call(pred, PO, gt, GO, max(N_PRED), max(N_GT), LATTICE_TAUS)
    assert_guards(res, PO[-1], GO[-1])
    raw, dp, ip, dg, ig = res
    want_raw = torch.from_numpy(np.stack([o[0] for o in oracle])).cuda()
    assert torch.equal(raw[:-1], want_raw), (raw[:-1] - want_raw).abs().amax(dim=(1, 2))
    for d, (dist, idx, n) in enumerate(((dp, ip, PO[-1]), (dg, ig, GO[-1]))):
        assert torch.equal(dist[:n], _dev(oracle_rows(oracle, d, 0))), d
        assert torch.equal(idx[:n], _dev(oracle_rows(oracle, d, 1))), d
    # the planted cases, on the device's own numbers
    assert float(dp[PO[0]]) == 5.0 and raw[0, 0, 3:5].tolist() == [0.0, 1.0]
    assert int(ip[PO[9]]) == 5 and float(dp[PO[9]]) == 0.0 and int(ig[GO[9]]) == 3 and int(ig[GO[9] + 1]) == 3 and float(dg[GO[9] + 1]) == 1.0
    # explicit chunks of 1024 candidates through the test-facing entry, both directions
    pd, gd, pod, god = _dev(pred), _dev(gt), _dev(PO), _dev(GO)
    # (at these sizes the automatic rule picks 1024 too; 2048 puts rows 5 .. 2047 into one chunk and 2048 .. 2499 into the next,
    # 3072 makes a single chunk of three tiles: the planted duplicates meet inside a chunk, across tiles, and across chunks)
    for chunk in (1024, 2048, 3072):
        d0, i0 = PP.nearest_neighbors_ragged(pd, pod, gd, god, max(N_PRED), max(N_GT), b_chunk=chunk)
        d1, i1 = PP.nearest_neighbors_ragged(gd, god, pd, pod, max(N_GT), max(N_PRED), b_chunk=chunk)
        assert torch.equal(d0, dp[:PO[-1]]) and torch.equal(i0, ip[:PO[-1]]), chunk
        assert torch.equal(d1, dg[:GO[-1]]) and torch.equal(i1, ig[:GO[-1]]), chunk
    # the Python entry: the metrics are the definitions applied to the oracle's raw
    m = PP.cloud_metrics_ragged(pd, pod, gd, god, max(N_PRED), max(N_GT), LATTICE_TAUS)
    host = {k: v.cpu().numpy() for k, v in m.items()}
    for f in range(len(FRAMES)):
        want = derive(oracle[f][0], N_PRED[f], N_GT[f])
        for k, w in want.items():
            assert np.allclose(host[k][f], w, rtol=1e-14, atol=0), (f, k, host[k][f], w)
    assert host["hausdorff"][4] == 50.0 and host["mhd"][4] < 2.0
    assert all(np.isinf(host[k][10]) and np.isinf(host[k][11]) for k in ("accuracy", "completeness", "cd", "cd_l2", "hausdorff", "mhd"))
    assert not host["f_score"][10:].any() and not host["precision"][10:].any() and not host["recall"][10:].any()
    # pred identical to gt: every distance 0, F = 1 at any positive threshold, Hausdorff 0
    same = PP.cloud_metrics(gd[GO[9]:GO[10]], gd[GO[9]:GO[10]], (0.5, 1e-9))
    assert same["hausdorff"] == 0.0 and same["cd"] == 0.0 and same["cd_l2"] == 0.0 and same["f_score"] == [1.0, 1.0]
    dist, idx = PP.nearest_neighbors(gd[GO[9]:GO[10]], gd[GO[9]:GO[10]])
    self_idx = oracle_nn(gt[GO[9]:GO[10]], gt[GO[9]:GO[10]])[1]
    assert self_idx[6] == 5 and self_idx[2499] == 5 and self_idx[2100] == 5 and self_idx[7] == 7
    assert not dist.any() and torch.equal(idx, _dev(self_idx))


# ---- 2. random fp32 clouds -------------------------------------------------------------------------------------------------------------------
@gpu
def test_random_clouds_match_the_float64_oracle():
    """Uniform coordinates in [-10, 10]^3 and one frame near 100 with 1e-3 spacing.  dist within 1e-12 relative (five correctly rounded
    float64 operations and a square root differ by a few 2^-53 at most; the bound is over a thousand times that), idx equal wherever the
    oracle's nearest and next distinct distance differ by more than 1e-12 relative (at most 0.1 % of a frame elsewhere; the seeds give
    none), sums and means within 1e-9 relative, counts exact (no oracle distance within 1e-9 relative of a threshold)."""
    from rald_amd import postprocess as PP
    pred, gt = random_clouds()
    oracle = oracle_batch("random", RANDOM_TAUS)
    res = raw_call(pred, PO, gt, GO, max(N_PRED), max(N_GT), RANDOM_TAUS)
    assert_guards(res, PO[-1], GO[-1])
    raw = res[0][:-1].cpu().numpy()
    for d, n in enumerate((PO[-1], GO[-1])):
        dist, idx = res[1 + 2 * d][:n].cpu().numpy(), res[2 + 2 * d][:n].cpu().numpy()
        want_d, want_i, nxt = (oracle_rows(oracle, d, w) for w in range(3))
        finite = np.isfinite(want_d)
        err = np.abs(dist[finite] - want_d[finite])
        print("direction", d, "largest relative distance error", (err / np.maximum(want_d[finite], 1e-300)).max(), "rows", n)
        assert np.array_equal(dist[~finite], want_d[~finite]) and np.all(err <= 1e-12 * want_d[finite])
        clear = ~finite | apart(want_d, nxt, 1e-12)
        off = (PO, GO)[d]
        for f in range(len(FRAMES)):
            s = slice(off[f], off[f + 1])
            assert np.array_equal(idx[s][clear[s]], want_i[s][clear[s]]), (d, f)
            assert (~clear[s]).sum() <= 0.001 * max(off[f + 1] - off[f], 1), (d, f)
    for f in range(len(FRAMES)):
        want = oracle[f][0]
        assert np.array_equal(raw[f, :, 3:], want[:, 3:]), (f, raw[f, :, 3:], want[:, 3:])
        assert np.all(np.abs(raw[f, :, :2] - want[:, :2]) <= 1e-9 * want[:, :2]), f
        assert np.all(np.abs(raw[f, :, 2] - want[:, 2]) <= 1e-12 * want[:, 2]), f
    m = {k: v.cpu().numpy() for k, v in PP.cloud_metrics_ragged(_dev(pred), _dev(PO), _dev(gt), _dev(GO), max(N_PRED), max(N_GT),
                                                                RANDOM_TAUS).items()}
    for f in range(len(FRAMES)):
        for k, w in derive(oracle[f][0], N_PRED[f], N_GT[f]).items():
            assert np.allclose(m[k][f], w, rtol=1e-9, atol=0), (f, k, m[k][f], w)


# ---- 3. against the existing path ------------------------------------------------------------------------------------------------------------
@gpu
def test_cd_equals_the_existing_chamfer_path():
    """cd of cloud_metrics_ragged against cal_metrics_ragged on the same batch and cal_metrics per frame: 1e-9 relative; inf for the
    empty prediction in both."""
    from rald_amd import postprocess as PP
    pred, gt = random_clouds()
    pd, gd, pod, god = _dev(pred), _dev(gt), _dev(PO), _dev(GO)
    cd = PP.cloud_metrics_ragged(pd, pod, gd, god, max(N_PRED), max(N_GT))["cd"].cpu().tolist()
    old = PP.cal_metrics_ragged(pd, pod, gd, god, max(N_PRED), max(N_GT)).cpu().tolist()
    for f, (n_p, n_g) in enumerate(FRAMES):
        if n_p == 0:
            assert cd[f] == float("inf") and old[f] == float("inf")
        elif n_g == 0:
            assert cd[f] == float("inf")                          # the existing path has no convention for an empty ground truth
        else:
            one = PP.cal_metrics(pd[PO[f]:PO[f + 1]], gd[GO[f]:GO[f + 1]])
            print("frame", f, "cd", cd[f], "cal_metrics_ragged", old[f], "cal_metrics", one)
            assert abs(cd[f] - old[f]) <= 1e-9 * old[f] and abs(cd[f] - one) <= 1e-9 * one, f


# ---- 4. determinism --------------------------------------------------------------------------------------------------------------------------
@gpu
def test_results_are_the_same_bits_in_every_call_batch_and_chunking():
    """Two calls: torch.equal raw, dist and idx.  Every frame alone: the raw bits it has inside the batch.  Chunks of 1024 and 2048
    candidates and the automatic choice: the same dist and idx bits."""
    from rald_amd import postprocess as PP
    pred, gt = random_clouds()
    first = raw_call(pred, PO, gt, GO, max(N_PRED), max(N_GT), RANDOM_TAUS)
    again = raw_call(pred, PO, gt, GO, max(N_PRED), max(N_GT), RANDOM_TAUS)
    assert all(torch.equal(x, y) for x, y in zip(first, again))
    for f, (n_p, n_g) in enumerate(FRAMES):
        alone = raw_call(pred[PO[f]:PO[f + 1]], _offsets([n_p]), gt[GO[f]:GO[f + 1]], _offsets([n_g]), n_p, n_g, RANDOM_TAUS, per_point=False)
        assert torch.equal(alone[0][0], first[0][f]), f
    pd, gd, pod, god = _dev(pred), _dev(gt), _dev(PO), _dev(GO)
    for chunk in (1024, 2048, 0, None):
        d0, i0 = PP.nearest_neighbors_ragged(pd, pod, gd, god, max(N_PRED), max(N_GT), b_chunk=chunk)
        d1, i1 = PP.nearest_neighbors_ragged(gd, god, pd, pod, max(N_GT), max(N_PRED), b_chunk=chunk)
        assert torch.equal(d0, first[1][:PO[-1]]) and torch.equal(i0, first[2][:PO[-1]]), chunk
        assert torch.equal(d1, first[3][:GO[-1]]) and torch.equal(i1, first[4][:GO[-1]]), chunk
    with pytest.raises(RuntimeError):
        PP.nearest_neighbors_ragged(pd, pod, gd, god, max(N_PRED), max(N_GT), b_chunk=1000)      # not a multiple of the tile


# ---- 5. bounds -------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_loose_host_bounds_change_nothing_and_no_row_outside_the_batch_is_written():
    """Host bounds of 10^5 rows for segments of at most 2500: the same bits (another chunk length and idle workgroups only).  Outputs
    300 rows longer than the clouds keep their poison behind offsets[B], and so does the row behind raw."""
    pred, gt = random_clouds()
    tight = raw_call(pred, PO, gt, GO, max(N_PRED), max(N_GT), RANDOM_TAUS)
    loose = raw_call(pred, PO, gt, GO, 100000, 100000, RANDOM_TAUS)
    assert_guards(loose, PO[-1], GO[-1])
    assert all(torch.equal(x, y) for x, y in zip(tight, loose))
    # clouds with rows behind offsets[B] (buffers sized for a worst case): those rows get no output
    B = 9
    part = raw_call(pred, PO[:B + 1], gt, GO[:B + 1], 100000, 100000, RANDOM_TAUS)
    assert_guards(part, PO[B], GO[B])
    assert torch.equal(part[0][:B], tight[0][:B]) and torch.equal(part[1][:PO[B]], tight[1][:PO[B]]) and torch.equal(part[4][:GO[B]], tight[4][:GO[B]])


# ---- 6. the engine ---------------------------------------------------------------------------------------------------------------------------
@gpu
def test_engine_reports_the_metrics_without_changing_anything_else(monkeypatch):
    """infer_point_clouds(..., metric_thresholds=(0.05, 0.1, 0.2)) on the 4-frame setup of test_gpu_infer_batch (3000 grid queries,
    0 / 1 / 500 / 1100 helper points, 2048 refine queries, 1000 surface points): pred and n_queries equal to the call without the
    argument, cd within 1e-9; out['metrics'] equals cloud_metrics per frame; the warm device call makes no host read."""
    from rald_amd import engine_generation as E, postprocess as PP, query_points as QP, synth
    from test_gpu_infer_batch import PC_RANGE, _small_vae, _tail_args
    vae, z9 = _small_vae()
    z = z9[:4].contiguous()
    n, aug, taus = 3000, 2048, (0.05, 0.1, 0.2)
    args = _tail_args(n, aug)
    helpers = [synth.queries(1, max(h, 1), seed=100 + h)[0][:h].cuda() for h in (0, 1, 500, 1100)]
    surfaces = synth.point_cloud(4, 1000, seed=62).cuda()
    draws = QP.draw_tail_randoms(4, n, aug, 10, torch.Generator("cuda").manual_seed(23))
    base = E.infer_point_clouds(vae, z, args, helper_points=helpers, surfaces=surfaces, draws=draws)
    assert "metrics" not in base
    res = E.infer_point_clouds(vae, z, args, helper_points=helpers, surfaces=surfaces, draws=draws, metric_thresholds=taus)
    assert res["n_queries"] == base["n_queries"] and all(torch.equal(a, b) for a, b in zip(res["pred"], base["pred"]))
    assert sum(p.shape[0] > 0 for p in res["pred"]) >= 2
    for b in range(4):
        if base["cd"][b] == float("inf"):
            assert res["cd"][b] == float("inf")
        else:
            assert abs(res["cd"][b] - base["cd"][b]) <= 1e-9 * base["cd"][b], (b, res["cd"][b], base["cd"][b])
        gt = PP.polar2cartesian(PP.inverse_norm_points(surfaces[b], PC_RANGE, True, False))
        want = PP.cloud_metrics(res["pred"][b], gt, taus)
        print("frame", b, res["metrics"][b])
        assert res["metrics"][b] == want and res["metrics"][b]["cd"] == res["cd"][b], (b, res["metrics"][b], want)
        assert len(want["f_score"]) == 3
    none = E.infer_point_clouds(vae, z, args, helper_points=helpers, surfaces=surfaces, draws=draws, metric_thresholds=())
    assert [m["cd"] for m in none["metrics"]] == res["cd"] and none["metrics"][0]["precision"] == []

    def forbidden(*a, **k):
        raise AssertionError("host read inside infer_point_clouds_device")
    real = {name: getattr(torch.Tensor, name) for name in ("__bool__", "__int__", "__float__")}

    def guard(name):
        def f(self, *a, **k):
            if self.is_cuda:
                forbidden()
            return real[name](self, *a, **k)
        return f
    with monkeypatch.context() as m:
        for name in ("item", "cpu", "tolist", "numpy"):
            m.setattr(torch.Tensor, name, forbidden)
        for name in real:
            m.setattr(torch.Tensor, name, guard(name))
        m.setattr(torch.cuda, "synchronize", forbidden)
        pts, off, cd, metrics = E.infer_point_clouds_device(vae, z, args, helper_points=helpers, surfaces=surfaces, draws=draws,
                                                            metric_thresholds=taus)
    off = off.cpu().tolist()
    assert all(torch.equal(pts[off[b]:off[b + 1]], res["pred"][b]) for b in range(4))
    assert cd.cpu().tolist() == res["cd"] and metrics["f_score"].shape == (4, 3)
    assert metrics["hausdorff"].cpu().tolist() == [m["hausdorff"] for m in res["metrics"]]
    assert len(E.infer_point_clouds_device(vae, z, args, helper_points=helpers, surfaces=surfaces, draws=draws)) == 3
