"""The definition of the RANSAC plane segmentation and the plane filter of ragged clouds (include/rald_hip.h) by
brute force in numpy, for the tests to compare with by equality: fp32 one numpy operation at a time (so every operation is rounded
once and nothing is contracted), float64 where the definition says so.  Philox is tests/churn_ref.py's, the Jacobi sweeps are
tests/normals_ref.py's; the fixed sum shape is restated here from the header.

segment_one is the reference: a loop over the hypotheses, index lists for the live rows.  segment_one_alt is an independent route
for tests/test_plane_host.py: Philox in Python integers, the scores of all hypotheses at once from a dense [m, H] array, the rounds
peeled with boolean masks, the sums by knn_ref.fixed_sum."""
import numpy as np

import churn_ref
import knn_ref
import normals_ref as N

F32 = np.float32
F64 = np.float64
SEG = 1024
TAG = 2                                                   # the key's second word: 0 and 1 are the sampler's
M32 = 0xFFFFFFFF


def fixed_sum(values):
    """float64 [m] -> their sum in the header's shape: blocks of 1024 in order, padded with +0.0; in a block v[i] += v[i + h] for h = 512,
    256 .. 1; the blocks' sums added left to right from +0.0."""
    values = np.asarray(values, F64)
    total = F64(0.0)
    for s in range(0, len(values), SEG):
        v = np.zeros(SEG, F64)
        v[:len(values[s:s + SEG])] = values[s:s + SEG]
        h = SEG // 2
        while h >= 1:
            v[:h] = v[:h] + v[h:2 * h]
            h //= 2
        total = total + v[0]
    return total


def hypotheses(L, j, H, seed, t):
    """Live rows f32 [m,3] (m >= 3), the round, H, the seed, the threshold -> dict(idx int64 [H,3], n f32 [H,3], p0 f32 [H,3], len2,
    bound f32 [H], valid bool [H])."""
    m = len(L)
    counter = np.zeros((H, 4), np.uint64)
    counter[:, 0] = np.arange(H, dtype=np.uint64)
    counter[:, 1] = j
    w = churn_ref.philox4x32_10(counter, np.array([[int(seed) % (1 << 32), TAG]], np.uint64))
    idx = ((w[:, :3].astype(np.uint64) * np.uint64(m)) >> np.uint64(32)).astype(np.int64)
    p0, p1, p2 = L[idx[:, 0]], L[idx[:, 1]], L[idx[:, 2]]
    with np.errstate(all="ignore"):
        e1, e2 = p1 - p0, p2 - p0
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        len2 = (nx * nx + ny * ny) + nz * nz
        bound = (F32(t) * F32(t)) * len2
        distinct = (idx[:, 0] != idx[:, 1]) & (idx[:, 0] != idx[:, 2]) & (idx[:, 1] != idx[:, 2])
        valid = distinct & np.isfinite(len2) & (len2 > 0)
    n = np.stack([nx, ny, nz], 1)
    assert n.dtype == F32 and bound.dtype == F32
    return dict(idx=idx, n=n, p0=p0, len2=len2, bound=bound, valid=valid)


def inliers_of(L, hyp, h, strict=False):
    """The fp32 inlier test of hypothesis h over the live rows -> bool [m].  strict: `<` in place of `<=` (the host test's mutation)."""
    with np.errstate(all="ignore"):
        d = L - hyp["p0"][h]
        n = hyp["n"][h]
        s = (n[0] * d[:, 0] + n[1] * d[:, 1]) + n[2] * d[:, 2]
        ss = s * s
        assert ss.dtype == F32
        return ss < hyp["bound"][h] if strict else ss <= hyp["bound"][h]


def scores_of(L, hyp, strict=False):
    """int64 [H]: the inliers of every hypothesis, -1 for an invalid one."""
    return np.array([int(inliers_of(L, hyp, h, strict).sum()) if hyp["valid"][h] else -1 for h in range(len(hyp["valid"]))], np.int64)


def orient(x, c0, view):
    """Unit normal float64 [3], a point of the plane, the view -> the plane (a, b, c, d) after the sign rule."""
    s = (x[0] * (view[0] - c0[0]) + x[1] * (view[1] - c0[1])) + x[2] * (view[2] - c0[2])
    first = x[0] if x[0] != 0.0 else (x[1] if x[1] != 0.0 else x[2])
    if s < 0.0 or (s == 0.0 and first < 0.0):
        x = -x
    return np.array([x[0], x[1], x[2], -((x[0] * c0[0] + x[1] * c0[1]) + x[2] * c0[2])], F64)


def _unit(v):
    return v / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def refined_plane(L, inl, view, sum_of=fixed_sum):
    """The float64 plane of the inliers `inl` of the live rows L: centroid and central moments in the fixed sum shape, the sweeps."""
    L64 = L.astype(F64)
    cnt = F64(int(inl.sum()))
    with np.errstate(all="ignore"):
        c = np.array([sum_of(np.where(inl, L64[:, k], 0.0)) / cnt for k in range(3)], F64)
        d = L64 - c
        terms = (d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 1], d[:, 1] * d[:, 2], d[:, 2] * d[:, 2])
        mom = np.array([[sum_of(np.where(inl, e, 0.0)) / cnt for e in terms]], F64)
        _, V, _ = N.jacobi(mom)
        plane = orient(_unit(V[0, :, 0].copy()), c, view)
        dist = (plane[0] * (L64[:, 0] - c[0]) + plane[1] * (L64[:, 1] - c[1])) + plane[2] * (L64[:, 2] - c[2])
    return plane, dist


def _view64(view):
    return np.zeros(3, F64) if view is None else np.asarray(view, F32).astype(F64)


def _empty(n, K):
    return dict(planes=np.full((K, 4), np.nan, F64), inliers=np.zeros(K, np.int32), best=np.full(K, -1, np.int32), num_planes=0,
                top=[], ties=[])


def segment_one(points, t, H, K=1, min_inliers=3, refine=True, seed=0, view=None, strict=False, tie="smallest", min_cmp="below"):
    """One cloud -> dict(labels int32 [n], planes float64 [K,4], num_planes, inliers int32 [K], best int32 [K]; top / ties: per round the
    best score and the hypotheses that reach it).  strict, tie="largest", min_cmp="not_above": the mutations the host test shows the
    constructions catch."""
    p = np.asarray(points, F32).reshape(-1, 3)
    usable = np.isfinite(p).all(axis=1)
    labels = np.where(usable, -1, -2).astype(np.int32)
    out = _empty(len(p), K)
    view = _view64(view)
    enough = (lambda c: c >= min_inliers) if min_cmp == "below" else (lambda c: c > min_inliers)
    for j in range(K):
        live = np.nonzero(labels == -1)[0]
        if len(live) < 3:
            break
        L = p[live]
        hyp = hypotheses(L, j, H, seed, t)
        score = scores_of(L, hyp, strict)
        if not hyp["valid"].any():
            break
        top = int(score.max())
        tied = np.nonzero(score == top)[0]
        h = int(tied[0] if tie == "smallest" else tied[-1])
        if not enough(top):
            break
        inl = inliers_of(L, hyp, h, strict)
        if refine:
            plane, dist = refined_plane(L, inl, view)
            inl = np.abs(dist) <= F64(F32(t))
            count = int(inl.sum())
            if not enough(count):
                break
        else:
            plane, count = orient(_unit(hyp["n"][h].astype(F64)), hyp["p0"][h].astype(F64), view), top
        out["planes"][j], out["inliers"][j], out["best"][j], out["num_planes"] = plane, count, h, j + 1
        out["top"].append(top)
        out["ties"].append(tied)
        labels[live[inl]] = j
    out["labels"] = labels
    return out


# ---- the independent route ----------------------------------------------------------------------------------------------------------------
def philox_int(counter, key):
    """Philox4x32-10 in Python integers: 4 counter words, 2 key words -> 4 words."""
    c, (k0, k1) = list(counter), key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & M32, (p0 >> 32) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c


def segment_one_alt(points, t, H, K=1, min_inliers=3, refine=True, seed=0, view=None):
    """segment_one by another route -> dict(labels, planes, num_planes, inliers, best)."""
    p = np.asarray(points, F32).reshape(-1, 3)
    lab = np.where(np.isfinite(p[:, 0]) & np.isfinite(p[:, 1]) & np.isfinite(p[:, 2]), -1, -2).astype(np.int32)
    out = _empty(len(p), K)
    view = _view64(view)
    t2 = F32(t) * F32(t)
    for j in range(K):
        mask = lab == -1
        m = int(mask.sum())
        if m < 3:
            break
        L = p[mask]
        idx = np.array([[(w * m) >> 32 for w in philox_int((h, j, 0, 0), (int(seed) & M32, TAG))[:3]] for h in range(H)], np.int64)
        with np.errstate(all="ignore"):
            a, e1, e2 = L[idx[:, 0]], L[idx[:, 1]] - L[idx[:, 0]], L[idx[:, 2]] - L[idx[:, 0]]
            n = np.stack([e1[:, (k + 1) % 3] * e2[:, (k + 2) % 3] - e1[:, (k + 2) % 3] * e2[:, (k + 1) % 3] for k in range(3)], 1)
            sq = n * n
            len2 = (sq[:, 0] + sq[:, 1]) + sq[:, 2]
            ok = np.array([len(set(r)) == 3 for r in idx.tolist()]) & np.isfinite(len2) & (len2 > 0)
            d = L[:, None, :] - a[None, :, :]                                            # [m, H, 3]
            s = (d[:, :, 0] * n[None, :, 0] + d[:, :, 1] * n[None, :, 1]) + d[:, :, 2] * n[None, :, 2]
            inl_all = (s * s <= (t2 * len2)[None, :]) & ok[None, :]                      # [m, H]
        assert s.dtype == F32
        score = np.where(ok, inl_all.sum(axis=0), -1)
        if not ok.any():
            break
        h = min(range(H), key=lambda q: (-int(score[q]), q))
        if score[h] < min_inliers:
            break
        inl = inl_all[:, h]
        if refine:
            plane, dist = refined_plane(L, inl, view, sum_of=knn_ref.fixed_sum)
            inl = ~(np.abs(dist) > F64(F32(t))) & ~np.isnan(dist)
            if inl.sum() < min_inliers:
                break
        else:
            n64 = n[h].astype(F64)
            plane = orient(n64 / np.sqrt((n64[0] ** 2 + n64[1] ** 2) + n64[2] ** 2), a[h].astype(F64), view)
        out["planes"][j], out["inliers"][j], out["best"][j], out["num_planes"] = plane, int(inl.sum()), h, j + 1
        sub = lab[mask]
        sub[inl] = j
        lab[mask] = sub
    out["labels"] = lab
    return out


# ---- ragged batches ------------------------------------------------------------------------------------------------------------------------
def _span(off, b, counts, max_per_sample):
    n = off[b + 1] - off[b]
    if counts is not None:
        n = min(n, max(int(counts[b]), 0))
    return max(min(n, int(max_per_sample)), 0)


def segment_ragged(points, offsets, t, H, max_per_sample, counts=None, **kw):
    """The ragged call -> dict(labels int32 [T], untouched bool [T], planes float64 [B,K,4], num_planes int32 [B], inliers, best int32
    [B,K])."""
    p = np.asarray(points, F32).reshape(-1, 3)
    off = [int(o) for o in offsets]
    B, K = len(off) - 1, kw.get("K", 1)
    out = dict(labels=np.zeros(len(p), np.int32), untouched=np.ones(len(p), bool), planes=np.zeros((B, K, 4), F64),
               num_planes=np.zeros(B, np.int32), inliers=np.zeros((B, K), np.int32), best=np.zeros((B, K), np.int32))
    for b in range(B):
        n = _span(off, b, counts, max_per_sample)
        one = segment_one(p[off[b]:off[b] + n], t, H, **kw)
        out["labels"][off[b]:off[b] + n] = one["labels"]
        out["untouched"][off[b]:off[b] + n] = False
        for k in ("planes", "num_planes", "inliers", "best"):
            out[k][b] = one[k]
    return out


def filter_ragged(points, offsets, t, H, max_per_sample, counts=None, keep_planes=False, labelled=None, **kw):
    """The ragged filter -> dict(points f32 [M,3], offsets i64 [B+1], index i64 [M], labels i32 [M] per kept row, planes, num_planes)."""
    p = np.asarray(points, F32).reshape(-1, 3)
    off = [int(o) for o in offsets]
    r = segment_ragged(p, off, t, H, max_per_sample, counts, **kw) if labelled is None else labelled
    pts, idx, labs, out_off = [], [], [], [0]
    for b in range(len(off) - 1):
        n = _span(off, b, counts, max_per_sample)
        lab = r["labels"][off[b]:off[b] + n]
        keep = np.nonzero(lab >= 0 if keep_planes else lab == -1)[0]
        pts.append(p[off[b] + keep])
        idx.append(keep.astype(np.int64))
        labs.append(lab[keep])
        out_off.append(out_off[-1] + len(keep))
    cat = lambda parts, empty: np.concatenate(parts) if parts else empty
    return dict(points=cat(pts, np.zeros((0, 3), F32)), offsets=np.array(out_off, np.int64), index=cat(idx, np.zeros(0, np.int64)),
                labels=cat(labs, np.zeros(0, np.int32)).astype(np.int32), planes=r["planes"], num_planes=r["num_planes"])


# ---- the constructions: each -> (points f32 [n,3], dict of the call's arguments) -----------------------------------------------------------------
T_SLAB = 0.0625                                           # 2^-4; T_SLAB * (1 + 2^-22) is a float32


def tiny_clouds():
    """Clouds of 0, 1, 2 and 3 rows, 3 collinear rows, and 3 rows of which two are equal -> (points, offsets)."""
    clouds = [np.zeros((0, 3)), [[1, 2, 3]], [[0, 0, 0], [1, 0, 0]], [[0, 0, 0], [1, 0, 0], [0, 1, 0.5]], [[0, 0, 0], [1, 1, 1], [2, 2, 2]],
              [[0, 0, 0], [1, 0, 0], [1, 0, 0]]]
    parts = [np.asarray(c, F32).reshape(-1, 3) for c in clouds]
    return np.concatenate(parts), [0] + np.cumsum([len(c) for c in parts]).tolist()


TINY = dict(t=0.01, H=64, K=2, min_inliers=3, refine=False)


def slab_cloud(n, seed=41):
    """Rows on the lattice (0 .. 31)^2 * 2^-3 in z = 0 (64 %), at z = +-t (12 % each) and at z = +-t (1 + 2^-22) (6 % each), in random
    order: with three z = 0 rows n = (0, 0, nz), nz * 64 a whole number below 2^11, so s, s * s and the bound are exact; the rows at
    +-t meet the bound exactly and are inliers, the others miss it by one part in 2^21."""
    rs = np.random.RandomState(seed + n)
    xy = rs.randint(0, 32, size=(n, 2)).astype(F32) * F32(0.125)
    far = F32(T_SLAB) * (F32(1) + F32(2.0 ** -22))
    z = rs.choice(np.array([0, T_SLAB, -T_SLAB, far, -far], F32), size=n, p=[0.64, 0.12, 0.12, 0.06, 0.06]).astype(F32)
    return np.concatenate([xy, z[:, None]], 1).astype(F32), F32(far)


SLAB_SIZES = (257, 1025, 2049)
SLAB = dict(t=T_SLAB, H=64, K=1, min_inliers=3, refine=False)


def tie_cloud(n=300, seed=42):
    """Two parallel lattice planes z = 0 and z = 4 with the same n sites each, interleaved row by row: every hypothesis inside one
    plane scores exactly n."""
    rs = np.random.RandomState(seed)
    xy = rs.randint(0, 32, size=(n, 2)).astype(F32) * F32(0.125)
    p = np.zeros((2 * n, 3), F32)
    p[0::2, :2] = xy
    p[1::2, :2] = xy
    p[1::2, 2] = 4.0
    return p


TIE = dict(t=T_SLAB, H=64, K=1, min_inliers=3, refine=False)


def faces_cloud(order="built", seed=43):
    """Three mutually orthogonal lattice faces of 24^2, 20^2 and 16^2 sites (step 2^-3, one step clear of the edges they would share)
    and 100 scattered rows in [0.5, 3.5]^3 -> (points, face of every row: 0, 1, 2 by size, -1 for the scatter)."""
    def face(side, axis):
        g = (np.stack(np.meshgrid(np.arange(1, side + 1), np.arange(1, side + 1), indexing="ij"), -1).reshape(-1, 2) * 0.125)
        return np.insert(g, axis, 0.0, axis=1)
    rs = np.random.RandomState(seed)
    p = np.concatenate([face(24, 2), face(20, 1), face(16, 0), rs.uniform(0.5, 3.5, size=(100, 3))]).astype(F32)
    truth = np.concatenate([np.full(576, 0), np.full(400, 1), np.full(256, 2), np.full(100, -1)])
    perm = dict(built=np.arange(len(p)), reversed=np.arange(len(p))[::-1], shuffled=rs.permutation(len(p)))[order]
    return p[perm], truth[perm]


FACES = dict(t=0.03125, H=256, K=4, min_inliers=256, refine=True)      # the smallest face's size exactly: `>` would lose it


def noisy_cloud(seed=44):
    """normals_ref.noisy_plane (1500 rows, sigma 0.01) plus 40 % uniform outliers around it and 12 NaN / inf rows, shuffled ->
    (points, the plane's true unit normal, a point on it)."""
    plane = N.noisy_plane()
    rs0 = np.random.RandomState(32)                       # noisy_plane's own draws, for its rotation
    rs0.uniform(0, 4, size=(1500, 2))
    rs0.normal(scale=0.01, size=(1500, 1))
    rot = np.linalg.qr(rs0.normal(size=(3, 3)))[0]
    rs = np.random.RandomState(seed)
    centre = plane.astype(F64).mean(axis=0)
    out = (centre + rs.uniform(-3.0, 3.0, size=(1000, 3))).astype(F32)
    bad = (centre + rs.uniform(-1.0, 1.0, size=(12, 3))).astype(F32)
    bad[np.arange(0, 4), rs.randint(0, 3, 4)] = np.nan
    bad[np.arange(4, 8), rs.randint(0, 3, 4)] = np.inf
    bad[np.arange(8, 12), rs.randint(0, 3, 4)] = -np.inf
    p = np.concatenate([plane, out, bad])
    return p[rs.permutation(len(p))], rot[:, 2], centre


NOISY = dict(t=0.03, H=256, K=1, min_inliers=500)
