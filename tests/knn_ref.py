"""The definition of the k nearest other rows and of the statistical outlier filter (include/rald_hip.h) by brute
force in numpy, for the tests to compare with by equality: d2 as tests/radius_ref.py computes it (one float32 operation at a time), the
means and the statistics one float64 operation at a time, the sums in the fixed shape written out.  Beside it an independent grid walk
with the header's termination rule (the host tests hold the two against each other) and the clouds both test files use."""
import numpy as np

import radius_ref as R

F32 = np.float32
F64 = np.float64
INF = F32(np.inf)
SEG = 1024


# ---- the definition by brute force ---------------------------------------------------------------------------------------------------------
def knn_one(points, grid, k, max_radius=None):
    """One cloud [n,3] -> dict(idx i64 [n,k], dist2 f32 [n,k], found i32 [n], inside bool [n])."""
    lo3, v3, dims3 = grid
    p = np.asarray(points, F32).reshape(-1, 3)
    n = len(p)
    inside = R.inside_of(p, lo3, dims3, v3)
    r2max = None if max_radius is None else F32(F32(max_radius) * F32(max_radius))
    idx = np.full((n, k), -1, np.int64)
    dist2 = np.full((n, k), INF, F32)
    found = np.full(n, -1, np.int32)
    cols = np.arange(n)
    for s in range(0, n, 256):
        rows = np.arange(s, min(s + 256, n))
        d2 = R.d2_rows(p, rows)
        with np.errstate(invalid="ignore"):
            cand = inside[None, :] & (cols[None, :] != rows[:, None])
            if r2max is not None:
                cand &= d2 <= r2max
        assert not np.isinf(d2[cand & inside[rows, None]]).any()            # the reference orders candidates behind a +inf sentinel
        order = np.argsort(np.where(cand, d2, INF), axis=1, kind="stable")[:, :k]     # (d2, j) ascending: stable over the row index
        f = np.minimum(cand.sum(axis=1), k)
        have = np.arange(order.shape[1])[None, :] < f[:, None]
        idx[rows, :order.shape[1]] = np.where(have, order, -1)
        dist2[rows, :order.shape[1]] = np.where(have, np.take_along_axis(d2, order, axis=1), INF)
        found[rows] = f
    idx[~inside], dist2[~inside], found[~inside] = -1, INF, -1
    return dict(idx=idx, dist2=dist2, found=found, inside=inside)


def fixed_sum(values):
    """The cloud sum in its fixed shape: float64 [n] (a row that does not count is +0.0 already) -> float64."""
    v = np.zeros(-(-max(len(values), 1) // SEG) * SEG, F64)
    v[:len(values)] = values
    v = v.reshape(-1, SEG)
    h = SEG // 2
    while h >= 1:
        v[:, :h] = v[:, :h] + v[:, h:2 * h]
        h //= 2
    s = F64(0.0)
    for g in range(len(v)):
        s = s + v[g, 0]
    return s


def mean_of(dist2, found):
    """m per row from the k-NN tables: the slots added in order in float64, divided by found; +inf for found = 0, NaN outside."""
    acc = np.zeros(len(found), F64)
    for s in range(dist2.shape[1]):
        acc = acc + np.where(s < found, np.sqrt(dist2[:, s].astype(F64)), 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = acc / np.maximum(found, 1).astype(F64)
    return np.where(found < 0, np.nan, np.where(found == 0, np.inf, m))


def statistics_of(m, found, std_ratio):
    """(mu, sigma, thr, n_f) of one cloud from its means."""
    inF = found >= 1
    nf = int(inF.sum())
    if nf == 0:
        return F64(np.nan), F64(np.nan), F64(np.nan), 0
    mu = fixed_sum(np.where(inF, m, 0.0)) / F64(nf)
    dev = np.where(inF, m, mu) - mu
    sigma = np.sqrt(fixed_sum(np.where(inF, dev * dev, 0.0)) / F64(nf - 1)) if nf >= 2 else F64(0.0)
    thr = mu + F64(std_ratio) * sigma
    return mu, sigma, thr, nf


def statistical_one(points, grid, k, std_ratio, max_radius=None, knn=None):
    """One cloud -> dict(mean f64 [n], stats f64 [3], keep bool [n], found)."""
    t = knn_one(points, grid, k, max_radius) if knn is None else knn
    m = mean_of(t["dist2"], t["found"])
    mu, sigma, thr, nf = statistics_of(m, t["found"], std_ratio)
    with np.errstate(invalid="ignore"):
        keep = (t["found"] >= 1) & (m <= thr)
    return dict(mean=m, stats=np.array([mu, sigma, thr], F64), keep=keep, found=t["found"], n_f=nf)


def knn_ragged(points, offsets, grid, k, max_per_sample, counts=None, max_radius=None):
    """The ragged search -> dict(idx [T,k], dist2 [T,k], found [T], untouched bool [T]: rows the call must not write)."""
    p = np.asarray(points, F32).reshape(-1, 3)
    off = [int(o) for o in offsets]
    T = len(p)
    out = dict(idx=np.zeros((T, k), np.int64), dist2=np.zeros((T, k), F32), found=np.zeros(T, np.int32), untouched=np.ones(T, bool))
    for b in range(len(off) - 1):
        n = R._span(off, b, counts, max_per_sample)
        one = knn_one(p[off[b]:off[b] + n], grid, k, max_radius)
        for key in ("idx", "dist2", "found"):
            out[key][off[b]:off[b] + n] = one[key]
        out["untouched"][off[b]:off[b] + n] = False
    return out


def statistical_ragged(points, offsets, grid, k, std_ratio, max_per_sample, counts=None, max_radius=None, knn=None):
    """The ragged filter -> dict(points f32 [M,3], offsets i64 [B+1], index i64 [M], mean f64 [T], stats f64 [B,3], untouched bool [T]).
    knn: knn_ragged's result for the same arguments, where the caller has it already."""
    p = np.asarray(points, F32).reshape(-1, 3)
    off = [int(o) for o in offsets]
    t = knn_ragged(p, off, grid, k, max_per_sample, counts, max_radius) if knn is None else knn
    B = len(off) - 1
    pts, idx, out_off, mean, stats = [], [], [0], np.zeros(len(p), F64), np.zeros((B, 3), F64)
    for b in range(B):
        n = R._span(off, b, counts, max_per_sample)
        sl = slice(off[b], off[b] + n)
        one = statistical_one(p[sl], grid, k, std_ratio, max_radius, knn=dict(dist2=t["dist2"][sl], found=t["found"][sl]))
        keep = np.nonzero(one["keep"])[0]
        pts.append(p[off[b] + keep])
        idx.append(keep.astype(np.int64))
        out_off.append(out_off[-1] + len(keep))
        mean[sl], stats[b] = one["mean"], one["stats"]
    return dict(points=np.concatenate(pts) if pts else np.zeros((0, 3), F32), offsets=np.array(out_off, np.int64),
                index=np.concatenate(idx) if idx else np.zeros(0, np.int64), mean=mean, stats=stats, untouched=t["untouched"])


# ---- an independent route: the cells of the grid, a box that doubles, and the header's termination rule ---------------------------------
def radius_for(w):
    """A float32 r with fl(r * r) >= w."""
    w = F32(w)
    r = F32(np.sqrt(w))
    while F32(r * r) < w:
        r = np.nextafter(r, INF)
    return r


def grid_walk_knn(points, grid, k, max_radius=None):
    """knn_one's outputs by a walk over a box of cells that doubles until it holds the scan range of the bound on the wanted
    candidates -> (dict, the widest box in cells over rows and axes)."""
    lo3, v3, dims3 = grid
    p = np.asarray(points, F32).reshape(-1, 3)
    n = len(p)
    inside = R.inside_of(p, lo3, dims3, v3)
    r2max = None if max_radius is None else F32(F32(max_radius) * F32(max_radius))
    with np.errstate(invalid="ignore"):
        cell = np.stack([R.cell_f(p[:, a], lo3[a], v3[a]) for a in range(3)], axis=1)
    cell = np.where(inside[:, None], cell, -1).astype(np.int64)
    dims = np.array([int(d) for d in dims3], np.int64)
    idx = np.full((n, k), -1, np.int64)
    dist2 = np.full((n, k), INF, F32)
    found = np.full(n, -1, np.int32)
    widest = 0
    for i in np.nonzero(inside)[0]:
        half = 1
        while True:
            c0, c1 = np.maximum(cell[i] - half, 0), np.minimum(cell[i] + half, dims - 1)
            cand = np.nonzero(inside & (cell >= c0).all(axis=1) & (cell <= c1).all(axis=1))[0]
            cand = cand[cand != i]
            d2 = R.d2_rows(p[np.concatenate([[i], cand])], np.array([0]))[0, 1:]
            if r2max is not None:
                cand, d2 = cand[d2 <= r2max], d2[d2 <= r2max]
            order = np.lexsort((cand, d2))[:k]
            cand, d2 = cand[order], d2[order]
            w = d2[-1] if len(cand) == k else r2max
            if (c0 == 0).all() and (c1 == dims - 1).all():
                break
            if w is not None:
                r = radius_for(w)
                rng = [R.scan_range(p[i, a], lo3[a], v3[a], int(dims[a]), r) for a in range(3)]
                if all(rng[a][0] >= c0[a] and rng[a][1] <= c1[a] for a in range(3)):
                    break
            half *= 2
        widest = max(widest, int((c1 - c0).max()) + 1)
        idx[i, :len(cand)], dist2[i, :len(cand)], found[i] = cand, d2, len(cand)
    return dict(idx=idx, dist2=dist2, found=found, inside=inside), widest


# ---- the clouds of the tests: each -> (points f32 [n,3], grid) -------------------------------------------------------------------------------
def uniform(seed=21, n=1200):
    return np.random.RandomState(seed).uniform(0, 1, size=(n, 3)).astype(F32), R.cube_grid(0.0, 1.0, 0.2)


def lattice(seed=22, n=1200):
    """The integer lattice with duplicates: many equal distances, ties go by row index."""
    p = np.random.RandomState(seed).randint(0, 7, size=(n, 3)).astype(F32)
    return p, R.cube_grid(0.0, 7.0, 1.0)


def lattice_ulp(seed=23, n=1200):
    p, grid, _ = R.lattice_ulp_cloud(seed, n)
    return p, grid


def one_cell(seed=24, n=600):
    return np.random.RandomState(seed).uniform(0.1, 0.9, size=(n, 3)).astype(F32), R.cube_grid(0.0, 0.5, 1.0)


def all_equal(n=300):
    return np.tile(np.array([[0.3, 0.6, 0.9]], F32), (n, 1)), R.cube_grid(0.0, 1.0, 0.25)


def far_row(seed=25, n=700):
    """A dense blob and one row far from it: that row's box must grow to the grid."""
    p = np.random.RandomState(seed).uniform(0.0, 0.4, size=(n, 3)).astype(F32)
    p[n // 2] = (60.3, 61.7, 59.1)
    return p, R.cube_grid(0.0, 64.0, 0.1)


def corner_blob(seed=26, n=700):
    """A blob in one corner of a grid 1290 cells wide on every axis, and three rows scattered over the rest."""
    p = np.random.RandomState(seed).uniform(0.0, 3.0, size=(n, 3)).astype(F32)
    p[[5, 300, 699]] = [[1289.5, 0.5, 644.0], [10.0, 1289.9, 1289.9], [644.2, 644.2, 0.1]]
    return p, ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (1290, 1290, 1290))


def faces(seed=27, n=1200):
    p, grid, _ = R.faces_cloud(seed, n)
    return p, grid


CONSTRUCTIONS = dict(uniform=uniform, lattice=lattice, lattice_ulp=lattice_ulp, one_cell=one_cell, all_equal=all_equal, far_row=far_row,
                     corner_blob=corner_blob, faces=faces)
