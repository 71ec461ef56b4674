"""The definition of the PCA normals, the surface variation and the covariance eigenvalues of ragged clouds, and of the normal
consistency (include/rald_hip.h) by brute force in numpy, for the tests to compare with by equality: the
neighbours are tests/knn_ref.py's, and everything behind them is one numpy float64 operation at a time in the header's order - the
sums from +0.0, the Jacobi rotations formula for formula, the three exchanges, the sign - so nothing is contracted and every
operation is rounded once.  The fixed sum shape is knn_ref.fixed_sum."""
import numpy as np

import knn_ref as K
import radius_ref as R

F32 = np.float32
F64 = np.float64
SWEEPS = 6
PAIRS = ((0, 1, 2), (0, 2, 1), (1, 2, 0))                 # (p, q, the third axis r)


def moments_of(p, idx, found):
    """Rows [n,3] f32, their neighbour table and found -> (float64 [n,6] xx xy xz yy yz zz, defined bool [n]); undefined rows hold 0."""
    n, k = idx.shape
    defined = found >= 2
    p64 = p.astype(F64)
    with np.errstate(invalid="ignore", over="ignore"):
        nb = p64[np.clip(idx, 0, max(n - 1, 0))] if n else np.zeros((0, k, 3), F64)       # [n,k,3]
        use = (np.arange(k)[None, :] < found[:, None]) & defined[:, None]
        m = np.where(defined, found + 1, 1).astype(F64)
        s = np.zeros((n, 3), F64)
        s = s + np.where(defined[:, None], p64, 0.0)
        for t in range(k):
            s = np.where(use[:, t, None], s + nb[:, t], s)
        c = s / m[:, None]
        acc = np.zeros((n, 6), F64)

        def add(acc, q, on):
            d = q - c
            terms = np.stack([d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 1], d[:, 1] * d[:, 2], d[:, 2] * d[:, 2]], 1)
            return np.where(on[:, None], acc + terms, acc)
        acc = add(acc, p64, defined)
        for t in range(k):
            acc = add(acc, nb[:, t], use[:, t])
        mom = acc / m[:, None]
    return np.where(defined[:, None], mom, 0.0), defined


def jacobi(mom, sweeps=SWEEPS):
    """Moments float64 [n,6] -> (eigenvalues float64 [n,3] ascending, V float64 [n,3,3] with the vectors as columns in that order)."""
    n = len(mom)
    A = np.zeros((n, 3, 3), F64)
    A[:, 0, 0], A[:, 0, 1], A[:, 0, 2], A[:, 1, 1], A[:, 1, 2], A[:, 2, 2] = (mom[:, e] for e in range(6))
    V = np.zeros((n, 3, 3), F64)
    V[:, 0, 0] = V[:, 1, 1] = V[:, 2, 2] = 1.0
    get = lambda M, a, b: M[:, min(a, b), max(a, b)].copy()                            # the upper triangle holds the symmetric matrix

    def put(M, a, b, v, on):
        M[:, min(a, b), max(a, b)] = np.where(on, v, get(M, a, b))
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p, q, r in PAIRS:
                apq, app, aqq, arp, arq = get(A, p, q), get(A, p, p), get(A, q, q), get(A, r, p), get(A, r, q)
                on = apq != 0.0
                theta = (aqq - app) / (2.0 * apq)
                den = np.abs(theta) + np.sqrt(theta * theta + 1.0)
                t = np.where(theta < 0.0, -1.0, 1.0) / den
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                h = t * apq
                put(A, p, p, app - h, on)
                put(A, q, q, aqq + h, on)
                put(A, p, q, np.zeros(n, F64), on)
                put(A, r, p, c * arp - s * arq, on)
                put(A, r, q, s * arp + c * arq, on)
                for u in range(3):
                    vp, vq = V[:, u, p].copy(), V[:, u, q].copy()
                    V[:, u, p] = np.where(on, c * vp - s * vq, vp)
                    V[:, u, q] = np.where(on, s * vp + c * vq, vq)
    lam = np.stack([A[:, 0, 0], A[:, 1, 1], A[:, 2, 2]], 1)
    for a, b in ((0, 1), (1, 2), (0, 1)):                                              # exchange iff the first is GREATER
        with np.errstate(invalid="ignore"):
            sw = lam[:, a] > lam[:, b]
        la, lb = lam[:, a].copy(), lam[:, b].copy()
        lam[:, a], lam[:, b] = np.where(sw, lb, la), np.where(sw, la, lb)
        va, vb = V[:, :, a].copy(), V[:, :, b].copy()
        V[:, :, a], V[:, :, b] = np.where(sw[:, None], vb, va), np.where(sw[:, None], va, vb)
    return lam, V, np.stack([A[:, 0, 1], A[:, 0, 2], A[:, 1, 2]], 1)


def normals_from(p, idx, found, view=None, sweeps=SWEEPS):
    """One cloud's rows and its neighbour table -> dict(normals f32 [n,3], curvature f32 [n], eigenvalues f32 [n,3], found,
    lam / vec float64: the eigenvalues and the oriented normal before rounding, off: the off-diagonals left)."""
    p = np.asarray(p, F32).reshape(-1, 3)
    mom, defined = moments_of(p, idx, found)
    lam, V, off = jacobi(mom, sweeps)
    with np.errstate(all="ignore"):
        total = (lam[:, 0] + lam[:, 1]) + lam[:, 2]
        curv = np.where(total == 0.0, 0.0, lam[:, 0] / np.where(total == 0.0, 1.0, total))
        x, y, z = V[:, 0, 0], V[:, 1, 0], V[:, 2, 0]
        length = np.sqrt((x * x + y * y) + z * z)
        x, y, z = x / length, y / length, z / length
        s = np.zeros(len(p), F64)
        if view is not None:
            v = np.asarray(view, F32).astype(F64)
            q = p.astype(F64)
            s = (x * (v[0] - q[:, 0]) + y * (v[1] - q[:, 1])) + z * (v[2] - q[:, 2])
        big = x.copy()
        big = np.where(np.abs(y) > np.abs(big), y, big)
        big = np.where(np.abs(z) > np.abs(big), z, big)
        flip = np.where(s == 0.0, big < 0.0, s < 0.0)
        vec = np.where(flip[:, None], -np.stack([x, y, z], 1), np.stack([x, y, z], 1))
    nan = F32(np.nan)
    return dict(normals=np.where(defined[:, None], vec.astype(F32), F32(0)).astype(F32),
                curvature=np.where(defined, curv.astype(F32), nan).astype(F32),
                eigenvalues=np.where(defined[:, None], lam.astype(F32), nan).astype(F32), found=found.astype(np.int32),
                lam=lam, vec=vec, off=off, defined=defined, moments=mom)


def normals_one(points, grid, k, max_radius=None, view=None, sweeps=SWEEPS):
    t = K.knn_one(points, grid, k, max_radius)
    return normals_from(points, t["idx"], t["found"], view, sweeps)


def normals_ragged(points, offsets, grid, k, max_per_sample, counts=None, max_radius=None, view=None):
    """The ragged call -> dict(normals [T,3], curvature [T], eigenvalues [T,3], found [T], untouched bool [T])."""
    p = np.asarray(points, F32).reshape(-1, 3)
    off = [int(o) for o in offsets]
    T = len(p)
    out = dict(normals=np.zeros((T, 3), F32), curvature=np.zeros(T, F32), eigenvalues=np.zeros((T, 3), F32), found=np.zeros(T, np.int32),
               untouched=np.ones(T, bool))
    for b in range(len(off) - 1):
        n = R._span(off, b, counts, max_per_sample)
        one = normals_one(p[off[b]:off[b] + n], grid, k, max_radius, view)
        for key in ("normals", "curvature", "eigenvalues", "found"):
            out[key][off[b]:off[b] + n] = one[key]
        out["untouched"][off[b]:off[b] + n] = False
    return out


# ---- normal consistency ----------------------------------------------------------------------------------------------------------------------
def nearest(a, b):
    """The exact nearest row of b [m,3] for every row of a [n,3]: float64 d^2 = dx*dx + dy*dy + dz*dz, the lowest index on ties."""
    a, b = np.asarray(a, F32).astype(F64), np.asarray(b, F32).astype(F64)
    out = np.zeros(len(a), np.int64)
    for s in range(0, len(a), 512):
        d = a[s:s + 512, None, :] - b[None, :, :]
        out[s:s + 512] = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).argmin(axis=1)
    return out


def usable(nrm):
    with np.errstate(invalid="ignore"):
        return np.isfinite(nrm).all(axis=1) & (nrm != 0).any(axis=1)


def consistency_one_way(a, na, b, nb):
    """(nc float64, counting rows) of one direction of one frame."""
    a, na, b, nb = (np.asarray(t, F32).reshape(-1, 3) for t in (a, na, b, nb))
    if len(a) == 0 or len(b) == 0:
        return F64(np.nan), 0
    j = nearest(a, b)
    x, y = na.astype(F64), nb[j].astype(F64)
    on = usable(na) & usable(nb[j])
    with np.errstate(invalid="ignore", over="ignore"):
        term = np.abs((x[:, 0] * y[:, 0] + x[:, 1] * y[:, 1]) + x[:, 2] * y[:, 2])
    cnt = int(on.sum())
    if cnt == 0:
        return F64(np.nan), 0
    return K.fixed_sum(np.where(on, term, 0.0)) / F64(cnt), cnt


def consistency_ragged(pred, pred_normals, pred_off, gt, gt_normals, gt_off):
    """-> (nc float64 [B,3], counts int64 [B,2])."""
    B = len(pred_off) - 1
    nc, cnt = np.zeros((B, 3), F64), np.zeros((B, 2), np.int64)
    for f in range(B):
        sp, sg = slice(int(pred_off[f]), int(pred_off[f + 1])), slice(int(gt_off[f]), int(gt_off[f + 1]))
        nc[f, 0], cnt[f, 0] = consistency_one_way(pred[sp], pred_normals[sp], gt[sg], gt_normals[sg])
        nc[f, 1], cnt[f, 1] = consistency_one_way(gt[sg], gt_normals[sg], pred[sp], pred_normals[sp])
        nc[f, 2] = (nc[f, 0] + nc[f, 1]) / F64(2.0)
    return nc, cnt


# ---- the clouds of the host test: each -> points f32 [n,3] -------------------------------------------------------------------------------------
def sphere_shell(seed=31, n=1500):
    d = np.random.RandomState(seed).normal(size=(n, 3))
    return (np.array([40.0, 5.0, 1.0]) + 10.0 * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)


def noisy_plane(seed=32, n=1500):
    rs = np.random.RandomState(seed)
    p = np.concatenate([rs.uniform(0, 4, size=(n, 2)), rs.normal(scale=0.01, size=(n, 1))], 1)
    rot = np.linalg.qr(rs.normal(size=(3, 3)))[0]
    return (p @ rot.T + np.array([3.0, -2.0, 7.0])).astype(F32)


def uniform_volume(seed=33, n=1500):
    return np.random.RandomState(seed).uniform(0, 1, size=(n, 3)).astype(F32)


def lattice_slab():
    g = np.stack(np.meshgrid(np.arange(12), np.arange(12), np.arange(2), indexing="ij"), -1).reshape(-1, 3)
    return g.astype(F32)


def box_grid(p, cell):
    """A grid over the cloud's own box, the cell edge `cell`."""
    lo, hi = p.min(axis=0).astype(F64), p.max(axis=0).astype(F64)
    return (tuple(float(F32(x)) for x in lo - 0.5 * cell), (float(F32(cell)),) * 3,
            tuple(int(np.floor((h - l + cell) / cell)) + 1 for l, h in zip(lo, hi)))


HOST_CLOUDS = dict(sphere_shell=sphere_shell, noisy_plane=noisy_plane, uniform_volume=uniform_volume, lattice_slab=lattice_slab)
