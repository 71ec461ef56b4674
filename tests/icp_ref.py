"""The definition of ICP registration and of the rigid transform of ragged clouds (include/rald_hip.h) by brute
force in numpy, for the tests to compare with by equality: every fp32 and float64 operation is one numpy operation, so it is rounded
once and never contracted; all target rows are scanned and the cell rule only drops the outside ones; the sums are knn_ref.fixed_sum.
Beside it an independent second route (route=1: the candidates from the scan range of the grid, a dense [m, 29] term array summed at
once in the fixed shape, the factorisation row by row), which the host tests hold against the first, and the constructions both test
files use."""
import numpy as np

import knn_ref as K
import radius_ref as R

F32 = np.float32
F64 = np.float64
INF = F32(np.inf)
SEG = 1024
NS = 29
FLOOR = F64(2.0 ** -30)
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], F64)
MUTATIONS = ("lt", "tie_high", "batch_blocks", "converge_before", "no_floor")


# ---- steps 1 and 2 ---------------------------------------------------------------------------------------------------------------------
def move(T, p):
    """p fp32 [n,3], T float64 [12] -> (p' float64 [n,3], pf fp32 [n,3])."""
    T = np.asarray(T, F64)
    q = np.asarray(p, F32).reshape(-1, 3).astype(F64)
    with np.errstate(invalid="ignore", over="ignore"):
        pp = np.stack([((T[k * 3] * q[:, 0] + T[k * 3 + 1] * q[:, 1]) + T[k * 3 + 2] * q[:, 2]) + T[9 + k] for k in range(3)], axis=1)
        return pp, pp.astype(F32)


def _d2(pf, t):
    """rad_d2(pf_i, t_j) -> fp32 [m, nt]: dx = fl(t.x - pf.x)."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = (t[None, :, :] - pf[:, None, :]).astype(F32)
        s = (d * d).astype(F32)
        return ((s[..., 0] + s[..., 1]).astype(F32) + s[..., 2]).astype(F32)


def correspond(pf, ok, tgt, inside, grid, max_dist, route=0, mutate=None):
    """The target row of every source row with ok (usable and pf finite) -> int64 [m], -1 for none.  mutate: a wrong rule, for the
    mutation checks of the host tests ('lt': d2 < r2; 'tie_high': the highest row on equal d2)."""
    m = len(pf)
    corr = np.full(m, -1, np.int64)
    if len(tgt) == 0 or m == 0:
        return corr
    r2 = F32(F32(max_dist) * F32(max_dist))
    lo3, v3, dims3 = grid
    if route == 1:                                                               # the cells of every target row, once
        with np.errstate(invalid="ignore", over="ignore"):
            cell = np.stack([R.cell_f(tgt[:, a], lo3[a], v3[a]) for a in range(3)], axis=1)
    for s in range(0, m, 256):
        rows = np.arange(s, min(s + 256, m))
        rows = rows[ok[rows]]
        if len(rows) == 0:
            continue
        d2 = _d2(pf[rows], tgt)
        with np.errstate(invalid="ignore"):
            cand = inside[None, :] & ((d2 < r2) if mutate == "lt" else (d2 <= r2))
        if route == 1:                                                           # only the rows of the scan range's cells are looked at
            rng = np.array([[R.scan_range(pf[i, a], lo3[a], v3[a], int(dims3[a]), max_dist) for a in range(3)] for i in rows], F64)
            with np.errstate(invalid="ignore"):
                seen = inside[None, :].copy()
                for a in range(3):
                    seen = seen & (cell[None, :, a] >= rng[:, a, 0:1]) & (cell[None, :, a] <= rng[:, a, 1:2])
            assert not (cand & ~seen).any(), "a candidate outside the scan range"
            cand = cand & seen
        masked = np.where(cand, d2, INF)
        best = masked.argmin(axis=1)                                             # the first of equal minima: the lowest row index
        if mutate == "tie_high":
            best = masked.shape[1] - 1 - masked[:, ::-1].argmin(axis=1)
        corr[rows] = np.where(cand.any(axis=1), best, -1)
    return corr


# ---- step 3 ----------------------------------------------------------------------------------------------------------------------------
def _products(pp, d, n):
    """One equation per row: the 28 products, a list of float64 [m]."""
    J = [pp[:, 1] * n[:, 2] - pp[:, 2] * n[:, 1], pp[:, 2] * n[:, 0] - pp[:, 0] * n[:, 2], pp[:, 0] * n[:, 1] - pp[:, 1] * n[:, 0],
         n[:, 0], n[:, 1], n[:, 2]]
    r = (n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2]
    return [J[i] * J[j] for i in range(6) for j in range(i, 6)] + [J[i] * r for i in range(6)] + [r * r]


def terms(pp, corr, tgt, normals, mode):
    """The rows' contributions float64 [m, 29] (+0.0 where the row does not count) and the counting flags."""
    m = len(pp)
    counts = corr >= 0
    q = np.zeros((m, 3), F64)
    n = np.zeros((m, 3), F64)
    if counts.any():
        q[counts] = tgt[corr[counts]].astype(F64)
    if mode == 1 and counts.any():
        nf = normals[corr[counts]]
        good = np.isfinite(nf).all(axis=1) & ~(nf == 0).all(axis=1)
        n[counts] = nf.astype(F64)
        counts = counts.copy()
        counts[np.nonzero(counts)[0][~good]] = False
    p = np.where(counts[:, None], pp, 0.0)
    n = np.where(counts[:, None], n, 0.0)
    d = np.where(counts[:, None], p - np.where(counts[:, None], q, 0.0), 0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        if mode == 1:
            prod = _products(p, d, n)
        else:
            e = [np.tile(np.array(v, F64), (m, 1)) for v in ((1, 0, 0), (0, 1, 0), (0, 0, 1))]
            a, b, c = (_products(p, d, x) for x in e)
            prod = [(a[k] + b[k]) + c[k] for k in range(28)]
        prod.append((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        return np.stack([np.where(counts, x, 0.0) for x in prod], axis=1), counts


def sums(contrib, route=0, lead=0):
    """The 29 cloud sums in the fixed shape.  lead (mutation checks): rows of +0.0 in front, as if the blocks were counted from another
    row than the cloud's first."""
    if lead:
        contrib = np.concatenate([np.zeros((lead, NS), F64), contrib])
    if route == 0:
        return np.array([K.fixed_sum(contrib[:, k]) for k in range(NS)], F64)
    m = len(contrib)                                                             # the dense array at once
    v = np.zeros((-(-max(m, 1) // SEG) * SEG, NS), F64)
    v[:m] = contrib
    v = v.reshape(-1, SEG, NS)
    with np.errstate(invalid="ignore", over="ignore"):
        h = SEG
        while h > 1:
            h //= 2
            v = v[:, :h] + v[:, h:]
        s = np.zeros(NS, F64)
        for g in range(len(v)):
            s = s + v[g, 0]
    return s


# ---- steps 4 and 5 ---------------------------------------------------------------------------------------------------------------------
def _matrix(S):
    A = np.zeros((6, 6), F64)
    k = 0
    for i in range(6):
        for j in range(i, 6):
            A[i, j] = A[j, i] = S[k]
            k += 1
    return A


def solve(S, route=0, floor=FLOOR):
    """x of A x = -g by the header's Cholesky, or None for a refused pivot / a non-finite x.  floor (mutation checks): 0 removes it."""
    A, g = _matrix(S), S[21:27]
    L = np.zeros((6, 6), F64)
    with np.errstate(all="ignore"):
        if route == 0:                                                           # column by column, as the header writes it
            for j in range(6):
                s = A[j, j]
                for k in range(j):
                    s = s - L[j, k] * L[j, k]
                if not (np.isfinite(s) and s > A[j, j] * floor):
                    return None
                L[j, j] = np.sqrt(s)
                for i in range(j + 1, 6):
                    t = A[j, i]
                    for k in range(j):
                        t = t - L[i, k] * L[j, k]
                    L[i, j] = t / L[j, j]
        else:                                                                    # row by row: the same operations in another loop order
            for i in range(6):
                for j in range(i):
                    t = A[j, i]
                    for k in range(j):
                        t = t - L[i, k] * L[j, k]
                    L[i, j] = t / L[j, j]
                s = A[i, i]
                for k in range(i):
                    s = s - L[i, k] * L[i, k]
                if not (np.isfinite(s) and s > A[i, i] * floor):
                    return None
                L[i, i] = np.sqrt(s)
        y, x = np.zeros(6, F64), np.zeros(6, F64)
        for i in range(6):
            s = -g[i]
            for k in range(i):
                s = s - L[i, k] * y[k]
            y[i] = s / L[i, i]
        for i in range(5, -1, -1):
            s = y[i]
            for k in range(i + 1, 6):
                s = s - L[k, i] * x[k]
            x[i] = s / L[i, i]
    return x if np.isfinite(x).all() else None


def update(T, x):
    """(R, t) <- (dR R, dR t + u) with the Cayley rotation of w / 2."""
    with np.errstate(all="ignore"):
        w, u = x[:3], x[3:]
        a = w * F64(0.5)
        aa = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
        den, c = F64(1.0) + aa, F64(1.0) - aa
        dR = [[(c + w[0] * a[0]) / den, (w[0] * a[1] - w[2]) / den, (w[0] * a[2] + w[1]) / den],
              [(w[1] * a[0] + w[2]) / den, (c + w[1] * a[1]) / den, (w[1] * a[2] - w[0]) / den],
              [(w[2] * a[0] - w[1]) / den, (w[2] * a[1] + w[0]) / den, (c + w[2] * a[2]) / den]]
        N = np.zeros(12, F64)
        for i in range(3):
            for j in range(3):
                N[i * 3 + j] = (dR[i][0] * T[j] + dR[i][1] * T[3 + j]) + dR[i][2] * T[6 + j]
            N[9 + i] = ((dR[i][0] * T[9] + dR[i][1] * T[10]) + dR[i][2] * T[11]) + u[i]
    return N


# ---- one pair, the ragged call, the transform ---------------------------------------------------------------------------------------
def icp_one(src, tgt, grid, max_dist, mode=0, normals=None, init=None, max_iterations=30, tolerance=1e-6, min_correspondences=6, route=0,
            trace=None, mutate=None, row0=0):
    """One pair -> dict(transform f64 [16], stats f64 [4], info i32 [3], corr i64 [m], moved f32 [m,3]).  trace: a list that receives
    (corr, T) of every iteration's step 2.  mutate: one of MUTATIONS, a wrong rule for the mutation checks; row0: the cloud's first row in
    its batch, which only the mutation 'batch_blocks' looks at."""
    src = np.asarray(src, F32).reshape(-1, 3)
    tgt = np.asarray(tgt, F32).reshape(-1, 3)
    normals = None if normals is None else np.asarray(normals, F32).reshape(-1, 3)
    lo3, v3, dims3 = grid
    inside = R.inside_of(tgt, lo3, dims3, v3)
    usable = np.isfinite(src).all(axis=1)
    T = IDENTITY.copy() if init is None else np.asarray(init, F64).reshape(12).copy()

    def pass_(T):
        pp, pf = move(T, src)
        ok = usable & np.isfinite(pf).all(axis=1)
        corr = correspond(pf, ok, tgt, inside, grid, max_dist, route, mutate)
        contrib, counts = terms(pp, corr, tgt, normals, mode)
        return pf, corr, sums(contrib, route, row0 % SEG if mutate == "batch_blocks" else 0), int(counts.sum())

    status, iters, step = 0, 0, F64(0.0)
    for _ in range(max_iterations):
        _, corr, S, count = pass_(T)
        if trace is not None:
            trace.append((corr, T.copy()))
        if count < min_correspondences:
            status = 2
            break
        x = solve(S, route, F64(0.0) if mutate == "no_floor" else FLOOR)
        if x is None:
            status = 3
            break
        if mutate == "converge_before" and np.abs(x).max() <= F64(tolerance):
            status, step = 1, np.abs(x).max()
            break
        T = update(T, x)
        iters += 1
        step = np.abs(x).max()
        if step <= F64(tolerance):
            status = 1
            break
    pf, corr, S, count = pass_(T)
    nu = int(usable.sum())
    out = np.zeros(16, F64)
    out[[0, 1, 2, 4, 5, 6, 8, 9, 10]] = T[:9]
    out[[3, 7, 11]] = T[9:]
    out[15] = 1.0
    with np.errstate(all="ignore"):
        stats = np.array([F64(count) / F64(nu) if nu else 0.0, np.sqrt(S[28] / F64(count)) if count else 0.0, step, S[27]], F64)
    return dict(transform=out, stats=stats, info=np.array([status, iters, count], np.int32), corr=corr, moved=pf)


def icp_ragged(src, src_off, tgt, tgt_off, grid, max_dist, max_src, max_tgt, mode=0, normals=None, init=None, src_counts=None,
               tgt_counts=None, **kw):
    """The ragged call -> dict(transform [B,16], stats [B,4], info [B,3], corr [Ts], moved [Ts,3], untouched bool [Ts])."""
    src = np.asarray(src, F32).reshape(-1, 3)
    tgt = np.asarray(tgt, F32).reshape(-1, 3)
    so, to = [int(o) for o in src_off], [int(o) for o in tgt_off]
    B = len(so) - 1
    out = dict(transform=np.zeros((B, 16), F64), stats=np.zeros((B, 4), F64), info=np.zeros((B, 3), np.int32),
               corr=np.zeros(len(src), np.int64), moved=np.zeros((len(src), 3), F32), untouched=np.ones(len(src), bool))
    for b in range(B):
        ns, nt = R._span(so, b, src_counts, max_src), R._span(to, b, tgt_counts, max_tgt)
        one = icp_one(src[so[b]:so[b] + ns], tgt[to[b]:to[b] + nt], grid, max_dist, mode,
                      None if normals is None else np.asarray(normals, F32).reshape(-1, 3)[to[b]:to[b] + nt],
                      None if init is None else np.asarray(init, F64).reshape(B, 12)[b], row0=so[b], **kw)
        for key in ("transform", "stats", "info"):
            out[key][b] = one[key]
        out["corr"][so[b]:so[b] + ns] = one["corr"]
        out["moved"][so[b]:so[b] + ns] = one["moved"]
        out["untouched"][so[b]:so[b] + ns] = False
    return out


def transform_ragged(points, off, transforms, max_per_sample, normals=None, counts=None):
    """The rigid transform -> (points f32 [T,3], normals f32 [T,3] or None, untouched bool [T]); transforms [B,12] or [B,16]."""
    p = np.asarray(points, F32).reshape(-1, 3)
    off = [int(o) for o in off]
    M = np.asarray(transforms, F64).reshape(len(off) - 1, -1)
    out, outn, untouched = np.zeros_like(p), None if normals is None else np.zeros_like(p), np.ones(len(p), bool)
    for b in range(len(off) - 1):
        n = R._span(off, b, counts, max_per_sample)
        T = M[b] if M.shape[1] == 12 else np.concatenate([M[b].reshape(4, 4)[:3, :3].reshape(9), M[b].reshape(4, 4)[:3, 3]])
        sl = slice(off[b], off[b] + n)
        out[sl] = move(T, p[sl])[1]
        if normals is not None:
            outn[sl] = move(np.concatenate([T[:9], np.zeros(3, F64)]), np.asarray(normals, F32).reshape(-1, 3)[sl])[1]
        untouched[sl] = False
    return out, outn, untouched


# ---- the constructions of the tests --------------------------------------------------------------------------------------------------
def rotation(axis, degrees):
    """Rodrigues in float64 (for the constructions only; the definition has no sine)."""
    k = np.asarray(axis, F64) / np.linalg.norm(axis)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]], F64)
    th = np.deg2rad(degrees)
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def motion_error(transform16, Rm, tm):
    """(degrees, metres) between the result and the inverse of the motion x -> Rm x + tm."""
    M = np.asarray(transform16, F64).reshape(4, 4)
    Re, te = Rm.T, -Rm.T @ tm
    dR = M[:3, :3] @ Re.T
    ang = np.degrees(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1)))
    return float(ang), float(np.linalg.norm(M[:3, 3] - te))


FACES_GRID = R.cube_grid(-1.0, 5.0, 0.5)
FACES_DIST = 0.5
MOTIONS = dict(small=(3.0, 0.05), large=(10.0, 0.20))


def faces(motion="small", seed=31, n_src=1000, extra=0):
    """Three orthogonal 4 m faces (x = 0, y = 0, z = 0 over [0, 4]^2) with their analytic normals, 3000 target rows; the source is
    n_src of them moved by `degrees` about (1, 2, 3) through the faces' centre of mass and `shift` along (2, -1, 2) / 3, rounded to
    fp32; `extra` further source rows far from every target row ->
    dict(src, tgt, normals, grid, max_dist, Rm, tm)."""
    rs = np.random.RandomState(seed)
    tgt = np.zeros((3000, 3), F64)
    nrm = np.zeros((3000, 3), F32)
    for f in range(3):
        uv = rs.uniform(0.0, 4.0, size=(1000, 2))
        tgt[f * 1000:(f + 1) * 1000, [(f + 1) % 3, (f + 2) % 3]] = uv
        nrm[f * 1000:(f + 1) * 1000, f] = 1.0
    order = rs.permutation(3000)
    tgt, nrm = tgt[order].astype(F32), nrm[order]
    degrees, shift = MOTIONS[motion]
    Rm = rotation((1, 2, 3), degrees)
    centre = tgt.astype(F64).mean(axis=0)
    tm = centre - Rm @ centre + shift * np.array([2, -1, 2], F64) / 3.0
    pick = rs.choice(3000, n_src, replace=n_src > 3000)
    src = (tgt[pick].astype(F64) @ Rm.T + tm).astype(F32)
    if extra:
        src = np.concatenate([src, rs.uniform(20.0, 24.0, size=(extra, 3)).astype(F32)])
    return dict(src=src, tgt=tgt, normals=nrm, grid=FACES_GRID, max_dist=FACES_DIST, Rm=Rm, tm=tm)


def tie(seed=32):
    """A lattice of spacing 1/4 (5^3 rows in a random order) and source rows exactly midway between two and between eight of them."""
    rs = np.random.RandomState(seed)
    g = np.stack(np.meshgrid(*[np.arange(5)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    tgt = (g[rs.permutation(len(g))] * 0.25).astype(F32)
    two = (rs.randint(0, 4, size=(60, 3)) * 0.25).astype(F32)
    two[np.arange(60), rs.randint(0, 3, size=60)] += F32(0.125)
    eight = (rs.randint(0, 4, size=(60, 3)) * 0.25 + 0.125).astype(F32)
    return dict(src=np.concatenate([two, eight]), tgt=tgt, normals=np.tile(np.array([[0, 0, 1]], F32), (len(tgt), 1)),
                grid=R.cube_grid(-0.25, 1.25, 0.25), max_dist=0.25)


def edge():
    """Target rows far apart, and per target row source rows at exactly d2 == fl(max_dist^2) (even source rows) and at the next float
    above (odd source rows), max_dist = 1/2."""
    tgt = np.array([[1, 1, 1], [3, 1, 1], [1, 3, 1], [1, 1, 3], [3, 3, 3], [3, 3, 1], [3, 1, 3]], F32)
    src = []
    for k, t in enumerate(tgt):
        on = t.copy()
        down = t[k % 3] == 3                                                     # 2.5 and 3 share a binade: 3 - nextafter(2.5, -inf) is exact
        on[k % 3] += F32(-0.5) if down else F32(0.5)
        off = on.copy()
        off[k % 3] = np.nextafter(on[k % 3], F32(-np.inf) if down else F32(np.inf))
        src += [on, off]
    return dict(src=np.array(src, F32), tgt=tgt, normals=np.tile(np.array([[1, 0, 0]], F32), (len(tgt), 1)),
                grid=R.cube_grid(0.0, 4.0, 0.5), max_dist=0.5)


def planar(seed=33):
    """A target on the exact plane z = 1 and a source that is 600 of its rows after a small motion."""
    rs = np.random.RandomState(seed)
    tgt = np.concatenate([rs.uniform(0.0, 4.0, size=(1500, 2)), np.ones((1500, 1))], axis=1).astype(F32)
    Rm = rotation((0, 0, 1), 2.0)
    tm = np.array([0.03, -0.02, 0.0], F64)
    src = (tgt[rs.choice(1500, 600, replace=False)].astype(F64) @ Rm.T + tm).astype(F32)
    return dict(src=src, tgt=tgt, normals=np.tile(np.array([[0, 0, 1]], F32), (1500, 1)), grid=R.cube_grid(-1.0, 5.0, 0.5), max_dist=0.5,
                Rm=Rm, tm=tm)


def line(seed=37):
    """400 target rows along the x axis at y = 1, z = 2 with a scatter of a few 1e-6 across it, the source the same rows moved by 1 cm
    along it: in point mode the rotation about the line is a direction the rows determine only to about 1e-12 of the diagonal - above
    the rounding noise, below the pivot floor."""
    rs = np.random.RandomState(seed)
    tgt = np.stack([rs.uniform(0.0, 4.0, 400), 1.0 + 4e-6 * rs.uniform(-1, 1, 400), 2.0 + 4e-6 * rs.uniform(-1, 1, 400)], axis=1).astype(F32)
    src = tgt.copy()
    src[:, 0] += F32(0.01)
    return dict(src=src, tgt=tgt, normals=np.tile(np.array([[0, 0, 1]], F32), (400, 1)), grid=R.cube_grid(-1.0, 5.0, 0.5), max_dist=0.5)


def few(n_counting, seed=34):
    """A source with exactly n_counting rows near the faces' target; the others are far, NaN or +-inf."""
    f = faces("small", seed)
    rs = np.random.RandomState(seed + 1)
    far = rs.uniform(20.0, 24.0, size=(9, 3)).astype(F32)
    far[2] = (np.nan, 1.0, 1.0)
    far[5] = (1.0, np.inf, 1.0)
    far[7] = (1.0, 1.0, -np.inf)
    src = np.concatenate([far[:4], f["src"][:n_counting], far[4:]])
    return dict(f, src=src)


def bad_rows(seed=35):
    """The faces pair with NaN / inf rows on both sides, rows outside the grid in the target, and zero and NaN target normals."""
    f = faces("small", seed)
    src, tgt, nrm = f["src"].copy(), f["tgt"].copy(), f["normals"].copy()
    src[[3, 500, 999]] = [[np.nan, 0, 0], [0, np.inf, 0], [1, 1, -np.inf]]
    tgt[[7, 1500]] = [[np.nan, 1, 1], [np.inf, 1, 1]]
    tgt[[20, 21]] += F32(100.0)                                                  # outside the grid
    nrm[0:3000:7] = 0.0
    nrm[1:3000:11, 1] = np.nan
    return dict(f, src=src, tgt=tgt, normals=nrm)


def ragged_of(pairs, pad=3, seed=36):
    """Pairs (dicts with src / tgt / normals) -> the arrays of a ragged batch with `pad` rows of NaN between the clouds, which no call
    may read: dict(src, src_off, tgt, tgt_off, normals, max_src, max_tgt, src_counts, tgt_counts).  The gaps are cut off by counts."""
    src, tgt, nrm, so, to, sc, tc = [], [], [], [0], [0], [], []
    for p in pairs:
        for rows, acc, off, cnt in ((p["src"], src, so, sc), (p["tgt"], tgt, to, tc)):
            acc += [np.asarray(rows, F32).reshape(-1, 3), np.full((pad, 3), np.nan, F32)]
            off.append(off[-1] + len(rows) + pad)
            cnt.append(len(rows))
        nrm += [np.asarray(p["normals"], F32).reshape(-1, 3), np.full((pad, 3), np.nan, F32)]
    return dict(src=np.concatenate(src), src_off=np.array(so, np.int64), tgt=np.concatenate(tgt), tgt_off=np.array(to, np.int64),
                normals=np.concatenate(nrm), src_counts=np.array(sc, np.int32), tgt_counts=np.array(tc, np.int32),
                max_src=max(max(sc), 1), max_tgt=max(max(tc), 1))


# ---- the cases of both test files: name -> (the pair, the arguments of icp_one) --------------------------------------------------------
def _cases():
    c = {}
    for motion in MOTIONS:
        for mode, mname in ((1, "plane"), (0, "point")):
            c[f"faces_{motion}_{mname}"] = (lambda motion=motion: faces(motion), dict(mode=mode))
    for mode, mname in ((1, "plane"), (0, "point")):
        c[f"overlap_{mname}"] = (lambda: faces("small", extra=300), dict(mode=mode))
        c[f"planar_{mname}"] = (planar, dict(mode=mode))
        c[f"bad_rows_{mname}"] = (bad_rows, dict(mode=mode))
        c[f"tie_step_{mname}"] = (tie, dict(mode=mode, max_iterations=1))
    c["tie_eval"] = (tie, dict(mode=0, max_iterations=1, min_correspondences=10 ** 6))
    c["edge_eval"] = (edge, dict(mode=0, max_iterations=1, min_correspondences=10 ** 6))
    c["edge_step"] = (edge, dict(mode=1, max_iterations=1, min_correspondences=1))
    c["line_point"] = (line, dict(mode=0))
    for n in (0, 1, 5, 6):
        c[f"few_{n}"] = (lambda n=n: few(n), dict(mode=1, min_correspondences=6))
    for n in (1023, 1024, 1025, 2049):
        c[f"length_{n}"] = (lambda n=n: faces("small", seed=40 + n % 7, n_src=n), dict(mode=n % 2))
    c["tolerance_0"] = (lambda: faces("small", n_src=300), dict(mode=1, tolerance=0.0, max_iterations=6))
    c["iterations_64"] = (lambda: faces("small", n_src=300), dict(mode=0, tolerance=0.0, max_iterations=64))
    c["iterations_1"] = (lambda: faces("large", n_src=300), dict(mode=1, max_iterations=1))
    return c


CASES = _cases()
_cache = {}


def case(name):
    """-> (the pair's dict, the arguments, icp_one's result), computed once."""
    if name not in _cache:
        make, kw = CASES[name]
        pair = make()
        _cache[name] = (pair, kw, icp_one(pair["src"], pair["tgt"], pair["grid"], pair["max_dist"], normals=pair["normals"], **kw))
    return _cache[name]
