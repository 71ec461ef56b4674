"""The definition of the fixed-radius neighbour count, the nearest other row and the radius outlier filter (include/rald_hip.h,
DESIGN.md section 22) by brute force in numpy float32, for the tests to compare with by equality: every operation is one numpy
float32 operation, so it is rounded once and never contracted.  Beside it an independent grid walk with the header's search-range
rule (the host tests hold the two against each other) and the clouds both test files use."""
import numpy as np

F32 = np.float32
INF = F32(np.inf)


def cell_f(x, lo, v):
    """floorf(fl(fl(x - lo) / v)) in float32, elementwise."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.floor(((np.asarray(x, F32) - F32(lo)).astype(F32) / F32(v)).astype(F32))


def inside_of(points, lo3, dims3, v3):
    p = np.asarray(points, F32).reshape(-1, 3)
    ok = np.ones(len(p), bool)
    with np.errstate(invalid="ignore"):
        for k in range(3):
            c = cell_f(p[:, k], lo3[k], v3[k])
            ok &= (c >= F32(0)) & (c < F32(int(dims3[k])))                  # compared in float; NaN fails both
    return ok


def d2_rows(p, rows):
    """d2(i, j) for i in rows, every j -> float32 [len(rows), n]."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = (p[None, :, :] - p[rows, None, :]).astype(F32)                   # dx = fl(p_j - p_i)
        s = (d * d).astype(F32)
        return ((s[..., 0] + s[..., 1]).astype(F32) + s[..., 2]).astype(F32)


def radius_one(points, grid, radius, max_count=0):
    """One cloud [n,3] -> dict(count i32 [n], nn_idx i64 [n], nn_dist2 f32 [n], inside bool [n]); nn_* are those of the uncapped search."""
    lo3, v3, dims3 = grid
    p = np.asarray(points, F32).reshape(-1, 3)
    n = len(p)
    inside = inside_of(p, lo3, dims3, v3)
    r2 = F32(F32(radius) * F32(radius))
    count = np.full(n, -1, np.int32)
    nn_idx = np.full(n, -1, np.int64)
    nn_dist2 = np.full(n, INF, F32)
    cols = np.arange(n)
    for s in range(0, n, 256):
        rows = np.arange(s, min(s + 256, n))
        d2 = d2_rows(p, rows)
        with np.errstate(invalid="ignore"):
            hit = (d2 <= r2) & inside[None, :] & (cols[None, :] != rows[:, None])
        c = hit.sum(axis=1)
        masked = np.where(hit, d2, INF)
        best = masked.argmin(axis=1)                                          # the first of equal minima: the smallest row index
        some = c > 0
        count[rows] = c
        nn_idx[rows] = np.where(some, best, -1)
        nn_dist2[rows] = np.where(some, masked[np.arange(len(rows)), best], INF)
    count[~inside], nn_idx[~inside], nn_dist2[~inside] = -1, -1, INF
    if max_count > 0:
        count = np.where(inside, np.minimum(count, max_count), -1).astype(np.int32)
    return dict(count=count, nn_idx=nn_idx, nn_dist2=nn_dist2, inside=inside)


def _span(off, b, counts, max_per_sample):
    n = off[b + 1] - off[b]
    if counts is not None:
        n = min(n, max(int(counts[b]), 0))
    return max(min(n, int(max_per_sample)), 0)


def radius_ragged(points, offsets, grid, radius, max_per_sample, counts=None, max_count=0):
    """The ragged count call -> dict(count, nn_idx, nn_dist2 per row [T], untouched bool [T]: rows the call must not write)."""
    p = np.asarray(points, F32).reshape(-1, 3)
    off = [int(o) for o in offsets]
    T = len(p)
    out = dict(count=np.zeros(T, np.int32), nn_idx=np.zeros(T, np.int64), nn_dist2=np.zeros(T, F32), untouched=np.ones(T, bool))
    for b in range(len(off) - 1):
        n = _span(off, b, counts, max_per_sample)
        one = radius_one(p[off[b]:off[b] + n], grid, radius, max_count)
        for k in ("count", "nn_idx", "nn_dist2"):
            out[k][off[b]:off[b] + n] = one[k]
        out["untouched"][off[b]:off[b] + n] = False
    return out


def filter_ragged(points, offsets, grid, radius, min_neighbors, max_per_sample, counts=None, uncapped=None):
    """The ragged filter -> dict(points f32 [M,3], offsets i64 [B+1], index i64 [M], count i32 [T] (min(count, min_neighbors), -1
    outside), untouched bool [T]).  uncapped: radius_ragged's result for the same arguments, where the caller has it already."""
    p = np.asarray(points, F32).reshape(-1, 3)
    off = [int(o) for o in offsets]
    r = radius_ragged(p, off, grid, radius, max_per_sample, counts) if uncapped is None else uncapped
    r = dict(r, count=np.where(r["count"] < 0, r["count"], np.minimum(r["count"], min_neighbors)).astype(np.int32))
    pts, idx, out_off = [], [], [0]
    for b in range(len(off) - 1):
        n = _span(off, b, counts, max_per_sample)
        keep = np.nonzero(r["count"][off[b]:off[b] + n] >= min_neighbors)[0]
        pts.append(p[off[b] + keep])
        idx.append(keep.astype(np.int64))
        out_off.append(out_off[-1] + len(keep))
    return dict(points=np.concatenate(pts) if pts else np.zeros((0, 3), F32), offsets=np.array(out_off, np.int64),
                index=np.concatenate(idx) if idx else np.zeros(0, np.int64), count=r["count"], untouched=r["untouched"])


# ---- an independent route: a dictionary of cells and the header's scan range --------------------------------------------------------
def scan_range(x, lo, v, dims, radius):
    """The cells a row at coordinate x scans on one axis -> (first, last), clamped to the grid."""
    rs = F32(F32(radius) * F32(1.0 + 2.0 ** -20))
    a = np.nextafter(F32(F32(x) - rs), F32(-np.inf))
    b = np.nextafter(F32(F32(x) + rs), F32(np.inf))
    ca, cb = float(cell_f(a, lo, v)), float(cell_f(b, lo, v))
    return int(min(max(ca, 0.0), dims - 1)), int(min(max(cb, 0.0), dims - 1))


def grid_walk_one(points, grid, radius):
    """radius_one's uncapped outputs by a walk over the cells of the scan range -> (dict, the widest scan in cells over rows and axes)."""
    lo3, v3, dims3 = grid
    p = np.asarray(points, F32).reshape(-1, 3)
    n = len(p)
    inside = inside_of(p, lo3, dims3, v3)
    r2 = F32(F32(radius) * F32(radius))
    cells = {}
    for i in np.nonzero(inside)[0]:
        c = tuple(int(cell_f(p[i, k], lo3[k], v3[k])) for k in range(3))
        cells.setdefault(c, []).append(int(i))
    count = np.full(n, -1, np.int32)
    nn_idx = np.full(n, -1, np.int64)
    nn_dist2 = np.full(n, INF, F32)
    widest = 0
    for i in np.nonzero(inside)[0]:
        rng = [scan_range(p[i, k], lo3[k], v3[k], int(dims3[k]), radius) for k in range(3)]
        widest = max(widest, max(b - a + 1 for a, b in rng))
        cand = []
        for x in range(rng[0][0], rng[0][1] + 1):
            for y in range(rng[1][0], rng[1][1] + 1):
                for z in range(rng[2][0], rng[2][1] + 1):
                    cand += cells.get((x, y, z), ())
        cand = np.array(sorted(j for j in cand if j != i), np.int64)
        c, best, bj = 0, INF, -1
        if len(cand):
            d2 = d2_rows(p[np.concatenate([[i], cand])], np.array([0]))[0, 1:]
            hit = d2 <= r2
            c = int(hit.sum())
            if c:
                m = np.where(hit, d2, INF)
                k = int(m.argmin())
                best, bj = m[k], int(cand[k])
        count[i], nn_idx[i], nn_dist2[i] = c, bj, best
    return dict(count=count, nn_idx=nn_idx, nn_dist2=nn_dist2, inside=inside), widest


# ---- the clouds of the tests: each -> (points f32 [n,3], grid (lo3, v3, dims3) with v = radius, radius) -----------------------------
def cube_grid(lo, hi, v):
    """(lo3, v3, dims3) of the cube [lo, hi]^3 with the cell edge v on every axis (one number or three), dims = floor((hi - lo) / v) + 1."""
    v3 = tuple(float(F32(x)) for x in (v if isinstance(v, (tuple, list)) else (v, v, v)))
    return (float(F32(lo)),) * 3, v3, tuple(int(np.floor((hi - lo) / x)) + 1 for x in v3)


def uniform_cloud(seed=1, n=1500, radius=0.1):
    rs = np.random.RandomState(seed)
    return rs.uniform(0, 1, size=(n, 3)).astype(F32), cube_grid(0.0, 1.0, radius), radius


def lattice_cloud(seed=2, n=1500, radius=0.125, side=10):
    """Coordinates k * radius, with duplicates (n draws from side^3 sites): face neighbours lie at exactly r2."""
    rs = np.random.RandomState(seed)
    p = (rs.randint(0, side, size=(n, 3)).astype(F32) * F32(radius)).astype(F32)
    return p, cube_grid(0.0, side * radius, radius), radius


def lattice_ulp_cloud(seed=3, n=1500, radius=0.125, side=10):
    """The lattice with every coordinate moved by -1, 0 or +1 ulp."""
    p, grid, radius = lattice_cloud(seed, n, radius, side)
    rs = np.random.RandomState(seed + 100)
    step = rs.randint(-1, 2, size=p.shape)
    q = np.where(step < 0, np.nextafter(p, F32(-np.inf)), np.where(step > 0, np.nextafter(p, F32(np.inf)), p)).astype(F32)
    return q, (((float(F32(-radius)),) * 3), grid[1], tuple(d + 1 for d in grid[2])), radius


def pairs_cloud(seed=4, pairs=750, radius=0.05):
    """Pairs at radius * (1 + k * 2^-23), k = -3 .. 3, in random directions, the pairs far apart from each other or not, as they fall."""
    rs = np.random.RandomState(seed)
    a = rs.uniform(0.2, 1.8, size=(pairs, 3))
    d = rs.normal(size=(pairs, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    k = rs.randint(-3, 4, size=(pairs, 1))
    b = a.astype(F32).astype(np.float64) + d * (float(F32(radius)) * (1.0 + k * 2.0 ** -23))
    p = np.empty((2 * pairs, 3), F32)
    p[0::2], p[1::2] = a.astype(F32), b.astype(F32)
    return p, cube_grid(0.0, 2.0, radius), radius


def faces_cloud(seed=5, n=1500, radius=0.1):
    """Every coordinate within 2 ulps of a cell face of the grid."""
    rs = np.random.RandomState(seed)
    side = 8
    face = (rs.randint(0, side + 1, size=(n, 3)).astype(F32) * F32(radius)).astype(F32)
    for _ in range(2):
        step = rs.randint(-1, 2, size=face.shape)
        face = np.where(step < 0, np.nextafter(face, F32(-np.inf)), np.where(step > 0, np.nextafter(face, F32(np.inf)), face)).astype(F32)
    return face, cube_grid(-radius, (side + 1) * radius, radius), radius


def far_box_cloud(seed=6, n=1500, radius=0.05):
    """A box of +-100 (on the first axis; +-1 on the others, so that cells of edge `radius` stay below 2^31) at radius 0.05: clusters,
    so that rows have neighbours, at coordinates whose ulp is 2^-17."""
    rs = np.random.RandomState(seed)
    centres = rs.uniform(-1, 1, size=(n // 10, 3)) * np.array([100.0, 0.9, 0.9])
    p = (centres[rs.randint(0, len(centres), size=n)] + rs.uniform(-0.06, 0.06, size=(n, 3))).astype(F32)
    v = float(F32(radius))
    return p, ((-100.5, -1.0, -1.0), (v, v, v), (int(201.0 / v) + 1, int(2.0 / v) + 1, int(2.0 / v) + 1)), radius


CONSTRUCTIONS = dict(uniform=uniform_cloud, lattice=lattice_cloud, lattice_ulp=lattice_ulp_cloud, pairs=pairs_cloud, faces=faces_cloud,
                     far_box=far_box_cloud)
