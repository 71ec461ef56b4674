"""The definition of the density clustering and of the small-cluster filter (include/rald_hip.h) by brute force
in numpy float32 with a plain host union-find, for the tests to compare with by equality.  Beside it an independent route - the cells
and the scan range of radius_ref's grid walk, then label propagation to a fixed point - and the clouds both test files use."""
import functools

import numpy as np

import radius_ref as R

F32 = np.float32
INF = R.INF


def _find(parent, x):
    while parent[x] != x:
        parent[x] = parent[parent[x]]
        x = parent[x]
    return x


def _finish(n, inside, core, comp, near, min_points, count):
    """Labels from a component id per core row (any ids) and the nearest core row of every other inside row (-1: none)."""
    rep = {}
    for i in np.nonzero(core)[0]:                                             # ascending: the first row of a component is its smallest
        rep.setdefault(int(comp[i]), int(i))
    order = {c: k for k, c in enumerate(sorted(rep, key=rep.get))}
    labels = np.full(n, -2, np.int32)
    labels[inside] = -1
    for i in np.nonzero(core)[0]:
        labels[i] = order[int(comp[i])]
    for i in np.nonzero(inside & ~core)[0]:
        if near[i] >= 0:
            labels[i] = labels[near[i]]
    C = len(order)
    sizes = np.zeros(n, np.int32)
    if C:
        sizes[:C] = np.bincount(labels[labels >= 0], minlength=C)
    cnt = np.where(inside, np.minimum(count, min_points), -1).astype(np.int32)
    return dict(labels=labels, num_clusters=C, sizes=sizes, count=cnt, inside=inside, core=core)


def cluster_one(points, grid, eps, min_points, tie="smallest", with_border=True):
    """One cloud [n,3] -> dict(labels i32 [n], num_clusters, sizes i32 [n], count i32 [n], inside, core).  tie: which core row a border
    row takes on equal d2 ("largest" is NOT the definition: the host tests use it to show that a cloud tells the two apart)."""
    lo3, v3, dims3 = grid
    p = np.asarray(points, F32).reshape(-1, 3)
    n = len(p)
    inside = R.inside_of(p, lo3, dims3, v3)
    r2 = F32(F32(eps) * F32(eps))
    count = np.zeros(n, np.int64)
    cols = np.arange(n)
    hits = []
    for s in range(0, n, 256):
        rows = np.arange(s, min(s + 256, n))
        d2 = R.d2_rows(p, rows)
        with np.errstate(invalid="ignore"):
            hit = (d2 <= r2) & inside[None, :] & inside[rows, None] & (cols[None, :] != rows[:, None])
        count[rows] = hit.sum(axis=1)
        hits.append((rows, hit, d2))
    core = inside & (count >= min_points)
    parent = list(range(n))
    near = np.full(n, -1, np.int64)
    for rows, hit, d2 in hits:
        for k, i in enumerate(rows):
            if not inside[i]:
                continue
            js = np.nonzero(hit[k] & core)[0]
            if core[i]:
                for j in js[js < i]:
                    a, b = _find(parent, int(i)), _find(parent, int(j))
                    if a != b:
                        parent[max(a, b)] = min(a, b)
            elif len(js) and with_border:
                d = d2[k, js]
                m = d.min()
                ties = js[d == m]
                near[i] = ties[0] if tie == "smallest" else ties[-1]
    comp = np.array([_find(parent, i) for i in range(n)], np.int64)
    return _finish(n, inside, core, comp, near, min_points, count)


@functools.lru_cache(maxsize=None)
def _walk_edges(key):
    """The directed pairs (i, j, d2) with d2 <= r2 of a construction, by the cells of radius_ref.grid_walk_one and its scan range."""
    p, grid, eps = _CLOUDS[key]
    lo3, v3, dims3 = grid
    inside = R.inside_of(p, lo3, dims3, v3)
    r2 = F32(F32(eps) * F32(eps))
    cells = {}
    for i in np.nonzero(inside)[0]:
        cells.setdefault(tuple(int(R.cell_f(p[i, k], lo3[k], v3[k])) for k in range(3)), []).append(int(i))
    src, dst, dd = [], [], []
    for i in np.nonzero(inside)[0]:
        rng = [R.scan_range(p[i, k], lo3[k], v3[k], int(dims3[k]), eps) for k in range(3)]
        cand = []
        for x in range(rng[0][0], rng[0][1] + 1):
            for y in range(rng[1][0], rng[1][1] + 1):
                for z in range(rng[2][0], rng[2][1] + 1):
                    cand += cells.get((x, y, z), ())
        cand = np.array([j for j in cand if j != i], np.int64)
        if len(cand):
            d2 = R.d2_rows(p[np.concatenate([[i], cand])], np.array([0]))[0, 1:]
            hit = d2 <= r2
            src.append(np.full(int(hit.sum()), i, np.int64)); dst.append(cand[hit]); dd.append(d2[hit])
    cat = lambda xs, t: np.concatenate(xs) if xs else np.zeros(0, t)
    return inside, cat(src, np.int64), cat(dst, np.int64), cat(dd, F32)


def cluster_walk(key, min_points):
    """cluster_one's result for the construction `key` by the independent route."""
    p, grid, eps = _CLOUDS[key]
    n = len(p)
    inside, src, dst, dd = _walk_edges(key)
    count = np.bincount(src, minlength=n)
    core = inside & (count >= min_points)
    e = core[src] & core[dst]
    lab = np.arange(n)
    for _ in range(n + 1):                                                    # min-label propagation with pointer jumping
        new = lab.copy()
        np.minimum.at(new, src[e], lab[dst[e]])
        new = new[new]
        if np.array_equal(new, lab):
            break
        lab = new
    near = np.full(n, -1, np.int64)
    b = ~core[src] & core[dst]
    order = np.lexsort((dst[b], dd[b], src[b]))                               # per source: by (d2, row)
    s, first = np.unique(src[b][order], return_index=True)
    near[s] = dst[b][order][first]
    return _finish(n, inside, core, lab, near, min_points, count)


def _span(off, b, counts, max_per_sample):
    return R._span(off, b, counts, max_per_sample)


def cluster_ragged(points, offsets, grid, eps, min_points, max_per_sample, counts=None):
    """The ragged labels call -> dict(labels, sizes, count i32 [T], num_clusters i32 [B], untouched bool [T])."""
    p = np.asarray(points, F32).reshape(-1, 3)
    off = [int(o) for o in offsets]
    T, B = len(p), len(off) - 1
    out = dict(labels=np.zeros(T, np.int32), sizes=np.zeros(T, np.int32), count=np.zeros(T, np.int32), num_clusters=np.zeros(B, np.int32),
               untouched=np.ones(T, bool))
    for b in range(B):
        n = _span(off, b, counts, max_per_sample)
        one = cluster_one(p[off[b]:off[b] + n], grid, eps, min_points)
        for k in ("labels", "sizes", "count"):
            out[k][off[b]:off[b] + n] = one[k]
        out["num_clusters"][b] = one["num_clusters"]
        out["untouched"][off[b]:off[b] + n] = False
    return out


def filter_ragged(points, offsets, grid, eps, min_points, min_cluster_size, max_per_sample, counts=None, largest_only=False, labelled=None,
                  count_border=True):
    """The ragged filter -> dict(points f32 [M,3], offsets i64 [B+1], index i64 [M], labels i32 [M], num_clusters i32 [B]).  labelled:
    cluster_ragged's result for the same arguments, where the caller has it already."""
    p = np.asarray(points, F32).reshape(-1, 3)
    off = [int(o) for o in offsets]
    r = cluster_ragged(p, off, grid, eps, min_points, max_per_sample, counts) if labelled is None else labelled
    pts, idx, labs, out_off = [], [], [], [0]
    for b in range(len(off) - 1):
        n = _span(off, b, counts, max_per_sample)
        lab, sizes, C = r["labels"][off[b]:off[b] + n], r["sizes"][off[b]:off[b] + n], int(r["num_clusters"][b])
        keep = lab >= 0
        keep[keep] = sizes[lab[keep]] >= min_cluster_size
        if largest_only:
            keep &= (lab == int(np.argmax(sizes[:C]))) if C else False        # the first of equal maxima: the smallest id
        keep = np.nonzero(keep)[0]
        pts.append(p[off[b] + keep]); idx.append(keep.astype(np.int64)); labs.append(lab[keep])
        out_off.append(out_off[-1] + len(keep))
    return dict(points=np.concatenate(pts) if pts else np.zeros((0, 3), F32), offsets=np.array(out_off, np.int64),
                index=np.concatenate(idx) if idx else np.zeros(0, np.int64), labels=np.concatenate(labs) if labs else np.zeros(0, np.int32),
                num_clusters=r["num_clusters"])


# ---- the clouds of the tests: each -> (points f32 [n,3], grid (lo3, v3, dims3) with v = eps, eps) -----------------------------------
EPS = 0.125                                                                    # a power of two: k * EPS and EPS * EPS are exact


def _line_grid(n_cells, rows=3):
    return (-EPS,) * 3, (EPS,) * 3, (n_cells + 3, rows + 2, 3)


def chain_cloud(order="ascending", n=2500, seed=7):
    """A lattice line with spacing exactly eps (d2 = r2 between neighbours): ONE component, at min_points = 2 with two border ends."""
    k = np.arange(n)
    if order == "descending":
        k = k[::-1]
    elif order == "shuffled":
        k = np.random.RandomState(seed).permutation(n)
    p = np.zeros((n, 3), F32)
    p[:, 0] = k.astype(F32) * F32(EPS)
    return p, _line_grid(n), EPS


def two_chains_cloud(n=1250, seed=8):
    """Two such lines side by side, eps * (1 + 2^-22) apart: fl of that gap's square lies above r2, so they must not merge."""
    k = np.random.RandomState(seed).permutation(2 * n)
    p = np.zeros((2 * n, 3), F32)
    p[:, 0] = (k % n).astype(F32) * F32(EPS)
    p[:, 1] = np.where(k >= n, F32(EPS) * F32(1.0 + 2.0 ** -22), F32(0)).astype(F32)
    return p, _line_grid(n), EPS


def border_tie_cloud(gadgets=100, seed=9):
    """Per gadget, on one lattice line: 6 duplicates at -eps, one row at 0, one at eps, one at 2 eps, 6 duplicates at 3 eps.  With
    min_points = 4 the rows at 0 and 2 eps are core rows of two clusters (7 neighbours each), the row at eps has those two alone and is
    a border row at d2 = r2 from both; the rows are shuffled, so either of the two has the smaller index."""
    xs = np.array([-1] * 6 + [0, 1, 2] + [3] * 6)
    p = np.zeros((gadgets * len(xs), 3), F32)
    for g in range(gadgets):
        p[g * len(xs):(g + 1) * len(xs), 0] = ((xs + 1).astype(F32) * F32(EPS))
        p[g * len(xs):(g + 1) * len(xs), 1] = F32(4 * g) * F32(EPS)
    p = p[np.random.RandomState(seed).permutation(len(p))]
    return p, ((-EPS,) * 3, (EPS,) * 3, (8, 4 * gadgets + 2, 3)), EPS


def clique_cloud(n=1500):
    """n duplicates of one point: every row sees n - 1 others at d2 = 0."""
    return np.full((n, 3), 0.3, F32), R.cube_grid(0.0, 1.0, EPS), EPS


def many_cloud(seed=10, n=2000, eps=0.02):
    """A sparse uniform cloud: at min_points = 0 most rows are a cluster of their own, more than 1024 in all."""
    rs = np.random.RandomState(seed)
    return rs.uniform(0, 1, size=(n, 3)).astype(F32), R.cube_grid(0.0, 1.0, eps), eps


# name -> (the cloud, the min_points the tests run it at)
CASES = {
    "chain_ascending": (lambda: chain_cloud("ascending"), (0, 2)),
    "chain_descending": (lambda: chain_cloud("descending"), (2,)),
    "chain_shuffled": (lambda: chain_cloud("shuffled"), (0, 2)),
    "two_chains": (two_chains_cloud, (0, 2)),
    "border_tie": (border_tie_cloud, (4,)),
    "clique": (clique_cloud, (0, 4, 1499, 1500)),
    "many": (many_cloud, (0, 1)),
}
# radius_ref's clouds; three of them thinner than its defaults (at those the cloud is ONE cluster without noise at min_points = 4), so
# that each has several clusters, border rows and noise rows (test_cluster_host.py asserts it)
_THINNER = dict(lattice=lambda: R.lattice_cloud(side=14), lattice_ulp=lambda: R.lattice_ulp_cloud(side=14), faces=lambda: R.faces_cloud(n=700))
for _name, _make in R.CONSTRUCTIONS.items():
    CASES[_name] = (_THINNER.get(_name, _make), (0, 1, 4))
CASE_IDS = [(name, mp) for name, (_, mps) in CASES.items() for mp in mps]


class _Clouds(dict):
    def __missing__(self, key):
        p, grid, eps = CASES[key][0]()
        self[key] = (np.ascontiguousarray(p, F32), grid, eps)
        return self[key]


_CLOUDS = _Clouds()


def cloud(name):
    """(points, grid, eps) of a case, made once."""
    return _CLOUDS[name]


@functools.lru_cache(maxsize=None)
def reference(name, min_points):
    """cluster_one on a case, computed once and shared; callers leave it unchanged."""
    p, grid, eps = _CLOUDS[name]
    return cluster_one(p, grid, eps, min_points)
