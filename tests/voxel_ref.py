"""The definition of voxel-grid down-sampling (include/rald_hip.h) in numpy, for the tests to compare with by
equality: float32 cell arithmetic with one rounding per operation, a dictionary from key to rows, centroids added one row after the
other in float64 (never np.sum: numpy adds pairwise, and the order shows where a cell holds values of very different exponents)."""
import numpy as np

F32 = np.float32


def passes(cells: int) -> int:
    """Radix passes of 8 bits for the keys 0 .. cells (the outside key is the largest)."""
    return (int(cells).bit_length() + 7) // 8


def cells_of(points, lo3, v3, dims3):
    """-> (inside bool [n], cell int64 [n,3] (0 where outside), key int64 [n] (-1 where outside))."""
    p = np.asarray(points, F32).reshape(-1, 3)
    lo, v = np.asarray(lo3, F32), np.asarray(v3, F32)
    dims = [int(d) for d in dims3]
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.floor(((p - lo).astype(F32) / v).astype(F32))                  # float32 throughout: one rounding per operation
        inside = np.ones(len(p), bool)
        for k in range(3):
            inside &= (c[:, k] >= F32(0)) & (c[:, k] < F32(dims[k]))          # compared in float; NaN fails both
    ci = np.where(inside[:, None], np.nan_to_num(c, nan=0.0, posinf=0.0, neginf=0.0), 0).astype(np.int64)
    ci[~inside] = 0
    key = (ci[:, 0] * dims[1] + ci[:, 1]) * dims[2] + ci[:, 2]
    key[~inside] = -1
    return inside, ci, key


def voxel_one(points, lo3, v3, dims3):
    """One cloud [n,3] -> dict(points f32 [m,3], count i32 [m], first i64 [m], cells i32 [m,3], inverse i64 [n], keys i64 [m])."""
    p = np.asarray(points, F32).reshape(-1, 3)
    inside, ci, key = cells_of(p, lo3, v3, dims3)
    rows = {}
    for i in np.nonzero(inside)[0]:
        rows.setdefault(int(key[i]), []).append(int(i))                       # ascending row order
    keys = sorted(rows)
    m = len(keys)
    out = dict(points=np.zeros((m, 3), F32), count=np.zeros(m, np.int32), first=np.zeros(m, np.int64), cells=np.zeros((m, 3), np.int32),
               inverse=np.full(len(p), -1, np.int64), keys=np.array(keys, np.int64))
    p64 = p.astype(np.float64)
    for r, k in enumerate(keys):
        s = np.zeros(3, np.float64)
        for i in rows[k]:
            s = s + p64[i]                                                    # left to right
        out["points"][r] = (s / np.float64(len(rows[k]))).astype(F32)         # one rounding
        out["count"][r] = len(rows[k])
        out["first"][r] = rows[k][0]
        out["cells"][r] = ci[rows[k][0]]
        out["inverse"][rows[k]] = r
    return out


def voxel_ragged(points, offsets, lo3, v3, dims3, max_per_sample, counts=None):
    """The ragged call -> dict(points [M,3], offsets i64 [B+1], count, first, cells, inverse i64 [T] with `untouched` (bool [T]: rows
    the call must not write) beside it)."""
    p = np.asarray(points, F32).reshape(-1, 3)
    off = [int(o) for o in offsets]
    B = len(off) - 1
    parts, out_off = [], [0]
    inverse = np.full(len(p), -1, np.int64)
    untouched = np.ones(len(p), bool)
    for b in range(B):
        n = off[b + 1] - off[b]
        if counts is not None:
            n = min(n, max(int(counts[b]), 0))
        n = max(min(n, int(max_per_sample)), 0)
        one = voxel_one(p[off[b]:off[b] + n], lo3, v3, dims3)
        inverse[off[b]:off[b] + n] = one["inverse"]
        untouched[off[b]:off[b] + n] = False
        parts.append(one)
        out_off.append(out_off[-1] + len(one["count"]))
    cat = lambda k, shape, dt: np.concatenate([q[k] for q in parts]) if parts else np.zeros(shape, dt)
    return dict(points=cat("points", (0, 3), F32), offsets=np.array(out_off, np.int64), count=cat("count", 0, np.int32),
                first=cat("first", 0, np.int64), cells=cat("cells", (0, 3), np.int32), inverse=inverse, untouched=untouched)


def voxel_brute_float64(points, lo3, v3, dims3):
    """An independent route for clouds with no coordinate near a cell face: cells in float64, np.unique on them, centroids by
    np.add.at in float64 -> (cells [m,3] in ascending key order, count [m], centroid float64 [m,3], inverse [n])."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    c = np.floor((p - np.asarray(lo3, np.float64)) / np.asarray(v3, np.float64)).astype(np.int64)
    d = np.asarray(dims3, np.int64)
    inside = ((c >= 0) & (c < d)).all(axis=1)
    uniq, inv, cnt = np.unique(c[inside], axis=0, return_inverse=True, return_counts=True)    # lexicographic = ascending key
    inv = inv.reshape(-1)
    s = np.zeros((len(uniq), 3))
    np.add.at(s, inv, p[inside])
    inverse = np.full(len(p), -1, np.int64)
    inverse[inside] = inv
    return uniq, cnt, s / cnt[:, None], inverse
