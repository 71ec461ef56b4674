"""Farthest-point sampling as include/rald_hip.h defines it, in numpy float32: the reference the kernel must
match bit for bit.  numpy rounds every float32 operation and never contracts a product into a sum.

    p' = fl(p * scale);  d2(i, c) = fl(fl(fl(dx*dx) + fl(dy*dy)) + fl(dz*dz));  mind = +inf;  first choice start mod n;
    after a choice c: mind = min(mind, d2(., c));  next choice: the largest mind, the smallest index on equal values.
"""
import numpy as np


def fps_one(points, k, start=0, scale=None):
    """One cloud [n,3] -> (idx int64 [k], dist2 float32 [k]): min(n, k) choices, then -1 / NaN."""
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    n = p.shape[0]
    idx = np.full(k, -1, dtype=np.int64)
    dist = np.full(k, np.nan, dtype=np.float32)
    if n == 0:
        return idx, dist
    if scale is not None:
        p = p * np.asarray(scale, dtype=np.float32)[None, :]                      # float32 * float32, rounded once
    c = int(start) % n                                                            # Python's modulo is the non-negative one
    mind = np.full(n, np.inf, dtype=np.float32)
    idx[0], dist[0] = c, np.inf
    for j in range(1, min(k, n)):
        d = p - p[c]
        d = d * d
        d2 = (d[:, 0] + d[:, 1]) + d[:, 2]
        mind = np.minimum(mind, d2)
        c = int(np.argmax(mind))                                                  # the first (smallest) index of the maximum
        idx[j], dist[j] = c, mind[c]
    return idx, dist


def fps_ragged(points, offsets, k, max_per_sample, counts=None, start=None, scale=None):
    """points [T,3], offsets [B+1] -> (idx int64 [B,k], dist2 float32 [B,k]).  counts: valid rows per cloud (capped at the segment);
    a cloud longer than max_per_sample is sampled from its first max_per_sample rows."""
    points = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    offsets = np.asarray(offsets, dtype=np.int64)
    B = len(offsets) - 1
    idx = np.empty((B, k), dtype=np.int64)
    dist = np.empty((B, k), dtype=np.float32)
    for b in range(B):
        n = int(offsets[b + 1] - offsets[b])
        if counts is not None:
            n = min(n, int(counts[b]))
        n = max(0, min(n, int(max_per_sample)))
        idx[b], dist[b] = fps_one(points[offsets[b]:offsets[b] + n], k, 0 if start is None else int(start[b]), scale)
    return idx, dist


def fps_dense(points, k, start=None, scale=None):
    points = np.asarray(points, dtype=np.float32)
    B, N = points.shape[0], points.shape[1]
    return fps_ragged(points.reshape(-1, 3), np.arange(B + 1, dtype=np.int64) * N, k, N, None, start, scale)


def fps_brute_float64(points, k, start=0):
    """The same greedy choice by brute force in float64 and plain Python comparisons: the distance of every point to every chosen
    one, the farthest by a strict > scan from index 0.  Agrees with fps_one index for index wherever float32 is exact."""
    p = [tuple(float(v) for v in row) for row in np.asarray(points, dtype=np.float64).reshape(-1, 3)]
    n = len(p)
    chosen = [int(start) % n]
    dist = [float("inf")]
    while len(chosen) < min(k, n):
        best, best_i = -1.0, -1
        for i in range(n):
            m = min((p[i][0] - p[c][0]) ** 2 + (p[i][1] - p[c][1]) ** 2 + (p[i][2] - p[c][2]) ** 2 for c in chosen)
            if m > best:
                best, best_i = m, i
        chosen.append(best_i)
        dist.append(best)
    return chosen, dist


def resample_ref(points, offsets, k, max_per_sample, counts=None, start=None, scale=None):
    """resample_points_ragged(pad='repeat'): [B,k,3] float32; slot j >= n of a short cloud takes slot j mod n, an empty cloud NaN."""
    points = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    idx, _ = fps_ragged(points, offsets, k, max_per_sample, counts, start, scale)
    out = np.full((idx.shape[0], k, 3), np.nan, dtype=np.float32)
    for b in range(idx.shape[0]):
        m = int((idx[b] >= 0).sum())
        for j in range(k if m else 0):
            out[b, j] = points[offsets[b] + idx[b, j % m]]
    return out, idx
