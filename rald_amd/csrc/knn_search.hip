// k nearest other rows inside each cloud of a ragged batch, and the statistical outlier filter on their mean distance (DESIGN.md
// section 23).  The definition is in include/rald_hip.h; in short
//   inside, d2(i,j)  those of radius_search.hip
//   candidates of i  the inside rows j != i of its cloud (with max_radius: those with d2 <= r2max), ordered by (d2, j) ascending
//   knn              slot s of row i holds the s-th candidate, -1 / +inf from `found` on
//   m[i]             float64: sum over the slots in order of sqrt((double)d2) / found; +inf with found = 0, NaN outside
//   filter           keep row i iff found >= 1 and m[i] <= thr = mu + std_ratio * sigma, mu and sigma over the rows with found >= 1,
//                    their sums in the fixed sum shape (cloud_index.h: block_tree_sum, fold_blocks)
// The index is cloud_index_build's (cell key, row) order and its sorted copy of the rows (cloud_index.h).  Launches behind it, all on
// one stream, none waits on another workgroup, no atomics:
//   knn_search       (128 sorted positions, cloud)  knn_search_lane of knn_search.h (cloud_normals.hip ends the same search in its own
//                                                   way), then the tables or the mean from the lane's list:
//                                                   one lane per SORTED position; its best-k list lies in LDS ([slot][lane], k * 8 bytes
//                                                   a lane), ordered by (d2, j).  It scans a first box, then the box of cells
//                                                   that the termination rule asks for (or, with no bound yet, one twice as wide), only
//                                                   the rows of the new shell, until the scanned box holds the scan range of
//                                                   cloud_index.h for a float r with fl(r * r) >= the list's worst d2 (or r2max)
//                                                   or is the whole grid.  Per x plane of the box ONE lower bound; the walk jumps
//                                                   over the keys between two columns' z ranges by a lower bound, and over empty planes.
//   the filter only, over ROW order:
//   knn_block_sums   (1024 rows, cloud)  the block's tree sum of m (pass 0) or (m - mu)^2 (pass 1), and its rows that count
//   knn_cloud_stats  one lane per cloud  the blocks left to right: mu (pass 0), sigma and thr (pass 1)
//   knn_flags        (256 rows, cloud)   1 for a kept row, 0 else, where `found` was; then cloud_index.hip's compaction on that flag
// Every loop is bounded by the cloud's length (<= max_per_sample, a host value), by the grid's dims, by k or by a constant.  A row
// index read from the scratch is clamped into the cloud before it addresses anything.
#include "knn_search.h"

namespace rald {

namespace {

__global__ __launch_bounds__(KNN_T) void knn_search(KnnArgs a) {
    extern __shared__ float knn_lds[];
    const KnnLane L = knn_search_lane(a, knn_lds);
    if (!L.live) return;
    const float* D = L.D;
    const int* J = L.J;
    const int64_t g = L.g;
    const int k = a.k, cnt = L.cnt;
    if (a.mean) {
        double m = NAN;
        if (cnt == 0) m = INFINITY;
        if (cnt > 0) {
            double s = 0.0;
            for (int t = 0; t < cnt; ++t) s += __dsqrt_rn((double)D[t * KNN_T]);
            m = s / (double)cnt;
        }
        a.mean[g] = m;
        a.found[g] = cnt;
        return;
    }
    for (int t = 0; t < k; ++t) {
        const bool have = t < cnt;
        a.out_idx[g * k + t] = have ? (int64_t)J[t * KNN_T] : -1;
        if (a.out_dist2) a.out_dist2[g * k + t] = have ? D[t * KNN_T] : INFINITY;
    }
    if (a.out_found) a.out_found[g] = cnt;
}

// ---- the filter's statistics in the fixed sum shape, over row order
__global__ __launch_bounds__(CLOUD_SEG) void knn_block_sums(KnnArgs a, int pass) {
#pragma clang fp contract(off)
    __shared__ double v[CLOUD_SEG];
    __shared__ int sh[CLOUD_SEG / 64];
    const int b = blockIdx.y, tid = threadIdx.x;
    int64_t row0;
    const int n = ragged_span(a.c, b, row0);
    const int64_t j = (int64_t)blockIdx.x * CLOUD_SEG + tid;
    if ((int64_t)blockIdx.x * CLOUD_SEG >= n) return;        // the whole workgroup
    const bool counts = j < n && a.found[row0 + j] >= 1;
    double x = 0.0;                                          // a row that does not count, and the padding: +0.0
    if (counts) {
        x = a.mean[row0 + j];
        if (pass) {
            const double d = x - a.stats[b * 4];
            x = d * d;
        }
    }
    int total;
    block_rank<CLOUD_SEG>(counts, sh, tid, &total);
    const double sum = block_tree_sum<CLOUD_SEG>(x, v, tid);
    if (tid == 0) {
        a.bsum[(int64_t)b * a.nseg_max + blockIdx.x] = sum;
        if (!pass) a.bcnt[(int64_t)b * a.nseg_max + blockIdx.x] = total;
    }
}

__global__ __launch_bounds__(64) void knn_cloud_stats(KnnArgs a, int pass) {
#pragma clang fp contract(off)
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.c.batch) return;
    int64_t row0;
    const int n = ragged_span(a.c, b, row0);
    const int nseg = (n + CLOUD_SEG - 1) / CLOUD_SEG;
    double* st = a.stats + b * 4;
    const double s = fold_blocks(a.bsum + (int64_t)b * a.nseg_max, nseg, 1);
    if (!pass) {
        const int nf = fold_blocks(a.bcnt + (int64_t)b * a.nseg_max, nseg, 1);   // <= n
        st[3] = (double)nf;
        st[0] = nf > 0 ? s / (double)nf : (double)NAN;
        return;
    }
    const double nf = st[3], mu = st[0];
    double sigma = NAN, thr = NAN;
    if (nf >= 1.0) {
        sigma = nf >= 2.0 ? __dsqrt_rn(s / (nf - 1.0)) : 0.0;
        const double t = a.std_ratio * sigma;
        thr = mu + t;
    }
    st[1] = sigma;
    st[2] = thr;
    if (a.out_stats) {
        a.out_stats[b * 3] = mu;
        a.out_stats[b * 3 + 1] = sigma;
        a.out_stats[b * 3 + 2] = thr;
    }
}

__global__ __launch_bounds__(256) void knn_flags(KnnArgs a) {
    const int b = blockIdx.y;
    int64_t row0;
    const int n = ragged_span(a.c, b, row0);
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const int64_t g = row0 + j;
    a.found[g] = a.found[g] >= 1 && a.mean[g] <= a.stats[b * 4 + 2] ? 1 : 0;
}

void stat_layout(KnnArgs& a, CloudIndex& ix, Carver& s, int64_t chunk) {
    knn_layout(a, ix, s, chunk);
    a.nseg_max = (a.c.max_per_sample + CLOUD_SEG - 1) / CLOUD_SEG;
    a.mean = s.take<double>(a.c.n_total);
    a.found = s.take<int32_t>(a.c.n_total);
    block_scan_layout(a.sc, a.c, s);
    a.bsum = s.take<double>(a.c.batch * a.nseg_max);
    a.bcnt = s.take<int>(a.c.batch * a.nseg_max);
    a.stats = s.take<double>((int64_t)a.c.batch * 4);
}

// knn_prepare, then the search into the tables or into the filter's means
template <typename Layout>
int knn_run(const std::string& who, KnnArgs& a, const RaggedCloud& c, const GridSpec& grid, int k, float max_radius, Layout layout, int64_t need,
            double* out_mean, void* scratch, int64_t scratch_bytes, int64_t chunk, hipStream_t st) {
    RALD_TRY(knn_prepare(who, a, c, grid, k, max_radius, layout, need, scratch, scratch_bytes, chunk, st));
    if (out_mean) a.mean = out_mean;
    hipLaunchKernelGGL(knn_search, knn_search_grid(c), dim3(KNN_T), knn_search_lds(k), st, a);
    return 0;
}

}  // namespace

int64_t knn_scratch_bytes(int B, int64_t n_total, int64_t max_per_sample, int64_t chunk) {
    return layout_bytes<KnnArgs>(B, n_total, max_per_sample, chunk, knn_layout);
}

int64_t statistical_scratch_bytes(int B, int64_t n_total, int64_t max_per_sample, int64_t chunk) {
    return layout_bytes<KnnArgs>(B, n_total, max_per_sample, chunk, stat_layout);
}

int knn_ragged(const RaggedCloud& c, const GridSpec& grid, int k, float max_radius, int64_t* out_idx, float* out_dist2, int32_t* out_found,
               void* scratch, int64_t scratch_bytes, int64_t chunk, hipStream_t st) {
    RALD_CHECK(c.points && out_idx, "knn_ragged: null pointer (points, out_idx)");
    KnnArgs a{};
    a.out_idx = out_idx; a.out_dist2 = out_dist2; a.out_found = out_found;
    RALD_TRY(knn_run("knn_ragged", a, c, grid, k, max_radius, knn_layout, knn_scratch_bytes(c.batch, c.n_total, c.max_per_sample, chunk), nullptr,
                     scratch, scratch_bytes, chunk, st));
    RALD_HIP(hipGetLastError());
    return 0;
}

int statistical_filter_ragged(const RaggedCloud& c, const GridSpec& grid, int k, float max_radius, double std_ratio, float* out_points,
                              int64_t* out_offsets, int64_t* out_index, double* out_mean, double* out_stats, void* scratch,
                              int64_t scratch_bytes, int64_t chunk, hipStream_t st) {
    RALD_CHECK(c.points && out_points && out_offsets, "statistical_filter_ragged: null pointer (points, out_points, out_offsets)");
    RALD_CHECK(std::isfinite(std_ratio) && std_ratio >= 0.0, "statistical_filter_ragged: std_ratio must be finite and >= 0");
    KnnArgs a{};
    a.std_ratio = std_ratio;
    a.out_stats = out_stats;
    RALD_TRY(knn_run("statistical_filter_ragged", a, c, grid, k, max_radius, stat_layout,
                     statistical_scratch_bytes(c.batch, c.n_total, c.max_per_sample, chunk), out_mean, scratch, scratch_bytes, chunk, st));
    const dim3 by_seg((unsigned)a.nseg_max, c.batch);
    for (int pass = 0; pass < 2; ++pass) {
        hipLaunchKernelGGL(knn_block_sums, by_seg, dim3(CLOUD_SEG), 0, st, a, pass);
        hipLaunchKernelGGL(knn_cloud_stats, dim3((c.batch + 63) / 64), dim3(64), 0, st, a, pass);
    }
    hipLaunchKernelGGL(knn_flags, dim3((unsigned)((c.max_per_sample + 255) / 256), c.batch), dim3(256), 0, st, a);
    a.sc.out_offsets = out_offsets;
    compact_rows_ragged(c, a.sc, a.found, 1, out_points, out_index, st);
    RALD_HIP(hipGetLastError());
    return 0;
}

}  // namespace rald
