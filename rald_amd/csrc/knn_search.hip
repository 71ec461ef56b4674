// k nearest other rows inside each cloud of a ragged batch, and the statistical outlier filter on their mean distance (DESIGN.md
// section 23).  The definition is in include/rald_hip.h; in short
//   inside, d2(i,j)  those of radius_search.hip
//   candidates of i  the inside rows j != i of its cloud (with max_radius: those with d2 <= r2max), ordered by (d2, j) ascending
//   knn              slot s of row i holds the s-th candidate, -1 / +inf from `found` on
//   m[i]             float64: sum over the slots in order of sqrt((double)d2) / found; +inf with found = 0, NaN outside
//   filter           keep row i iff found >= 1 and m[i] <= thr = mu + std_ratio * sigma, mu and sigma over the rows with found >= 1,
//                    their sums in one fixed shape: 1024-row blocks in row order, a halving tree inside a block, the blocks left to right
// The index is cloud_index_build's (cell key, row) order and its sorted copy of the rows (cloud_index.h).  Launches behind it, all on
// one stream, none waits on another workgroup, no atomics:
//   knn_search       (128 sorted positions, cloud)  one lane per SORTED position; its best-k list lies in LDS ([slot][lane], k * 8 bytes
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
#include "cloud_index.h"
#include "kernels.h"

namespace rald {

namespace {

constexpr int KNN_T = 128;                                   // sorted positions per workgroup of knn_search
constexpr int KNN_SEG = 1024;                                // rows per block of the fixed sum shape
constexpr int KNN_AHEAD = 4;                                 // rows of a key interval whose loads are issued together
constexpr int KNN_PASSES = 40;                               // boxes per lane: the own cell, <= 32 doublings, two boxes by the rule

struct KnnArgs {
    RaggedCloud c;
    CellGrid g;
    int64_t nseg_max;
    int k;
    float r2lim;                                             // r2max, +inf without max_radius
    int bounded;                                             // max_radius given
    double std_ratio;
    const unsigned* skey; const float4* srow;                // [n_total] the sorted keys and rows
    int64_t* out_idx; float* out_dist2; int32_t* out_found;  // the tables, per input row
    double* mean; int32_t* found;                            // the filter: per input row, in place of the tables
    double* bsum; int* bcnt;                                 // [batch][nseg_max]
    double* stats;                                           // [batch][4] mu, sigma, thr, n_f
    double* out_stats;                                       // [batch][3], nullable
    BlockScan sc;                                            // the filter's compaction
};

// (d, j) comes before (wd, wj)
__device__ __forceinline__ bool knn_before(float d, int j, float wd, int wj) { return d < wd || (d == wd && j < wj); }

// the cells that hold every row with d2 <= w: the scan range for a float r with fl(r * r) >= w
__device__ __forceinline__ void knn_need(const KnnArgs& a, const float* pc, float w, int* n0, int* n1) {
#pragma clang fp contract(off)
    float r = sqrtf(w);
    bool ok = false;
    for (int s = 0; s < 4 && !ok; ++s) {
        if (r * r >= w) ok = true;
        else r = nextafterf(r, INFINITY);
    }
    if (!ok) r = INFINITY;                                   // the whole grid
    scan_range(a.g, pc, scan_reach(r), n0, n1);
}

__global__ __launch_bounds__(KNN_T) void knn_search(KnnArgs a) {
    extern __shared__ float knn_lds[];
    float* D = knn_lds + threadIdx.x;                        // slot s: D[s * KNN_T], J[s * KNN_T]
    int* J = (int*)(knn_lds + a.k * KNN_T) + threadIdx.x;
    const int b = blockIdx.y;
    int64_t row0;
    const int n = ragged_span(a.c, b, row0);
    const int64_t j = (int64_t)blockIdx.x * KNN_T + threadIdx.x;
    if (j >= n) return;                                      // no barrier below
    const unsigned* sk = a.skey + row0;
    const float4* sr = a.srow + row0;
    const unsigned key = sk[j];
    const float4 me = sr[j];
    const int i = rad_clamp(__float_as_int(me.w), n);
    const int64_t g = row0 + i;
    const int k = a.k;
    int cnt = -1;
    if (key < a.g.cells) {
        cnt = 0;
        float wd = INFINITY;                                 // the list's worst pair once it is full; before, everything enters
        int wj = 0x7fffffff;
        const float pc[3] = {me.x, me.y, me.z};
        const unsigned d2u = (unsigned)a.g.dims[2], plane = (unsigned)a.g.dims[1] * d2u;
        int c[3];
        c[0] = (int)(key / plane);
        const unsigned rem = key - (unsigned)c[0] * plane;
        c[1] = (int)(rem / d2u);
        c[2] = (int)(rem - (unsigned)c[1] * d2u);
        int c0[3], c1[3], o0[3] = {1, 1, 1}, o1[3] = {0, 0, 0};   // the box to scan; the box already scanned (empty)
        // the first box: the row's own cell where that holds more than 4 k rows (seen from the sorted keys 4 k places away: its k nearest
        // then lie within a fraction of a cell), else the cells around it as well - a cell with barely k rows gives a loose bound and a
        // wide second box.  Any first box gives the same result; this one is a matter of time alone
        const int far = 4 * k;
        int64_t R = (j + far < n && sk[j + far] == key) || (j >= far && sk[j - far] == key) ? 0 : 1;
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            c0[t] = c[t] - R > 0 ? (int)(c[t] - R) : 0;
            c1[t] = c[t] + R < a.g.dims[t] ? (int)(c[t] + R) : a.g.dims[t] - 1;
        }
        // at most 1 + 32 + 2 boxes (the first box, the doublings, two boxes by the rule), so KNN_PASSES never
        // runs out; if a change to the sequence of boxes made it, the row says so with found = -2 instead of a list that is not final
        bool settled = false;
        for (int pass = 0; pass < KNN_PASSES; ++pass) {
            const unsigned zspan = (unsigned)(c1[2] - c0[2]);
            int q = 0;
            for (int x = c0[0]; x <= c1[0];) {
                const unsigned pbase = (unsigned)x * plane;
                const unsigned khi = pbase + (unsigned)c1[1] * d2u + (unsigned)c1[2];
                int y = c0[1];
                unsigned cur_lo = pbase + (unsigned)y * d2u + (unsigned)c0[2], cur_hi = cur_lo + zspan;
                const bool xold = x >= o0[0] && x <= o1[0];
                q = sorted_lower_bound(sk, q, n, cur_lo);
                while (q < n) {                              // every turn moves q on, or lands on a row it then takes
                    const unsigned kq = sk[q];
                    if (kq > cur_hi) {
                        if (kq > khi) break;
                        const unsigned rel = kq - pbase;
                        unsigned yk = rel / d2u;
                        if (rel - yk * d2u > (unsigned)c1[2]) ++yk;   // behind the column's range: the next column (<= c1[1], as kq <= khi)
                        y = (int)yk;
                        cur_lo = pbase + yk * d2u + (unsigned)c0[2];
                        cur_hi = cur_lo + zspan;
                        if (kq < cur_lo) q = sorted_lower_bound(sk, q + 1, n, cur_lo);
                        continue;
                    }
                    // up to KNN_AHEAD rows of this key interval at a time, their loads in flight together (a row far from the rest walks
                    // thousands of rows alone: the walk is bound by the latency of one load after the other)
                    unsigned kk[KNN_AHEAD];
                    float4 oo[KNN_AHEAD];
                    kk[0] = kq;
#pragma unroll
                    for (int u = 0; u < KNN_AHEAD; ++u) {
                        const int qu = q + u < n ? q + u : n - 1;
                        if (u) kk[u] = sk[qu];
                        oo[u] = sr[qu];
                    }
                    bool go = true;
                    int took = 0;
#pragma unroll
                    for (int u = 0; u < KNN_AHEAD; ++u) {
                        go = go && (u == 0 || (q + u < n && kk[u] <= cur_hi));   // sorted keys: >= cur_lo already
                        if (!go) continue;
                        ++took;
                        const int z = (int)(kk[u] - cur_lo) + c0[2];
                        if (xold && y >= o0[1] && y <= o1[1] && z >= o0[2] && z <= o1[2]) continue;   // scanned with an earlier box
                        const float4 o = oo[u];
                        const int jr = rad_clamp(__float_as_int(o.w), n);
                        const float d2 = rad_d2(me, o);
                        if (jr != i && d2 <= a.r2lim && knn_before(d2, jr, wd, wj)) {
                            int pos = cnt < k ? cnt : k - 1;
                            while (pos > 0) {
                                const float pd = D[(pos - 1) * KNN_T];
                                const int pj = J[(pos - 1) * KNN_T];
                                if (!knn_before(d2, jr, pd, pj)) break;
                                D[pos * KNN_T] = pd;
                                J[pos * KNN_T] = pj;
                                --pos;
                            }
                            D[pos * KNN_T] = d2;
                            J[pos * KNN_T] = jr;
                            if (cnt < k) ++cnt;
                            if (cnt == k) { wd = D[(k - 1) * KNN_T]; wj = J[(k - 1) * KNN_T]; }
                        }
                    }
                    q += took;
                }
                if (q >= n) break;
                const int xn = (int)(sk[q] / plane);          // the next plane that holds a row (an outside row's key: behind the grid)
                x = xn > x + 1 ? xn : x + 1;
            }
            // the rule: stop when the scanned box holds the scan range of the bound on the wanted candidates, or the whole grid
            bool whole = true;
#pragma unroll
            for (int t = 0; t < 3; ++t) whole = whole && c0[t] == 0 && c1[t] == a.g.dims[t] - 1;
            if (whole) { settled = true; break; }
            int m0[3], m1[3];
            const bool bound = cnt == k || a.bounded;
            if (bound) {                                     // the scanned box and the range of the bound
                int n0[3], n1[3];
                knn_need(a, pc, cnt == k ? wd : a.r2lim, n0, n1);
                bool held = true;
#pragma unroll
                for (int t = 0; t < 3; ++t) {
                    held = held && n0[t] >= c0[t] && n1[t] <= c1[t];
                    m0[t] = n0[t] < c0[t] ? n0[t] : c0[t];
                    m1[t] = n1[t] > c1[t] ? n1[t] : c1[t];
                }
                if (held) { settled = true; break; }
            }
            if (cnt < k) {                                   // the list is not full: twice as wide, inside the range of r2max if there is one
                R = R == 0 ? 1 : (R < (1ll << 31) ? 2 * R : R);
#pragma unroll
                for (int t = 0; t < 3; ++t) {
                    const int w0 = c[t] - R > 0 ? (int)(c[t] - R) : 0;
                    const int w1 = c[t] + R < a.g.dims[t] ? (int)(c[t] + R) : a.g.dims[t] - 1;
                    m0[t] = bound && m0[t] > w0 ? m0[t] : w0;
                    m1[t] = bound && m1[t] < w1 ? m1[t] : w1;
                }
            }
#pragma unroll
            for (int t = 0; t < 3; ++t) { o0[t] = c0[t]; o1[t] = c1[t]; c0[t] = m0[t]; c1[t] = m1[t]; }
        }
        if (!settled) cnt = -2;
    }
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
__global__ __launch_bounds__(KNN_SEG) void knn_block_sums(KnnArgs a, int pass) {
#pragma clang fp contract(off)
    __shared__ double v[KNN_SEG];
    __shared__ int sh[KNN_SEG / 64];
    const int b = blockIdx.y, tid = threadIdx.x;
    int64_t row0;
    const int n = ragged_span(a.c, b, row0);
    const int64_t j = (int64_t)blockIdx.x * KNN_SEG + tid;
    if ((int64_t)blockIdx.x * KNN_SEG >= n) return;          // the whole workgroup
    const bool counts = j < n && a.found[row0 + j] >= 1;
    double x = 0.0;                                          // a row that does not count, and the padding: +0.0
    if (counts) {
        x = a.mean[row0 + j];
        if (pass) {
            const double d = x - a.stats[b * 4];
            x = d * d;
        }
    }
    v[tid] = x;
    const unsigned long long bm = __ballot(counts);
    if ((tid & 63) == 0) sh[tid >> 6] = __popcll(bm);
    __syncthreads();
    for (int h = KNN_SEG / 2; h >= 1; h >>= 1) {
        if (tid < h) v[tid] += v[tid + h];
        __syncthreads();
    }
    if (tid == 0) {
        int s = 0;
        for (int w = 0; w < KNN_SEG / 64; ++w) s += sh[w];
        a.bsum[(int64_t)b * a.nseg_max + blockIdx.x] = v[0];
        if (!pass) a.bcnt[(int64_t)b * a.nseg_max + blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(64) void knn_cloud_stats(KnnArgs a, int pass) {
#pragma clang fp contract(off)
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.c.batch) return;
    int64_t row0;
    const int n = ragged_span(a.c, b, row0);
    const int nseg = (n + KNN_SEG - 1) / KNN_SEG;
    double* st = a.stats + b * 4;
    double s = 0.0;
    for (int gk = 0; gk < nseg; ++gk) s += a.bsum[(int64_t)b * a.nseg_max + gk];
    if (!pass) {
        int64_t nf = 0;
        for (int gk = 0; gk < nseg; ++gk) nf += a.bcnt[(int64_t)b * a.nseg_max + gk];
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

void knn_layout(KnnArgs& a, CloudIndex& ix, Carver& s, int64_t chunk) { cloud_index_layout(ix, a.c, s, chunk, true); }

void stat_layout(KnnArgs& a, CloudIndex& ix, Carver& s, int64_t chunk) {
    knn_layout(a, ix, s, chunk);
    a.nseg_max = (a.c.max_per_sample + KNN_SEG - 1) / KNN_SEG;
    a.mean = s.take<double>(a.c.n_total);
    a.found = s.take<int32_t>(a.c.n_total);
    block_scan_layout(a.sc, a.c, s);
    a.bsum = s.take<double>(a.c.batch * a.nseg_max);
    a.bcnt = s.take<int>(a.c.batch * a.nseg_max);
    a.stats = s.take<double>((int64_t)a.c.batch * 4);
}

// the checks of both entries that the index does not make, then the scratch by the entry's layout, the index and the search
template <typename Layout>
int knn_run(const std::string& who, KnnArgs& a, const RaggedCloud& c, const GridSpec& grid, int k, float max_radius, Layout layout, int64_t need,
            double* out_mean, void* scratch, int64_t scratch_bytes, int64_t chunk, hipStream_t st) {
    RALD_CHECK(grid.lo && grid.v && grid.dims, who + ": null grid (lo3, v3, dims3)");
    RALD_CHECK(k >= 1 && k <= 32, who + ": k must be 1 .. 32");
    RALD_CHECK(max_radius == 0.f || (std::isfinite(max_radius) && max_radius > 0.f), who + ": max_radius must be 0 (none) or finite and > 0");
    RALD_TRY(scratch_check(who, scratch, scratch_bytes, need));
    RALD_TRY(cloud_grid_check(who, c, grid, chunk, &a.g));
    a.c = c;
    CloudIndex ix;
    Carver s{(char*)scratch, 0};
    layout(a, ix, s, chunk);
    if (out_mean) a.mean = out_mean;
    a.k = k;
    a.bounded = max_radius > 0.f;
    a.r2lim = a.bounded ? max_radius * max_radius : INFINITY;
    const SortedCloud sorted = cloud_index_build(ix, a.g, nullptr, st);
    a.skey = sorted.key; a.srow = sorted.rows;
    const dim3 by_pos((unsigned)((c.max_per_sample + KNN_T - 1) / KNN_T), c.batch);
    hipLaunchKernelGGL(knn_search, by_pos, dim3(KNN_T), (size_t)k * KNN_T * 8, st, a);
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
        hipLaunchKernelGGL(knn_block_sums, by_seg, dim3(KNN_SEG), 0, st, a, pass);
        hipLaunchKernelGGL(knn_cloud_stats, dim3((c.batch + 63) / 64), dim3(64), 0, st, a, pass);
    }
    hipLaunchKernelGGL(knn_flags, dim3((unsigned)((c.max_per_sample + 255) / 256), c.batch), dim3(256), 0, st, a);
    a.sc.out_offsets = out_offsets;
    compact_rows_ragged(c, a.sc, a.found, 1, out_points, out_index, st);
    RALD_HIP(hipGetLastError());
    return 0;
}

}  // namespace rald
