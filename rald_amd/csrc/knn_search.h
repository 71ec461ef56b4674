// The k-NN search of one lane over the grid index, shared by the kernels that end it differently: knn_search
// (knn_search.hip: the tables, or the mean distance of the statistical filter) and normals_search (cloud_normals.hip: the moments of the
// neighbourhood).  Each entry inlines knn_search_lane and then reads its own best-k list from LDS; the arguments, the checks and the
// index build of a call are knn_prepare's.
#pragma once
#include "cloud_index.h"
#include "kernels.h"

namespace rald {

namespace {

constexpr int KNN_T = 128;                                   // sorted positions per workgroup of a search kernel
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

// what a lane of a search kernel knows once its search is over
struct KnnLane {
    float* D; int* J;                                        // its list: slot s at D[s * KNN_T], J[s * KNN_T], ordered by (d2, j)
    float4 me;                                               // its row (w: the row's index, its bits)
    int64_t row0, g;                                         // the cloud's first row; the lane's input row
    int n, i;                                                // the cloud's rows; the lane's row inside its cloud (clamped)
    int cnt;                                                 // found: -1 outside, -2 for a list that is not final
    bool live;                                               // false: the position lies behind the cloud, the lane has nothing to do
};

// one lane per SORTED position (blockIdx.x * KNN_T + threadIdx.x of cloud blockIdx.y); lds: k * KNN_T * 8 bytes.  No barrier inside
__device__ __forceinline__ KnnLane knn_search_lane(const KnnArgs& a, float* lds) {
    KnnLane L;
    float* D = lds + threadIdx.x;                            // slot s: D[s * KNN_T], J[s * KNN_T]
    int* J = (int*)(lds + a.k * KNN_T) + threadIdx.x;
    L.D = D; L.J = J;
    const int b = blockIdx.y;
    int64_t row0;
    const int n = ragged_span(a.c, b, row0);
    const int64_t j = (int64_t)blockIdx.x * KNN_T + threadIdx.x;
    L.row0 = row0; L.n = n;
    L.live = j < n;
    if (!L.live) return L;
    const unsigned* sk = a.skey + row0;
    const float4* sr = a.srow + row0;
    const unsigned key = sk[j];
    const float4 me = sr[j];
    const int i = rad_clamp(__float_as_int(me.w), n);
    L.me = me; L.i = i; L.g = row0 + i;
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
    L.cnt = cnt;
    return L;
}

// the index's share of the scratch with the sorted rows: the whole layout of the search with tables, the head of every other
inline void knn_layout(KnnArgs& a, CloudIndex& ix, Carver& s, int64_t chunk) { cloud_index_layout(ix, a.c, s, chunk, true); }

// the checks of every entry that the index does not make, then the scratch by the entry's layout and the index: `a` is ready for a
// search kernel, launched over knn_search_grid with knn_search_lds bytes
template <typename Layout>
int knn_prepare(const std::string& who, KnnArgs& a, const RaggedCloud& c, const GridSpec& grid, int k, float max_radius, Layout layout, int64_t need,
                void* scratch, int64_t scratch_bytes, int64_t chunk, hipStream_t st) {
    RALD_CHECK(grid.lo && grid.v && grid.dims, who + ": null grid (lo3, v3, dims3)");
    RALD_CHECK(k >= 1 && k <= 32, who + ": k must be 1 .. 32");
    RALD_CHECK(max_radius == 0.f || (std::isfinite(max_radius) && max_radius > 0.f), who + ": max_radius must be 0 (none) or finite and > 0");
    RALD_TRY(scratch_check(who, scratch, scratch_bytes, need));
    RALD_TRY(cloud_grid_check(who, c, grid, chunk, &a.g));
    a.c = c;
    CloudIndex ix;
    Carver s{(char*)scratch, 0};
    layout(a, ix, s, chunk);
    a.k = k;
    a.bounded = max_radius > 0.f;
    a.r2lim = a.bounded ? max_radius * max_radius : INFINITY;
    const SortedCloud sorted = cloud_index_build(ix, a.g, nullptr, st);
    a.skey = sorted.key; a.srow = sorted.rows;
    return 0;
}
inline dim3 knn_search_grid(const RaggedCloud& c) { return dim3((unsigned)((c.max_per_sample + KNN_T - 1) / KNN_T), c.batch); }
inline size_t knn_search_lds(int k) { return (size_t)k * KNN_T * 8; }

}  // namespace

}  // namespace rald
