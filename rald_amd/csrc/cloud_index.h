// What the operations on ragged clouds share (cloud_index.hip; voxel_reduce.hip, radius_search.hip, knn_search.hip, cloud_normals.hip,
// cloud_cluster.hip, cloud_plane.hip and cloud_icp.hip use it): the layout and the grid as two plain structs, the
// scratch carver, the spatial index, the compaction in row order with the gather of the kept rows' labels, and the device helpers of
// the cell rule, the scan range, the radius walk, the block scans, the fixed shape of the float64 sums and
// the argmax of a workgroup.
#pragma once
#include <cmath>

#include "common.h"

namespace rald {

// a ragged batch as the C ABI passes it: cloud b is rows offsets[b] .. offsets[b + 1] of points (b * n_dense .. without offsets), at most
// counts[b] and at most max_per_sample of them
struct RaggedCloud {
    const int64_t* offsets; const int32_t* counts;           // what ragged_span reads comes first, 16-byte aligned in the kernel
    int64_t n_dense, n_total, max_per_sample;                // arguments: the compiler fetches it with the fewest scalar loads
    const float* points;
    int batch;
};
// in the C ABI's argument order
inline RaggedCloud ragged_cloud(const float* points, const int64_t* offsets, const int32_t* counts, int batch, int64_t n_dense, int64_t n_total,
                                int64_t max_per_sample) {
    return RaggedCloud{offsets, counts, n_dense, n_total, max_per_sample, points, batch};
}
// the grid as the C ABI passes it, three host arrays, and as the kernels take it (cloud_grid_check makes the one from the other)
struct GridSpec { const float* lo; const float* v; const int32_t* dims; };
struct CellGrid {
    float lo[3], v[3];
    int dims[3];
    unsigned cells;
};

// rows (or sorted positions) per workgroup of a flag / rank kernel, one per thread, and the block of the fixed sum shape (below)
constexpr int CLOUD_SEG = 1024;

// ---- scratch: every operation describes its buffers once, in a layout function that takes them from a carver in order; the function
// runs on a null base for the size and on the caller's scratch for the call
struct Carver {
    char* base;
    int64_t used;
    template <typename T>
    T* take(int64_t count) {
        T* p = base ? (T*)(base + used) : nullptr;
        used += round_up(count * (int64_t)sizeof(T), 16);
        return p;
    }
};
// bytes >= need, scratch non-null and 16-byte aligned; need < 0 passes (the layout check names the size it refuses)
int scratch_check(const std::string& who, const void* scratch, int64_t bytes, int64_t need);

// ---- the spatial index: the cell key of every row and a stable radix sort of (key, row) per cloud, optionally the rows in that order
//   cell   c = floorf(fl(fl(p - lo) / v)) per axis, fp32, no contraction, inside iff 0 <= c < dims in float (NaN fails both)
//   key    (c0 * dims1 + c1) * dims2 + c2, `cells` for a row outside the grid (the largest key: outside rows sort behind every cell)
struct CloudIndex {                                          // the argument block of the index kernels
    int64_t chunk, nch_max;                                  // beside the span's fields: the sort's kernels fetch both at once
    RaggedCloud c;
    CellGrid g;
    int passes;
    unsigned* key[2]; int* idx[2];                           // [n_total] ping / pong of the sort
    unsigned* hist;                                          // [batch][256 * nch_max]
    float4* rows;                                            // [n_total] x, y, z, the row's index (its bits) in sorted order; nullable
    int64_t* out_inverse;                                    // nullable: -1 for every outside row
};
struct SortedCloud { const unsigned* key; const int* idx; const float4* rows; };   // every cloud's pairs at its own span, ascending key
// the layout and grid rules of every entry (messages start with `who`); *g the grid for the kernels
int cloud_grid_check(const std::string& who, const RaggedCloud& c, const GridSpec& grid, int64_t chunk, CellGrid* g);
// the index's share of the scratch, the first of every operation; chunk 0 = the automatic rule
void cloud_index_layout(CloudIndex& ix, const RaggedCloud& c, Carver& s, int64_t chunk, bool rows);
SortedCloud cloud_index_build(CloudIndex& ix, const CellGrid& g, int64_t* out_inverse, hipStream_t st);

bool cloud_sizes_ok(int B, int64_t n_total, int64_t max_per_sample, int64_t chunk);
// the bytes `layout(args, index, carver, chunk)` takes for a batch of these sizes, -1 for sizes the calls refuse
template <typename Args, typename Layout>
int64_t layout_bytes(int B, int64_t n_total, int64_t max_per_sample, int64_t chunk, Layout layout) {
    if (!cloud_sizes_ok(B, n_total, max_per_sample, chunk)) return -1;
    Args a{};
    a.c = ragged_cloud(nullptr, nullptr, nullptr, B, 0, n_total, max_per_sample);
    CloudIndex ix{};
    Carver s{nullptr, 0};
    layout(a, ix, s, chunk);
    return s.used;
}

// ---- the compaction: per-cloud block counts -> exclusive scan per cloud -> out_offsets over the batch
struct BlockScan {
    int64_t nseg_max;
    int* blocks;                                             // [batch][nseg_max] counts per block of CLOUD_SEG, then their exclusive scan
    int* total;                                              // [batch] per cloud
    int64_t* out_offsets;                                    // [batch + 1]
};
void block_scan_layout(BlockScan& sc, const RaggedCloud& c, Carver& s);
// after a kernel has left the block counts: the two scans
void block_scan_launch(const RaggedCloud& c, const BlockScan& sc, hipStream_t st);
// row i of a cloud is kept iff keep[row0 + i] >= at_least (a 0 / 1 flag: at_least = 1), in row order; out_index nullable.  Nothing is
// checked: the layout is one cloud_grid_check has accepted
void compact_rows_ragged(const RaggedCloud& c, BlockScan sc, const int32_t* keep, int at_least, float* out_points, int64_t* out_index,
                         hipStream_t st);
// behind a compaction that left out_offsets and the kept rows' indices: out_labels[kept row] = labels[its row]
void cloud_kept_labels_ragged(const RaggedCloud& c, const int64_t* out_offsets, const int64_t* kept, const int32_t* labels, int32_t* out_labels,
                              hipStream_t st);

// ---- device helpers
// the cloud's first row and its number of rows: the segment, capped by counts and by the host bound, clamped into [0, n_total]
__device__ __forceinline__ int ragged_span(const RaggedCloud& c, int b, int64_t& row0) {
    const int64_t* offsets = c.offsets;                      // the five fields up front: one run of the kernel arguments, fetched at once
    const int32_t* counts = c.counts;
    const int64_t n_dense = c.n_dense, n_total = c.n_total, max_per_sample = c.max_per_sample;
    int64_t len;
    if (offsets) { row0 = offsets[b]; len = offsets[b + 1] - row0; }
    else { row0 = (int64_t)b * n_dense; len = n_dense; }
    if (counts) { const int64_t n = counts[b]; len = n < len ? n : len; }
    len = len < max_per_sample ? len : max_per_sample;
    if (row0 < 0 || row0 > n_total) { row0 = 0; len = 0; }
    len = len < n_total - row0 ? len : n_total - row0;
    return len > 0 ? (int)len : 0;                           // <= 2^24
}
// the cell of a coordinate, in float: floorf(fl(fl(p - lo) / v)), no contraction; monotone in p
__device__ __forceinline__ float voxel_cell(float p, float lo, float v) {
#pragma clang fp contract(off)
    return floorf((p - lo) / v);
}
__device__ __forceinline__ int rad_clamp(int r, int n) { return r < 0 ? 0 : (r < n ? r : n - 1); }
__device__ __forceinline__ int64_t rad_clamp(int64_t r, int64_t n) { return r < 0 ? 0 : (r < n ? r : n - 1); }
// the cell of a scan bound as an index of the grid: the cell function of the keys, clamped in float (a NaN cannot occur: p is finite)
__device__ __forceinline__ int rad_cell(float p, float lo, float v, int dims) {
    float cf = voxel_cell(p, lo, v);
    cf = fminf(fmaxf(cf, 0.f), 2147483520.f);                // the largest float below 2^31
    const int c = (int)cf;
    return c < dims ? c : dims - 1;
}
__device__ __forceinline__ float rad_d2(const float4& p, const float4& q) {
#pragma clang fp contract(off)
    const float dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
    return (dx * dx + dy * dy) + dz * dz;
}
// the scan range of a radius r: rs = fl(r * (1 + 2^-20)), then per axis cell(nextafter(p - rs, -inf)) .. cell(nextafter(p + rs, +inf)),
// clamped to the grid.  It holds every row with d2 <= fl(r * r)
__host__ __device__ __forceinline__ float scan_reach(float r) {
#pragma clang fp contract(off)
    return r * (1.f + 9.5367431640625e-07f);                 // 2^-20
}
__device__ __forceinline__ void scan_range(const CellGrid& g, const float* pc, float rs, int* c0, int* c1) {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        c0[k] = rad_cell(nextafterf(pc[k] - rs, -INFINITY), g.lo[k], g.v[k], g.dims[k]);
        c1[k] = rad_cell(nextafterf(pc[k] + rs, INFINITY), g.lo[k], g.v[k], g.dims[k]);
    }
}
// the first position in [lo, hi) of a cloud's sorted keys with key >= t
__device__ __forceinline__ int sorted_lower_bound(const unsigned* sk, int lo, int hi, unsigned t) {
    for (int s = 0; s < 32 && lo < hi; ++s) {
        const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
        if (sk[mid] < t) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
// the radius walk around the sorted row `me` of a cloud of n rows (sk, sr: its sorted keys and rows; rs = scan_reach(radius)):
// visit(q, row, d2) for every sorted position q of the scan range, in ascending key order, until it returns true.  Per (x, y) column of
// the range the z range is one key interval: a lower bound on the sorted keys, then a walk while key <= hi
template <typename Visit>
__device__ __forceinline__ void radius_walk(const CellGrid& g, float rs, const unsigned* sk, const float4* sr, int n, const float4& me,
                                            Visit visit) {
    const float pc[3] = {me.x, me.y, me.z};
    int c0[3], c1[3];
    scan_range(g, pc, rs, c0, c1);
    int from = 0;                                            // the columns come in ascending key order: a column starts behind the last
    bool done = false;
    for (int x = c0[0]; x <= c1[0] && !done; ++x) {
        for (int y = c0[1]; y <= c1[1] && !done; ++y) {
            const unsigned base = (unsigned)(((int64_t)x * g.dims[1] + y) * g.dims[2]);
            const unsigned klo = base + (unsigned)c0[2], khi = base + (unsigned)c1[2];
            int q = sorted_lower_bound(sk, from, n, klo);
            for (; q < n; ++q) {
                if (sk[q] > khi) break;
                const float4 o = sr[q];
                if (visit(q, o, rad_d2(me, o))) { done = true; break; }
            }
            from = q < n ? q : n;
        }
    }
}
__device__ __forceinline__ unsigned long long vox_lanes_below(int lane) { return (1ull << lane) - 1ull; }
// exclusive prefix over the workgroup of one value per thread; *total the sum.  sh: NT / 64 ints
template <int NT>
__device__ __forceinline__ int vox_block_excl(int v, int* sh, int tid, int* total) {
    const int lane = tid & 63, w = tid >> 6;
    int incl = v;
    for (int s = 1; s < 64; s <<= 1) {
        const int t = __shfl_up(incl, s);
        if (lane >= s) incl += t;
    }
    if (lane == 63) sh[w] = incl;
    __syncthreads();
    int base = 0, tot = 0;
    for (int i = 0; i < NT / 64; ++i) {
        const int x = sh[i];
        if (i < w) base += x;
        tot += x;
    }
    __syncthreads();
    *total = tot;
    return base + incl - v;
}
// from one boolean per thread: the thread's rank among the workgroup's true ones, and with `total` their number.  sh: NT / 64 ints; one
// barrier, which every thread of the workgroup reaches
template <int NT>
__device__ __forceinline__ int block_rank(bool f, int* sh, int tid, int* total) {
    const int lane = tid & 63, w = tid >> 6;
    const unsigned long long bm = __ballot(f);
    if (lane == 0) sh[w] = __popcll(bm);
    __syncthreads();
    if (total) {
        int s = 0;
        for (int i = 0; i < NT / 64; ++i) s += sh[i];
        *total = s;
    }
    int rank = __popcll(bm & vox_lanes_below(lane));
    for (int i = 0; i < w; ++i) rank += sh[i];
    return rank;
}

// ---- the fixed sum shape of a cloud's float64 sums (include/rald_hip.h): blocks of CLOUD_SEG consecutive rows, a
// row that does not count as +0.0; inside a block the halving tree v[i] += v[i + h], h = NT / 2 .. 1; the blocks' sums added left to
// right from +0.0.  No contraction anywhere.  icp_sums and icp_solve (cloud_icp.hip) are the hand-scheduled instance of the same
// shape - two tree levels in registers, sixteen block sums in flight - which tests/test_gpu_icp.py pins against this one by bits.
// The tree over one value per thread -> v[0], in every thread.  v: NT doubles; every thread of the workgroup calls it; the barrier
// behind the read lets the next call reuse v
template <int NT>
__device__ __forceinline__ double block_tree_sum(double x, double* v, int tid) {
#pragma clang fp contract(off)
    v[tid] = x;
    __syncthreads();
    for (int h = NT / 2; h >= 1; h >>= 1) {
        if (tid < h) v[tid] += v[tid + h];
        __syncthreads();
    }
    const double r = v[0];
    __syncthreads();
    return r;
}
// the blocks left to right: bs[0], bs[stride], .. of nseg blocks; the counts of their rows likewise
__device__ __forceinline__ double fold_blocks(const double* bs, int nseg, int64_t stride) {
#pragma clang fp contract(off)
    double s = 0.0;
    int g = 0;
    for (; g + 16 <= nseg; g += 16) {                        // sixteen loads in flight, then their adds in order: one lane runs this
        double v[16];                                        // loop, and a load behind every add would leave it waiting on each
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = bs[(g + u) * stride];
#pragma unroll
        for (int u = 0; u < 16; ++u) s = s + v[u];
    }
    for (; g < nseg; ++g) s = s + bs[g * stride];
    return s;
}
__device__ __forceinline__ int fold_blocks(const int* bc, int nseg, int64_t stride) {
    int s = 0;
    for (int g = 0; g < nseg; ++g) s += bc[g * stride];
    return s;
}
// the tree of the "larger value, else smaller index" over one (value, index) per thread; an index < 0 is no candidate.  The winner
// stands in sv[0], sc[0], valid in thread 0.  sv, sc: NT ints each
template <int NT>
__device__ __forceinline__ void block_argmax(int value, int index, int* sv, int* sc, int tid) {
    sv[tid] = value; sc[tid] = index;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (tid < s) {
            const int v = sv[tid + s], c = sc[tid + s];
            if (c >= 0 && (v > sv[tid] || (v == sv[tid] && c < sc[tid]))) { sv[tid] = v; sc[tid] = c; }
        }
        __syncthreads();
    }
}

}  // namespace rald
