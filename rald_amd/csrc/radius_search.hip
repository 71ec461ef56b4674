// Fixed-radius neighbour search inside each cloud of a ragged batch, and the radius outlier filter on it.  The
// definition is in include/rald_hip.h; in short
//   inside   the cell rule of voxel_reduce.hip: c = floorf(fl(fl(p - lo) / v)) per axis, 0 <= c < dims in float
//   d2(i,j)  fl(fl(fl(dx*dx) + fl(dy*dy)) + fl(dz*dz)), dx = fl(p_j.x - p_i.x): fp32, no contraction
//   count[i] the inside rows j != i of the same cloud with d2(i,j) <= r2 = fl(radius * radius), min(count, cap) with a cap; -1 outside
//   nearest  the j of the smallest d2 among them, the smallest j on equal d2
//   filter   keep row i iff count[i] >= min_neighbors, in row order
// The grid is only the index: voxel_sort_ragged (voxel_reduce.hip) leaves every cloud's (cell key, row) pairs in ascending key order.
// Launches behind it, all on one stream, none waits on another workgroup:
//   rad_gather      (256 sorted positions, cloud)  the coordinates in sorted order, 16 bytes a row: x, y, z, the row's index
//   rad_count       (256 sorted positions, cloud)  one lane per SORTED position, so a wave's lanes are neighbours in space and walk the
//                                                  same lines.  The lane's scan range per axis is cell(nextafter(p - rs, -inf)) ..
//                                                  cell(nextafter(p + rs, +inf)), rs = fl(radius * (1 + 2^-20)), clamped to the grid; per
//                                                  (x, y) column of it the z range is one key interval: a lower bound on the cloud's
//                                                  sorted keys, then a walk while key <= hi.  The result goes back to the row's place.
//   the filter only, over ROW order:
//   rad_flags       (1024 rows, cloud)   kept rows per block
//   rad_block_scan  (cloud)              exclusive scan of the block counts in place, the cloud's kept rows
//   rad_offsets     one workgroup        out_offsets = exclusive scan of the kept counts over the batch
//   rad_compact     (1024 rows, cloud)   a kept row to out_offsets[b] + its rank
// knn_search.hip uses rad_gather and the four compaction kernels through radius_gather_sorted and
// radius_compact_ragged (kernels.h), and the device helpers rad_clamp / rad_cell / rad_d2 that live there.
// No atomics at all.  Every loop is bounded by the cloud's length (<= max_per_sample, a host value), by the grid's dims (host values) or
// by 32.  A row index read from the scratch is clamped into the cloud before it addresses anything.
#include <cmath>

#include "common.h"
#include "kernels.h"

namespace rald {

namespace {

constexpr int RAD_T = 256;                                   // sorted positions per workgroup of rad_gather / rad_count
constexpr int RAD_SEG = 1024;                                // rows per workgroup of the compaction (one per thread)

struct RadiusArgs {
    const float* points; const int64_t* offsets; const int32_t* counts;
    int64_t n_dense, n_total, max_per_sample, nseg_max;
    float lo[3], v[3];
    int dims[3];
    unsigned cells;
    float r2, rs;
    int cap;                                                 // 0 = none; the walk stops at it
    int min_neighbors;
    const unsigned* skey; const int* sidx;                   // [n_total] the sorted pairs
    float4* srow;                                            // [n_total] x, y, z, row in sorted order
    int32_t* cnt;                                            // [n_total] per row
    int64_t* nn_idx; float* nn_dist2;                        // per row, nullable
    int* blocks;                                             // [batch][nseg_max]
    int* total;                                              // [batch] kept rows per cloud
    int batch;
    float* out_points; int64_t* out_offsets; int64_t* out_index;
};

__device__ __forceinline__ int rad_span(const RadiusArgs& a, int b, int64_t& row0) {
    return ragged_span(a.offsets, a.counts, a.n_dense, a.n_total, a.max_per_sample, b, row0);
}

__global__ __launch_bounds__(RAD_T) void rad_gather(RadiusArgs a) {
    const int b = blockIdx.y;
    int64_t row0;
    const int n = rad_span(a, b, row0);
    const int64_t j = (int64_t)blockIdx.x * RAD_T + threadIdx.x;
    if (j >= n) return;
    const int r = rad_clamp(a.sidx[row0 + j], n);
    const float* p = a.points + (row0 + r) * 3;
    a.srow[row0 + j] = make_float4(p[0], p[1], p[2], __int_as_float(r));
}

__global__ __launch_bounds__(RAD_T) void rad_count(RadiusArgs a) {
    const int b = blockIdx.y;
    int64_t row0;
    const int n = rad_span(a, b, row0);
    const int64_t j = (int64_t)blockIdx.x * RAD_T + threadIdx.x;
    if (j >= n) return;
    const unsigned* sk = a.skey + row0;
    const float4* sr = a.srow + row0;
    const unsigned key = sk[j];
    const float4 me = sr[j];
    const int i = rad_clamp(__float_as_int(me.w), n);
    const int64_t g = row0 + i;
    int count = -1, bestj = -1;
    float best = INFINITY;
    if (key < a.cells) {
        count = 0;
        const float pc[3] = {me.x, me.y, me.z};
        int c0[3], c1[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            c0[k] = rad_cell(nextafterf(pc[k] - a.rs, -INFINITY), a.lo[k], a.v[k], a.dims[k]);
            c1[k] = rad_cell(nextafterf(pc[k] + a.rs, INFINITY), a.lo[k], a.v[k], a.dims[k]);
        }
        int from = 0;                                        // the columns come in ascending key order: a column starts behind the last
        bool done = false;
        for (int x = c0[0]; x <= c1[0] && !done; ++x) {
            for (int y = c0[1]; y <= c1[1] && !done; ++y) {
                const unsigned base = (unsigned)(((int64_t)x * a.dims[1] + y) * a.dims[2]);
                const unsigned klo = base + (unsigned)c0[2], khi = base + (unsigned)c1[2];
                int lo = from, hi = n;
                for (int s = 0; s < 32 && lo < hi; ++s) {    // the first position with key >= klo
                    const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
                    if (sk[mid] < klo) lo = mid + 1;
                    else hi = mid;
                }
                int q = lo;
                for (; q < n; ++q) {
                    if (sk[q] > khi) break;
                    const float4 o = sr[q];
                    const int jr = __float_as_int(o.w);
                    const float d2 = rad_d2(me, o);
                    if (jr != i && d2 <= a.r2) {
                        ++count;
                        if (d2 < best || (d2 == best && jr < bestj)) { best = d2; bestj = jr; }
                        if (count == a.cap) { done = true; break; }
                    }
                }
                from = q < n ? q : n;
            }
        }
    }
    a.cnt[g] = count;
    if (a.nn_idx) a.nn_idx[g] = bestj;
    if (a.nn_dist2) a.nn_dist2[g] = best;
}

// ---- the filter's compaction over row order
__device__ __forceinline__ bool rad_keep(const RadiusArgs& a, int64_t row0, int64_t j, int n) {
    return j < n && a.cnt[row0 + j] >= a.min_neighbors;
}

__global__ __launch_bounds__(RAD_SEG) void rad_flags(RadiusArgs a) {
    __shared__ int sh[RAD_SEG / 64];
    const int b = blockIdx.y, tid = threadIdx.x;
    int64_t row0;
    const int n = rad_span(a, b, row0);
    const int64_t j = (int64_t)blockIdx.x * RAD_SEG + tid;
    if ((int64_t)blockIdx.x * RAD_SEG >= n) return;          // the whole workgroup
    const unsigned long long bm = __ballot(rad_keep(a, row0, j, n));
    if ((tid & 63) == 0) sh[tid >> 6] = __popcll(bm);
    __syncthreads();
    if (tid == 0) {
        int s = 0;
        for (int w = 0; w < RAD_SEG / 64; ++w) s += sh[w];
        a.blocks[(int64_t)b * a.nseg_max + blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(256) void rad_block_scan(RadiusArgs a) {
    __shared__ int sh[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    int64_t row0;
    const int n = rad_span(a, b, row0);
    const int nseg = (n + RAD_SEG - 1) / RAD_SEG;
    int* h = a.blocks + (int64_t)b * a.nseg_max;
    int carry = 0;
    for (int s0 = 0; s0 < nseg; s0 += 256) {
        const int s = s0 + tid;
        const int v = s < nseg ? h[s] : 0;
        int total;
        const int ex = vox_block_excl<256>(v, sh, tid, &total);
        if (s < nseg) h[s] = carry + ex;
        carry += total;
    }
    if (tid == 0) a.total[b] = carry;
}

__global__ __launch_bounds__(256) void rad_offsets(RadiusArgs a) {
    __shared__ int sh[4];
    const int tid = threadIdx.x;
    int64_t carry = 0;
    if (tid == 0) a.out_offsets[0] = 0;
    for (int b0 = 0; b0 < a.batch; b0 += 256) {
        const int b = b0 + tid;
        const int v = b < a.batch ? a.total[b] : 0;
        int total;
        const int ex = vox_block_excl<256>(v, sh, tid, &total);   // <= n_total < 2^31 in all
        if (b < a.batch) a.out_offsets[b + 1] = carry + ex + v;
        carry += total;
    }
}

__global__ __launch_bounds__(RAD_SEG) void rad_compact(RadiusArgs a) {
    __shared__ int sh[RAD_SEG / 64];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int64_t row0;
    const int n = rad_span(a, b, row0);
    const int64_t j = (int64_t)blockIdx.x * RAD_SEG + tid;
    if ((int64_t)blockIdx.x * RAD_SEG >= n) return;
    const bool keep = rad_keep(a, row0, j, n);
    const unsigned long long bm = __ballot(keep);
    if (lane == 0) sh[w] = __popcll(bm);
    __syncthreads();
    if (!keep) return;                                       // no barrier below
    int rank = a.blocks[(int64_t)b * a.nseg_max + blockIdx.x] + __popcll(bm & vox_lanes_below(lane));
    for (int u = 0; u < w; ++u) rank += sh[u];
    const int64_t vo = a.out_offsets[b] + rank;
    if (vo >= a.n_total) return;                             // cannot happen with offsets that do not overlap
    const float* p = a.points + (row0 + j) * 3;
    a.out_points[vo * 3] = p[0];
    a.out_points[vo * 3 + 1] = p[1];
    a.out_points[vo * 3 + 2] = p[2];
    if (a.out_index) a.out_index[vo] = j;
}

inline int64_t rad_align16(int64_t bytes) { return (bytes + 15) / 16 * 16; }

void rad_layout(RadiusArgs& a, const float* points, const int64_t* offsets, const int32_t* counts, int B, int64_t n_dense, int64_t n_total,
                int64_t max_per_sample) {
    a.points = points; a.offsets = offsets; a.counts = counts;
    a.n_dense = n_dense; a.n_total = n_total; a.max_per_sample = max_per_sample;
    a.nseg_max = (max_per_sample + RAD_SEG - 1) / RAD_SEG;
    a.batch = B;
}

// the checks of both entries that the sort does not make, then the sort and the two search launches
int rad_search(const std::string& who, RadiusArgs& a, const float* points, const int64_t* offsets, const int32_t* counts, int B,
               int64_t n_dense, int64_t n_total, int64_t max_per_sample, const float* lo3_host, const float* v3_host,
               const int32_t* dims3_host, float radius, int cap, int32_t* cnt_or_null, void* scratch, int64_t scratch_bytes, int64_t chunk,
               hipStream_t st) {
    RALD_CHECK(lo3_host && v3_host && dims3_host, who + ": null grid (lo3, v3, dims3)");
    RALD_CHECK(std::isfinite(radius) && radius > 0.f, who + ": radius must be finite and > 0");
    for (int k = 0; k < 3; ++k) RALD_CHECK(v3_host[k] >= radius, who + ": every cell edge must be >= radius");   // NaN fails
    const int64_t need = radius_scratch_bytes(B, n_total, max_per_sample, chunk);
    if (need >= 0) {                                         // else the sort names the size it refuses
        RALD_CHECK(scratch_bytes >= need, who + ": scratch too small");
        RALD_CHECK(scratch && (uintptr_t)scratch % 16 == 0, who + ": null or unaligned scratch");
    }
    VoxelSorted sorted;
    RALD_TRY(voxel_sort_ragged(who.c_str(), points, offsets, counts, B, n_dense, n_total, max_per_sample, lo3_host, v3_host, dims3_host,
                               nullptr, scratch, chunk, st, &sorted));
    rad_layout(a, points, offsets, counts, B, n_dense, n_total, max_per_sample);
    for (int k = 0; k < 3; ++k) { a.lo[k] = lo3_host[k]; a.v[k] = v3_host[k]; a.dims[k] = dims3_host[k]; }
    a.cells = sorted.cells;
    a.r2 = radius * radius;
    a.rs = radius * (1.f + 9.5367431640625e-07f);            // 2^-20
    a.cap = cap;
    a.skey = sorted.key; a.sidx = sorted.idx;
    char* s = (char*)scratch + voxel_sort_scratch_bytes(B, n_total, max_per_sample, chunk);
    a.srow = (float4*)s; s += rad_align16(n_total * 16);
    a.cnt = cnt_or_null ? cnt_or_null : (int32_t*)s; s += rad_align16(n_total * 4);
    a.blocks = (int*)s;                                      // the compaction's share: radius_compact_ragged lays it out
    const dim3 by_pos((unsigned)((max_per_sample + RAD_T - 1) / RAD_T), B);
    hipLaunchKernelGGL(rad_gather, by_pos, dim3(RAD_T), 0, st, a);
    hipLaunchKernelGGL(rad_count, by_pos, dim3(RAD_T), 0, st, a);
    return 0;
}

}  // namespace

void radius_gather_sorted(const float* points, const int64_t* offsets, const int32_t* counts, int B, int64_t n_dense, int64_t n_total,
                          int64_t max_per_sample, const int* sidx, float4* srow, hipStream_t st) {
    RadiusArgs a{};
    rad_layout(a, points, offsets, counts, B, n_dense, n_total, max_per_sample);
    a.sidx = sidx; a.srow = srow;
    hipLaunchKernelGGL(rad_gather, dim3((unsigned)((max_per_sample + RAD_T - 1) / RAD_T), B), dim3(RAD_T), 0, st, a);
}

int64_t radius_compact_scratch_bytes(int B, int64_t max_per_sample) {
    const int64_t nseg = (max_per_sample + RAD_SEG - 1) / RAD_SEG;
    return rad_align16((int64_t)B * nseg * 4) + rad_align16((int64_t)B * 4);
}

void radius_compact_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int B, int64_t n_dense, int64_t n_total,
                           int64_t max_per_sample, const int32_t* cnt, int min_neighbors, float* out_points, int64_t* out_offsets,
                           int64_t* out_index, void* scratch, hipStream_t st) {
    RadiusArgs a{};
    rad_layout(a, points, offsets, counts, B, n_dense, n_total, max_per_sample);
    a.cnt = const_cast<int32_t*>(cnt); a.min_neighbors = min_neighbors;
    a.out_points = out_points; a.out_offsets = out_offsets; a.out_index = out_index;
    a.blocks = (int*)scratch;
    a.total = (int*)((char*)scratch + rad_align16((int64_t)B * a.nseg_max * 4));
    const dim3 by_seg((unsigned)a.nseg_max, B);
    hipLaunchKernelGGL(rad_flags, by_seg, dim3(RAD_SEG), 0, st, a);
    hipLaunchKernelGGL(rad_block_scan, dim3(B), dim3(256), 0, st, a);
    hipLaunchKernelGGL(rad_offsets, dim3(1), dim3(256), 0, st, a);
    hipLaunchKernelGGL(rad_compact, by_seg, dim3(RAD_SEG), 0, st, a);
}

int64_t radius_scratch_bytes(int B, int64_t n_total, int64_t max_per_sample, int64_t chunk) {
    const int64_t sort = voxel_sort_scratch_bytes(B, n_total, max_per_sample, chunk);
    if (sort < 0) return -1;
    return sort + rad_align16(n_total * 16) + rad_align16(n_total * 4) + radius_compact_scratch_bytes(B, max_per_sample);
}

int radius_count_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int B, int64_t n_dense, int64_t n_total,
                        int64_t max_per_sample, const float* lo3_host, const float* v3_host, const int32_t* dims3_host, float radius,
                        int max_count, int32_t* out_count, int64_t* out_nn_idx, float* out_nn_dist2, void* scratch, int64_t scratch_bytes,
                        int64_t chunk, hipStream_t st) {
    RALD_CHECK(points && out_count, "radius_count_ragged: null pointer (points, out_count)");
    RALD_CHECK(max_count >= 0, "radius_count_ragged: max_count must be >= 0 (0 = no cap)");
    RALD_CHECK(max_count == 0 || (!out_nn_idx && !out_nn_dist2), "radius_count_ragged: the nearest row needs max_count = 0");
    RadiusArgs a{};
    a.nn_idx = out_nn_idx; a.nn_dist2 = out_nn_dist2;
    RALD_TRY(rad_search("radius_count_ragged", a, points, offsets, counts, B, n_dense, n_total, max_per_sample, lo3_host, v3_host, dims3_host,
                        radius, max_count, out_count, scratch, scratch_bytes, chunk, st));
    RALD_HIP(hipGetLastError());
    return 0;
}

int radius_filter_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int B, int64_t n_dense, int64_t n_total,
                         int64_t max_per_sample, const float* lo3_host, const float* v3_host, const int32_t* dims3_host, float radius,
                         int min_neighbors, float* out_points, int64_t* out_offsets, int64_t* out_index, int32_t* out_count, void* scratch,
                         int64_t scratch_bytes, int64_t chunk, hipStream_t st) {
    RALD_CHECK(points && out_points && out_offsets, "radius_filter_ragged: null pointer (points, out_points, out_offsets)");
    RALD_CHECK(min_neighbors >= 1, "radius_filter_ragged: min_neighbors must be >= 1");
    RadiusArgs a{};
    RALD_TRY(rad_search("radius_filter_ragged", a, points, offsets, counts, B, n_dense, n_total, max_per_sample, lo3_host, v3_host,
                        dims3_host, radius, min_neighbors, out_count, scratch, scratch_bytes, chunk, st));
    radius_compact_ragged(points, offsets, counts, B, n_dense, n_total, max_per_sample, a.cnt, min_neighbors, out_points, out_offsets, out_index,
                          a.blocks, st);
    RALD_HIP(hipGetLastError());
    return 0;
}

}  // namespace rald
