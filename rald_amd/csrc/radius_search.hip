// Fixed-radius neighbour search inside each cloud of a ragged batch, and the radius outlier filter on it.  The
// definition is in include/rald_hip.h; in short
//   inside   the cell rule of the index (cloud_index.h): c = floorf(fl(fl(p - lo) / v)) per axis, 0 <= c < dims in float
//   d2(i,j)  fl(fl(fl(dx*dx) + fl(dy*dy)) + fl(dz*dz)), dx = fl(p_j.x - p_i.x): fp32, no contraction
//   count[i] the inside rows j != i of the same cloud with d2(i,j) <= r2 = fl(radius * radius), min(count, cap) with a cap; -1 outside
//   nearest  the j of the smallest d2 among them, the smallest j on equal d2
//   filter   keep row i iff count[i] >= min_neighbors, in row order
// The grid is only the index: cloud_index_build leaves every cloud's cell keys in ascending order and the rows in that order, 16 bytes
// a row.  One launch behind it, then for the filter the compaction of cloud_index.hip on count >= min_neighbors:
//   rad_count       (256 sorted positions, cloud)  one lane per SORTED position, so a wave's lanes are neighbours in space and walk the
//                                                  same lines.  The walk is radius_walk of cloud_index.h, which the cluster kernels
//                                                  share; the visitor here counts, keeps the nearest row and stops at the cap.  The
//                                                  result goes back to the row's place.
// No atomics at all.  Every loop is bounded by the cloud's length (<= max_per_sample, a host value), by the grid's dims (host values) or
// by 32.  A row index read from the scratch is clamped into the cloud before it addresses anything.
#include "cloud_index.h"
#include "kernels.h"

namespace rald {

namespace {

constexpr int RAD_T = 256;                                   // sorted positions per workgroup of rad_count

struct RadiusArgs {
    RaggedCloud c;
    CellGrid g;
    float r2, rs;
    int cap;                                                 // 0 = none; the walk stops at it
    const unsigned* skey; const float4* srow;                // [n_total] the sorted keys and rows
    int32_t* cnt;                                            // [n_total] per row
    int64_t* nn_idx; float* nn_dist2;                        // per row, nullable
    BlockScan sc;                                            // the filter's compaction
};

__global__ __launch_bounds__(RAD_T) void rad_count(RadiusArgs a) {
    const int b = blockIdx.y;
    int64_t row0;
    const int n = ragged_span(a.c, b, row0);
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
    if (key < a.g.cells) {
        count = 0;
        const float r2 = a.r2;
        const int cap = a.cap;
        radius_walk(a.g, a.rs, sk, sr, n, me, [&](int, const float4& o, float d2) {
            const int jr = __float_as_int(o.w);
            if (jr == i || !(d2 <= r2)) return false;
            if (d2 < best || (d2 == best && jr < bestj)) { best = d2; bestj = jr; }
            return ++count == cap;
        });
    }
    a.cnt[g] = count;
    if (a.nn_idx) a.nn_idx[g] = bestj;
    if (a.nn_dist2) a.nn_dist2[g] = best;
}

void rad_layout(RadiusArgs& a, CloudIndex& ix, Carver& s, int64_t chunk) {
    cloud_index_layout(ix, a.c, s, chunk, true);
    a.cnt = s.take<int32_t>(a.c.n_total);
    block_scan_layout(a.sc, a.c, s);
}

// the checks of both entries that the index does not make, then the index and the search
int rad_search(const std::string& who, RadiusArgs& a, const RaggedCloud& c, const GridSpec& grid, float radius, int cap, int32_t* out_count,
               void* scratch, int64_t scratch_bytes, int64_t chunk, hipStream_t st) {
    RALD_CHECK(grid.lo && grid.v && grid.dims, who + ": null grid (lo3, v3, dims3)");
    RALD_CHECK(std::isfinite(radius) && radius > 0.f, who + ": radius must be finite and > 0");
    for (int k = 0; k < 3; ++k) RALD_CHECK(grid.v[k] >= radius, who + ": every cell edge must be >= radius");   // NaN fails
    RALD_TRY(scratch_check(who, scratch, scratch_bytes, radius_scratch_bytes(c.batch, c.n_total, c.max_per_sample, chunk)));
    RALD_TRY(cloud_grid_check(who, c, grid, chunk, &a.g));
    a.c = c;
    CloudIndex ix;
    Carver s{(char*)scratch, 0};
    rad_layout(a, ix, s, chunk);
    if (out_count) a.cnt = out_count;
    a.r2 = radius * radius;
    a.rs = scan_reach(radius);
    a.cap = cap;
    const SortedCloud sorted = cloud_index_build(ix, a.g, nullptr, st);
    a.skey = sorted.key; a.srow = sorted.rows;
    hipLaunchKernelGGL(rad_count, dim3((unsigned)((c.max_per_sample + RAD_T - 1) / RAD_T), c.batch), dim3(RAD_T), 0, st, a);
    return 0;
}

}  // namespace

int64_t radius_scratch_bytes(int B, int64_t n_total, int64_t max_per_sample, int64_t chunk) {
    return layout_bytes<RadiusArgs>(B, n_total, max_per_sample, chunk, rad_layout);
}

int radius_count_ragged(const RaggedCloud& c, const GridSpec& grid, float radius, int max_count, int32_t* out_count, int64_t* out_nn_idx,
                        float* out_nn_dist2, void* scratch, int64_t scratch_bytes, int64_t chunk, hipStream_t st) {
    RALD_CHECK(c.points && out_count, "radius_count_ragged: null pointer (points, out_count)");
    RALD_CHECK(max_count >= 0, "radius_count_ragged: max_count must be >= 0 (0 = no cap)");
    RALD_CHECK(max_count == 0 || (!out_nn_idx && !out_nn_dist2), "radius_count_ragged: the nearest row needs max_count = 0");
    RadiusArgs a{};
    a.nn_idx = out_nn_idx; a.nn_dist2 = out_nn_dist2;
    RALD_TRY(rad_search("radius_count_ragged", a, c, grid, radius, max_count, out_count, scratch, scratch_bytes, chunk, st));
    RALD_HIP(hipGetLastError());
    return 0;
}

int radius_filter_ragged(const RaggedCloud& c, const GridSpec& grid, float radius, int min_neighbors, float* out_points, int64_t* out_offsets,
                         int64_t* out_index, int32_t* out_count, void* scratch, int64_t scratch_bytes, int64_t chunk, hipStream_t st) {
    RALD_CHECK(c.points && out_points && out_offsets, "radius_filter_ragged: null pointer (points, out_points, out_offsets)");
    RALD_CHECK(min_neighbors >= 1, "radius_filter_ragged: min_neighbors must be >= 1");
    RadiusArgs a{};
    RALD_TRY(rad_search("radius_filter_ragged", a, c, grid, radius, min_neighbors, out_count, scratch, scratch_bytes, chunk, st));
    a.sc.out_offsets = out_offsets;
    compact_rows_ragged(c, a.sc, a.cnt, min_neighbors, out_points, out_index, st);
    RALD_HIP(hipGetLastError());
    return 0;
}

}  // namespace rald
