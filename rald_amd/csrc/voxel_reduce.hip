// Voxel-grid down-sampling of a ragged batch: every cloud becomes one point per occupied cell of a fixed grid,
// the cells in ascending key order, the point the centroid of the cell's rows.  The definition is in include/rald_hip.h; the cell and
// the key are those of the index (cloud_index.h), and
//   voxel  a run of equal keys < cells after the index's STABLE sort of (key, row): its rows stand in ascending row order
// Launches behind cloud_index_build, all on one stream, none waits on another workgroup:
//   vox_heads       (1024 rows, cloud)  segment heads (first position of a run of equal keys < cells) per block of sorted positions
//   the two scans of cloud_index.hip    the heads before each block, the cloud's voxel count, out_offsets over the batch
//   vox_reduce      (1024 rows, cloud)  the lane at a head walks its segment in order: float64 sums left to right, / (double)n, one
//                                       rounding to fp32; count, first (the segment's first row: the smallest, the sort is stable),
//                                       cells from the key, and the voxel's rank into out_inverse of every row it walks
// No atomics.  Every loop is bounded by the cloud's length (<= max_per_sample, a host value).
#include "cloud_index.h"
#include "kernels.h"

namespace rald {

namespace {

struct VoxelArgs {
    RaggedCloud c;
    CellGrid g;
    const unsigned* skey; const int* sidx;                   // [n_total] the sorted pairs
    BlockScan sc;                                            // blocks: the heads per block of sorted positions; total: voxels per cloud
    float* out_points; int32_t* out_count; int64_t* out_first; int32_t* out_cells; int64_t* out_inverse;
};

__device__ __forceinline__ bool vox_is_head(const unsigned* sk, int64_t j, int n, unsigned cells) {
    if (j >= n) return false;
    const unsigned k = sk[j];
    return k < cells && (j == 0 || sk[j - 1] != k);
}

__global__ __launch_bounds__(CLOUD_SEG) void vox_heads(VoxelArgs a) {
    __shared__ int sh[CLOUD_SEG / 64];
    const int b = blockIdx.y, tid = threadIdx.x;
    int64_t row0;
    const int n = ragged_span(a.c, b, row0);
    const int64_t j = (int64_t)blockIdx.x * CLOUD_SEG + tid;
    if ((int64_t)blockIdx.x * CLOUD_SEG >= n) return;
    int total;
    block_rank<CLOUD_SEG>(vox_is_head(a.skey + row0, j, n, a.g.cells), sh, tid, &total);
    if (tid == 0) a.sc.blocks[(int64_t)b * a.sc.nseg_max + blockIdx.x] = total;
}

__global__ __launch_bounds__(CLOUD_SEG) void vox_reduce(VoxelArgs a) {
    __shared__ int sh[CLOUD_SEG / 64];
    const int b = blockIdx.y, tid = threadIdx.x;
    int64_t row0;
    const int n = ragged_span(a.c, b, row0);
    const int64_t j = (int64_t)blockIdx.x * CLOUD_SEG + tid;
    if ((int64_t)blockIdx.x * CLOUD_SEG >= n) return;
    const unsigned* sk = a.skey + row0;
    const int* si = a.sidx + row0;
    const bool head = vox_is_head(sk, j, n, a.g.cells);
    const int in_block = block_rank<CLOUD_SEG>(head, sh, tid, nullptr);
    if (!head) return;                                       // no barrier below
    const int rank = a.sc.blocks[(int64_t)b * a.sc.nseg_max + blockIdx.x] + in_block;
    const int64_t vo = a.sc.out_offsets[b] + rank;
    const unsigned key = sk[j];
    const int first = si[j];
    const float* p = a.c.points + row0 * 3;
    int64_t* inv = a.out_inverse ? a.out_inverse + row0 : nullptr;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    int cnt = 0;
    for (int64_t e = j;; e += 4) {                           // the segment, four rows per step so that the gathers overlap
        int r[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t q = e + u;
            r[u] = q < n && sk[q] == key ? si[q] : -1;       // sorted: equal keys are contiguous
        }
        float x[4], y[4], z[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t o = (int64_t)(r[u] >= 0 ? r[u] : first) * 3;
            x[u] = p[o]; y[u] = p[o + 1]; z[u] = p[o + 2];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (r[u] >= 0) {
                sx += (double)x[u]; sy += (double)y[u]; sz += (double)z[u];
                ++cnt;
                if (inv) inv[r[u]] = rank;
            }
        }
        if (r[3] < 0) break;
    }
    if (vo >= a.c.n_total) return;                           // cannot happen with offsets that do not overlap
    const double dn = (double)cnt;
    a.out_points[vo * 3] = (float)(sx / dn);
    a.out_points[vo * 3 + 1] = (float)(sy / dn);
    a.out_points[vo * 3 + 2] = (float)(sz / dn);
    if (a.out_count) a.out_count[vo] = cnt;
    if (a.out_first) a.out_first[vo] = first;
    if (a.out_cells) {
        const unsigned d2 = (unsigned)a.g.dims[2], d1 = (unsigned)a.g.dims[1];
        const unsigned q = key / d2;
        a.out_cells[vo * 3] = (int)(q / d1);
        a.out_cells[vo * 3 + 1] = (int)(q % d1);
        a.out_cells[vo * 3 + 2] = (int)(key % d2);
    }
}

void vox_layout(VoxelArgs& a, CloudIndex& ix, Carver& s, int64_t chunk) {
    cloud_index_layout(ix, a.c, s, chunk, false);
    block_scan_layout(a.sc, a.c, s);
}

}  // namespace

int64_t voxel_scratch_bytes(int B, int64_t n_total, int64_t max_per_sample, int64_t chunk) {
    return layout_bytes<VoxelArgs>(B, n_total, max_per_sample, chunk, vox_layout);
}

int voxel_downsample_ragged(const RaggedCloud& c, const GridSpec& grid, float* out_points, int64_t* out_offsets, int32_t* out_count,
                            int64_t* out_first, int32_t* out_cells, int64_t* out_inverse, void* scratch, int64_t scratch_bytes, int64_t chunk,
                            hipStream_t st) {
    const std::string who = "voxel_downsample_ragged";
    RALD_CHECK(c.points && out_points && out_offsets, who + ": null pointer (points, out_points, out_offsets)");
    VoxelArgs a{};
    RALD_TRY(cloud_grid_check(who, c, grid, chunk, &a.g));
    RALD_TRY(scratch_check(who, scratch, scratch_bytes, voxel_scratch_bytes(c.batch, c.n_total, c.max_per_sample, chunk)));
    a.c = c;
    CloudIndex ix;
    Carver s{(char*)scratch, 0};
    vox_layout(a, ix, s, chunk);
    a.sc.out_offsets = out_offsets;
    a.out_points = out_points; a.out_count = out_count; a.out_first = out_first; a.out_cells = out_cells; a.out_inverse = out_inverse;
    const SortedCloud sorted = cloud_index_build(ix, a.g, out_inverse, st);
    a.skey = sorted.key; a.sidx = sorted.idx;
    const dim3 by_seg((unsigned)a.sc.nseg_max, c.batch);
    hipLaunchKernelGGL(vox_heads, by_seg, dim3(CLOUD_SEG), 0, st, a);
    block_scan_launch(c, a.sc, st);
    hipLaunchKernelGGL(vox_reduce, by_seg, dim3(CLOUD_SEG), 0, st, a);
    RALD_HIP(hipGetLastError());
    return 0;
}

}  // namespace rald
