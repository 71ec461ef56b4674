// The spatial index of the grid-indexed operations on ragged clouds, and their compaction in row order (cloud_index.h; DESIGN.md
// section 21).  A voxel of voxel_reduce.hip, a key interval of radius_search.hip and knn_search.hip is a run of the sorted keys: the
// sort is STABLE, so the rows of equal keys stand in ascending row order.
// Launches of the index, all on one stream, none waits on another workgroup:
//   vox_keys        (256-row block, cloud)   key and row index of every row; out_inverse = -1 for outside rows
//   the sort, `passes` = ceil(bits(cells) / 8) LSD passes of 8 bits between the ping and the pong buffer:
//     split route (the bound exceeds one chunk), per pass
//       vox_hist     (chunk, cloud)   the chunk's 256 digit counts -> hist[cloud][digit * nch + chunk]  (nch = the cloud's own chunk count)
//       vox_scan     (cloud)          exclusive scan of that array in place: digit-major, chunks in order inside a digit
//       vox_scatter  (chunk, cloud)   the chunk's rows to their places: wave w ranks its quarter of the chunk with the ballot loop, the
//                                     waves in order behind the chunk's scanned base, so equal keys keep their row order
//     one-workgroup route (the bound fits one chunk)
//       vox_sort_one (cloud)          all passes in one workgroup of 16 waves, block barriers between the steps
//   cloud_gather    (256 sorted positions, cloud)  with rows: the coordinates in sorted order, 16 bytes a row: x, y, z, the row's index
// Launches of the compaction, behind a kernel that counts the true flags of every block of 1024 (cloud_flags for the rows):
//   cloud_block_scan  (cloud)             exclusive scan of the block counts in place, the cloud's total
//   cloud_offsets     one workgroup       out_offsets = exclusive scan of the totals over the batch
//   cloud_compact     (1024 rows, cloud)  a kept row to out_offsets[b] + its rank
// and behind it, for the filters that keep labels (cloud_cluster.hip, cloud_plane.hip):
//   cloud_kept_labels (256 kept rows, cloud)  the label of every kept row, by the row index the compaction left
// Integer LDS atomics only count digits.  Every loop is bounded by the cloud's length (<= max_per_sample, a host value), by the batch
// or by 256.  A cloud's span is clamped into [0, n_total] before anything is addressed, so device offsets of any value reach neither
// past `points` nor past the scratch; a row index read from the scratch is clamped into the cloud before it addresses anything.
#include "cloud_index.h"

namespace rald {

namespace {

constexpr int VOX_KT = 256;                                  // rows per workgroup of vox_keys and cloud_gather
constexpr int VOX_CW = 4;                                    // waves per chunk workgroup of the split route
constexpr int VOX_CT = 64 * VOX_CW;
constexpr int VOX_OW = 16;                                   // waves of the one-workgroup route
constexpr int VOX_OT = 64 * VOX_OW;
constexpr int64_t VOX_MAX_POINTS = (int64_t)1 << 24;         // rows per cloud
constexpr int64_t VOX_MAX_TOTAL = ((int64_t)1 << 31) - 1;    // rows in all, and cells of the grid
constexpr int VOX_MAX_BATCH = 65535;                         // clouds (the grids' second dimension)
constexpr int64_t VOX_AUTO_CHUNK = 4096;
constexpr int64_t VOX_MIN_AUTO_CHUNK = 2048;

__global__ __launch_bounds__(VOX_KT) void vox_keys(CloudIndex a) {
    const int b = blockIdx.y;
    int64_t row0;
    const int n = ragged_span(a.c, b, row0);
    const int64_t j = (int64_t)blockIdx.x * VOX_KT + threadIdx.x;
    if (j >= n) return;
    const int64_t g = row0 + j;
    const float* p = a.c.points + g * 3;
    int c[3];
    bool in = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float cf = voxel_cell(p[k], a.g.lo[k], a.g.v[k]);
        in = in && cf >= 0.f && cf < (float)a.g.dims[k];     // NaN fails both
        c[k] = in ? (int)cf : 0;
    }
    a.key[0][g] = in ? (unsigned)(((int64_t)c[0] * a.g.dims[1] + c[1]) * a.g.dims[2] + c[2]) : a.g.cells;
    a.idx[0][g] = (int)j;
    if (!in && a.out_inverse) a.out_inverse[g] = -1;
}

// wave w of W owns the contiguous range [lo, hi) of [c0, c1), a multiple of 64 long
template <int W>
__device__ __forceinline__ void vox_wave_range(int64_t c0, int64_t c1, int w, int64_t& lo, int64_t& hi) {
    const int64_t per = ((c1 - c0 + W - 1) / W + 63) / 64 * 64;
    lo = c0 + per * w;
    lo = lo < c1 ? lo : c1;
    hi = lo + per < c1 ? lo + per : c1;
}

// the wave's digit counts into its row of cnt (LDS, zeroed before)
__device__ __forceinline__ void vox_count(const unsigned* ks, int64_t lo, int64_t hi, int lane, int shift, unsigned* cnt_w) {
    for (int64_t j = lo + lane; j < hi; j += 64) atomicAdd(&cnt_w[(ks[j] >> shift) & 255u], 1u);
}

// the wave moves its range, 64 rows at a time in order: a row's place is the wave's running offset of its digit plus the number of
// lanes below it with the same digit (eight ballots), so equal digits keep their order
__device__ __forceinline__ void vox_scatter_wave(const unsigned* ks, const int* is, unsigned* kd, int* id, int64_t lo, int64_t hi, int lane,
                                                 int shift, unsigned* cnt_w) {
    for (int64_t j0 = lo; j0 < hi; j0 += 64) {
        const int64_t j = j0 + lane;
        const bool valid = j < hi;
        const unsigned key = valid ? ks[j] : 0u;
        const int idx = valid ? is[j] : 0;
        const unsigned dg = (key >> shift) & 255u;
        unsigned long long m = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool set = (dg >> bit) & 1u;
            const unsigned long long bb = __ballot(valid && set);
            m &= set ? bb : ~bb;
        }
        const unsigned rank = (unsigned)__popcll(m & vox_lanes_below(lane));
        const unsigned pos = valid ? cnt_w[dg] + rank : 0u;
        __builtin_amdgcn_wave_barrier();
        if (valid && rank == 0) cnt_w[dg] += (unsigned)__popcll(m);
        __builtin_amdgcn_wave_barrier();
        if (valid) {
            kd[pos] = key;
            id[pos] = idx;
        }
    }
}

// ---- split route
__global__ __launch_bounds__(VOX_CT) void vox_hist(CloudIndex a, int pass) {
    __shared__ unsigned h[256];
    const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
    int64_t row0;
    const int n = ragged_span(a.c, b, row0);
    const int64_t c0 = (int64_t)chunk * a.chunk;
    if (c0 >= n) return;                                     // the whole workgroup
    const int64_t c1 = c0 + a.chunk < n ? c0 + a.chunk : n;
    const int nch = (int)((n + a.chunk - 1) / a.chunk);
    const unsigned* ks = a.key[pass & 1] + row0;
    h[tid] = 0;
    __syncthreads();
    const int shift = 8 * pass;
    for (int64_t j = c0 + tid; j < c1; j += VOX_CT) atomicAdd(&h[(ks[j] >> shift) & 255u], 1u);
    __syncthreads();
    a.hist[(int64_t)b * 256 * a.nch_max + (int64_t)tid * nch + chunk] = h[tid];
}

// thread d owns digit d: its nch chunk counts are contiguous, so the digit-major scan is a plain scan of 256 * nch values
__global__ __launch_bounds__(256) void vox_scan(CloudIndex a) {
    __shared__ int sh[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    int64_t row0;
    const int n = ragged_span(a.c, b, row0);
    if (n == 0) return;
    const int nch = (int)((n + a.chunk - 1) / a.chunk);
    unsigned* h = a.hist + (int64_t)b * 256 * a.nch_max + (int64_t)tid * nch;
    int sum = 0;
    for (int c = 0; c < nch; ++c) sum += (int)h[c];
    int total;
    unsigned run = (unsigned)vox_block_excl<256>(sum, sh, tid, &total);
    for (int c = 0; c < nch; ++c) {
        const unsigned x = h[c];
        h[c] = run;
        run += x;
    }
}

__global__ __launch_bounds__(VOX_CT) void vox_scatter(CloudIndex a, int pass) {
    __shared__ unsigned cnt[VOX_CW][256];
    const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int64_t row0;
    const int n = ragged_span(a.c, b, row0);
    const int64_t c0 = (int64_t)chunk * a.chunk;
    if (c0 >= n) return;
    const int64_t c1 = c0 + a.chunk < n ? c0 + a.chunk : n;
    const int nch = (int)((n + a.chunk - 1) / a.chunk);
    const unsigned* ks = a.key[pass & 1] + row0;
    const int* is = a.idx[pass & 1] + row0;
    unsigned* kd = a.key[(pass & 1) ^ 1] + row0;
    int* id = a.idx[(pass & 1) ^ 1] + row0;
    const int shift = 8 * pass;
    for (int i = tid; i < VOX_CW * 256; i += VOX_CT) (&cnt[0][0])[i] = 0;
    __syncthreads();
    int64_t lo, hi;
    vox_wave_range<VOX_CW>(c0, c1, w, lo, hi);
    vox_count(ks, lo, hi, lane, shift, cnt[w]);
    __syncthreads();
    {                                                        // VOX_CT == 256: thread d, digit d
        unsigned run = a.hist[(int64_t)b * 256 * a.nch_max + (int64_t)tid * nch + chunk];
        for (int ww = 0; ww < VOX_CW; ++ww) {
            const unsigned c = cnt[ww][tid];
            cnt[ww][tid] = run;
            run += c;
        }
    }
    __syncthreads();
    vox_scatter_wave(ks, is, kd, id, lo, hi, lane, shift, cnt[w]);
}

// ---- one-workgroup route
__global__ __launch_bounds__(VOX_OT) void vox_sort_one(CloudIndex a) {
    __shared__ unsigned cnt[VOX_OW][256];
    __shared__ int tot[256];
    __shared__ int sh[VOX_OW];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int64_t row0;
    const int n = ragged_span(a.c, b, row0);
    if (n == 0) return;
    int64_t lo, hi;
    vox_wave_range<VOX_OW>(0, n, w, lo, hi);
    for (int pass = 0; pass < a.passes; ++pass) {
        const unsigned* ks = a.key[pass & 1] + row0;
        const int* is = a.idx[pass & 1] + row0;
        unsigned* kd = a.key[(pass & 1) ^ 1] + row0;
        int* id = a.idx[(pass & 1) ^ 1] + row0;
        const int shift = 8 * pass;
        for (int i = tid; i < VOX_OW * 256; i += VOX_OT) (&cnt[0][0])[i] = 0;
        __syncthreads();
        vox_count(ks, lo, hi, lane, shift, cnt[w]);
        __syncthreads();
        int sum = 0;
        if (tid < 256) {
            for (int ww = 0; ww < VOX_OW; ++ww) {
                const unsigned c = cnt[ww][tid];
                cnt[ww][tid] = (unsigned)sum;
                sum += (int)c;
            }
        }
        int total;                                           // threads 256 .. 1023 add 0 behind the digits
        const int base = vox_block_excl<VOX_OT>(sum, sh, tid, &total);
        if (tid < 256) tot[tid] = base;
        __syncthreads();
        if (tid < 256)
            for (int ww = 0; ww < VOX_OW; ++ww) cnt[ww][tid] += (unsigned)tot[tid];
        __syncthreads();
        vox_scatter_wave(ks, is, kd, id, lo, hi, lane, shift, cnt[w]);
        __syncthreads();                                     // the pass's stores, before the next pass reads them (one workgroup)
    }
}

__global__ __launch_bounds__(VOX_KT) void cloud_gather(CloudIndex a) {
    const int b = blockIdx.y;
    int64_t row0;
    const int n = ragged_span(a.c, b, row0);
    const int64_t j = (int64_t)blockIdx.x * VOX_KT + threadIdx.x;
    if (j >= n) return;
    const int r = rad_clamp(a.idx[a.passes & 1][row0 + j], n);
    const float* p = a.c.points + (row0 + r) * 3;
    a.rows[row0 + j] = make_float4(p[0], p[1], p[2], __int_as_float(r));
}

// the chunk of the split route; a bound that fits one chunk takes the one-workgroup route.  0 = the automatic rule, a function of
// (batch, max_per_sample) alone
// Set from tools/bench_voxel_downsample.py's `rule` section (profiles/voxel_downsample.json): the one-workgroup route wherever it
// was not slower than the best split beyond its own spread - every batch up to 8192 rows, 64 clouds and more up to 16384, 256 clouds
// and more up to 65536 (the chip is full of clouds then) - and chunks of 2048 where few clouds of middle size leave CUs idle.
inline int64_t vox_pick_chunk(int B, int64_t max_per_sample, int64_t chunk) {
    if (chunk > 0) return chunk;
    const int64_t one = (max_per_sample + 1023) / 1024 * 1024;
    if (max_per_sample <= 8192 || (B >= 64 && max_per_sample <= 16384) || (B >= 256 && max_per_sample <= 65536)) return one;
    return B <= 8 && max_per_sample <= 65536 ? VOX_MIN_AUTO_CHUNK : VOX_AUTO_CHUNK;
}

}  // namespace

bool cloud_sizes_ok(int B, int64_t n_total, int64_t max_per_sample, int64_t chunk) {
    return B >= 1 && B <= VOX_MAX_BATCH && n_total >= 0 && n_total <= VOX_MAX_TOTAL && max_per_sample >= 1 && max_per_sample <= VOX_MAX_POINTS &&
           chunk >= 0 && chunk % 1024 == 0;
}

int scratch_check(const std::string& who, const void* scratch, int64_t bytes, int64_t need) {
    if (need < 0) return 0;
    RALD_CHECK(bytes >= need, who + ": scratch too small");
    RALD_CHECK(scratch && (uintptr_t)scratch % 16 == 0, who + ": null or unaligned scratch");
    return 0;
}

int voxel_passes(int64_t cells) {
    if (cells < 1 || cells > VOX_MAX_TOTAL) return -1;
    int bits = 0;
    while ((cells >> bits) != 0) ++bits;
    return (bits + 7) / 8;
}

int cloud_grid_check(const std::string& who, const RaggedCloud& c, const GridSpec& grid, int64_t chunk, CellGrid* g) {
    RALD_CHECK(grid.lo && grid.v && grid.dims, who + ": null grid (lo3, v3, dims3)");
    RALD_CHECK(c.batch >= 1 && c.batch <= VOX_MAX_BATCH, who + ": batch must be 1 .. 65535");
    RALD_CHECK(c.offsets || c.n_dense >= 0, who + ": n_dense must be >= 0 without offsets");
    RALD_CHECK(c.n_total >= 0 && c.n_total <= VOX_MAX_TOTAL, who + ": n_total must be 0 .. 2^31 - 1");
    RALD_CHECK(c.max_per_sample >= 1 && c.max_per_sample <= VOX_MAX_POINTS, who + ": max_per_sample must be 1 .. 16777216");
    RALD_CHECK(chunk >= 0 && chunk % 1024 == 0, who + ": chunk must be 0 (automatic) or a multiple of 1024");
    int64_t cells = 1;
    for (int k = 0; k < 3; ++k) {
        RALD_CHECK(grid.dims[k] >= 1, who + ": every dim must be >= 1");
        cells *= grid.dims[k];                               // <= (2^31 - 1)^2 after two factors: checked before the third
        RALD_CHECK(cells <= VOX_MAX_TOTAL, who + ": the grid must have at most 2^31 - 1 cells");
        RALD_CHECK(std::isfinite(grid.v[k]) && grid.v[k] > 0.f, who + ": every cell edge must be finite and > 0");
        RALD_CHECK(std::isfinite(grid.lo[k]), who + ": lo must be finite");
        g->lo[k] = grid.lo[k]; g->v[k] = grid.v[k]; g->dims[k] = grid.dims[k];
    }
    g->cells = (unsigned)cells;
    return 0;
}

void cloud_index_layout(CloudIndex& ix, const RaggedCloud& c, Carver& s, int64_t chunk, bool rows) {
    ix.c = c;
    ix.chunk = vox_pick_chunk(c.batch, c.max_per_sample, chunk);
    ix.nch_max = (c.max_per_sample + ix.chunk - 1) / ix.chunk;
    ix.key[0] = s.take<unsigned>(c.n_total);
    ix.key[1] = s.take<unsigned>(c.n_total);
    ix.idx[0] = s.take<int>(c.n_total);
    ix.idx[1] = s.take<int>(c.n_total);
    // automatic: sized for the smallest chunk the rule picks, so the size grows with every argument whatever the rule chooses
    const int64_t ch = chunk > 0 ? chunk : VOX_MIN_AUTO_CHUNK;
    ix.hist = s.take<unsigned>((int64_t)c.batch * 256 * ((c.max_per_sample + ch - 1) / ch));
    ix.rows = rows ? s.take<float4>(c.n_total) : nullptr;
}

SortedCloud cloud_index_build(CloudIndex& ix, const CellGrid& g, int64_t* out_inverse, hipStream_t st) {
    ix.g = g;
    ix.passes = voxel_passes(g.cells);
    ix.out_inverse = out_inverse;
    const int B = ix.c.batch;
    const dim3 by_row((unsigned)((ix.c.max_per_sample + VOX_KT - 1) / VOX_KT), B);
    hipLaunchKernelGGL(vox_keys, by_row, dim3(VOX_KT), 0, st, ix);
    if (ix.nch_max == 1) {
        hipLaunchKernelGGL(vox_sort_one, dim3(B), dim3(VOX_OT), 0, st, ix);
    } else {
        const dim3 by_chunk((unsigned)ix.nch_max, B);
        for (int pass = 0; pass < ix.passes; ++pass) {
            hipLaunchKernelGGL(vox_hist, by_chunk, dim3(VOX_CT), 0, st, ix, pass);
            hipLaunchKernelGGL(vox_scan, dim3(B), dim3(256), 0, st, ix);
            hipLaunchKernelGGL(vox_scatter, by_chunk, dim3(VOX_CT), 0, st, ix, pass);
        }
    }
    if (ix.rows) hipLaunchKernelGGL(cloud_gather, by_row, dim3(VOX_KT), 0, st, ix);
    return SortedCloud{ix.key[ix.passes & 1], ix.idx[ix.passes & 1], ix.rows};
}

// ---- the compaction
namespace {

struct CompactArgs {
    RaggedCloud c;
    BlockScan sc;
    const int32_t* keep;
    int at_least;
    float* out_points; int64_t* out_index;
};

__global__ __launch_bounds__(256) void cloud_block_scan(RaggedCloud c, BlockScan sc) {
    __shared__ int sh[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    int64_t row0;
    const int n = ragged_span(c, b, row0);
    const int nseg = (n + CLOUD_SEG - 1) / CLOUD_SEG;
    int* h = sc.blocks + (int64_t)b * sc.nseg_max;
    int carry = 0;
    for (int s0 = 0; s0 < nseg; s0 += 256) {
        const int s = s0 + tid;
        const int v = s < nseg ? h[s] : 0;
        int total;
        const int ex = vox_block_excl<256>(v, sh, tid, &total);
        if (s < nseg) h[s] = carry + ex;
        carry += total;
    }
    if (tid == 0) sc.total[b] = carry;
}

__global__ __launch_bounds__(256) void cloud_offsets(RaggedCloud c, BlockScan sc) {
    __shared__ int sh[4];
    const int tid = threadIdx.x;
    int64_t carry = 0;
    if (tid == 0) sc.out_offsets[0] = 0;
    for (int b0 = 0; b0 < c.batch; b0 += 256) {
        const int b = b0 + tid;
        const int v = b < c.batch ? sc.total[b] : 0;
        int total;
        const int ex = vox_block_excl<256>(v, sh, tid, &total);   // <= n_total < 2^31 in all
        if (b < c.batch) sc.out_offsets[b + 1] = carry + ex + v;
        carry += total;
    }
}

__device__ __forceinline__ bool cloud_keep(const CompactArgs& a, int64_t row0, int64_t j, int n) {
    return j < n && a.keep[row0 + j] >= a.at_least;
}

__global__ __launch_bounds__(CLOUD_SEG) void cloud_flags(CompactArgs a) {
    __shared__ int sh[CLOUD_SEG / 64];
    const int b = blockIdx.y, tid = threadIdx.x;
    int64_t row0;
    const int n = ragged_span(a.c, b, row0);
    const int64_t j = (int64_t)blockIdx.x * CLOUD_SEG + tid;
    if ((int64_t)blockIdx.x * CLOUD_SEG >= n) return;        // the whole workgroup
    int total;
    block_rank<CLOUD_SEG>(cloud_keep(a, row0, j, n), sh, tid, &total);
    if (tid == 0) a.sc.blocks[(int64_t)b * a.sc.nseg_max + blockIdx.x] = total;
}

__global__ __launch_bounds__(CLOUD_SEG) void cloud_compact(CompactArgs a) {
    __shared__ int sh[CLOUD_SEG / 64];
    const int b = blockIdx.y, tid = threadIdx.x;
    int64_t row0;
    const int n = ragged_span(a.c, b, row0);
    const int64_t j = (int64_t)blockIdx.x * CLOUD_SEG + tid;
    if ((int64_t)blockIdx.x * CLOUD_SEG >= n) return;
    const bool keep = cloud_keep(a, row0, j, n);
    const int in_block = block_rank<CLOUD_SEG>(keep, sh, tid, nullptr);
    if (!keep) return;                                       // no barrier below
    const int rank = a.sc.blocks[(int64_t)b * a.sc.nseg_max + blockIdx.x] + in_block;
    const int64_t vo = a.sc.out_offsets[b] + rank;
    if (vo >= a.c.n_total) return;                           // cannot happen with offsets that do not overlap
    const float* p = a.c.points + (row0 + j) * 3;
    a.out_points[vo * 3] = p[0];
    a.out_points[vo * 3 + 1] = p[1];
    a.out_points[vo * 3 + 2] = p[2];
    if (a.out_index) a.out_index[vo] = j;
}

__global__ __launch_bounds__(VOX_KT) void cloud_kept_labels(RaggedCloud c, const int64_t* out_offsets, const int64_t* kept,
                                                            const int32_t* labels, int32_t* out_labels) {
    const int b = blockIdx.y;
    int64_t row0;
    const int n = ragged_span(c, b, row0);
    const int64_t j = (int64_t)blockIdx.x * VOX_KT + threadIdx.x;
    const int64_t o0 = out_offsets[b];
    if (j >= n || j >= out_offsets[b + 1] - o0) return;
    const int64_t vo = o0 + j;
    if (vo < 0 || vo >= c.n_total) return;                   // cannot happen with offsets that do not overlap
    out_labels[vo] = labels[row0 + rad_clamp(kept[vo], (int64_t)n)];
}

}  // namespace

void block_scan_layout(BlockScan& sc, const RaggedCloud& c, Carver& s) {
    sc.nseg_max = (c.max_per_sample + CLOUD_SEG - 1) / CLOUD_SEG;
    sc.blocks = s.take<int>(c.batch * sc.nseg_max);
    sc.total = s.take<int>(c.batch);
}

void block_scan_launch(const RaggedCloud& c, const BlockScan& sc, hipStream_t st) {
    hipLaunchKernelGGL(cloud_block_scan, dim3(c.batch), dim3(256), 0, st, c, sc);
    hipLaunchKernelGGL(cloud_offsets, dim3(1), dim3(256), 0, st, c, sc);
}

void compact_rows_ragged(const RaggedCloud& c, BlockScan sc, const int32_t* keep, int at_least, float* out_points, int64_t* out_index,
                         hipStream_t st) {
    const CompactArgs a{c, sc, keep, at_least, out_points, out_index};
    const dim3 by_seg((unsigned)sc.nseg_max, c.batch);
    hipLaunchKernelGGL(cloud_flags, by_seg, dim3(CLOUD_SEG), 0, st, a);
    block_scan_launch(c, sc, st);
    hipLaunchKernelGGL(cloud_compact, by_seg, dim3(CLOUD_SEG), 0, st, a);
}

void cloud_kept_labels_ragged(const RaggedCloud& c, const int64_t* out_offsets, const int64_t* kept, const int32_t* labels, int32_t* out_labels,
                              hipStream_t st) {
    const dim3 by_row((unsigned)((c.max_per_sample + VOX_KT - 1) / VOX_KT), c.batch);
    hipLaunchKernelGGL(cloud_kept_labels, by_row, dim3(VOX_KT), 0, st, c, out_offsets, kept, labels, out_labels);
}

}  // namespace rald
