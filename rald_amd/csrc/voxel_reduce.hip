// Voxel-grid down-sampling of a ragged batch: every cloud becomes one point per occupied cell of a fixed grid,
// the cells in ascending key order, the point the centroid of the cell's rows.  The definition is in include/rald_hip.h; in short
//   cell   c = floorf(fl(fl(p - lo) / v)) per axis, fp32, no contraction, inside iff 0 <= c < dims in float (NaN fails both)
//   key    (c0 * dims1 + c1) * dims2 + c2, `cells` for a row outside the grid (the largest key: outside rows sort behind every voxel)
//   voxel  a run of equal keys < cells after a STABLE sort of (key, row): its rows stand in ascending row order
// The key and sort phases (vox_keys and the two sort routes) are also the spatial index of radius_search.hip, behind voxel_sort_ragged.
// Launches, all on one stream, none waits on another workgroup:
//   vox_keys        (256-row block, cloud)   key and row index of every row; out_inverse = -1 for outside rows
//   the sort, `passes` = ceil(bits(cells) / 8) LSD passes of 8 bits between the ping and the pong buffer:
//     split route (the bound exceeds one chunk), per pass
//       vox_hist     (chunk, cloud)   the chunk's 256 digit counts -> hist[cloud][digit * nch + chunk]  (nch = the cloud's own chunk count)
//       vox_scan     (cloud)          exclusive scan of that array in place: digit-major, chunks in order inside a digit
//       vox_scatter  (chunk, cloud)   the chunk's rows to their places: wave w ranks its quarter of the chunk with the ballot loop, the
//                                     waves in order behind the chunk's scanned base, so equal keys keep their row order
//     one-workgroup route (the bound fits one chunk)
//       vox_sort_one (cloud)          all passes in one workgroup of 16 waves, block barriers between the steps
//   vox_heads       (1024 rows, cloud)  segment heads (first position of a run of equal keys < cells) per block of sorted positions
//   vox_head_scan   (cloud)             exclusive scan of the block counts in place, the cloud's voxel count
//   vox_offsets     one workgroup       out_offsets = exclusive scan of the voxel counts over the batch
//   vox_reduce      (1024 rows, cloud)  the lane at a head walks its segment in order: float64 sums left to right, / (double)n, one
//                                       rounding to fp32; count, first (the segment's first row: the smallest, the sort is stable),
//                                       cells from the key, and the voxel's rank into out_inverse of every row it walks
// Integer LDS atomics only count digits.  Every loop is bounded by the cloud's length (<= max_per_sample, a host value) or by 256.
// A cloud's span is clamped into [0, n_total] before anything is addressed, so device offsets of any value reach neither past `points`
// nor past the scratch.
#include <cmath>

#include "common.h"
#include "kernels.h"

namespace rald {

namespace {

constexpr int VOX_KT = 256;                                  // rows per workgroup of vox_keys
constexpr int VOX_SEG = 1024;                                // sorted positions per workgroup of vox_heads / vox_reduce (one per thread)
constexpr int VOX_CW = 4;                                    // waves per chunk workgroup of the split route
constexpr int VOX_CT = 64 * VOX_CW;
constexpr int VOX_OW = 16;                                   // waves of the one-workgroup route
constexpr int VOX_OT = 64 * VOX_OW;
constexpr int64_t VOX_MAX_POINTS = (int64_t)1 << 24;         // rows per cloud
constexpr int64_t VOX_MAX_TOTAL = ((int64_t)1 << 31) - 1;    // rows in all, and cells of the grid
constexpr int VOX_MAX_BATCH = 65535;                         // clouds (the grids' second dimension)
constexpr int64_t VOX_AUTO_CHUNK = 4096;
constexpr int64_t VOX_MIN_AUTO_CHUNK = 2048;

struct VoxelArgs {
    const float* points; const int64_t* offsets; const int32_t* counts;
    int64_t n_dense, n_total, max_per_sample, chunk, nch_max, nseg_max;
    float lo[3], v[3];
    int dims[3];
    unsigned cells;
    int passes;
    unsigned* key[2]; int* idx[2];                           // [n_total] ping / pong of the sort
    unsigned* hist;                                          // [batch][256 * nch_max]
    int* heads;                                              // [batch][nseg_max]
    int* total;                                              // [batch] voxels per cloud
    int batch;
    float* out_points; int64_t* out_offsets; int32_t* out_count; int64_t* out_first; int32_t* out_cells; int64_t* out_inverse;
};

// the cloud's first row and its number of rows (kernels.h: the layout is shared with radius_search.hip)
__device__ __forceinline__ int vox_span(const VoxelArgs& a, int b, int64_t& row0) {
    return ragged_span(a.offsets, a.counts, a.n_dense, a.n_total, a.max_per_sample, b, row0);
}

__global__ __launch_bounds__(VOX_KT) void vox_keys(VoxelArgs a) {
    const int b = blockIdx.y;
    int64_t row0;
    const int n = vox_span(a, b, row0);
    const int64_t j = (int64_t)blockIdx.x * VOX_KT + threadIdx.x;
    if (j >= n) return;
    const int64_t g = row0 + j;
    const float* p = a.points + g * 3;
    int c[3];
    bool in = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float cf = voxel_cell(p[k], a.lo[k], a.v[k]);
        in = in && cf >= 0.f && cf < (float)a.dims[k];       // NaN fails both
        c[k] = in ? (int)cf : 0;
    }
    a.key[0][g] = in ? (unsigned)(((int64_t)c[0] * a.dims[1] + c[1]) * a.dims[2] + c[2]) : a.cells;
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
__global__ __launch_bounds__(VOX_CT) void vox_hist(VoxelArgs a, int pass) {
    __shared__ unsigned h[256];
    const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
    int64_t row0;
    const int n = vox_span(a, b, row0);
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
__global__ __launch_bounds__(256) void vox_scan(VoxelArgs a) {
    __shared__ int sh[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    int64_t row0;
    const int n = vox_span(a, b, row0);
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

__global__ __launch_bounds__(VOX_CT) void vox_scatter(VoxelArgs a, int pass) {
    __shared__ unsigned cnt[VOX_CW][256];
    const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int64_t row0;
    const int n = vox_span(a, b, row0);
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
__global__ __launch_bounds__(VOX_OT) void vox_sort_one(VoxelArgs a) {
    __shared__ unsigned cnt[VOX_OW][256];
    __shared__ int tot[256];
    __shared__ int sh[VOX_OW];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int64_t row0;
    const int n = vox_span(a, b, row0);
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

// ---- segments
__device__ __forceinline__ bool vox_is_head(const unsigned* sk, int64_t j, int n, unsigned cells) {
    if (j >= n) return false;
    const unsigned k = sk[j];
    return k < cells && (j == 0 || sk[j - 1] != k);
}

__global__ __launch_bounds__(VOX_SEG) void vox_heads(VoxelArgs a) {
    __shared__ int sh[VOX_SEG / 64];
    const int b = blockIdx.y, tid = threadIdx.x;
    int64_t row0;
    const int n = vox_span(a, b, row0);
    const int64_t j = (int64_t)blockIdx.x * VOX_SEG + tid;
    if ((int64_t)blockIdx.x * VOX_SEG >= n) return;
    const unsigned* sk = a.key[a.passes & 1] + row0;
    const unsigned long long bm = __ballot(vox_is_head(sk, j, n, a.cells));
    if ((tid & 63) == 0) sh[tid >> 6] = __popcll(bm);
    __syncthreads();
    if (tid == 0) {
        int s = 0;
        for (int i = 0; i < VOX_SEG / 64; ++i) s += sh[i];
        a.heads[(int64_t)b * a.nseg_max + blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(256) void vox_head_scan(VoxelArgs a) {
    __shared__ int sh[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    int64_t row0;
    const int n = vox_span(a, b, row0);
    const int nseg = (n + VOX_SEG - 1) / VOX_SEG;
    int* h = a.heads + (int64_t)b * a.nseg_max;
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

__global__ __launch_bounds__(256) void vox_offsets(VoxelArgs a) {
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

__global__ __launch_bounds__(VOX_SEG) void vox_reduce(VoxelArgs a) {
    __shared__ int sh[VOX_SEG / 64];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int64_t row0;
    const int n = vox_span(a, b, row0);
    const int64_t j = (int64_t)blockIdx.x * VOX_SEG + tid;
    if ((int64_t)blockIdx.x * VOX_SEG >= n) return;
    const unsigned* sk = a.key[a.passes & 1] + row0;
    const int* si = a.idx[a.passes & 1] + row0;
    const bool head = vox_is_head(sk, j, n, a.cells);
    const unsigned long long bm = __ballot(head);
    if (lane == 0) sh[w] = __popcll(bm);
    __syncthreads();
    if (!head) return;                                       // no barrier below
    int rank = a.heads[(int64_t)b * a.nseg_max + blockIdx.x] + __popcll(bm & vox_lanes_below(lane));
    for (int i = 0; i < w; ++i) rank += sh[i];
    const int64_t vo = a.out_offsets[b] + rank;
    const unsigned key = sk[j];
    const int first = si[j];
    const float* p = a.points + row0 * 3;
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
    if (vo >= a.n_total) return;                             // cannot happen with offsets that do not overlap
    const double dn = (double)cnt;
    a.out_points[vo * 3] = (float)(sx / dn);
    a.out_points[vo * 3 + 1] = (float)(sy / dn);
    a.out_points[vo * 3 + 2] = (float)(sz / dn);
    if (a.out_count) a.out_count[vo] = cnt;
    if (a.out_first) a.out_first[vo] = first;
    if (a.out_cells) {
        const unsigned d2 = (unsigned)a.dims[2], d1 = (unsigned)a.dims[1];
        const unsigned q = key / d2;
        a.out_cells[vo * 3] = (int)(q / d1);
        a.out_cells[vo * 3 + 1] = (int)(q % d1);
        a.out_cells[vo * 3 + 2] = (int)(key % d2);
    }
}

inline int64_t vox_align16(int64_t bytes) { return (bytes + 15) / 16 * 16; }

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

inline bool vox_sizes_ok(int B, int64_t n_total, int64_t max_per_sample, int64_t chunk) {
    return B >= 1 && B <= VOX_MAX_BATCH && n_total >= 0 && n_total <= VOX_MAX_TOTAL && max_per_sample >= 1 && max_per_sample <= VOX_MAX_POINTS &&
           chunk >= 0 && chunk % 1024 == 0;
}

}  // namespace

int voxel_passes(int64_t cells) {
    if (cells < 1 || cells > VOX_MAX_TOTAL) return -1;
    int bits = 0;
    while ((cells >> bits) != 0) ++bits;
    return (bits + 7) / 8;
}

int64_t voxel_sort_scratch_bytes(int B, int64_t n_total, int64_t max_per_sample, int64_t chunk) {
    if (!vox_sizes_ok(B, n_total, max_per_sample, chunk)) return -1;
    // automatic: sized for the smallest chunk the rule picks, so the size grows with every argument whatever the rule chooses
    const int64_t ch = chunk > 0 ? chunk : VOX_MIN_AUTO_CHUNK;
    const int64_t nch = (max_per_sample + ch - 1) / ch;
    return 4 * vox_align16(n_total * 4) + vox_align16((int64_t)B * 256 * nch * 4);
}

int64_t voxel_scratch_bytes(int B, int64_t n_total, int64_t max_per_sample, int64_t chunk) {
    const int64_t sort = voxel_sort_scratch_bytes(B, n_total, max_per_sample, chunk);
    if (sort < 0) return -1;
    const int64_t nseg = (max_per_sample + VOX_SEG - 1) / VOX_SEG;
    return sort + vox_align16((int64_t)B * nseg * 4) + vox_align16((int64_t)B * 4);
}

namespace {

// the layout and grid rules of both entries
int vox_check(const std::string& who, const int64_t* offsets, int B, int64_t n_dense, int64_t n_total, int64_t max_per_sample,
              const float* lo3_host, const float* v3_host, const int32_t* dims3_host, int64_t chunk) {
    RALD_CHECK(lo3_host && v3_host && dims3_host, who + ": null grid (lo3, v3, dims3)");
    RALD_CHECK(B >= 1 && B <= VOX_MAX_BATCH, who + ": batch must be 1 .. 65535");
    RALD_CHECK(offsets || n_dense >= 0, who + ": n_dense must be >= 0 without offsets");
    RALD_CHECK(n_total >= 0 && n_total <= VOX_MAX_TOTAL, who + ": n_total must be 0 .. 2^31 - 1");
    RALD_CHECK(max_per_sample >= 1 && max_per_sample <= VOX_MAX_POINTS, who + ": max_per_sample must be 1 .. 16777216");
    RALD_CHECK(chunk >= 0 && chunk % 1024 == 0, who + ": chunk must be 0 (automatic) or a multiple of 1024");
    int64_t cells = 1;
    for (int k = 0; k < 3; ++k) {
        RALD_CHECK(dims3_host[k] >= 1, who + ": every dim must be >= 1");
        cells *= dims3_host[k];                              // <= (2^31 - 1)^2 after two factors: checked before the third
        RALD_CHECK(cells <= VOX_MAX_TOTAL, who + ": the grid must have at most 2^31 - 1 cells");
        RALD_CHECK(std::isfinite(v3_host[k]) && v3_host[k] > 0.f, who + ": every cell edge must be finite and > 0");
        RALD_CHECK(std::isfinite(lo3_host[k]), who + ": lo must be finite");
    }
    return 0;
}

// the sort's part of the arguments (checked ones) -> the scratch behind the sort's share
char* vox_sort_args(VoxelArgs& a, const float* points, const int64_t* offsets, const int32_t* counts, int B, int64_t n_dense, int64_t n_total,
                    int64_t max_per_sample, const float* lo3_host, const float* v3_host, const int32_t* dims3_host, void* scratch,
                    int64_t chunk) {
    a = VoxelArgs{};
    a.points = points; a.offsets = offsets; a.counts = counts;
    a.n_dense = n_dense; a.n_total = n_total; a.max_per_sample = max_per_sample;
    a.chunk = vox_pick_chunk(B, max_per_sample, chunk);
    a.nch_max = (max_per_sample + a.chunk - 1) / a.chunk;
    a.nseg_max = (max_per_sample + VOX_SEG - 1) / VOX_SEG;
    for (int k = 0; k < 3; ++k) { a.lo[k] = lo3_host[k]; a.v[k] = v3_host[k]; a.dims[k] = dims3_host[k]; }
    const int64_t cells = (int64_t)a.dims[0] * a.dims[1] * a.dims[2];
    a.cells = (unsigned)cells;
    a.passes = voxel_passes(cells);
    char* s = (char*)scratch;
    const int64_t row_bytes = vox_align16(n_total * 4);
    a.key[0] = (unsigned*)s; s += row_bytes;
    a.key[1] = (unsigned*)s; s += row_bytes;
    a.idx[0] = (int*)s; s += row_bytes;
    a.idx[1] = (int*)s; s += row_bytes;
    a.hist = (unsigned*)s; s += vox_align16((int64_t)B * 256 * a.nch_max * 4);
    a.batch = B;
    return s;
}

// vox_keys and the sort: the sorted pairs end in key[passes & 1], idx[passes & 1]
void vox_launch_sort(const VoxelArgs& a, hipStream_t st) {
    const int B = a.batch;
    hipLaunchKernelGGL(vox_keys, dim3((unsigned)((a.max_per_sample + VOX_KT - 1) / VOX_KT), B), dim3(VOX_KT), 0, st, a);
    if (a.nch_max == 1) {
        hipLaunchKernelGGL(vox_sort_one, dim3(B), dim3(VOX_OT), 0, st, a);
    } else {
        const dim3 by_chunk((unsigned)a.nch_max, B);
        for (int pass = 0; pass < a.passes; ++pass) {
            hipLaunchKernelGGL(vox_hist, by_chunk, dim3(VOX_CT), 0, st, a, pass);
            hipLaunchKernelGGL(vox_scan, dim3(B), dim3(256), 0, st, a);
            hipLaunchKernelGGL(vox_scatter, by_chunk, dim3(VOX_CT), 0, st, a, pass);
        }
    }
}

}  // namespace

int voxel_sort_ragged(const char* who, const float* points, const int64_t* offsets, const int32_t* counts, int B, int64_t n_dense,
                      int64_t n_total, int64_t max_per_sample, const float* lo3_host, const float* v3_host, const int32_t* dims3_host,
                      int64_t* out_inverse, void* scratch, int64_t chunk, hipStream_t st, VoxelSorted* out) {
    RALD_TRY(vox_check(who, offsets, B, n_dense, n_total, max_per_sample, lo3_host, v3_host, dims3_host, chunk));
    VoxelArgs a;
    vox_sort_args(a, points, offsets, counts, B, n_dense, n_total, max_per_sample, lo3_host, v3_host, dims3_host, scratch, chunk);
    a.out_inverse = out_inverse;
    vox_launch_sort(a, st);
    RALD_HIP(hipGetLastError());
    out->key = a.key[a.passes & 1];
    out->idx = a.idx[a.passes & 1];
    out->cells = a.cells;
    return 0;
}

int voxel_downsample_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int B, int64_t n_dense, int64_t n_total,
                            int64_t max_per_sample, const float* lo3_host, const float* v3_host, const int32_t* dims3_host, float* out_points,
                            int64_t* out_offsets, int32_t* out_count, int64_t* out_first, int32_t* out_cells, int64_t* out_inverse,
                            void* scratch, int64_t scratch_bytes, int64_t chunk, hipStream_t st) {
    RALD_CHECK(points && out_points && out_offsets, "voxel_downsample_ragged: null pointer (points, out_points, out_offsets)");
    RALD_TRY(vox_check("voxel_downsample_ragged", offsets, B, n_dense, n_total, max_per_sample, lo3_host, v3_host, dims3_host, chunk));
    const int64_t need = voxel_scratch_bytes(B, n_total, max_per_sample, chunk);
    RALD_CHECK(scratch_bytes >= need, "voxel_downsample_ragged: scratch too small");
    RALD_CHECK(scratch && (uintptr_t)scratch % 16 == 0, "voxel_downsample_ragged: null or unaligned scratch");
    VoxelArgs a;
    char* s = vox_sort_args(a, points, offsets, counts, B, n_dense, n_total, max_per_sample, lo3_host, v3_host, dims3_host, scratch, chunk);
    a.heads = (int*)s; s += vox_align16((int64_t)B * a.nseg_max * 4);
    a.total = (int*)s;
    a.out_points = out_points; a.out_offsets = out_offsets; a.out_count = out_count; a.out_first = out_first; a.out_cells = out_cells;
    a.out_inverse = out_inverse;
    vox_launch_sort(a, st);
    const dim3 by_cloud(B);
    const dim3 by_seg((unsigned)a.nseg_max, B);
    hipLaunchKernelGGL(vox_heads, by_seg, dim3(VOX_SEG), 0, st, a);
    hipLaunchKernelGGL(vox_head_scan, by_cloud, dim3(256), 0, st, a);
    hipLaunchKernelGGL(vox_offsets, dim3(1), dim3(256), 0, st, a);
    hipLaunchKernelGGL(vox_reduce, by_seg, dim3(VOX_SEG), 0, st, a);
    RALD_HIP(hipGetLastError());
    return 0;
}

}  // namespace rald
