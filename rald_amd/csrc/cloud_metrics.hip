// Point-cloud metrics on the device: exact nearest neighbours of a ragged batch in fp64, per point (distance and
// index) and reduced per frame (sum of d, sum of d^2, max of d, rows with d < tau_k) - what accuracy / completeness, both Chamfer
// variants, (modified) Hausdorff distance and precision / recall / F-score derive from.  Three kernels per direction, no atomics:
//   nn_chunk_kernel   grid (block of 1024 a rows, frame, chunk of b): (d^2, index) of the nearest b row INSIDE the chunk -> workspace
//   nn_finish_kernel  grid (block of 1024 a rows, frame): merges the chunks (minimum, lowest index on equal d^2), writes the optional
//                     per-row outputs and one partial reduction per workgroup, laid out from the frame's own first row
//   nn_reduce_kernel  grid (frame): adds a frame's partials in index order -> raw[frame][dir][3 + K]
// Minimum and lowest-index argmin do not depend on the order of the candidates, so neither the chunk length nor the batch a frame
// sits in changes a bit of the result.
#include <cmath>

#include "common.h"
#include "kernels.h"

namespace rald {

namespace {

constexpr int NN_TILE = 1024;              // b points per LDS tile (and the unit of the chunk length)
constexpr int NN_R = 4;                    // a rows per lane: one LDS read of a b point serves 4 pairs
constexpr int NN_ROWS = 256 * NN_R;        // a rows per workgroup (nn_chunk_kernel and nn_finish_kernel)
constexpr int NN_SEG = 16;                 // the k-loop keeps the minimum per group of 16 candidates; the index inside the group is found afterwards
constexpr int64_t NN_MAX_CHUNK = (int64_t)1 << 30;     // a group's position inside its chunk is a 32-bit int
constexpr int NN_TARGET_WG = 2048;         // workgroups the automatic chunking aims for (8 per CU of an MI355X)
constexpr int NN_MAX_K = 8;
constexpr int NN_NRED = 3 + NN_MAX_K;      // doubles per partial / per raw row at K = 8

struct NnThresholds { double tau[NN_MAX_K]; int k; };

__device__ __forceinline__ double pair_d2(double ax, double ay, double az, double bx, double by, double bz) {
#pragma clang fp contract(off)                                   // three products and two sums, each rounded: what numpy float64 computes
    const double dx = ax - bx, dy = ay - by, dz = az - bz;
    return dx * dx + dy * dy + dz * dz;
}

// workspace: d2 [n_chunks][B][max_a] doubles, then idx [n_chunks][B][max_a] int64 (index of the b row from the frame's first b row)
__global__ __launch_bounds__(256) void nn_chunk_kernel(const float* __restrict__ a, const int64_t* __restrict__ a_off, const float* __restrict__ b,
                                                       const int64_t* __restrict__ b_off, int B, int64_t max_a, int64_t max_b,
                                                       int64_t chunk, double* __restrict__ ws_d2, int64_t* __restrict__ ws_idx) {
    __shared__ double sb[3][NN_TILE];
    const int f = blockIdx.y;
    const int64_t a0 = a_off[f], b0 = b_off[f];
    int64_t na = a_off[f + 1] - a0, nb = b_off[f + 1] - b0;
    na = na < max_a ? na : max_a;                                // the workspace holds max_a rows and ceil(max_b / chunk) chunks per frame:
    nb = nb < max_b ? nb : max_b;                                // a bound below a segment's length leaves the rows behind it out
    const int64_t row0 = (int64_t)blockIdx.x * NN_ROWS;
    const int64_t j_begin = (int64_t)blockIdx.z * chunk;
    if (row0 >= na || j_begin >= nb) return;                     // a row block behind the segment, a chunk behind nb, an empty side
    const int64_t j_end = j_begin + chunk < nb ? j_begin + chunk : nb;
    a += a0 * 3; b += b0 * 3;

    double ax[NN_R], ay[NN_R], az[NN_R], best[NN_R];
    int seg[NN_R];                                               // first candidate of the winning group, from j_begin
#pragma unroll
    for (int r = 0; r < NN_R; ++r) {
        const int64_t i = row0 + r * 256 + threadIdx.x;
        const int64_t ic = i < na ? i : na - 1;                  // lanes behind the segment redo its last row and store nothing
        ax[r] = a[ic * 3]; ay[r] = a[ic * 3 + 1]; az[r] = a[ic * 3 + 2];
        best[r] = INFINITY; seg[r] = 0;
    }
    for (int64_t j0 = j_begin; j0 < j_end; j0 += NN_TILE) {
        const int cnt = (int)(j_end - j0 < NN_TILE ? j_end - j0 : NN_TILE);
        const int padded = (cnt + NN_SEG - 1) / NN_SEG * NN_SEG;
        __syncthreads();
        for (int j = threadIdx.x; j < padded; j += 256) {
            const bool in = j < cnt;                             // a group's tail behind the chunk: infinitely far, never the minimum
            sb[0][j] = in ? (double)b[(j0 + j) * 3] : (double)INFINITY;
            sb[1][j] = in ? (double)b[(j0 + j) * 3 + 1] : 0.0;
            sb[2][j] = in ? (double)b[(j0 + j) * 3 + 2] : 0.0;
        }
        __syncthreads();
        for (int j = 0; j < padded; j += NN_SEG) {
            double bx[NN_SEG], by[NN_SEG], bz[NN_SEG];
#pragma unroll
            for (int s = 0; s < NN_SEG; ++s) { bx[s] = sb[0][j + s]; by[s] = sb[1][j + s]; bz[s] = sb[2][j + s]; }
#pragma unroll
            for (int r = 0; r < NN_R; ++r) {
                double m = pair_d2(ax[r], ay[r], az[r], bx[0], by[0], bz[0]);
#pragma unroll
                for (int s = 1; s < NN_SEG; ++s) m = fmin(m, pair_d2(ax[r], ay[r], az[r], bx[s], by[s], bz[s]));
                seg[r] = m < best[r] ? (int)(j0 - j_begin) + j : seg[r];    // strict: the first group that reaches the minimum keeps it
                best[r] = fmin(best[r], m);
            }
        }
    }
    // the lowest row of the winning group whose distance IS the minimum (the same operations on the same values give the same bits)
#pragma unroll
    for (int r = 0; r < NN_R; ++r) {
        const int64_t i = row0 + r * 256 + threadIdx.x;
        if (i >= na) continue;
        const int64_t s_begin = j_begin + seg[r];
        const int64_t s_end = s_begin + NN_SEG < j_end ? s_begin + NN_SEG : j_end;
        int64_t idx = s_begin;
        for (int64_t j = s_end - 1; j >= s_begin; --j)
            if (pair_d2(ax[r], ay[r], az[r], (double)b[j * 3], (double)b[j * 3 + 1], (double)b[j * 3 + 2]) == best[r]) idx = j;
        const int64_t w = ((int64_t)blockIdx.z * B + f) * max_a + i;
        ws_d2[w] = best[r];
        ws_idx[w] = idx;
    }
}

// partial [B][n_blocks][NN_NRED]: block x of frame f covers the frame's rows x * 1024 .. x * 1024 + 1023
__global__ __launch_bounds__(256) void nn_finish_kernel(const int64_t* __restrict__ a_off, const int64_t* __restrict__ b_off, int B, int64_t max_a,
                                                        int64_t max_b, int64_t chunk, const double* __restrict__ ws_d2, const int64_t* __restrict__ ws_idx,
                                                        double* __restrict__ out_dist, int64_t* __restrict__ out_idx, NnThresholds thr,
                                                        double* __restrict__ partial) {
    __shared__ double red[4][NN_NRED];
    const int f = blockIdx.y;
    const int64_t a0 = a_off[f];
    int64_t na = a_off[f + 1] - a0, nb = b_off[f + 1] - b_off[f];
    na = na < max_a ? na : max_a;
    nb = nb < max_b ? nb : max_b;                                 // as nn_chunk_kernel: only chunks that kernel wrote are read
    const int64_t row0 = (int64_t)blockIdx.x * NN_ROWS;
    if (row0 >= na) return;
    const int64_t n_chunks = nb > 0 ? (nb + chunk - 1) / chunk : 0;
    double v[NN_NRED];
#pragma unroll
    for (int k = 0; k < NN_NRED; ++k) v[k] = 0.0;
    for (int r = 0; r < NN_R; ++r) {                              // rows in ascending order per lane: the sum's order is fixed
        const int64_t i = row0 + r * 256 + threadIdx.x;
        if (i >= na) continue;
        if (n_chunks == 0) {                                      // no candidate: no neighbour, and nothing for the frame's sums
            if (out_dist) out_dist[a0 + i] = INFINITY;
            if (out_idx) out_idx[a0 + i] = -1;
            continue;
        }
        double d2 = ws_d2[(int64_t)f * max_a + i];
        int64_t idx = ws_idx[(int64_t)f * max_a + i];
        for (int64_t c = 1; c < n_chunks; ++c) {                  // chunks hold ascending indices: strict < keeps the lowest on equal d^2
            const int64_t w = (c * B + f) * max_a + i;
            const double e = ws_d2[w];
            if (e < d2) { d2 = e; idx = ws_idx[w]; }
        }
        const double d = sqrt(d2);
        if (out_dist) out_dist[a0 + i] = d;
        if (out_idx) out_idx[a0 + i] = idx;
        v[0] += d; v[1] += d2; v[2] = d > v[2] ? d : v[2];
#pragma unroll
        for (int k = 0; k < NN_MAX_K; ++k) v[3 + k] += (k < thr.k && d < thr.tau[k]) ? 1.0 : 0.0;
    }
    if (!partial) return;
#pragma unroll
    for (int k = 0; k < NN_NRED; ++k) {                           // butterfly over the wave: the same tree whatever the data
        for (int o = 32; o > 0; o >>= 1) {
            const double u = __shfl_xor(v[k], o, 64);
            v[k] = k == 2 ? (u > v[k] ? u : v[k]) : v[k] + u;
        }
    }
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < NN_NRED; ++k) red[threadIdx.x >> 6][k] = v[k];
    __syncthreads();
    if (threadIdx.x < NN_NRED) {
        const int k = threadIdx.x;
        double t = red[0][k];
        for (int w = 1; w < 4; ++w) t = k == 2 ? (red[w][k] > t ? red[w][k] : t) : t + red[w][k];
        partial[((int64_t)f * gridDim.x + blockIdx.x) * NN_NRED + k] = t;
    }
}

// raw[f][dir][0 .. 2 + K] = the frame's partials added in block order (max for [2]); zeros for a frame with an empty side
__global__ __launch_bounds__(256) void nn_reduce_kernel(const int64_t* __restrict__ a_off, const int64_t* __restrict__ b_off, int64_t max_a,
                                                        int64_t max_b, int64_t n_blocks, const double* __restrict__ partial, int K, int dir,
                                                        double* __restrict__ raw) {
    __shared__ double sh[256][NN_NRED];
    const int f = blockIdx.x;
    int64_t na = a_off[f + 1] - a_off[f], nb = b_off[f + 1] - b_off[f];
    na = na < max_a ? na : max_a;
    nb = nb < max_b ? nb : max_b;
    const int64_t used = (na > 0 && nb > 0) ? (na + NN_ROWS - 1) / NN_ROWS : 0;       // <= n_blocks: na <= max_a
    const int k = threadIdx.x;
    double t = 0.0;
    for (int64_t x0 = 0; x0 < used; x0 += 256) {
        const int cnt = (int)(used - x0 < 256 ? used - x0 : 256);
        __syncthreads();
        if ((int)threadIdx.x < cnt)
#pragma unroll
            for (int q = 0; q < NN_NRED; ++q) sh[threadIdx.x][q] = partial[((int64_t)f * n_blocks + x0 + threadIdx.x) * NN_NRED + q];
        __syncthreads();
        if (k < 3 + K)
            for (int x = 0; x < cnt; ++x) t = k == 2 ? (sh[x][k] > t ? sh[x][k] : t) : t + sh[x][k];
    }
    if (k < 3 + K) raw[((int64_t)f * 2 + dir) * (3 + K) + k] = t;
}

inline int64_t nn_blocks(int64_t max_a) { return (max_a + NN_ROWS - 1) / NN_ROWS; }

// the b rows per chunk: a pure function of the host arguments
inline int64_t nn_auto_chunk(int B, int64_t max_a, int64_t max_b) {
    const int64_t tiles = (max_b + NN_TILE - 1) / NN_TILE;
    const int64_t row_blocks = nn_blocks(max_a) * B;
    if (tiles <= 1 || row_blocks <= 0) return NN_TILE;
    int64_t want = (NN_TARGET_WG + row_blocks - 1) / row_blocks;
    want = want < tiles ? want : tiles;
    const int64_t chunk = (tiles + want - 1) / want * NN_TILE;
    return chunk < NN_MAX_CHUNK ? chunk : NN_MAX_CHUNK;
}

inline int64_t nn_chunks(int64_t max_b, int64_t chunk) { const int64_t n = (max_b + chunk - 1) / chunk; return n > 0 ? n : 1; }
// -1 where the workspace would pass 2^60 bytes (the product is taken in 128 bits: the accepted ranges alone do not bound it below 2^63)
inline int64_t nn_ws_bytes(int B, int64_t max_a, int64_t max_b, int64_t chunk) {
    const __int128 n = (__int128)nn_chunks(max_b, chunk) * B * max_a * 16;
    return n < ((__int128)1 << 60) ? (int64_t)n : -1;
}
inline int64_t nn_partial_bytes(int B, int64_t max_a) { return nn_blocks(max_a) * B * NN_NRED * 8; }

// one direction: a's rows against b's
int nn_direction(const float* a, const int64_t* a_off, const float* b, const int64_t* b_off, int B, int64_t max_a, int64_t max_b, int64_t chunk,
                 double* out_dist, int64_t* out_idx, const NnThresholds& thr, int dir, double* raw, char* scratch, hipStream_t st) {
    const int64_t n_blocks = nn_blocks(max_a), n_chunks = nn_chunks(max_b, chunk);
    double* partial = raw ? reinterpret_cast<double*>(scratch) : nullptr;
    char* ws = scratch + nn_partial_bytes(B, max_a);
    double* ws_d2 = reinterpret_cast<double*>(ws);
    int64_t* ws_idx = reinterpret_cast<int64_t*>(ws + n_chunks * B * max_a * 8);
    if (max_a > 0) {
        if (max_b > 0)
            hipLaunchKernelGGL(nn_chunk_kernel, dim3((unsigned)n_blocks, B, (unsigned)n_chunks), dim3(256), 0, st, a, a_off, b, b_off, B, max_a, max_b,
                               chunk, ws_d2, ws_idx);
        if (out_dist || out_idx || raw)
            hipLaunchKernelGGL(nn_finish_kernel, dim3((unsigned)n_blocks, B), dim3(256), 0, st, a_off, b_off, B, max_a, max_b, chunk, ws_d2, ws_idx, out_dist,
                               out_idx, thr, partial);
    }
    if (raw) hipLaunchKernelGGL(nn_reduce_kernel, dim3(B), dim3(256), 0, st, a_off, b_off, max_a, max_b, n_blocks, partial, thr.k, dir, raw);
    RALD_HIP(hipGetLastError());
    return 0;
}

}  // namespace

int64_t cloud_metrics_scratch_bytes(int B, int64_t max_pred, int64_t max_gt) {
    if (B < 1 || B > 65535 || max_pred < 0 || max_gt < 0 || max_pred >= (int64_t)1 << 38 || max_gt >= (int64_t)1 << 38) return -1;
    const int64_t w0 = nn_ws_bytes(B, max_pred, max_gt, nn_auto_chunk(B, max_pred, max_gt));
    const int64_t w1 = nn_ws_bytes(B, max_gt, max_pred, nn_auto_chunk(B, max_gt, max_pred));
    if (w0 < 0 || w1 < 0) return -1;
    const int64_t d0 = nn_partial_bytes(B, max_pred) + w0, d1 = nn_partial_bytes(B, max_gt) + w1;
    return (d0 > d1 ? d0 : d1) + 16;
}

int64_t cloud_nn_scratch_bytes(int B, int64_t max_a, int64_t max_b, int64_t b_chunk) {
    if (B < 1 || B > 65535 || max_a < 0 || max_b < 0 || max_a >= (int64_t)1 << 38 || max_b >= (int64_t)1 << 38) return -1;
    if (b_chunk < 0 || b_chunk % NN_TILE != 0 || b_chunk > NN_MAX_CHUNK) return -1;
    const int64_t w = nn_ws_bytes(B, max_a, max_b, b_chunk ? b_chunk : nn_auto_chunk(B, max_a, max_b));
    return w < 0 ? -1 : nn_partial_bytes(B, max_a) + w + 16;
}

int cloud_nn_ragged(const float* a, const int64_t* a_off, const float* b, const int64_t* b_off, int B, int64_t max_a, int64_t max_b, int64_t b_chunk,
                    double* out_dist, int64_t* out_idx, void* scratch, int64_t scratch_bytes, hipStream_t st) {
    RALD_CHECK(a_off && b_off && B >= 1 && B <= 65535 && max_a >= 0 && max_b >= 0, "cloud_nn_ragged: bad argument");
    RALD_CHECK(max_a < (int64_t)1 << 38 && max_b < (int64_t)1 << 38, "cloud_nn_ragged: point sets too large");
    RALD_CHECK(b_chunk >= 0 && b_chunk % NN_TILE == 0 && b_chunk <= NN_MAX_CHUNK, "cloud_nn_ragged: b_chunk must be 0 or a multiple of 1024 up to 2^30");
    RALD_CHECK(scratch && (uintptr_t)scratch % 8 == 0, "cloud_nn_ragged: null or unaligned scratch");
    const int64_t need = cloud_nn_scratch_bytes(B, max_a, max_b, b_chunk);
    RALD_CHECK(need >= 0, "cloud_nn_ragged: workspace too large");
    RALD_CHECK(scratch_bytes >= need, "cloud_nn_ragged: scratch too small");
    RALD_CHECK(b_chunk == 0 || nn_chunks(max_b, b_chunk) <= 65535, "cloud_nn_ragged: too many chunks");
    RALD_CHECK((max_a == 0 || max_b == 0) || (a && b), "cloud_nn_ragged: null pointer");
    NnThresholds thr = {};
    return nn_direction(a, a_off, b, b_off, B, max_a, max_b, b_chunk ? b_chunk : nn_auto_chunk(B, max_a, max_b), out_dist, out_idx, thr, 0, nullptr,
                        (char*)scratch, st);
}

int cloud_metrics_ragged(const float* pred, const int64_t* pred_off, const float* gt, const int64_t* gt_off, int B, int64_t max_pred, int64_t max_gt,
                         const double* thresholds_host, int n_thr, double* out_raw, double* out_dist_pred, int64_t* out_idx_pred,
                         double* out_dist_gt, int64_t* out_idx_gt, void* scratch, hipStream_t st) {
    RALD_CHECK(pred_off && gt_off && out_raw && B >= 1 && B <= 65535 && max_pred >= 0 && max_gt >= 0, "cloud_metrics_ragged: bad argument");
    RALD_CHECK(max_pred < (int64_t)1 << 38 && max_gt < (int64_t)1 << 38, "cloud_metrics_ragged: point sets too large");
    RALD_CHECK(cloud_metrics_scratch_bytes(B, max_pred, max_gt) >= 0, "cloud_metrics_ragged: workspace too large");
    RALD_CHECK(n_thr >= 0 && n_thr <= NN_MAX_K && (n_thr == 0 || thresholds_host), "cloud_metrics_ragged: at most 8 thresholds");
    NnThresholds thr = {};
    thr.k = n_thr;
    for (int k = 0; k < n_thr; ++k) {
        RALD_CHECK(std::isfinite(thresholds_host[k]) && thresholds_host[k] >= 0.0, "cloud_metrics_ragged: thresholds must be finite and >= 0");
        thr.tau[k] = thresholds_host[k];
    }
    RALD_CHECK(scratch && (uintptr_t)scratch % 8 == 0, "cloud_metrics_ragged: null or unaligned scratch");
    RALD_CHECK((max_pred == 0 || max_gt == 0) || (pred && gt), "cloud_metrics_ragged: null pointer");
    int rc = nn_direction(pred, pred_off, gt, gt_off, B, max_pred, max_gt, nn_auto_chunk(B, max_pred, max_gt), out_dist_pred, out_idx_pred, thr, 0,
                          out_raw, (char*)scratch, st);
    if (rc) return rc;
    return nn_direction(gt, gt_off, pred, pred_off, B, max_gt, max_pred, nn_auto_chunk(B, max_gt, max_pred), out_dist_gt, out_idx_gt, thr, 1, out_raw,
                        (char*)scratch, st);
}

}  // namespace rald
