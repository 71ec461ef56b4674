// ICP registration of the clouds of one ragged batch onto the clouds of another, point-to-point and point-to-plane, and the rigid
// transform of a ragged batch.  The definition is in include/rald_hip.h; in short, per pair b and iteration
//   move        p' = ((R_k0 px + R_k1 py) + R_k2 pz) + t_k in float64, pf = fp32(p')
//   correspond  q = the target row inside the grid of the smallest fp32 rad_d2(pf, q) <= fl(max_dist^2), the lowest row on equal d2
//   accumulate  the 21 + 6 + 1 + 1 float64 sums of J^T J, J^T r, r r, |d|^2 and the count over the source rows in the fixed sum shape
//   solve       Cholesky of the 6 x 6 system with the pivot floor A_jj 2^-30, x = (w, u)
//   update      the Cayley rotation of a = w / 2, R <- dR R, t <- dR t + u; converged iff max |x_k| <= tolerance
// Launches, all on one stream, none waits on another workgroup, no atomics at all:
//   the index of the TARGET (cloud_index.hip: keys, stable sort, the rows in sorted order), once
//   icp_init       one lane per pair               the transform (init or the identity), done / status / iterations / last step
//   icp_transform, the index build over the SOURCE under the initial transform (no rows): the lane order of icp_correspond, once
//   per iteration, and once more with the final transform (the evaluation, which skips nothing):
//   icp_correspond (256 sorted positions, pair)    the hot path: one lane per source row, in the order of the rows' INITIAL cells, so a
//                                                  wave's lanes walk the same lines while the motion is small; it moves its row and
//                                                  walks the target's index with radius_walk of cloud_index.h - `me` is the moved row,
//                                                  the keys and rows are the target's; the row's target index (4 bytes) goes to the
//                                                  scratch at the row's place
//   icp_sums       (1024 source rows, pair)        256 lanes, four rows a lane: a lane holds rows t, t + 256, t + 512, t + 768 of the
//                                                  block, so the first two levels of the halving tree are register adds; the 29 trees
//                                                  meet in LDS once (58 KiB, one barrier), wave w finishes the trees k = w mod 4 with
//                                                  the levels 128 and 64 from LDS and the last six by lane shifts
//   icp_solve      one wave per pair               lane k adds sum k's blocks left to right (29 lanes, two more for the counts), lane 0
//                                                  then solves, updates and sets the status; in the evaluation it writes the outputs
// A pair that is finished sets done[b]; every kernel of a later iteration returns on it.  The iterations are a host loop over the
// same launches with no host read.
// Every loop is bounded by the cloud's length, the scan range's cells, 6, 29 or 32.  Every index read from the scratch (a sorted row's
// index, a correspondence) is clamped into its cloud before it addresses anything.
#include "cloud_index.h"
#include "kernels.h"

namespace rald {

namespace {

constexpr int ICP_T = 256;                                   // threads of icp_correspond, icp_sums and the transform kernel
constexpr int ICP_R = CLOUD_SEG / ICP_T;                     // rows per lane of icp_sums
constexpr int ICP_NS = 29;                                   // float64 sums: 21 of J^T J, 6 of J^T r, r r, |d|^2
constexpr int ICP_MAX_ITER = 64;
static_assert(ICP_R == 4, "icp_sums holds the first two tree levels in registers");

struct IcpArgs {
    RaggedCloud s, t;                                        // source and target
    CellGrid g;
    float r2, rs;
    int mode, min_corr, final;                               // final: the evaluation pass
    double tol;
    const float* tnormals;                                   // [n_tgt_total, 3], plane mode
    const double* init;                                      // [batch, 12], nullable
    const unsigned* tkey; const float4* trow;                // [n_tgt_total] the target's sorted keys and rows
    int64_t nseg_max;
    float* pf0; const int* sorder;                           // [n_src_total] the source under the initial transform; its rows sorted by cell
    int32_t* corr;                                           // [n_src_total] per source row: its target row, -1 for none
    double* bsum; int* bcnt;                                 // [batch][nseg_max][29], [batch][nseg_max][2] (counting, usable)
    double* T;                                               // [batch][12] R row-major, t
    double* lastx;                                           // [batch]
    int* done; int* status; int* iters;                      // [batch]
    double* out_transform; double* out_stats; int32_t* out_info; int64_t* out_corr; float* out_moved;
};

// step 1 of the definition: the moved row in float64, R and t the twelve doubles at T
__device__ __forceinline__ void icp_move(const double* T, float x, float y, float z, double* p) {
#pragma clang fp contract(off)
    const double px = (double)x, py = (double)y, pz = (double)z;
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = ((T[k * 3] * px + T[k * 3 + 1] * py) + T[k * 3 + 2] * pz) + T[9 + k];
}

__global__ __launch_bounds__(64) void icp_init(IcpArgs a) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.s.batch) return;
    double* T = a.T + (int64_t)b * 12;
    for (int k = 0; k < 12; ++k) T[k] = a.init ? a.init[(int64_t)b * 12 + k] : ((k == 0 || k == 4 || k == 8) ? 1.0 : 0.0);
    a.done[b] = 0; a.status[b] = 0; a.iters[b] = 0;
    a.lastx[b] = 0.0;
}

// the transform's twelve doubles come as an argument of their own: `const __restrict__` lets the uniform reads be scalar loads
__global__ __launch_bounds__(ICP_T) void icp_correspond(IcpArgs a, const double* __restrict__ Tall) {
    const int b = blockIdx.y;
    if (!a.final && a.done[b]) return;
    int64_t s0, t0;
    const int n = ragged_span(a.s, b, s0);
    int64_t j = (int64_t)blockIdx.x * ICP_T + threadIdx.x;
    if (j >= n) return;
    j = rad_clamp(a.sorder[s0 + j], n);                      // a wave's lanes are neighbours in space while the motion is small
    const int nt = ragged_span(a.t, b, t0);
    const float* p = a.s.points + (s0 + j) * 3;
    const float x = p[0], y = p[1], z = p[2];
    double pd[3];
    icp_move(Tall + (int64_t)b * 12, x, y, z, pd);
    const float4 me = make_float4((float)pd[0], (float)pd[1], (float)pd[2], 0.f);
    int bestj = -1;
    if (isfinite(x) && isfinite(y) && isfinite(z) && isfinite(me.x) && isfinite(me.y) && isfinite(me.z) && nt > 0) {
        float best = INFINITY;
        const float r2 = a.r2;
        radius_walk(a.g, a.rs, a.tkey + t0, a.trow + t0, nt, me, [&](int, const float4& o, float d2) {
            if (!(d2 <= r2)) return false;
            const int jr = rad_clamp(__float_as_int(o.w), nt);               // a row index from the scratch
            if (d2 < best || (d2 == best && jr < bestj)) { best = d2; bestj = jr; }
            return false;
        });
    }
    a.corr[s0 + j] = bestj;
    if (a.final) {
        if (a.out_corr) a.out_corr[s0 + j] = bestj;
        if (a.out_moved) { float* m = a.out_moved + (s0 + j) * 3; m[0] = me.x; m[1] = me.y; m[2] = me.z; }
    }
}

// one equation of a row: J = (p x n, n), r = n . d; its 28 products are added to acc (the first equation: stored)
template <bool FIRST>
__device__ __forceinline__ void icp_equation(const double* p, const double* d, double n0, double n1, double n2, double* acc) {
#pragma clang fp contract(off)
    const double J[6] = {p[1] * n2 - p[2] * n1, p[2] * n0 - p[0] * n2, p[0] * n1 - p[1] * n0, n0, n1, n2};
    const double r = (n0 * d[0] + n1 * d[1]) + n2 * d[2];
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = i; j < 6; ++j, ++k) acc[k] = FIRST ? J[i] * J[j] : acc[k] + J[i] * J[j];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i, ++k) acc[k] = FIRST ? J[i] * r : acc[k] + J[i] * r;
    acc[27] = FIRST ? r * r : acc[27] + r * r;
}

template <int MODE>
__global__ __launch_bounds__(ICP_T) void icp_sums(IcpArgs a, const double* __restrict__ Tall) {
#pragma clang fp contract(off)
    __shared__ double v[ICP_NS][ICP_T];
    __shared__ int sh[2][ICP_T / 64];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (!a.final && a.done[b]) return;                       // the whole workgroup, here and below
    int64_t s0, t0;
    const int n = ragged_span(a.s, b, s0);
    const int64_t base = (int64_t)blockIdx.x * CLOUD_SEG;
    if (base >= n) return;
    const int nt = ragged_span(a.t, b, t0);
    const double* T = Tall + (int64_t)b * 12;
    double row[ICP_R][ICP_NS];
    int counting = 0, usable = 0;
#pragma unroll
    for (int r = 0; r < ICP_R; ++r) {
        const int64_t j = base + r * ICP_T + tid;
        bool counts = false;
        double pd[3] = {0.0, 0.0, 0.0}, d[3] = {0.0, 0.0, 0.0}, nr[3] = {0.0, 0.0, 0.0};
        if (j < n) {
            const float* p = a.s.points + (s0 + j) * 3;
            const float x = p[0], y = p[1], z = p[2];
            usable += isfinite(x) && isfinite(y) && isfinite(z);
            const int c = a.corr[s0 + j];
            if (c >= 0 && nt > 0) {                          // a correspondence: the row is usable and its pf finite
                const int64_t q = t0 + (c < nt ? c : nt - 1);
                icp_move(T, x, y, z, pd);
                const float* tq = a.t.points + q * 3;
#pragma unroll
                for (int k = 0; k < 3; ++k) d[k] = pd[k] - (double)tq[k];
                counts = true;
                if (MODE == 1) {
                    const float* tn = a.tnormals + q * 3;
                    const float n0 = tn[0], n1 = tn[1], n2 = tn[2];
                    counts = isfinite(n0) && isfinite(n1) && isfinite(n2) && !(n0 == 0.f && n1 == 0.f && n2 == 0.f);
                    nr[0] = (double)n0; nr[1] = (double)n1; nr[2] = (double)n2;
                }
            }
        }
        counting += counts;
        if (MODE == 1) {
            icp_equation<true>(pd, d, nr[0], nr[1], nr[2], row[r]);
        } else {
            icp_equation<true>(pd, d, 1.0, 0.0, 0.0, row[r]);
            icp_equation<false>(pd, d, 0.0, 1.0, 0.0, row[r]);
            icp_equation<false>(pd, d, 0.0, 0.0, 1.0, row[r]);
        }
        row[r][28] = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
#pragma unroll
        for (int k = 0; k < ICP_NS; ++k) row[r][k] = counts ? row[r][k] : 0.0;
    }
    // the halving tree over the block's 1024 values: the levels 512 and 256 in registers
#pragma unroll
    for (int k = 0; k < ICP_NS; ++k) v[k][tid] = (row[0][k] + row[2][k]) + (row[1][k] + row[3][k]);
    int cw = counting, uw = usable;
    for (int s = 32; s >= 1; s >>= 1) { cw += __shfl_down(cw, s); uw += __shfl_down(uw, s); }
    if (lane == 0) { sh[0][w] = cw; sh[1][w] = uw; }
    __syncthreads();
    double* bs = a.bsum + ((int64_t)b * a.nseg_max + blockIdx.x) * ICP_NS;
    for (int k = w; k < ICP_NS; k += ICP_T / 64) {           // the levels 128 and 64, then 32 .. 1 inside the wave
        double x = (v[k][lane] + v[k][lane + 128]) + (v[k][lane + 64] + v[k][lane + 192]);
        for (int s = 32; s >= 1; s >>= 1) x = x + __shfl_down(x, s);
        if (lane == 0) bs[k] = x;
    }
    if (tid == 0) {
        int* bc2 = a.bcnt + ((int64_t)b * a.nseg_max + blockIdx.x) * 2;
        bc2[0] = (sh[0][0] + sh[0][1]) + (sh[0][2] + sh[0][3]);
        bc2[1] = (sh[1][0] + sh[1][1]) + (sh[1][2] + sh[1][3]);
    }
}

// steps 4 and 5 of the definition; false iff a pivot was refused or x is not finite (T untouched then)
__device__ __forceinline__ bool icp_step(const double* S, double* T, double* max_x) {
#pragma clang fp contract(off)
    double A[6][6], L[6][6], y[6], x[6];
    int k = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j, ++k) A[i][j] = S[k];
    for (int j = 0; j < 6; ++j) {
        double s = A[j][j];
        for (int q = 0; q < j; ++q) s = s - L[j][q] * L[j][q];
        if (!(isfinite(s) && s > A[j][j] * 9.313225746154785e-10)) return false;     // 2^-30
        const double ljj = __dsqrt_rn(s);
        L[j][j] = ljj;
        for (int i = j + 1; i < 6; ++i) {
            double t = A[j][i];
            for (int q = 0; q < j; ++q) t = t - L[i][q] * L[j][q];
            L[i][j] = t / ljj;
        }
    }
    for (int i = 0; i < 6; ++i) {
        double s = -S[21 + i];
        for (int q = 0; q < i; ++q) s = s - L[i][q] * y[q];
        y[i] = s / L[i][i];
    }
    for (int i = 5; i >= 0; --i) {
        double s = y[i];
        for (int q = i + 1; q < 6; ++q) s = s - L[q][i] * x[q];
        x[i] = s / L[i][i];
    }
    double mx = 0.0;
    for (int i = 0; i < 6; ++i) {
        if (!isfinite(x[i])) return false;
        const double ax = fabs(x[i]);
        mx = ax > mx ? ax : mx;
    }
    const double w0 = x[0], w1 = x[1], w2 = x[2];
    const double a0 = w0 * 0.5, a1 = w1 * 0.5, a2 = w2 * 0.5;
    const double aa = (a0 * a0 + a1 * a1) + a2 * a2;
    const double den = 1.0 + aa, c = 1.0 - aa;
    const double dR[3][3] = {{(c + w0 * a0) / den, (w0 * a1 - w2) / den, (w0 * a2 + w1) / den},
                             {(w1 * a0 + w2) / den, (c + w1 * a1) / den, (w1 * a2 - w0) / den},
                             {(w2 * a0 - w1) / den, (w2 * a1 + w0) / den, (c + w2 * a2) / den}};
    double N[12];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) N[i * 3 + j] = (dR[i][0] * T[j] + dR[i][1] * T[3 + j]) + dR[i][2] * T[6 + j];
        N[9 + i] = ((dR[i][0] * T[9] + dR[i][1] * T[10]) + dR[i][2] * T[11]) + x[3 + i];
    }
    for (int i = 0; i < 12; ++i) T[i] = N[i];
    *max_x = mx;
    return true;
}

__global__ __launch_bounds__(64) void icp_solve(IcpArgs a) {
#pragma clang fp contract(off)
    const int b = blockIdx.x, lane = threadIdx.x;
    if (!a.final && a.done[b]) return;                       // the whole wave
    int64_t s0;
    const int n = ragged_span(a.s, b, s0);
    const int nseg = (n + CLOUD_SEG - 1) / CLOUD_SEG;        // <= nseg_max: n <= max_per_sample
    const double* bs = a.bsum + (int64_t)b * a.nseg_max * ICP_NS;
    const int* bc = a.bcnt + (int64_t)b * a.nseg_max * 2;
    double sum = 0.0;                                        // lane k < 29: sum k, the blocks left to right; lanes 29, 30: the counts
    int cnt = 0;
    if (lane < ICP_NS) {
        int g = 0;
        for (; g + 16 <= nseg; g += 16) {                    // sixteen loads in flight, then their adds in order
            double v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = bs[(int64_t)(g + u) * ICP_NS + lane];
#pragma unroll
            for (int u = 0; u < 16; ++u) sum = sum + v[u];
        }
        for (; g < nseg; ++g) sum = sum + bs[(int64_t)g * ICP_NS + lane];
    } else if (lane < ICP_NS + 2) {
        for (int g = 0; g < nseg; ++g) cnt += bc[g * 2 + (lane - ICP_NS)];
    }
    double S[ICP_NS];
#pragma unroll
    for (int k = 0; k < ICP_NS; ++k) S[k] = __shfl(sum, k);
    const int count = __shfl(cnt, ICP_NS), usable = __shfl(cnt, ICP_NS + 1);
    if (lane != 0) return;
    double* T = a.T + (int64_t)b * 12;
    if (!a.final) {
        if (count < a.min_corr) { a.done[b] = 1; a.status[b] = 2; return; }
        double mx;
        if (!icp_step(S, T, &mx)) { a.done[b] = 1; a.status[b] = 3; return; }
        a.iters[b] += 1;
        a.lastx[b] = mx;
        if (mx <= a.tol) { a.done[b] = 1; a.status[b] = 1; }
        return;
    }
    double* o = a.out_transform + (int64_t)b * 16;
    for (int i = 0; i < 3; ++i) {
        o[i * 4] = T[i * 3]; o[i * 4 + 1] = T[i * 3 + 1]; o[i * 4 + 2] = T[i * 3 + 2]; o[i * 4 + 3] = T[9 + i];
    }
    o[12] = 0.0; o[13] = 0.0; o[14] = 0.0; o[15] = 1.0;
    double* st = a.out_stats + (int64_t)b * 4;
    st[0] = usable > 0 ? (double)count / (double)usable : 0.0;
    st[1] = count > 0 ? __dsqrt_rn(S[28] / (double)count) : 0.0;
    st[2] = a.lastx[b];
    st[3] = S[27];
    int32_t* info = a.out_info + (int64_t)b * 3;
    info[0] = a.status[b]; info[1] = a.iters[b]; info[2] = count;
}

// the scratch, described once; a.s and a.t are set
void icp_layout(IcpArgs& a, CloudIndex& ix, CloudIndex& ixs, Carver& s, int64_t chunk) {
    const int64_t B = a.s.batch;
    cloud_index_layout(ix, a.t, s, chunk, true);
    a.nseg_max = (a.s.max_per_sample + CLOUD_SEG - 1) / CLOUD_SEG;
    a.corr = s.take<int32_t>(a.s.n_total);
    a.bsum = s.take<double>(B * a.nseg_max * ICP_NS);
    a.bcnt = s.take<int>(B * a.nseg_max * 2);
    a.T = s.take<double>(B * 12);
    a.lastx = s.take<double>(B);
    a.done = s.take<int>(B);
    a.status = s.take<int>(B);
    a.iters = s.take<int>(B);
    a.pf0 = s.take<float>(a.s.n_total * 3);
    cloud_index_layout(ixs, a.s, s, 0, false);               // the source's lane order: keys and row indices, no rows
}

struct TransformArgs {
    RaggedCloud c;
    const double* T;
    int stride;                                              // 12 or 16 doubles a cloud
    const float* normals;
    float* out_points; float* out_normals;
};

__global__ __launch_bounds__(ICP_T) void icp_transform(TransformArgs a, const double* __restrict__ Tall) {
#pragma clang fp contract(off)
    const int b = blockIdx.y;
    int64_t row0;
    const int n = ragged_span(a.c, b, row0);
    const int64_t j = (int64_t)blockIdx.x * ICP_T + threadIdx.x;
    if (j >= n) return;
    const double* M = Tall + (int64_t)b * a.stride;
    double T[12];
    if (a.stride == 12) {
        for (int k = 0; k < 12; ++k) T[k] = M[k];
    } else {
        for (int i = 0; i < 3; ++i) { T[i * 3] = M[i * 4]; T[i * 3 + 1] = M[i * 4 + 1]; T[i * 3 + 2] = M[i * 4 + 2]; T[9 + i] = M[i * 4 + 3]; }
    }
    const float* p = a.c.points + (row0 + j) * 3;
    double pd[3];
    icp_move(T, p[0], p[1], p[2], pd);
    float* o = a.out_points + (row0 + j) * 3;
    o[0] = (float)pd[0]; o[1] = (float)pd[1]; o[2] = (float)pd[2];
    if (a.normals) {
        const float* m = a.normals + (row0 + j) * 3;
        T[9] = 0.0; T[10] = 0.0; T[11] = 0.0;
        icp_move(T, m[0], m[1], m[2], pd);
        float* on = a.out_normals + (row0 + j) * 3;
        on[0] = (float)pd[0]; on[1] = (float)pd[1]; on[2] = (float)pd[2];
    }
}

bool icp_sizes_ok(int B, int64_t n_src_total, int64_t max_src, int64_t n_tgt_total, int64_t max_tgt, int64_t chunk) {
    return cloud_sizes_ok(B, n_src_total, max_src, 0) && cloud_sizes_ok(B, n_tgt_total, max_tgt, chunk);
}

}  // namespace

int64_t icp_scratch_bytes(int B, int64_t n_src_total, int64_t max_src, int64_t n_tgt_total, int64_t max_tgt, int64_t chunk) {
    if (!icp_sizes_ok(B, n_src_total, max_src, n_tgt_total, max_tgt, chunk)) return -1;
    IcpArgs a{};
    a.s = ragged_cloud(nullptr, nullptr, nullptr, B, 0, n_src_total, max_src);
    a.t = ragged_cloud(nullptr, nullptr, nullptr, B, 0, n_tgt_total, max_tgt);
    CloudIndex ix{}, ixs{};
    Carver s{nullptr, 0};
    icp_layout(a, ix, ixs, s, chunk);
    return s.used;
}

int icp_ragged(const RaggedCloud& src, const RaggedCloud& tgt, const float* target_normals, const GridSpec& grid, int mode, float max_dist,
               int max_iterations, double tolerance, int min_correspondences, const double* init, double* out_transform, double* out_stats,
               int32_t* out_info, int64_t* out_corr, float* out_moved, void* scratch, int64_t scratch_bytes, int64_t chunk, hipStream_t st) {
#pragma clang fp contract(off)
    const std::string who = "icp_ragged";
    RALD_CHECK(src.points && tgt.points && out_transform && out_stats && out_info,
               who + ": null pointer (source, target, out_transform, out_stats, out_info)");
    RALD_CHECK(mode == 0 || mode == 1, who + ": mode must be 0 (point) or 1 (plane)");
    RALD_CHECK(mode == 0 || target_normals, who + ": plane mode needs target_normals");
    RALD_CHECK(std::isfinite(max_dist) && max_dist > 0.f, who + ": max_distance must be finite and > 0");
    RALD_CHECK(max_iterations >= 1 && max_iterations <= ICP_MAX_ITER, who + ": max_iterations must be in 1 .. 64");
    RALD_CHECK(tolerance >= 0.0, who + ": tolerance must be >= 0");                    // NaN fails
    RALD_CHECK(min_correspondences >= 1, who + ": min_correspondences must be >= 1");
    RALD_CHECK(src.batch == tgt.batch, who + ": source and target must have the same batch");
    RALD_CHECK(grid.lo && grid.v && grid.dims, who + ": null grid (lo3, v3, dims3)");
    for (int k = 0; k < 3; ++k) RALD_CHECK(grid.v[k] >= max_dist, who + ": every cell edge must be >= max_distance");   // NaN fails
    IcpArgs a{};
    RALD_TRY(cloud_grid_check(who + " (source)", src, grid, 0, &a.g));
    RALD_TRY(cloud_grid_check(who + " (target)", tgt, grid, chunk, &a.g));
    RALD_TRY(scratch_check(who, scratch, scratch_bytes,
                           icp_scratch_bytes(src.batch, src.n_total, src.max_per_sample, tgt.n_total, tgt.max_per_sample, chunk)));
    a.s = src; a.t = tgt;
    a.mode = mode; a.min_corr = min_correspondences; a.tol = tolerance;
    a.r2 = max_dist * max_dist;
    a.rs = scan_reach(max_dist);
    a.tnormals = target_normals; a.init = init;
    a.out_transform = out_transform; a.out_stats = out_stats; a.out_info = out_info; a.out_corr = out_corr; a.out_moved = out_moved;
    CloudIndex ix, ixs;
    Carver s{(char*)scratch, 0};
    icp_layout(a, ix, ixs, s, chunk);
    const SortedCloud sorted = cloud_index_build(ix, a.g, nullptr, st);
    a.tkey = sorted.key; a.trow = sorted.rows;
    const int B = src.batch;
    const dim3 by_row((unsigned)((src.max_per_sample + ICP_T - 1) / ICP_T), B);
    const dim3 by_seg((unsigned)a.nseg_max, B);
    const dim3 by_cloud((B + 63) / 64);
    hipLaunchKernelGGL(icp_init, by_cloud, dim3(64), 0, st, a);
    // the lane order of icp_correspond: the source rows sorted by the target grid's cell of their INITIAL pf, by the same index build
    const TransformArgs first{src, a.T, 12, nullptr, a.pf0, nullptr};
    hipLaunchKernelGGL(icp_transform, by_row, dim3(ICP_T), 0, st, first, (const double*)a.T);
    ixs.c.points = a.pf0;
    a.sorder = cloud_index_build(ixs, a.g, nullptr, st).idx;
    for (int i = 0; i <= max_iterations; ++i) {              // the last turn is the evaluation
        a.final = i == max_iterations;
        hipLaunchKernelGGL(icp_correspond, by_row, dim3(ICP_T), 0, st, a, (const double*)a.T);
        if (mode == 1) hipLaunchKernelGGL(icp_sums<1>, by_seg, dim3(ICP_T), 0, st, a, (const double*)a.T);
        else hipLaunchKernelGGL(icp_sums<0>, by_seg, dim3(ICP_T), 0, st, a, (const double*)a.T);
        hipLaunchKernelGGL(icp_solve, dim3(B), dim3(64), 0, st, a);
    }
    RALD_HIP(hipGetLastError());
    return 0;
}

int rigid_transform_ragged(const RaggedCloud& c, const double* transforms, int stride, const float* normals, float* out_points,
                           float* out_normals, hipStream_t st) {
    const std::string who = "rigid_transform_ragged";
    RALD_CHECK(c.points && transforms && out_points, who + ": null pointer (points, transforms, out_points)");
    RALD_CHECK(stride == 12 || stride == 16, who + ": a transform has 12 (R row-major, t) or 16 (4 x 4 row-major) doubles");
    RALD_CHECK(!normals == !out_normals, who + ": normals and out_normals come together");
    RALD_CHECK(cloud_sizes_ok(c.batch, c.n_total, c.max_per_sample, 0), who + ": batch 1 .. 65535, n_total 0 .. 2^31 - 1, max_per_sample 1 .. 2^24");
    RALD_CHECK(c.offsets || c.n_dense >= 0, who + ": n_dense must be >= 0 without offsets");
    const TransformArgs a{c, transforms, stride, normals, out_points, out_normals};
    hipLaunchKernelGGL(icp_transform, dim3((unsigned)((c.max_per_sample + ICP_T - 1) / ICP_T), c.batch), dim3(ICP_T), 0, st, a, transforms);
    RALD_HIP(hipGetLastError());
    return 0;
}

}  // namespace rald
