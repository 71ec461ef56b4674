// RANSAC plane segmentation inside each cloud of a ragged batch, and the filter that keeps or drops the planes' rows (DESIGN.md section
// 26).  The definition is in include/rald_hip.h; in short, for round j = 0 .. max_planes - 1 of a cloud
//   LIVE_j      the rows with three finite coordinates that no earlier round labelled, in row order; m of them (m < 3: finished)
//   hypothesis  h = 0 .. H - 1: Philox4x32-10(counter (h, j, 0, 0), key (seed mod 2^32, 2)) -> w0 w1 w2, rows LIVE_j[(w_k * m) >> 32];
//               n = (p1 - p0) x (p2 - p0), len2 = |n|^2, all fp32 without contraction; invalid on equal indices or len2 not finite, not > 0
//   inlier      a live row p with fl(s * s) <= fl(fl(t * t) * len2), s = (nx dx + ny dy) + nz dz, d = p - p0: no root, no division
//   winner      the valid h of the largest inlier count, the smallest h on equal counts; below min_inliers (or none): finished
//   plane       refine = 0: n / |n| in float64, through p0.  refine = 1: float64 centroid and central moments of the winner's inliers in
//               the fixed sum shape, six Jacobi sweeps, the smallest eigenvalue's vector through the centroid; the round's inliers are
//               then the live rows with |n . (p - c0)| <= t in float64 (fewer than min_inliers: finished, no plane j)
// Launches, all on one stream, none waits on another workgroup; the only atomics are integer adds on the scores:
//   pln_init         (256 rows, cloud)             labels -1 / -2, the live flag, and the cloud's outputs at "no plane"
//   per round: the compaction of cloud_index.hip over the live flag (the live rows and their indices, in row order), then
//   pln_hypotheses   (256 hypotheses, cloud)       Philox, the three rows, eight floats a hypothesis: n, fl(t*t)*len2 | p0, valid
//   pln_score        (1024 live rows, cloud)       the hot path: 512 lanes, 2 rows a lane in registers, every hypothesis in turn (its eight floats
//                                                  are uniform: scalar loads), ballot + popcount per wave, lane h % 64 keeps the count of
//                                                  h, 64 hypotheses' counts meet in LDS, one atomicAdd per workgroup and hypothesis
//   pln_argmax       (cloud)                       the winner
//   pln_mark 0       (1024 live rows, cloud)       the winner's inlier flags; with refine the block sums of x, y, z and the count
//   pln_fit 0        one lane per cloud            refine = 0: the plane and the commit.  refine = 1: the centroid, blocks left to right
//   pln_mark 1, pln_fit 1   (refine)               the block sums of the six central moments; the sweeps, the plane
//   pln_mark 2, pln_fit 2   (refine)               the float64 flags over the live rows and their block counts; the commit
//   pln_label        (256 live rows, cloud)        the round's number to its inliers, their live flag cleared
// A cloud that is finished sets done[b]; every kernel of a later round returns on it.  The float64 re-mark is pln_mark 2, one lane
// per live row, not the one lane per cloud of pln_fit: a cloud may have 2^24 rows.
// Every loop is bounded by H, K, the cloud's length or 64.  Every index read from the scratch (a live row's index, the winner, the
// live list's offset and length) is clamped into its range before it addresses anything.
#include "cloud_index.h"
#include "kernels.h"
#include "philox.h"
#include "sym3_jacobi.h"

namespace rald {

namespace {

constexpr int PLN_T = 256;                                   // threads of the per-row and per-hypothesis kernels
constexpr int PLN_ST = 512;                                  // threads of pln_score
constexpr int PLN_R = 2;                                     // live rows per lane of pln_score
constexpr int PLN_TILE = PLN_ST * PLN_R;                     // = CLOUD_SEG: the grid of pln_score is the compaction's
constexpr int PLN_SWEEPS = 6;
constexpr int PLN_MAX_H = 65536, PLN_MAX_K = 8;
static_assert(PLN_TILE == CLOUD_SEG, "pln_score shares the grid of the flag kernels");

struct PlaneArgs {
    RaggedCloud c;
    float t, t2;                                             // the threshold, fl(t * t)
    int H, K, min_inliers, refine, round, keep_planes;
    uint32_t seed;
    double view[3];
    int64_t nseg_max;
    int32_t* live;                                           // [n_total] per row: 1 while no round has taken the (usable) row
    float* lp; int64_t* li;                                  // [n_total] the live rows and their indices, compacted per cloud
    BlockScan ls;                                            // the live list's compaction: its offsets and lengths
    float4* hyp;                                             // [batch][H][2]
    int32_t* score;                                          // [batch][H]
    int* best; int* bscore;                                  // [batch] the round's winner (-1: none) and its count
    int* done; int* took;                                    // [batch] finished; the last round that wrote a plane
    unsigned char* inl;                                      // [n_total] per live position: an inlier of the round
    double* bsum; int* bcnt;                                 // [batch][nseg_max][6], [batch][nseg_max]
    double* fit;                                             // [batch][8] the centroid, the plane, the count
    int32_t* labels; double* planes; int32_t* nplanes; int32_t* inliers; int32_t* bests;   // the outputs, or scratch
    int64_t* kept;                                           // the filter: the kept rows' indices
    BlockScan fs;
};

// the cloud's live list: its first position in lp / li / inl and its length, clamped into the cloud and the tensors
__device__ __forceinline__ int pln_live(const PlaneArgs& a, int b, int n, int64_t& l0) {
    l0 = a.ls.out_offsets[b];
    int m = a.ls.total[b];
    m = m < 0 ? 0 : (m < n ? m : n);
    if (l0 < 0 || l0 > a.c.n_total - m) { l0 = 0; m = 0; }
    return m;
}
__device__ __forceinline__ int pln_best(const PlaneArgs& a, int b) {
    const int h = a.best[b];
    return h < a.H ? h : a.H - 1;                            // < 0: none
}

__global__ __launch_bounds__(PLN_T) void pln_init(PlaneArgs a) {
    const int b = blockIdx.y, tid = threadIdx.x;
    int64_t row0;
    const int n = ragged_span(a.c, b, row0);
    if (blockIdx.x == 0) {
        if (tid < a.K) {
            double* p = a.planes + ((int64_t)b * a.K + tid) * 4;
            p[0] = NAN; p[1] = NAN; p[2] = NAN; p[3] = NAN;
            a.inliers[(int64_t)b * a.K + tid] = 0;
            a.bests[(int64_t)b * a.K + tid] = -1;
        }
        if (tid == 0) { a.nplanes[b] = 0; a.done[b] = 0; a.took[b] = -1; }
    }
    const int64_t j = (int64_t)blockIdx.x * PLN_T + tid;
    if (j >= n) return;
    const float* p = a.c.points + (row0 + j) * 3;
    const bool usable = isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]);
    a.labels[row0 + j] = usable ? -1 : -2;
    a.live[row0 + j] = usable;
}

__global__ __launch_bounds__(PLN_T) void pln_hypotheses(PlaneArgs a) {
#pragma clang fp contract(off)
    const int b = blockIdx.y;
    const int h = blockIdx.x * PLN_T + threadIdx.x;
    if (h >= a.H || a.done[b]) return;
    int64_t row0, l0;
    const int n = ragged_span(a.c, b, row0);
    const int m = pln_live(a, b, n, l0);
    float4 A = make_float4(0.f, 0.f, 0.f, NAN), P0 = make_float4(0.f, 0.f, 0.f, 0.f);   // a NaN bound: nobody's inlier
    if (m >= 3) {
        uint32_t w[4] = {(uint32_t)h, (uint32_t)a.round, 0u, 0u};
        philox4x32_10(w, a.seed, 2u);
        const uint32_t i0 = (uint32_t)(((uint64_t)w[0] * (uint32_t)m) >> 32), i1 = (uint32_t)(((uint64_t)w[1] * (uint32_t)m) >> 32),
                       i2 = (uint32_t)(((uint64_t)w[2] * (uint32_t)m) >> 32);                // < m
        const float* L = a.lp + l0 * 3;
        const float p0x = L[(int64_t)i0 * 3], p0y = L[(int64_t)i0 * 3 + 1], p0z = L[(int64_t)i0 * 3 + 2];
        const float e1x = L[(int64_t)i1 * 3] - p0x, e1y = L[(int64_t)i1 * 3 + 1] - p0y, e1z = L[(int64_t)i1 * 3 + 2] - p0z;
        const float e2x = L[(int64_t)i2 * 3] - p0x, e2y = L[(int64_t)i2 * 3 + 1] - p0y, e2z = L[(int64_t)i2 * 3 + 2] - p0z;
        const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
        const float len2 = (nx * nx + ny * ny) + nz * nz;
        if (i0 != i1 && i0 != i2 && i1 != i2 && isfinite(len2) && len2 > 0.f) {
            A = make_float4(nx, ny, nz, a.t2 * len2);
            P0 = make_float4(p0x, p0y, p0z, 1.f);
        }
    }
    const int64_t at = (int64_t)b * a.H + h;
    a.hyp[at * 2] = A;
    a.hyp[at * 2 + 1] = P0;
    a.score[at] = 0;
}

// s = (nx dx + ny dy) + nz dz with d = p - p0, squared; the inlier test is fl(s * s) <= bound
__device__ __forceinline__ float pln_s2(const float4& A, const float4& P0, float x, float y, float z) {
#pragma clang fp contract(off)
    const float dx = x - P0.x, dy = y - P0.y, dz = z - P0.z;
    const float s = (A.x * dx + A.y * dy) + A.z * dz;
    return s * s;
}

// the table and the scores come as arguments of their own: `const __restrict__` lets the uniform reads of a hypothesis be scalar loads
__global__ __launch_bounds__(PLN_ST) void pln_score(PlaneArgs a, const float4* __restrict__ hyp, int32_t* __restrict__ score) {
#pragma clang fp contract(off)
    __shared__ int cnt[64];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    if (a.done[b]) return;                                   // the whole workgroup
    int64_t row0, l0;
    const int n = ragged_span(a.c, b, row0);
    const int m = pln_live(a, b, n, l0);
    const int64_t base = (int64_t)blockIdx.x * PLN_TILE;
    if (base >= m) return;
    const float* L = a.lp + l0 * 3;
    float x[PLN_R], y[PLN_R], z[PLN_R];
#pragma unroll
    for (int r = 0; r < PLN_R; ++r) {
        const int64_t q = base + r * PLN_ST + tid;
        const bool on = q < m;                               // the padding is NaN: no hypothesis counts it
        x[r] = on ? L[q * 3] : NAN; y[r] = on ? L[q * 3 + 1] : NAN; z[r] = on ? L[q * 3 + 2] : NAN;
    }
    if (tid < 64) cnt[tid] = 0;
    __syncthreads();
    const int H = a.H;
    const float4* hb = hyp + (int64_t)b * H * 2;
    int32_t* sb = score + (int64_t)b * H;
    for (int h0 = 0; h0 < H; h0 += 64) {
        const int hn = H - h0 < 64 ? H - h0 : 64;
        int acc = 0;                                         // lane hh: the wave's count of hypothesis h0 + hh
        for (int hh = 0; hh < hn; ++hh) {
            const float4 A = hb[(h0 + hh) * 2], P0 = hb[(h0 + hh) * 2 + 1];
            int c = 0;
#pragma unroll
            for (int r = 0; r < PLN_R; ++r) c += __popcll(__ballot(pln_s2(A, P0, x[r], y[r], z[r]) <= A.w));
            acc = lane == hh ? c : acc;
        }
        if (acc) atomicAdd(&cnt[lane], acc);
        __syncthreads();
        if (tid < hn) {
            const int v = cnt[tid];
            if (v) atomicAdd(sb + h0 + tid, v);
            cnt[tid] = 0;
        }
        __syncthreads();
    }
}

// the valid hypothesis of the largest count, the smallest h on equal counts; -1 without one or below min_inliers
__global__ __launch_bounds__(PLN_T) void pln_argmax(PlaneArgs a) {
    __shared__ int sv[PLN_T], sc[PLN_T];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (a.done[b]) return;
    int bv = -1, bc = -1;
    for (int h = tid; h < a.H; h += PLN_T) {                 // ascending h: a later one wins only when larger
        const int64_t at = (int64_t)b * a.H + h;
        const int v = a.hyp[at * 2 + 1].w != 0.f ? a.score[at] : -1;
        if (v > bv) { bv = v; bc = h; }
    }
    block_argmax<PLN_T>(bv, bc, sv, sc, tid);
    if (tid == 0) {
        const bool found = sc[0] >= 0 && sv[0] >= a.min_inliers;
        a.best[b] = found ? sc[0] : -1;
        a.bscore[b] = found ? sv[0] : 0;
    }
}

__global__ __launch_bounds__(CLOUD_SEG) void pln_mark(PlaneArgs a, int stage) {
#pragma clang fp contract(off)
    __shared__ double v[CLOUD_SEG];
    __shared__ int sh[CLOUD_SEG / 64];
    const int b = blockIdx.y, tid = threadIdx.x;
    if (a.done[b]) return;                                   // the whole workgroup, here and below
    const int best = pln_best(a, b);
    if (best < 0) return;
    int64_t row0, l0;
    const int n = ragged_span(a.c, b, row0);
    const int m = pln_live(a, b, n, l0);
    const int64_t q = (int64_t)blockIdx.x * CLOUD_SEG + tid;
    if ((int64_t)blockIdx.x * CLOUD_SEG >= m) return;
    const bool on = q < m;
    float px = 0.f, py = 0.f, pz = 0.f;
    if (on) { px = a.lp[(l0 + q) * 3]; py = a.lp[(l0 + q) * 3 + 1]; pz = a.lp[(l0 + q) * 3 + 2]; }
    const double* f = a.fit + (int64_t)b * 8;
    double* bs = a.bsum + ((int64_t)b * a.nseg_max + blockIdx.x) * 6;
    bool flag = false;
    if (stage == 0) {
        const float4 A = a.hyp[((int64_t)b * a.H + best) * 2], P0 = a.hyp[((int64_t)b * a.H + best) * 2 + 1];
        flag = on && pln_s2(A, P0, px, py, pz) <= A.w;
        if (on) a.inl[l0 + q] = flag;
        if (!a.refine) return;
        const double sx = block_tree_sum<CLOUD_SEG>(flag ? (double)px : 0.0, v, tid),
                     sy = block_tree_sum<CLOUD_SEG>(flag ? (double)py : 0.0, v, tid),
                     sz = block_tree_sum<CLOUD_SEG>(flag ? (double)pz : 0.0, v, tid);
        if (tid == 0) { bs[0] = sx; bs[1] = sy; bs[2] = sz; }
    } else if (stage == 1) {
        flag = on && a.inl[l0 + q];
        const double dx = (double)px - f[0], dy = (double)py - f[1], dz = (double)pz - f[2];
        const double e[6] = {dx * dx, dx * dy, dx * dz, dy * dy, dy * dz, dz * dz};
        double s[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) s[k] = block_tree_sum<CLOUD_SEG>(flag ? e[k] : 0.0, v, tid);
        if (tid == 0) {
#pragma unroll
            for (int k = 0; k < 6; ++k) bs[k] = s[k];
        }
        return;
    } else {
        const double d = (f[3] * ((double)px - f[0]) + f[4] * ((double)py - f[1])) + f[5] * ((double)pz - f[2]);
        flag = on && fabs(d) <= (double)a.t;
        if (on) a.inl[l0 + q] = flag;
    }
    int total;
    block_rank<CLOUD_SEG>(flag, sh, tid, &total);
    if (tid == 0) a.bcnt[(int64_t)b * a.nseg_max + blockIdx.x] = total;
}

// the plane of the unit normal (x, y, z) through c0, turned to the view, and the round's outputs; fewer than min_inliers: finished
__device__ __forceinline__ void pln_plane(const PlaneArgs& a, double* f, double x, double y, double z) {
#pragma clang fp contract(off)
    const double s = (x * (a.view[0] - f[0]) + y * (a.view[1] - f[1])) + z * (a.view[2] - f[2]);
    const double first = x != 0.0 ? x : (y != 0.0 ? y : z);
    const bool flip = s < 0.0 || (s == 0.0 && first < 0.0);
    x = flip ? -x : x; y = flip ? -y : y; z = flip ? -z : z;
    f[3] = x; f[4] = y; f[5] = z;
    f[6] = -((x * f[0] + y * f[1]) + z * f[2]);
}
__device__ __forceinline__ void pln_commit(const PlaneArgs& a, int b, const double* f, int count, int best) {
    if (count < a.min_inliers) { a.done[b] = 1; return; }
    const int64_t at = (int64_t)b * a.K + a.round;
    a.planes[at * 4] = f[3]; a.planes[at * 4 + 1] = f[4]; a.planes[at * 4 + 2] = f[5]; a.planes[at * 4 + 3] = f[6];
    a.inliers[at] = count;
    a.bests[at] = best;
    a.nplanes[b] = a.round + 1;
    a.took[b] = a.round;
}

__global__ __launch_bounds__(64) void pln_fit(PlaneArgs a, int stage) {
#pragma clang fp contract(off)
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.c.batch || a.done[b]) return;
    const int best = pln_best(a, b);
    if (best < 0) { a.done[b] = 1; return; }
    int64_t row0, l0;
    const int n = ragged_span(a.c, b, row0);
    const int m = pln_live(a, b, n, l0);
    const int nseg = (m + CLOUD_SEG - 1) / CLOUD_SEG;        // <= nseg_max: m <= max_per_sample
    double* f = a.fit + (int64_t)b * 8;
    const double* bs = a.bsum + (int64_t)b * a.nseg_max * 6;
    const int* bc = a.bcnt + (int64_t)b * a.nseg_max;
    if (stage == 0 && !a.refine) {
        const float4 A = a.hyp[((int64_t)b * a.H + best) * 2], P0 = a.hyp[((int64_t)b * a.H + best) * 2 + 1];
        const double nx = (double)A.x, ny = (double)A.y, nz = (double)A.z;
        const double len = __dsqrt_rn((nx * nx + ny * ny) + nz * nz);
        f[0] = (double)P0.x; f[1] = (double)P0.y; f[2] = (double)P0.z;
        pln_plane(a, f, nx / len, ny / len, nz / len);
        pln_commit(a, b, f, a.bscore[b], best);
    } else if (stage == 0) {
        const double mm = (double)fold_blocks(bc, nseg, 1);  // >= min_inliers >= 3
#pragma unroll
        for (int k = 0; k < 3; ++k) f[k] = fold_blocks(bs + k, nseg, 6) / mm;
        f[7] = mm;
    } else if (stage == 1) {
        double s[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) s[k] = fold_blocks(bs + k, nseg, 6);
        const double mm = f[7];
        double a00 = s[0] / mm, a01 = s[1] / mm, a02 = s[2] / mm, a11 = s[3] / mm, a12 = s[4] / mm, a22 = s[5] / mm;
        double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#pragma unroll 1
        for (int sweep = 0; sweep < PLN_SWEEPS; ++sweep) {
            nrm_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
            nrm_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
            nrm_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
        }
        nrm_order(a00, a11, v00, v10, v20, v01, v11, v21);
        nrm_order(a11, a22, v01, v11, v21, v02, v12, v22);
        nrm_order(a00, a11, v00, v10, v20, v01, v11, v21);
        const double len = __dsqrt_rn((v00 * v00 + v10 * v10) + v20 * v20);
        pln_plane(a, f, v00 / len, v10 / len, v20 / len);
    } else {
        pln_commit(a, b, f, fold_blocks(bc, nseg, 1), best);
    }
}

__global__ __launch_bounds__(PLN_T) void pln_label(PlaneArgs a) {
    const int b = blockIdx.y;
    if (a.done[b] || a.took[b] != a.round) return;
    int64_t row0, l0;
    const int n = ragged_span(a.c, b, row0);
    const int m = pln_live(a, b, n, l0);
    const int64_t q = (int64_t)blockIdx.x * PLN_T + threadIdx.x;
    if (q >= m || !a.inl[l0 + q]) return;
    const int64_t g = row0 + rad_clamp(a.li[l0 + q], (int64_t)n);
    a.labels[g] = a.round;
    a.live[g] = 0;
}

__global__ __launch_bounds__(PLN_T) void pln_keep(PlaneArgs a) {
    const int b = blockIdx.y;
    int64_t row0;
    const int n = ragged_span(a.c, b, row0);
    const int64_t j = (int64_t)blockIdx.x * PLN_T + threadIdx.x;
    if (j >= n) return;
    const int label = a.labels[row0 + j];
    a.live[row0 + j] = a.keep_planes ? label >= 0 : label == -1;
}

// the scratch, described once; a.c, a.H and a.K are set
void pln_layout(PlaneArgs& a, Carver& s) {
    const int64_t T = a.c.n_total, B = a.c.batch;
    a.nseg_max = (a.c.max_per_sample + CLOUD_SEG - 1) / CLOUD_SEG;
    a.live = s.take<int32_t>(T);
    a.lp = s.take<float>(T * 3);
    a.li = s.take<int64_t>(T);
    block_scan_layout(a.ls, a.c, s);
    a.ls.out_offsets = s.take<int64_t>(B + 1);
    a.hyp = s.take<float4>(B * a.H * 2);
    a.score = s.take<int32_t>(B * a.H);
    a.best = s.take<int>(B);
    a.bscore = s.take<int>(B);
    a.done = s.take<int>(B);
    a.took = s.take<int>(B);
    a.inl = s.take<unsigned char>(T);
    a.bsum = s.take<double>(B * a.nseg_max * 6);
    a.bcnt = s.take<int>(B * a.nseg_max);
    a.fit = s.take<double>(B * 8);
    a.labels = s.take<int32_t>(T);
    a.inliers = s.take<int32_t>(B * a.K);
    a.bests = s.take<int32_t>(B * a.K);
    a.kept = s.take<int64_t>(T);
    block_scan_layout(a.fs, a.c, s);
}

bool pln_sizes_ok(int B, int64_t n_total, int64_t max_per_sample, int H, int K) {
    return cloud_sizes_ok(B, n_total, max_per_sample, 0) && H >= 1 && H <= PLN_MAX_H && K >= 1 && K <= PLN_MAX_K;
}

// the checks of both entries, then every launch up to the labels
int pln_segment(const std::string& who, PlaneArgs& a, const RaggedCloud& c, float threshold, int H, int K, int min_inliers, int refine,
                int64_t seed, const float* view3_host, int32_t* out_labels, double* out_planes, int32_t* out_num_planes, int32_t* out_inliers,
                int32_t* out_best, void* scratch, int64_t scratch_bytes, hipStream_t st) {
#pragma clang fp contract(off)
    RALD_CHECK(std::isfinite(threshold) && threshold > 0.f, who + ": threshold must be finite and > 0");
    RALD_CHECK(H >= 1 && H <= PLN_MAX_H, who + ": num_hypotheses must be in 1 .. 65536");
    RALD_CHECK(K >= 1 && K <= PLN_MAX_K, who + ": max_planes must be in 1 .. 8");
    RALD_CHECK(min_inliers >= 3, who + ": min_inliers must be >= 3");
    RALD_CHECK(refine == 0 || refine == 1, who + ": refine must be 0 or 1");
    if (view3_host)
        RALD_CHECK(std::isfinite(view3_host[0]) && std::isfinite(view3_host[1]) && std::isfinite(view3_host[2]), who + ": view must be finite");
    RALD_CHECK(pln_sizes_ok(c.batch, c.n_total, c.max_per_sample, H, K),
               who + ": batch 1 .. 65535, n_total 0 .. 2^31 - 1, max_per_sample 1 .. 2^24");
    RALD_CHECK(c.offsets || c.n_dense >= 0, who + ": n_dense must be >= 0 without offsets");
    RALD_TRY(scratch_check(who, scratch, scratch_bytes, plane_scratch_bytes(c.batch, c.n_total, c.max_per_sample, H, K)));
    a.c = c;
    a.H = H; a.K = K; a.min_inliers = min_inliers; a.refine = refine;
    a.t = threshold;
    a.t2 = threshold * threshold;
    a.seed = (uint32_t)((uint64_t)seed & 0xffffffffu);
    for (int k = 0; k < 3; ++k) a.view[k] = view3_host ? (double)view3_host[k] : 0.0;
    Carver s{(char*)scratch, 0};
    pln_layout(a, s);
    if (out_labels) a.labels = out_labels;
    if (out_inliers) a.inliers = out_inliers;
    if (out_best) a.bests = out_best;
    a.planes = out_planes; a.nplanes = out_num_planes;
    const dim3 by_row((unsigned)((c.max_per_sample + PLN_T - 1) / PLN_T), c.batch);
    const dim3 by_seg((unsigned)a.nseg_max, c.batch);
    const dim3 by_cloud((c.batch + 63) / 64);
    hipLaunchKernelGGL(pln_init, by_row, dim3(PLN_T), 0, st, a);
    for (int j = 0; j < K; ++j) {
        a.round = j;
        compact_rows_ragged(c, a.ls, a.live, 1, a.lp, a.li, st);
        hipLaunchKernelGGL(pln_hypotheses, dim3((H + PLN_T - 1) / PLN_T, c.batch), dim3(PLN_T), 0, st, a);
        hipLaunchKernelGGL(pln_score, by_seg, dim3(PLN_ST), 0, st, a, (const float4*)a.hyp, a.score);
        hipLaunchKernelGGL(pln_argmax, dim3(c.batch), dim3(PLN_T), 0, st, a);
        for (int stage = 0; stage < (refine ? 3 : 1); ++stage) {
            hipLaunchKernelGGL(pln_mark, by_seg, dim3(CLOUD_SEG), 0, st, a, stage);
            hipLaunchKernelGGL(pln_fit, by_cloud, dim3(64), 0, st, a, stage);
        }
        hipLaunchKernelGGL(pln_label, by_row, dim3(PLN_T), 0, st, a);
    }
    return 0;
}

}  // namespace

int64_t plane_scratch_bytes(int B, int64_t n_total, int64_t max_per_sample, int num_hypotheses, int max_planes) {
    if (!pln_sizes_ok(B, n_total, max_per_sample, num_hypotheses, max_planes)) return -1;
    PlaneArgs a{};
    a.c = ragged_cloud(nullptr, nullptr, nullptr, B, 0, n_total, max_per_sample);
    a.H = num_hypotheses; a.K = max_planes;
    Carver s{nullptr, 0};
    pln_layout(a, s);
    return s.used;
}

int plane_segment_ragged(const RaggedCloud& c, float threshold, int num_hypotheses, int max_planes, int min_inliers, int refine, int64_t seed,
                         const float* view3_host, int32_t* out_labels, double* out_planes, int32_t* out_num_planes, int32_t* out_inliers,
                         int32_t* out_best, void* scratch, int64_t scratch_bytes, hipStream_t st) {
    RALD_CHECK(c.points && out_labels && out_planes && out_num_planes, "plane_segment_ragged: null pointer (points, out_labels, out_planes, out_num_planes)");
    PlaneArgs a{};
    RALD_TRY(pln_segment("plane_segment_ragged", a, c, threshold, num_hypotheses, max_planes, min_inliers, refine, seed, view3_host, out_labels,
                         out_planes, out_num_planes, out_inliers, out_best, scratch, scratch_bytes, st));
    RALD_HIP(hipGetLastError());
    return 0;
}

int plane_filter_ragged(const RaggedCloud& c, float threshold, int num_hypotheses, int max_planes, int min_inliers, int refine, int64_t seed,
                        const float* view3_host, int keep_planes, float* out_points, int64_t* out_offsets, int64_t* out_index,
                        int32_t* out_labels, double* out_planes, int32_t* out_num_planes, void* scratch, int64_t scratch_bytes, hipStream_t st) {
    RALD_CHECK(c.points && out_points && out_offsets && out_labels && out_planes && out_num_planes,
               "plane_filter_ragged: null pointer (points, out_points, out_offsets, out_labels, out_planes, out_num_planes)");
    PlaneArgs a{};
    RALD_TRY(pln_segment("plane_filter_ragged", a, c, threshold, num_hypotheses, max_planes, min_inliers, refine, seed, view3_host, nullptr,
                         out_planes, out_num_planes, nullptr, nullptr, scratch, scratch_bytes, st));
    a.keep_planes = keep_planes != 0;
    if (out_index) a.kept = out_index;
    a.fs.out_offsets = out_offsets;
    const dim3 by_row((unsigned)((c.max_per_sample + PLN_T - 1) / PLN_T), c.batch);
    hipLaunchKernelGGL(pln_keep, by_row, dim3(PLN_T), 0, st, a);
    compact_rows_ragged(c, a.fs, a.live, 1, out_points, a.kept, st);
    cloud_kept_labels_ragged(c, out_offsets, a.kept, a.labels, out_labels, st);
    RALD_HIP(hipGetLastError());
    return 0;
}

}  // namespace rald
