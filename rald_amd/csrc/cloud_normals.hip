// PCA normals, surface variation and covariance eigenvalues of every row of a ragged batch from its k nearest other rows, and the
// normal consistency of two ragged batches with normals.  The definition is in include/rald_hip.h; in short
//   neighbourhood of i  row i, then its `found` neighbours of the k-NN search in slot order (found >= 2, else the row is undefined)
//   mean, moments       float64, added from +0.0 in that order, divided by m = found + 1; the moments of (p - mean)
//   eigen               6 cyclic Jacobi sweeps over (0,1), (0,2), (1,2), a rotation skipped only on an off-diagonal of exactly 0
//   normal              the column of the smallest eigenvalue (stable order), renormalised, turned to the view / its largest component
// Launches behind cloud_index_build, all on one stream, none waits on another workgroup, no atomics:
//   normals_search      (128 sorted positions, cloud)  knn_search_lane (knn_search.h), then the lane walks its own LDS list in slot order,
//                                                      gathers the neighbours from `points` twice (mean, then moments) and leaves 6 doubles
//                                                      and `found` per input row: no [n_total, k] table exists
//   normals_eigen       (256 rows, cloud)              one lane per input row: the sweeps on registers, the order, the sign, the outputs
// and for the consistency, per direction, behind cloud_nn_ragged (cloud_metrics.hip):
//   nc_block_sums       (1024 rows, cloud)  |n_a . n_nn(a)| of the rows that count, the block's tree sum and their number
//   nc_cloud            one lane per cloud  the blocks left to right, both directions: the three values and the two numbers
// Every loop is bounded by k, a constant or the cloud's length.  Every index read from memory is clamped into its cloud before use.
#include "knn_search.h"
#include "sym3_jacobi.h"

namespace rald {

namespace {

constexpr int NRM_SWEEPS = 6;
constexpr int NRM_T = 256;                                   // rows per workgroup of normals_eigen

struct NormalArgs {
    double* mom;                                             // [n_total][6] xx, xy, xz, yy, yz, zz of the neighbourhood, per input row
    int32_t* found;                                          // [n_total] the search's found
    int has_view;
    float view[3];
    float* out_normals; float* out_curvature; float* out_eigenvalues; int32_t* out_found;
};

__global__ __launch_bounds__(KNN_T) void normals_search(KnnArgs a, NormalArgs m) {
#pragma clang fp contract(off)
    extern __shared__ float nrm_lds[];
    const KnnLane L = knn_search_lane(a, nrm_lds);
    if (!L.live) return;
    const int cnt = L.cnt;
    m.found[L.g] = cnt;
    if (cnt < 2) return;
    const float* P = a.c.points + L.row0 * 3;
    const double px = (double)L.me.x, py = (double)L.me.y, pz = (double)L.me.z;
    const double mm = (double)(cnt + 1);
    double sx = 0.0, sy = 0.0, sz = 0.0;
    sx += px; sy += py; sz += pz;
    for (int t = 0; t < cnt; ++t) {                          // cnt <= k
        const int64_t r = rad_clamp(L.J[t * KNN_T], L.n);
        sx += (double)P[r * 3]; sy += (double)P[r * 3 + 1]; sz += (double)P[r * 3 + 2];
    }
    const double cx = sx / mm, cy = sy / mm, cz = sz / mm;
    double xx = 0.0, xy = 0.0, xz = 0.0, yy = 0.0, yz = 0.0, zz = 0.0;
    {
        const double dx = px - cx, dy = py - cy, dz = pz - cz;
        xx += dx * dx; xy += dx * dy; xz += dx * dz; yy += dy * dy; yz += dy * dz; zz += dz * dz;
    }
    for (int t = 0; t < cnt; ++t) {
        const int64_t r = rad_clamp(L.J[t * KNN_T], L.n);
        const double dx = (double)P[r * 3] - cx, dy = (double)P[r * 3 + 1] - cy, dz = (double)P[r * 3 + 2] - cz;
        xx += dx * dx; xy += dx * dy; xz += dx * dz; yy += dy * dy; yz += dy * dz; zz += dz * dz;
    }
    double* o = m.mom + L.g * 6;
    o[0] = xx / mm; o[1] = xy / mm; o[2] = xz / mm; o[3] = yy / mm; o[4] = yz / mm; o[5] = zz / mm;
}

__global__ __launch_bounds__(NRM_T) void normals_eigen(RaggedCloud cl, NormalArgs m) {
#pragma clang fp contract(off)
    const int b = blockIdx.y;
    int64_t row0;
    const int n = ragged_span(cl, b, row0);
    const int64_t j = (int64_t)blockIdx.x * NRM_T + threadIdx.x;
    if (j >= n) return;
    const int64_t g = row0 + j;
    const int found = m.found[g];
    if (m.out_found) m.out_found[g] = found;
    float nx = 0.f, ny = 0.f, nz = 0.f, curv = NAN, e0 = NAN, e1 = NAN, e2 = NAN;
    if (found >= 2) {
        const double* o = m.mom + g * 6;
        double a00 = o[0], a01 = o[1], a02 = o[2], a11 = o[3], a12 = o[4], a22 = o[5];
        double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#pragma unroll 1
        for (int sweep = 0; sweep < NRM_SWEEPS; ++sweep) {
            nrm_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);    // (0, 1); the third row is 2
            nrm_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);    // (0, 2); the third row is 1
            nrm_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);    // (1, 2); the third row is 0
        }
        nrm_order(a00, a11, v00, v10, v20, v01, v11, v21);
        nrm_order(a11, a22, v01, v11, v21, v02, v12, v22);
        nrm_order(a00, a11, v00, v10, v20, v01, v11, v21);
        const double sum = (a00 + a11) + a22;
        curv = sum == 0.0 ? 0.f : (float)(a00 / sum);
        e0 = (float)a00; e1 = (float)a11; e2 = (float)a22;
        const double len = __dsqrt_rn((v00 * v00 + v10 * v10) + v20 * v20);
        double x = v00 / len, y = v10 / len, z = v20 / len;
        double s = 0.0;
        if (m.has_view) {
            const float* p = cl.points + g * 3;
            s = (x * ((double)m.view[0] - (double)p[0]) + y * ((double)m.view[1] - (double)p[1])) + z * ((double)m.view[2] - (double)p[2]);
        }
        double big = x;                                      // the component of the largest magnitude, the lowest axis on equal ones
        if (fabs(y) > fabs(big)) big = y;
        if (fabs(z) > fabs(big)) big = z;
        // turned away from the view; with no view, or a view in the row's tangent plane, so that the largest component is positive
        const bool flip = s < 0.0 || (s == 0.0 && big < 0.0);
        x = flip ? -x : x; y = flip ? -y : y; z = flip ? -z : z;
        nx = (float)x; ny = (float)y; nz = (float)z;
    }
    m.out_normals[g * 3] = nx; m.out_normals[g * 3 + 1] = ny; m.out_normals[g * 3 + 2] = nz;
    if (m.out_curvature) m.out_curvature[g] = curv;
    if (m.out_eigenvalues) { m.out_eigenvalues[g * 3] = e0; m.out_eigenvalues[g * 3 + 1] = e1; m.out_eigenvalues[g * 3 + 2] = e2; }
}

void normals_layout(KnnArgs& a, CloudIndex& ix, Carver& s, int64_t chunk, NormalArgs& m) {
    knn_layout(a, ix, s, chunk);
    m.mom = s.take<double>(a.c.n_total * 6);
    m.found = s.take<int32_t>(a.c.n_total);
}

// ---- normal consistency
struct NcArgs {
    const int64_t* a_off; const int64_t* b_off;
    const float* na; const float* nb;                        // the normals of either side, laid out like its rows
    const int64_t* idx;                                      // cloud_nn_ragged's out_idx of a -> b
    int64_t max_a, max_b, nseg_max, ta, tb;                  // ta, tb: the rows of either side's tensors
    double* bsum; int* bcnt;                                 // [2][batch][nseg_max]
    int batch, dir;
};

__device__ __forceinline__ bool nc_usable(float x, float y, float z) {
    return isfinite(x) && isfinite(y) && isfinite(z) && (x != 0.f || y != 0.f || z != 0.f);
}
// a frame's first row and rows of one side, as cloud_nn_ragged takes them, clamped into the side's tensor
__device__ __forceinline__ int64_t nc_span(const int64_t* off, int f, int64_t bound, int64_t total, int64_t& row0) {
    row0 = off[f];
    int64_t len = off[f + 1] - row0;
    len = len < bound ? len : bound;
    if (row0 < 0 || row0 > total) { row0 = 0; len = 0; }
    len = len < total - row0 ? len : total - row0;
    return len > 0 ? len : 0;
}

__global__ __launch_bounds__(CLOUD_SEG) void nc_block_sums(NcArgs a) {
#pragma clang fp contract(off)
    __shared__ double v[CLOUD_SEG];
    __shared__ int sh[CLOUD_SEG / 64];
    const int f = blockIdx.y, tid = threadIdx.x;
    int64_t a0, b0;
    const int64_t na = nc_span(a.a_off, f, a.max_a, a.ta, a0), nb = nc_span(a.b_off, f, a.max_b, a.tb, b0);
    const int64_t j = (int64_t)blockIdx.x * CLOUD_SEG + tid;
    if ((int64_t)blockIdx.x * CLOUD_SEG >= na) return;       // the whole workgroup
    bool counts = false;
    double x = 0.0;                                          // a row that does not count, and the padding: +0.0
    if (j < na && nb > 0) {
        const int64_t r = rad_clamp(a.idx[a0 + j], nb);
        const float* p = a.na + (a0 + j) * 3;
        const float* q = a.nb + (b0 + r) * 3;
        const float px = p[0], py = p[1], pz = p[2], qx = q[0], qy = q[1], qz = q[2];
        counts = nc_usable(px, py, pz) && nc_usable(qx, qy, qz);
        if (counts) x = fabs(((double)px * (double)qx + (double)py * (double)qy) + (double)pz * (double)qz);
    }
    int total;
    block_rank<CLOUD_SEG>(counts, sh, tid, &total);
    const double sum = block_tree_sum<CLOUD_SEG>(x, v, tid);
    if (tid == 0) {
        const int64_t at = ((int64_t)a.dir * a.batch + f) * a.nseg_max + blockIdx.x;
        a.bsum[at] = sum;
        a.bcnt[at] = total;
    }
}

// a.a_off / a.max_a / a.ta: pred's, a.b_off / a.max_b / a.tb: gt's
__global__ __launch_bounds__(64) void nc_cloud(NcArgs a, double* out_nc, int64_t* out_counts) {
#pragma clang fp contract(off)
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= a.batch) return;
    int64_t r0;
    const int64_t len[2] = {nc_span(a.a_off, f, a.max_a, a.ta, r0), nc_span(a.b_off, f, a.max_b, a.tb, r0)};
    double nc[2];
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        const int nseg = (int)((len[d] + CLOUD_SEG - 1) / CLOUD_SEG);   // <= nseg_max: len <= the side's bound < 2^31
        const int64_t at = ((int64_t)d * a.batch + f) * a.nseg_max;
        const double s = fold_blocks(a.bsum + at, nseg, 1);
        const int cnt = fold_blocks(a.bcnt + at, nseg, 1);  // <= len
        nc[d] = cnt > 0 ? s / (double)cnt : (double)NAN;
        out_counts[f * 2 + d] = cnt;
        out_nc[f * 3 + d] = nc[d];
    }
    out_nc[f * 3 + 2] = (nc[0] + nc[1]) / 2.0;
}

inline bool nc_sizes_ok(int B, int64_t tp, int64_t tg, int64_t max_pred, int64_t max_gt) {
    const int64_t lim = (int64_t)1 << 31;
    return B >= 1 && B <= 65535 && tp >= 0 && tg >= 0 && tp < lim && tg < lim && max_pred >= 0 && max_gt >= 0 && max_pred < lim && max_gt < lim;
}
struct NcScratch { int64_t* idx; double* bsum; int* bcnt; char* nn; int64_t nn_bytes; };
// the scratch of the consistency, described once: the neighbour indices of one direction, the block sums of both, the search's own
int64_t nc_layout(NcScratch& w, NcArgs& a, Carver& s, int B, int64_t tp, int64_t tg, int64_t max_pred, int64_t max_gt) {
    const int64_t w0 = cloud_nn_scratch_bytes(B, max_pred, max_gt, 0), w1 = cloud_nn_scratch_bytes(B, max_gt, max_pred, 0);
    if (w0 < 0 || w1 < 0) return -1;
    a.nseg_max = ((max_pred > max_gt ? max_pred : max_gt) + CLOUD_SEG - 1) / CLOUD_SEG;
    w.idx = s.take<int64_t>(tp > tg ? tp : tg);
    w.bsum = s.take<double>(2 * (int64_t)B * a.nseg_max);
    w.bcnt = s.take<int>(2 * (int64_t)B * a.nseg_max);
    w.nn_bytes = w0 > w1 ? w0 : w1;
    w.nn = s.take<char>(w.nn_bytes);
    return s.used;
}

}  // namespace

int64_t normals_scratch_bytes(int B, int64_t n_total, int64_t max_per_sample, int64_t chunk) {
    NormalArgs m{};
    return layout_bytes<KnnArgs>(B, n_total, max_per_sample, chunk,
                                 [&m](KnnArgs& a, CloudIndex& ix, Carver& s, int64_t ch) { normals_layout(a, ix, s, ch, m); });
}

int normals_ragged(const RaggedCloud& c, const GridSpec& grid, int k, float max_radius, const float* view3_host, float* out_normals,
                   float* out_curvature, float* out_eigenvalues, int32_t* out_found, void* scratch, int64_t scratch_bytes, int64_t chunk,
                   hipStream_t st) {
    RALD_CHECK(c.points && out_normals, "normals_ragged: null pointer (points, out_normals)");
    NormalArgs m{};
    if (view3_host) {
        RALD_CHECK(std::isfinite(view3_host[0]) && std::isfinite(view3_host[1]) && std::isfinite(view3_host[2]), "normals_ragged: view must be finite");
        m.has_view = 1;
        for (int t = 0; t < 3; ++t) m.view[t] = view3_host[t];
    }
    KnnArgs a{};
    RALD_TRY(knn_prepare("normals_ragged", a, c, grid, k, max_radius,
                         [&m](KnnArgs& ka, CloudIndex& ix, Carver& s, int64_t ch) { normals_layout(ka, ix, s, ch, m); },
                         normals_scratch_bytes(c.batch, c.n_total, c.max_per_sample, chunk), scratch, scratch_bytes, chunk, st));
    m.out_normals = out_normals; m.out_curvature = out_curvature; m.out_eigenvalues = out_eigenvalues; m.out_found = out_found;
    hipLaunchKernelGGL(normals_search, knn_search_grid(c), dim3(KNN_T), knn_search_lds(k), st, a, m);
    hipLaunchKernelGGL(normals_eigen, dim3((unsigned)((c.max_per_sample + NRM_T - 1) / NRM_T), c.batch), dim3(NRM_T), 0, st, a.c, m);
    RALD_HIP(hipGetLastError());
    return 0;
}

int64_t normal_consistency_scratch_bytes(int B, int64_t n_pred_total, int64_t n_gt_total, int64_t max_pred, int64_t max_gt) {
    if (!nc_sizes_ok(B, n_pred_total, n_gt_total, max_pred, max_gt)) return -1;
    NcScratch w{};
    NcArgs a{};
    Carver s{nullptr, 0};
    return nc_layout(w, a, s, B, n_pred_total, n_gt_total, max_pred, max_gt);
}

int normal_consistency_ragged(const float* pred, const float* pred_normals, const int64_t* pred_off, int64_t n_pred_total, const float* gt,
                              const float* gt_normals, const int64_t* gt_off, int64_t n_gt_total, int B, int64_t max_pred, int64_t max_gt,
                              double* out_nc, int64_t* out_counts, void* scratch, int64_t scratch_bytes, hipStream_t st) {
    const std::string who = "normal_consistency_ragged";
    RALD_CHECK(pred && pred_normals && pred_off && gt && gt_normals && gt_off && out_nc && out_counts,
               who + ": null pointer (pred, pred_normals, pred_offsets, gt, gt_normals, gt_offsets, out_nc, out_counts)");
    RALD_CHECK(nc_sizes_ok(B, n_pred_total, n_gt_total, max_pred, max_gt),
               who + ": batch 1 .. 65535, the totals and the bounds 0 .. 2^31 - 1");
    const int64_t need = normal_consistency_scratch_bytes(B, n_pred_total, n_gt_total, max_pred, max_gt);
    RALD_CHECK(need >= 0, who + ": workspace too large");
    RALD_TRY(scratch_check(who, scratch, scratch_bytes, need));
    NcScratch w{};
    NcArgs a{};
    Carver s{(char*)scratch, 0};
    nc_layout(w, a, s, B, n_pred_total, n_gt_total, max_pred, max_gt);
    a.batch = B; a.bsum = w.bsum; a.bcnt = w.bcnt; a.idx = w.idx;
    for (int dir = 0; dir < 2; ++dir) {
        a.dir = dir;
        a.a_off = dir ? gt_off : pred_off; a.b_off = dir ? pred_off : gt_off;
        a.na = dir ? gt_normals : pred_normals; a.nb = dir ? pred_normals : gt_normals;
        a.max_a = dir ? max_gt : max_pred; a.max_b = dir ? max_pred : max_gt;
        a.ta = dir ? n_gt_total : n_pred_total; a.tb = dir ? n_pred_total : n_gt_total;
        if (a.max_a == 0 || a.ta == 0) continue;             // no row on this side: nc_cloud reads no block of it
        RALD_TRY(cloud_nn_ragged(dir ? gt : pred, a.a_off, dir ? pred : gt, a.b_off, B, a.max_a, a.max_b, 0, nullptr, w.idx, w.nn, w.nn_bytes, st));
        hipLaunchKernelGGL(nc_block_sums, dim3((unsigned)((a.max_a + CLOUD_SEG - 1) / CLOUD_SEG), B), dim3(CLOUD_SEG), 0, st, a);
    }
    a.a_off = pred_off; a.b_off = gt_off; a.max_a = max_pred; a.max_b = max_gt; a.ta = n_pred_total; a.tb = n_gt_total;
    hipLaunchKernelGGL(nc_cloud, dim3((B + 63) / 64), dim3(64), 0, st, a, out_nc, out_counts);
    RALD_HIP(hipGetLastError());
    return 0;
}

}  // namespace rald
