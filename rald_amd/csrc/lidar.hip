// LiDAR front end on the device: the reference's offline crop (dataset_preprocessor/lidar.py:123-194) and the per-sample voxel and
// occupancy-query chain of ColoRadarDataset.__getitem__ (datasets/aligned_coloradar/Coloradar_dataset.py:70-135, :237-418, with
// spconv's Point2VoxelCPU3d behind datasets/utils/voxelize.py), for a batch of frames of different lengths.
//   crop       lid_crop_stage (chunk, frame)   empty-point test, extrinsic, polar, FOV filter, back to cartesian, all in double
//              lid_crop_emit  (chunk, frame)   ordered compaction of the survivors (input order kept)
//   voxelize   lid_vox_keys   (chunk, frame)   float32 polar (view-cone mode), float32 cell index, linear key (x Gy + y) Gz + z
//              lid_vox_sort   (frame)          stable LSD radix sort of (key, point index), 8 bits per pass, through the workspace
//              lid_vox_segs   (frame)          segment heads -> first-appearance voxel ids (exclusive scan in point order), the
//                                              max_voxels cap, zyx coordinates, per-voxel counts, sorted kept keys, voxel contents
//   queries    lid_queries    (chunk, frame)   sampled points, voxel centres + in-voxel offsets, the r-th empty cell by a binary
//                                              search on the sorted kept keys (no dense grid), labels, normalisation
// No float atomics: LDS integer atomics only count (histograms), and every ordered result comes from a prefix sum, so a frame's
// output does not depend on the batch.  The one-workgroup-per-frame sort bounds the latency at B = 1.
#include <cmath>
#include <vector>

#include "lidar.h"

namespace rald {

namespace {

constexpr int CT = 256;              // points per chunk workgroup
constexpr int CW = CT / 64;
constexpr int FT = 1024;             // one workgroup per frame: sort and segment passes
constexpr int FW = FT / 64;

struct Derived {
    double T[16];
    double fov[6];
    float lo[3], v[3];               // pc_range lo / voxel size as float32 (the cell index is float32 arithmetic)
    float c_off[3];                  // float32(v / 2 + lo): the voxel-centre offset of transform_voxels_to_query_points
    int g[3];
    int cells;
    int maxv, maxp, F;
    int aniso, iso;
    float n_off[3], n_scale[3];      // norm_points, anisotropic branch: float32 offsets / scales
    double d_off[3], d_smax;         // isotropic branch: float64 offset array, max scale
};

Derived derive(const Lidar& h) {
    const rald_lidar_config& c = h.cfg;
    Derived d{};
    for (int i = 0; i < 16; ++i) d.T[i] = c.extrinsic[i];
    for (int i = 0; i < 6; ++i) d.fov[i] = c.fov[i];
    d.d_smax = 0.0;
    for (int a = 0; a < 3; ++a) {
        d.lo[a] = (float)c.pc_range[a];
        d.v[a] = (float)c.voxel_size[a];
        d.c_off[a] = (float)(c.voxel_size[a] / 2 + c.pc_range[a]);
        d.g[a] = (int)h.grid[a];
        const double off = (c.pc_range[3 + a] + c.pc_range[a]) / 2, sc = (c.pc_range[3 + a] - c.pc_range[a]) / 2;
        d.n_off[a] = (float)off;
        d.n_scale[a] = (float)sc;
        d.d_off[a] = off;
        if (sc > d.d_smax) d.d_smax = sc;
    }
    d.cells = (int)h.cells;
    d.maxv = c.max_voxels;
    d.maxp = c.max_points_per_voxel;
    d.F = c.num_point_features;
    d.aniso = c.norm_anisotropy;
    d.iso = c.norm_isotropy;
    return d;
}

__device__ __forceinline__ unsigned long long lanes_below(int lane) { return (1ull << lane) - 1ull; }

// numpy's float32 rad2deg factor: float32(180) / float32(pi)
#define RAD2DEG_F32 57.295776f
// numpy's float64 factors: 180.0 / NPY_PI and NPY_PI / 180.0
#define RAD2DEG_F64 (180.0 / 3.141592653589793238462643383279502884)
#define DEG2RAD_F64 (3.141592653589793238462643383279502884 / 180.0)

// ------------------------------------------------------------------------------------------------ crop
struct CropArgs {
    const float* pts;
    int stride;
    const int64_t* off;        // device copy of the offsets [B + 1]
    float* stage;              // [total][3] the cartesian float32 result of every point
    unsigned char* flag;       // [total] kept
    int* ccnt;                 // [B][chunks] kept per chunk
    int chunks;
    float* out;                // [total][3] compacted at the frame's offset
    int* counts;               // [B]
    Derived d;
};

// lidar.py:170-182 on one point: remove_empty_points (float32 norm > 0), [x y z 1] @ T.T, cartesian2polar, filter_points_polar
// (inclusive bounds), polar2cartesian, all in float64; the float32 rounding is save_lidar_data's astype
__global__ __launch_bounds__(CT) void lid_crop_stage(CropArgs a) {
#pragma clang fp contract(off)
    __shared__ int wk[CW];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t o = a.off[b], n = a.off[b + 1] - o, j = (int64_t)blockIdx.x * CT + tid;
    bool keep = false;
    if (j < n) {
        const float* p = a.pts + (o + j) * a.stride;
        const float fx = p[0], fy = p[1], fz = p[2];
        const float s = fx * fx + fy * fy + fz * fz;            // np.linalg.norm > 0 <=> the float32 sum of squares > 0
        const double x = fx, y = fy, z = fz, *T = a.d.T;
        const double X = x * T[0] + y * T[1] + z * T[2] + T[3];
        const double Y = x * T[4] + y * T[5] + z * T[6] + T[7];
        const double Z = x * T[8] + y * T[9] + z * T[10] + T[11];
        const double r = sqrt(X * X + Y * Y + Z * Z);
        const double az = -(atan2(Y, X) * RAD2DEG_F64);
        const double el = asin(Z / r) * RAD2DEG_F64;
        const double* f = a.d.fov;
        keep = s > 0.f && r >= f[0] && r <= f[1] && az >= f[2] && az <= f[3] && el >= f[4] && el <= f[5];
        const double azr = -(az * DEG2RAD_F64), elr = el * DEG2RAD_F64;
        float* q = a.stage + (o + j) * 3;
        q[0] = (float)(r * cos(elr) * cos(azr));
        q[1] = (float)(r * cos(elr) * sin(azr));
        q[2] = (float)(r * sin(elr));
        a.flag[o + j] = keep ? 1 : 0;
    }
    const unsigned long long bk = __ballot(keep);
    if (lane == 0) wk[w] = __popcll(bk);
    __syncthreads();
    if (tid == 0) {
        int t = 0;
        for (int i = 0; i < CW; ++i) t += wk[i];
        a.ccnt[(size_t)b * a.chunks + blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(CT) void lid_crop_emit(CropArgs a) {
    __shared__ int wk[CW];
    __shared__ int s_pre, s_all;
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = blockIdx.x;
    const int64_t o = a.off[b], n = a.off[b + 1] - o, j = (int64_t)c * CT + tid;
    const int nch = (int)((n + CT - 1) / CT);
    if (tid == 0) { s_pre = 0; s_all = 0; }
    __syncthreads();
    int pre = 0, all = 0;
    for (int q = tid; q < nch; q += CT) {
        const int v = a.ccnt[(size_t)b * a.chunks + q];
        if (q < c) pre += v;
        all += v;
    }
    if (pre) atomicAdd(&s_pre, pre);
    if (c == 0 && all) atomicAdd(&s_all, all);
    __syncthreads();
    if (c == 0 && tid == 0) a.counts[b] = s_all;
    if ((int64_t)c * CT >= n) return;
    const bool keep = j < n && a.flag[o + j];
    const unsigned long long bk = __ballot(keep);
    if (lane == 0) wk[w] = __popcll(bk);
    __syncthreads();
    int pos = s_pre;
    for (int i = 0; i < w; ++i) pos += wk[i];
    pos += __popcll(bk & lanes_below(lane));
    if (keep) {
        const float* s = a.stage + (o + j) * 3;
        float* q = a.out + (o + pos) * 3;
        q[0] = s[0];
        q[1] = s[1];
        q[2] = s[2];
    }
}

// ------------------------------------------------------------------------------------------------ voxelize
struct VoxArgs {
    const float* pts;          // [total][F]
    const int64_t* off;
    const int* counts;         // [B] or null: frame b is points off[b] .. off[b] + min(counts[b], off[b+1] - off[b])
    int to_polar;
    float* polar;              // [total][3] (to_polar) or null
    unsigned* keyA;            // [total] ping / pong of the sort
    unsigned* keyB;
    int* idxA;
    int* idxB;
    int* hf;                   // [total] point order: 1 at the first point of each voxel, then its voxel id
    int* segst;                // [total] sorted order: start of the element's segment
    int* seglen;               // [total] sorted order: segment length, at the segment's start
    int passes;
    float* voxels;             // [B][maxv][maxp][F] or null
    int* coords;               // [B][maxv][3] zyx
    int* npts;                 // [B][maxv]
    int* kkeys;                // [B][maxv] kept keys, ascending
    int* vcount;               // [B]
    Derived d;
};

__device__ __forceinline__ int64_t frame_len(const int64_t* off, const int* counts, int b) {
    const int64_t n = off[b + 1] - off[b];
    return counts ? min(n, (int64_t)max(counts[b], 0)) : n;
}

__device__ __forceinline__ const float* vox_feat(const VoxArgs& a, int64_t g) {
    return a.to_polar ? a.polar + g * 3 : a.pts + g * a.d.F;
}

// cartesian2polar on a float32 array as numpy evaluates it (Coloradar_dataset.py:88): every operation rounded to float32, the
// transcendentals in double and rounded once (the correctly rounded float32 value); then the cell index c = floor((p - lo) / v)
// in float32 and the linear key, `cells` outside the grid
__global__ __launch_bounds__(CT) void lid_vox_keys(VoxArgs a) {
#pragma clang fp contract(off)
    const int b = blockIdx.y;
    const int64_t o = a.off[b], n = frame_len(a.off, a.counts, b), j = (int64_t)blockIdx.x * CT + threadIdx.x;
    if (j >= n) return;
    const int64_t g = o + j;
    float f[3];
    if (a.to_polar) {
        const float* p = a.pts + g * 3;
        const float x = p[0], y = p[1], z = p[2];
        const float s = x * x + y * y + z * z;
        const float r = (float)sqrt((double)s);
        const float at = (float)atan2((double)y, (double)x);
        const float q = z / r;
        const float as = (float)asin((double)q);
        f[0] = r;
        f[1] = -(at * RAD2DEG_F32);
        f[2] = as * RAD2DEG_F32;
        float* o3 = a.polar + g * 3;
        o3[0] = f[0];
        o3[1] = f[1];
        o3[2] = f[2];
    } else {
        const float* p = a.pts + g * a.d.F;
        f[0] = p[0];
        f[1] = p[1];
        f[2] = p[2];
    }
    int c[3];
    bool in = true;
    for (int k = 0; k < 3; ++k) {
        const float cf = floorf((f[k] - a.d.lo[k]) / a.d.v[k]);
        in = in && cf >= 0.f && cf < (float)a.d.g[k];          // NaN fails both
        c[k] = in ? (int)cf : 0;
    }
    a.keyA[g] = in ? (unsigned)(((int64_t)c[0] * a.d.g[1] + c[1]) * a.d.g[2] + c[2]) : (unsigned)a.d.cells;
    a.idxA[g] = (int)j;
    a.hf[g] = 0;
}

// wave w of the frame workgroup owns the contiguous range [lo, hi) of n elements (a multiple of 64 long)
__device__ __forceinline__ void wave_range(int64_t n, int w, int64_t& lo, int64_t& hi) {
    const int64_t per = ((n + FW - 1) / FW + 63) / 64 * 64;
    lo = min(n, per * w);
    hi = min(n, lo + per);
}

// exclusive prefix of one value per wave; returns this wave's base, *total the sum
__device__ __forceinline__ int wave_prefix(int* sh, int v, int w, int lane, int* total) {
    if (lane == 0) sh[w] = v;
    __syncthreads();
    int base = 0, t = 0;
    for (int i = 0; i < FW; ++i) {
        const int x = sh[i];
        if (i < w) base += x;
        t += x;
    }
    __syncthreads();
    *total = t;
    return base;
}

// grid (B), FT threads: stable LSD radix sort of the frame's (key, index) pairs, ascending key.  Each wave scatters its own range in
// order through per-(wave, digit) offsets, so equal keys keep their input (point-index) order and no block barrier sits in the
// scatter loop.  After `passes` passes the result is in keyA / idxA (even) or keyB / idxB (odd).
__global__ __launch_bounds__(FT) void lid_vox_sort(VoxArgs a) {
    __shared__ unsigned cnt[FW][256];
    __shared__ unsigned tot[256];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t o = a.off[b], n = frame_len(a.off, a.counts, b);
    if (n <= 1) return;
    int64_t lo, hi;
    wave_range(n, w, lo, hi);
    unsigned *ks = a.keyA + o, *kd = a.keyB + o;
    int *is = a.idxA + o, *id = a.idxB + o;
    for (int pass = 0; pass < a.passes; ++pass) {
        const int shift = 8 * pass;
        for (int i = tid; i < FW * 256; i += FT) (&cnt[0][0])[i] = 0;
        __syncthreads();
        for (int64_t j = lo + lane; j < hi; j += 64) atomicAdd(&cnt[w][(ks[j] >> shift) & 255u], 1u);
        __syncthreads();
        if (tid < 256) {
            unsigned run = 0;
            for (int ww = 0; ww < FW; ++ww) {
                const unsigned c = cnt[ww][tid];
                cnt[ww][tid] = run;
                run += c;
            }
            tot[tid] = run;
        }
        __syncthreads();
        if (w == 0) {                     // exclusive scan over digits, lane l holds 4l .. 4l + 3
            unsigned c[4], sum = 0;
            for (int k = 0; k < 4; ++k) {
                c[k] = tot[4 * lane + k];
                sum += c[k];
            }
            unsigned incl = sum;
            for (int s = 1; s < 64; s <<= 1) {
                const unsigned t = __shfl_up(incl, s);
                if (lane >= s) incl += t;
            }
            unsigned run = incl - sum;
            for (int k = 0; k < 4; ++k) {
                tot[4 * lane + k] = run;
                run += c[k];
            }
        }
        __syncthreads();
        if (tid < 256)
            for (int ww = 0; ww < FW; ++ww) cnt[ww][tid] += tot[tid];
        __syncthreads();
        for (int64_t j0 = lo; j0 < hi; j0 += 64) {
            const int64_t j = j0 + lane;
            const bool valid = j < hi;
            const unsigned key = valid ? ks[j] : 0u;
            const int idx = valid ? is[j] : 0;
            const unsigned dg = (key >> shift) & 255u;
            unsigned long long m = __ballot(valid);
            for (int bit = 0; bit < 8; ++bit) {
                const bool set = (dg >> bit) & 1u;
                const unsigned long long bb = __ballot(valid && set);
                m &= set ? bb : ~bb;
            }
            const unsigned rank = (unsigned)__popcll(m & lanes_below(lane));
            const unsigned pos = valid ? cnt[w][dg] + rank : 0u;
            __builtin_amdgcn_wave_barrier();
            if (valid && rank == 0) cnt[w][dg] += (unsigned)__popcll(m);
            __builtin_amdgcn_wave_barrier();
            if (valid) {
                kd[pos] = key;
                id[pos] = idx;
            }
        }
        __syncthreads();
        unsigned* tk = ks; ks = kd; kd = tk;
        int* ti = is; is = id; id = ti;
    }
}

// grid (B), FT threads: the spconv rules on the sorted pairs.  A segment (equal keys) is one voxel, its elements in point order.
//   A (sorted)  segment starts and lengths; a flag at the point index of each segment's first (lowest-index) point
//   B (points)  exclusive scan of the flags in point order: the first-appearance voxel id of each first point
//   C (sorted)  voxels with id < max_voxels are kept: zyx coordinates, min(length, max_points), the kept keys compacted in key
//               order, and each element of rank < max_points copied to voxels[id][rank]
__global__ __launch_bounds__(FT) void lid_vox_segs(VoxArgs a) {
    __shared__ int sh[FW];
    __shared__ int s_carry[FW];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t o = a.off[b], n = frame_len(a.off, a.counts, b);
    const bool odd = (a.passes & 1) && n > 1;
    const unsigned* sk = (odd ? a.keyB : a.keyA) + o;
    const int* si = (odd ? a.idxB : a.idxA) + o;
    int* hf = a.hf + o;
    int* segst = a.segst + o;
    int* seglen = a.seglen + o;
    const unsigned cells = (unsigned)a.d.cells;
    const int maxv = a.d.maxv, maxp = a.d.maxp, F = a.d.F;
    int64_t lo, hi;
    wave_range(n, w, lo, hi);
    auto head = [&](int64_t j) { return sk[j] < cells && (j == 0 || sk[j - 1] != sk[j]); };

    // A: the last head of each wave's range carries into the next range
    int last = -1;
    for (int64_t j0 = lo; j0 < hi; j0 += 64) {
        const int64_t j = j0 + lane;
        const unsigned long long bm = __ballot(j < hi && head(j));
        if (bm) last = (int)(j0 + 63 - __clzll(bm));
    }
    if (lane == 0) s_carry[w] = last;
    __syncthreads();
    int carry = -1;
    for (int i = 0; i < w; ++i) carry = max(carry, s_carry[i]);
    for (int64_t j0 = lo; j0 < hi; j0 += 64) {
        const int64_t j = j0 + lane;
        const bool valid = j < hi && sk[j] < cells;
        const bool h = valid && head(j);
        const unsigned long long bm = __ballot(h);
        const unsigned long long mine = bm & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));
        const int st = mine ? (int)(j0 + 63 - __clzll(mine)) : carry;
        if (bm) carry = (int)(j0 + 63 - __clzll(bm));
        if (valid) {
            segst[j] = st;
            if (h) hf[si[j]] = 1;
            if (j + 1 == n || sk[j + 1] != sk[j]) seglen[st] = (int)(j - st + 1);
        }
    }
    __syncthreads();

    // B: voxel ids in order of first appearance
    int heads = 0;
    for (int64_t j = lo + lane; j < hi; j += 64) heads += hf[j];
    for (int s = 32; s > 0; s >>= 1) heads += __shfl_xor(heads, s);
    int H = 0;
    int run = wave_prefix(sh, heads, w, lane, &H);
    for (int64_t j0 = lo; j0 < hi; j0 += 64) {
        const int64_t j = j0 + lane;
        const bool f = j < hi && hf[j] != 0;
        const unsigned long long bm = __ballot(f);
        if (f) hf[j] = run + __popcll(bm & lanes_below(lane));
        run += __popcll(bm);
    }
    __syncthreads();

    // C: the kept voxels
    int kept = 0;
    for (int64_t j = lo + lane; j < hi; j += 64)
        if (sk[j] < cells && segst[j] == (int)j && hf[si[j]] < maxv) ++kept;
    for (int s = 32; s > 0; s >>= 1) kept += __shfl_xor(kept, s);
    int V = 0;
    int krun = wave_prefix(sh, kept, w, lane, &V);
    int* coords = a.coords + (size_t)b * maxv * 3;
    int* npts = a.npts + (size_t)b * maxv;
    int* kk = a.kkeys + (size_t)b * maxv;
    float* vox = a.voxels ? a.voxels + (size_t)b * maxv * maxp * F : nullptr;
    const int G1 = a.d.g[1], G2 = a.d.g[2];
    for (int64_t j0 = lo; j0 < hi; j0 += 64) {
        const int64_t j = j0 + lane;
        const bool valid = j < hi && sk[j] < cells;
        int st = 0, v = maxv;
        if (valid) {
            st = segst[j];
            v = hf[si[st]];
        }
        const bool kh = valid && st == (int)j && v < maxv;
        const unsigned long long bm = __ballot(kh);
        if (kh) {
            const unsigned key = sk[j];
            const int z = (int)(key % (unsigned)G2), y = (int)((key / (unsigned)G2) % (unsigned)G1), x = (int)(key / ((unsigned)G2 * G1));
            coords[(size_t)v * 3 + 0] = z;
            coords[(size_t)v * 3 + 1] = y;
            coords[(size_t)v * 3 + 2] = x;
            npts[v] = min(seglen[j], maxp);
            kk[krun + __popcll(bm & lanes_below(lane))] = (int)key;
        }
        krun += __popcll(bm);
        const int rank = (int)(j - st);
        if (vox && valid && v < maxv && rank < maxp) {
            const float* src = vox_feat(a, o + si[j]);
            float* dst = vox + ((size_t)v * maxp + rank) * F;
            for (int k = 0; k < F; ++k) dst[k] = src[k];
        }
    }
    if (tid == 0) a.vcount[b] = min(H, maxv);
}

// ------------------------------------------------------------------------------------------------ queries
struct QueryArgs {
    const float* pts;          // [total][3] the frame's points the samples index (float32 polar in view-cone mode)
    const int64_t* off;
    int S, in_num;
    const int64_t* sidx;       // [B][S]
    const double* u_in;        // [B][in_num][3]
    const int64_t* vidx;       // [B][in_num]
    const double* u_out;       // [B][S - in_num][3]
    const int64_t* erank;      // [B][S - in_num]
    const int* coords;         // [B][maxv][3] zyx
    const int* kkeys;          // [B][maxv]
    const int* vcount;         // [B]
    float* lp;                 // [B][S][3]
    float* qp;                 // [B][S][3]
    float* lab;                // [B][S]
    Derived d;
};

// Coloradar_dataset.py norm_points (:365-418) on torch float32 rows: the anisotropic branch casts the float64 scalars to float32 and
// rounds each operation; the isotropic one (applied after it when both are on) subtracts a float64 array and rounds once on assignment
__device__ __forceinline__ void norm3(const Derived& d, float* p) {
#pragma clang fp contract(off)
    if (d.aniso)
        for (int k = 0; k < 3; ++k) p[k] = (p[k] - d.n_off[k]) / d.n_scale[k];
    if (d.iso)
        for (int k = 0; k < 3; ++k) p[k] = (float)(((double)p[k] - d.d_off[k]) / d.d_smax);
}

// coords[:, k].to(float32) * voxel_k + offset_k: float32 product, float32 sum (:249-251, :359-361)
__device__ __forceinline__ float centre(const Derived& d, int k, int c) {
#pragma clang fp contract(off)
    const float t = (float)c * d.v[k];
    return t + d.c_off[k];
}

__global__ __launch_bounds__(CT) void lid_queries(QueryArgs a) {
#pragma clang fp contract(off)
    const int b = blockIdx.y, s = blockIdx.x * CT + threadIdx.x;
    if (s >= a.S) return;
    const float qnan = __int_as_float(0x7fc00000);
    const int64_t o = a.off[b], n = a.off[b + 1] - o;
    const size_t bs = (size_t)b * a.S + s;
    float p[3] = {qnan, qnan, qnan};
    const int64_t pi = a.sidx[bs];
    if (pi >= 0 && pi < n)
        for (int k = 0; k < 3; ++k) p[k] = a.pts[(o + pi) * 3 + k];
    norm3(a.d, p);
    for (int k = 0; k < 3; ++k) a.lp[bs * 3 + k] = p[k];

    const int V = a.vcount[b], maxv = a.d.maxv;
    float q[3] = {qnan, qnan, qnan};
    if (s < a.in_num) {
        const size_t bi = (size_t)b * a.in_num + s;
        const int64_t vi = a.vidx[bi];
        if (vi >= 0 && vi < V) {
            const int* c = a.coords + ((size_t)b * maxv + vi) * 3;
            for (int k = 0; k < 3; ++k) q[k] = centre(a.d, k, c[2 - k]) + (float)a.u_in[bi * 3 + k];
        }
        a.lab[bs] = 1.f;
    } else {
        const int out_num = a.S - a.in_num;
        const size_t bo = (size_t)b * out_num + (s - a.in_num);
        const int64_t r = a.erank[bo];
        if (r >= 0 && r < (int64_t)a.d.cells - V) {
            // the r-th empty cell in row-major order: with the kept keys k_0 < k_1 < ..., the smallest j with k_j - j > r; cell r + j
            const int* kk = a.kkeys + (size_t)b * maxv;
            int lo = 0, hi = V;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if ((int64_t)kk[mid] - mid > r) hi = mid;
                else lo = mid + 1;
            }
            const int64_t cell = r + lo;
            const int G1 = a.d.g[1], G2 = a.d.g[2];
            const int c[3] = {(int)(cell / ((int64_t)G1 * G2)), (int)((cell / G2) % G1), (int)(cell % G2)};
            for (int k = 0; k < 3; ++k) q[k] = centre(a.d, k, c[k]) + (float)a.u_out[bo * 3 + k];
        }
        a.lab[bs] = 0.f;
    }
    norm3(a.d, q);
    for (int k = 0; k < 3; ++k) a.qp[bs * 3 + k] = q[k];
}

// ------------------------------------------------------------------------------------------------ host
struct Frames {
    int64_t total = 0, max_n = 0;
};

int check_offsets(const int64_t* offsets, int32_t batch, Frames* f, const char* who) {
    RALD_CHECK(offsets && batch >= 1 && batch <= 65535, std::string(who) + ": offsets required and 1 <= batch <= 65535");
    RALD_CHECK(offsets[0] == 0, std::string(who) + ": offsets[0] must be 0");
    for (int b = 0; b < batch; ++b) {
        const int64_t n = offsets[b + 1] - offsets[b];
        RALD_CHECK(n >= 0 && n <= INT32_MAX, std::string(who) + ": frame " + std::to_string(b) + " has " + std::to_string(n) +
                                                 " points (offsets must be non-decreasing, frames below 2^31 points)");
        f->max_n = std::max(f->max_n, n);
    }
    f->total = offsets[batch];
    return 0;
}

struct Ws {
    char* base;
    size_t o = 0;
    char* take(int64_t bytes) { char* q = base + o; o += round_up(std::max<int64_t>(bytes, 1), 256); return q; }
};

int64_t ws_offsets(int32_t batch) { return round_up((int64_t)(batch + 1) * 8, 256); }

// the offsets are the caller's (pageable) host array: the copy completes before this returns, so the caller may free it at once
int upload_offsets(const int64_t* offsets, int32_t batch, void* ws, hipStream_t st) {
    RALD_HIP(hipMemcpyWithStream(ws, offsets, (size_t)(batch + 1) * 8, hipMemcpyHostToDevice, st));
    return 0;
}

}  // namespace

int lidar_check_config(const rald_lidar_config& c, Lidar* out) {
    Lidar h{};
    h.cfg = c;
    int64_t cells = 1;
    for (int a = 0; a < 3; ++a) {
        RALD_CHECK(std::isfinite(c.voxel_size[a]) && c.voxel_size[a] > 0, "lidar: voxel_size must be positive (axis " + std::to_string(a) + ")");
        RALD_CHECK(std::isfinite(c.pc_range[a]) && std::isfinite(c.pc_range[3 + a]), "lidar: pc_range must be finite");
        const double g = std::round((c.pc_range[3 + a] - c.pc_range[a]) / c.voxel_size[a]);
        RALD_CHECK(g >= 1 && g < 2147483648.0, "lidar: the grid needs at least one cell per axis (axis " + std::to_string(a) + ")");
        h.grid[a] = (int64_t)g;
        cells = cells * h.grid[a];
        RALD_CHECK(cells < 2147483648LL, "lidar: the grid has over 2^31 cells");
    }
    h.cells = cells;
    h.key_passes = 0;
    for (int64_t m = cells; m > 0; m >>= 8) ++h.key_passes;
    RALD_CHECK(c.max_points_per_voxel >= 1 && c.max_voxels >= 1, "lidar: max_points_per_voxel and max_voxels must be positive");
    RALD_CHECK(c.num_point_features >= 3, "lidar: num_point_features must be at least 3");
    RALD_CHECK((int64_t)c.max_voxels * c.max_points_per_voxel * c.num_point_features < ((int64_t)1 << 40), "lidar: voxel tensor too large");
    if (out) *out = h;
    return 0;
}

int64_t lidar_workspace_bytes(const Lidar& h, int32_t batch, int64_t total) {
    (void)h;
    const int64_t B = batch, T = std::max<int64_t>(total, 1);
    const int64_t chunks = (T + CT - 1) / CT;
    const int64_t crop = round_up(T * 12, 256) + round_up(T, 256) + round_up(B * chunks * 4, 256);
    const int64_t vox = 7 * round_up(T * 4, 256);
    return ws_offsets(batch) + std::max(crop, vox);
}

int lidar_crop(const Lidar& h, const float* points, int32_t in_stride, const int64_t* offsets, int32_t batch, float* out, int32_t* counts,
               void* workspace, int64_t workspace_bytes, hipStream_t st) {
    Frames f;
    RALD_TRY(check_offsets(offsets, batch, &f, "lidar_crop"));
    RALD_CHECK(out && counts && workspace && (points || f.total == 0) && in_stride >= 3, "lidar_crop: bad argument");
    RALD_CHECK(workspace_bytes >= lidar_workspace_bytes(h, batch, f.total), "lidar_crop: workspace too small (rald_lidar_workspace_bytes)");
    Ws ws{(char*)workspace};
    CropArgs a{};
    a.off = (const int64_t*)ws.take((batch + 1) * 8);
    RALD_TRY(upload_offsets(offsets, batch, (void*)a.off, st));
    const int64_t T = std::max<int64_t>(f.total, 1);
    a.chunks = (int)std::max<int64_t>((f.max_n + CT - 1) / CT, 1);
    a.stage = (float*)ws.take(T * 12);
    a.flag = (unsigned char*)ws.take(T);
    a.ccnt = (int*)ws.take((int64_t)batch * a.chunks * 4);
    a.pts = points;
    a.stride = in_stride;
    a.out = out;
    a.counts = counts;
    a.d = derive(h);
    const dim3 g(a.chunks, batch);
    hipLaunchKernelGGL(lid_crop_stage, g, dim3(CT), 0, st, a);
    hipLaunchKernelGGL(lid_crop_emit, g, dim3(CT), 0, st, a);
    RALD_HIP(hipGetLastError());
    return 0;
}

int lidar_voxelize(const Lidar& h, const float* points, const int64_t* offsets, const int32_t* counts, int32_t batch, int32_t to_polar,
                   float* polar_out, float* voxels, int32_t* coords, int32_t* num_points, int32_t* kept_keys, int32_t* voxel_counts,
                   void* workspace, int64_t workspace_bytes, hipStream_t st) {
    Frames f;
    RALD_TRY(check_offsets(offsets, batch, &f, "lidar_voxelize"));
    RALD_CHECK(coords && num_points && kept_keys && voxel_counts && workspace && (points || f.total == 0), "lidar_voxelize: bad argument");
    RALD_CHECK(!to_polar || (polar_out && h.cfg.num_point_features == 3),
               "lidar_voxelize: the polar conversion needs num_point_features == 3 and a polar_out buffer [total][3]");
    RALD_CHECK(workspace_bytes >= lidar_workspace_bytes(h, batch, f.total), "lidar_voxelize: workspace too small (rald_lidar_workspace_bytes)");
    const rald_lidar_config& c = h.cfg;
    Ws ws{(char*)workspace};
    VoxArgs a{};
    a.off = (const int64_t*)ws.take((batch + 1) * 8);
    RALD_TRY(upload_offsets(offsets, batch, (void*)a.off, st));
    const int64_t T = std::max<int64_t>(f.total, 1);
    a.keyA = (unsigned*)ws.take(T * 4);
    a.keyB = (unsigned*)ws.take(T * 4);
    a.idxA = (int*)ws.take(T * 4);
    a.idxB = (int*)ws.take(T * 4);
    a.hf = (int*)ws.take(T * 4);
    a.segst = (int*)ws.take(T * 4);
    a.seglen = (int*)ws.take(T * 4);
    a.pts = points;
    a.counts = counts;
    a.to_polar = to_polar ? 1 : 0;
    a.polar = polar_out;
    a.passes = h.key_passes;
    a.voxels = voxels;
    a.coords = coords;
    a.npts = num_points;
    a.kkeys = kept_keys;
    a.vcount = voxel_counts;
    a.d = derive(h);
    if (voxels)
        RALD_HIP(hipMemsetAsync(voxels, 0, (size_t)batch * c.max_voxels * c.max_points_per_voxel * c.num_point_features * 4, st));
    const int chunks = (int)std::max<int64_t>((f.max_n + CT - 1) / CT, 1);
    hipLaunchKernelGGL(lid_vox_keys, dim3(chunks, batch), dim3(CT), 0, st, a);
    hipLaunchKernelGGL(lid_vox_sort, dim3(batch), dim3(FT), 0, st, a);
    hipLaunchKernelGGL(lid_vox_segs, dim3(batch), dim3(FT), 0, st, a);
    RALD_HIP(hipGetLastError());
    return 0;
}

int lidar_queries(const Lidar& h, const float* points, const int64_t* offsets, int32_t batch, int32_t num_samples, int32_t in_num,
                  const int64_t* sample_idx, const double* u_in, const int64_t* voxel_idx, const double* u_out, const int64_t* empty_rank,
                  const int32_t* coords, const int32_t* kept_keys, const int32_t* voxel_counts, float* lidar_points, float* query_points,
                  float* query_labels, void* workspace, int64_t workspace_bytes, hipStream_t st) {
    Frames f;
    RALD_TRY(check_offsets(offsets, batch, &f, "lidar_queries"));
    RALD_CHECK(num_samples >= 1 && in_num >= 0 && in_num <= num_samples, "lidar_queries: need 1 <= num_samples and 0 <= in_num <= num_samples");
    const bool has_out = in_num < num_samples;
    RALD_CHECK(sample_idx && (in_num == 0 || (u_in && voxel_idx)) && (!has_out || (u_out && empty_rank)) && coords && kept_keys &&
                   voxel_counts && lidar_points && query_points && query_labels && workspace && (points || f.total == 0),
               "lidar_queries: bad argument");
    RALD_CHECK(workspace_bytes >= ws_offsets(batch), "lidar_queries: workspace too small (rald_lidar_workspace_bytes)");
    QueryArgs a{};
    a.off = (const int64_t*)workspace;
    RALD_TRY(upload_offsets(offsets, batch, workspace, st));
    a.pts = points;
    a.S = num_samples;
    a.in_num = in_num;
    a.sidx = sample_idx;
    a.u_in = u_in;
    a.vidx = voxel_idx;
    a.u_out = u_out;
    a.erank = empty_rank;
    a.coords = coords;
    a.kkeys = kept_keys;
    a.vcount = voxel_counts;
    a.lp = lidar_points;
    a.qp = query_points;
    a.lab = query_labels;
    a.d = derive(h);
    hipLaunchKernelGGL(lid_queries, dim3((num_samples + CT - 1) / CT, batch), dim3(CT), 0, st, a);
    RALD_HIP(hipGetLastError());
    return 0;
}

}  // namespace rald
