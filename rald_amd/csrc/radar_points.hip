// Helper-point extraction on the device: RAEIVV intensity cubes -> the CFAR query points the decoder's aug_query_helper reads
// (dataset_preprocessor/cache_test_cfar.py:68-93 with cache_test_cfar_utils.py rae_interpo / weighted_allocation /
// RA2DDetectorTensor / cube_idx2coord and lidar.filter_points_polar, a host chain in the reference).  Per frame:
//   pts_slice_sums  (slice, frame)  trilinear value of every voxel of a target range slice, summed in double in a fixed order
//   pts_allocate    (frame)         the per-slice point counts (weighted_allocation, in double), exclusive offsets, frame status
//   pts_select      (slice, frame)  the slice regenerated into LDS as order-preserving keys, radix select of the k-th largest,
//                                   ordered compaction of the k chosen (ties at the k-th value: lowest flat index first), stable
//                                   LSD radix sort of the chosen indices by value descending through the workspace
//   pts_emit        (slice, frame)  peaks / intensities in output order, float32 table lookup, keep masks, ordered compaction
// The upsampled cube is never stored: a target slice depends on two source range rows, read strided from channel 0 of the cube.
// No float atomics (only LDS integer counters): a frame's output is bit-identical in any batch and from run to run.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "radar_points.h"

namespace rald {

namespace {

constexpr int SUM_THREADS = 256;
constexpr int SEL_THREADS = 1024;
constexpr int SEL_WAVES = SEL_THREADS / 64;
constexpr int EMIT_THREADS = 256;
constexpr int EMIT_WAVES = EMIT_THREADS / 64;
constexpr int MAX_SLICE = 32768;         // tgt_a * tgt_e: the keys of one slice in LDS (128 KiB) and 16-bit flat indices

struct PtsArgs {
    const float* cubes;
    const PtsLerp* lr;
    const PtsLerp* la;
    const PtsLerp* le;
    const float* ax_r;
    const float* ax_a;
    const float* ax_e;
    const uint8_t* keep_r;
    const uint8_t* keep_a;
    const uint8_t* keep_e;
    double* sums;             // [B][tgt_r]
    int* cnt;                 // [B][tgt_r] points of each slice
    int* off;                 // [B][tgt_r] exclusive offsets of the slices in the frame's output
    int* kept;                // [B][tgt_r] points of each slice the FOV filter keeps
    int* sel;                 // [B][tgt_r] which index buffer holds the slice's sorted indices
    int* status;              // [B] 0, -1 (no positive finite total), -2 (a slice count outside [0, tgt_a * tgt_e])
    unsigned short* idx0;     // [B][num] flat indices a * tgt_e + e, ping
    unsigned short* idx1;     // [B][num] pong
    float* points;            // [B][num][3]
    int* counts;              // [B]
    int* peaks;               // [B][num][3] or null
    float* intens;            // [B][num] or null
    int in_r, in_a, in_e, C, tgt_r, tgt_a, tgt_e, num;
};

// torch's CPU kernel evaluates t0 * w0 + t1 * w1 per axis, each product rounded.  Contraction is off here so that every kernel
// (the select keys, the emitted intensities, the slice sums) computes the same bits: hipcc would otherwise fuse differently per kernel.
__device__ __forceinline__ float lerp2(float x0, float x1, float w0, float w1) {
#pragma clang fp contract(off)
    return x0 * w0 + x1 * w1;
}

// F.interpolate(mode='trilinear', align_corners=False) at (r, a, e): range outermost, elevation innermost
__device__ __forceinline__ float interp(const PtsArgs& p, const float* __restrict__ cube, const PtsLerp& lr, int a, int e) {
    const PtsLerp la = p.la[a], le = p.le[e];
    auto X = [&](int ri, int ai, int ei) { return cube[(((size_t)ri * p.in_a + ai) * p.in_e + ei) * p.C]; };
    auto ve = [&](int ri, int ai) { return lerp2(X(ri, ai, le.i0), X(ri, ai, le.i1), le.w0, le.w1); };
    auto va = [&](int ri) { return lerp2(ve(ri, la.i0), ve(ri, la.i1), la.w0, la.w1); };
    return lerp2(va(lr.i0), va(lr.i1), lr.w0, lr.w1);
}

__device__ __forceinline__ const float* frame_cube(const PtsArgs& p, int b) {
    return p.cubes + (size_t)b * p.in_r * p.in_a * p.in_e * p.C;
}

// order-preserving key of a float (larger value -> larger key), -0.0 folded to +0.0
__device__ __forceinline__ unsigned fkey(float v) {
    const unsigned u = __float_as_uint(v == 0.f ? 0.f : v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ unsigned long long lanes_below(int lane) { return (1ull << lane) - 1ull; }

// grid (tgt_r, B): sums[b][r] = sum over the slice's voxels of the interpolated value, in double, fixed order
__global__ __launch_bounds__(SUM_THREADS) void pts_slice_sums(PtsArgs p) {
    __shared__ double red[SUM_THREADS];
    const int r = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, n = p.tgt_a * p.tgt_e;
    const float* cube = frame_cube(p, b);
    const PtsLerp lr = p.lr[r];
    double s = 0.0;
    for (int i = tid; i < n; i += SUM_THREADS) {
        const int a = i / p.tgt_e, e = i - a * p.tgt_e;
        s += (double)interp(p, cube, lr, a, e);
    }
    red[tid] = s;
    __syncthreads();
    for (int o = SUM_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) p.sums[(size_t)b * p.tgt_r + r] = red[0];
}

// grid (B), one thread: weighted_allocation in double.  count_r = floor(num * s_r / S); the surplus num - sum(count) goes to the
// first slice of largest weight.  Status -1 when S is not positive and finite (the reference divides 0 by 0 and fails in
// np.argpartition), -2 when a count falls outside [0, tgt_a * tgt_e] (the reference's assert).
__global__ void pts_allocate(PtsArgs p) {
    if (threadIdx.x != 0) return;
    const int b = blockIdx.x, R = p.tgt_r, cap = p.tgt_a * p.tgt_e;
    const double* s = p.sums + (size_t)b * R;
    int* cnt = p.cnt + (size_t)b * R;
    int* off = p.off + (size_t)b * R;
    double S = 0.0;
    int amax = 0;
    for (int r = 0; r < R; ++r) {
        S += s[r];
        if (s[r] > s[amax]) amax = r;
    }
    if (!(S > 0.0) || !isfinite(S)) {
        p.status[b] = -1;
        return;
    }
    double sumc = 0.0;
    for (int r = 0; r < R; ++r) sumc += floor(s[r] / S * (double)p.num);
    int status = 0, run = 0;
    for (int r = 0; r < R; ++r) {
        double c = floor(s[r] / S * (double)p.num);
        if (r == amax) c += (double)p.num - sumc;
        if (!(c >= 0.0 && c <= (double)cap)) {
            status = -2;
            break;
        }
        cnt[r] = (int)c;
        off[r] = run;
        run += (int)c;
    }
    if (status == 0 && run != p.num) status = -2;    // sums that lose integers in double (negative weights of huge magnitude)
    p.status[b] = status;
}

// grid (tgt_r, B), dynamic LDS tgt_a * tgt_e keys: the k = cnt[b][r] chosen flat indices of the slice, by value descending and
// flat index ascending, into idx0 or idx1 (sel[b][r]) at the slice's offset; kept[b][r] = how many the keep masks pass
__global__ __launch_bounds__(SEL_THREADS) void pts_select(PtsArgs p) {
    extern __shared__ unsigned keys[];
    __shared__ unsigned hist[256], base[256];
    __shared__ unsigned wcnt[SEL_WAVES][256];
    __shared__ unsigned wtot[SEL_WAVES];
    __shared__ unsigned s_T, s_krem, s_run, s_kept, s_skip;
    const int r = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const size_t br = (size_t)b * p.tgt_r + r;
    if (p.status[b] < 0) return;
    const int k = p.cnt[br];
    if (k == 0) {
        if (tid == 0) {
            p.kept[br] = 0;
            p.sel[br] = 0;
        }
        return;
    }
    const int n = p.tgt_a * p.tgt_e, E = p.tgt_e;
    const size_t seg = (size_t)b * p.num + p.off[br];
    const float* cube = frame_cube(p, b);
    const PtsLerp lr = p.lr[r];
    for (int i = tid; i < n; i += SEL_THREADS) {
        const int a = i / E, e = i - a * E;
        keys[i] = fkey(interp(p, cube, lr, a, e));
    }
    for (int i = tid; i < SEL_WAVES * 256; i += SEL_THREADS) (&wcnt[0][0])[i] = 0;
    if (tid == 0) {
        s_run = 0;
        s_kept = 0;
    }
    __syncthreads();

    // radix select, 8 bits per pass from the top: T = the k-th largest key, krem = how many keys equal to T are taken
    unsigned prefix = 0, mask = 0, krem = (unsigned)k;
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        for (int i = tid; i < n; i += SEL_THREADS) {
            const unsigned u = keys[i];
            if ((u & mask) == prefix) atomicAdd(&hist[(u >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (w == 0) {                       // lane l holds digits 255 - 4l .. 252 - 4l: a prefix over lanes counts from the top
            unsigned c[4], sum = 0;
            for (int j = 0; j < 4; ++j) {
                c[j] = hist[255 - 4 * lane - j];
                sum += c[j];
            }
            unsigned incl = sum;
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned t = __shfl_up(incl, o);
                if (lane >= o) incl += t;
            }
            unsigned above = incl - sum;
            for (int j = 0; j < 4; ++j) {
                if (above < krem && krem <= above + c[j]) {
                    s_T = prefix | ((unsigned)(255 - 4 * lane - j) << shift);
                    s_krem = krem - above;
                }
                above += c[j];
            }
        }
        __syncthreads();
        prefix = s_T;
        krem = s_krem;
        mask |= 255u << shift;
    }
    const unsigned T = prefix, need = krem;

    // ordered compaction in flat-index order: everything above T, then the first `need` keys equal to T.  A chosen element's
    // position is (#above before it) + min(#equal before it, need); the running counts travel packed (above << 16 | equal).
    const bool keep_r = p.keep_r[r] != 0;
    unsigned short* const seg0 = p.idx0 + seg;
    unsigned short* const seg1 = p.idx1 + seg;
    unsigned kept = 0;
    for (int t0 = 0; t0 < n; t0 += SEL_THREADS) {
        const int i = t0 + tid;
        const unsigned u = i < n ? keys[i] : 0u;
        const bool gt = i < n && u > T, eq = i < n && u == T;
        const unsigned long long bg = __ballot(gt), be = __ballot(eq), lt = lanes_below(lane);
        if (lane == 0) wtot[w] = ((unsigned)__popcll(bg) << 16) | (unsigned)__popcll(be);
        __syncthreads();
        unsigned pre = s_run, tot = 0;
        for (int j = 0; j < w; ++j) pre += wtot[j];
        if (tid == 0)
            for (int j = 0; j < SEL_WAVES; ++j) tot += wtot[j];
        const unsigned gb = (pre >> 16) + (unsigned)__popcll(bg & lt), eb = (pre & 0xffffu) + (unsigned)__popcll(be & lt);
        if (gt || (eq && eb < need)) {
            seg0[gb + min(eb, need)] = (unsigned short)i;
            const int a = i / E, e = i - a * E;
            kept += (keep_r && p.keep_a[a] && p.keep_e[e]) ? 1u : 0u;
        }
        __syncthreads();
        if (tid == 0) s_run += tot;
    }
    if (kept) atomicAdd(&s_kept, kept);

    // stable LSD radix sort of the k indices on 255 - digit (value descending); they enter in ascending flat index, so equal values
    // stay in that order.  A pass whose digits are all equal moves nothing and is skipped.
    unsigned short* src = seg0;
    unsigned short* dst = seg1;
    int which = 0;
    for (int shift = 0; shift < 32; shift += 8) {
        if (tid < 256) hist[tid] = 0;
        if (tid == 0) s_skip = 0;
        __syncthreads();
        for (int j = tid; j < k; j += SEL_THREADS) atomicAdd(&hist[255u - ((keys[src[j]] >> shift) & 255u)], 1u);
        __syncthreads();
        if (w == 0) {                       // exclusive scan in ascending digit order, lane l holds digits 4l .. 4l + 3
            unsigned c[4], sum = 0;
            for (int j = 0; j < 4; ++j) {
                c[j] = hist[4 * lane + j];
                sum += c[j];
                if (c[j] == (unsigned)k) s_skip = 1;
            }
            unsigned incl = sum;
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned t = __shfl_up(incl, o);
                if (lane >= o) incl += t;
            }
            unsigned run = incl - sum;
            for (int j = 0; j < 4; ++j) {
                base[4 * lane + j] = run;
                run += c[j];
            }
        }
        __syncthreads();
        const bool skip = s_skip != 0;
        __syncthreads();
        if (skip) continue;
        for (int t0 = 0; t0 < k; t0 += SEL_THREADS) {
            const int j = t0 + tid;
            const bool valid = j < k;
            const unsigned id = valid ? src[j] : 0u;
            const unsigned dg = valid ? 255u - ((keys[id] >> shift) & 255u) : 0u;
            unsigned long long m = __ballot(valid);
            for (int bit = 0; bit < 8; ++bit) {
                const bool set = (dg >> bit) & 1u;
                const unsigned long long bb = __ballot(valid && set);
                m &= set ? bb : ~bb;
            }
            const unsigned rank = (unsigned)__popcll(m & lanes_below(lane));
            if (valid && rank == 0) wcnt[w][dg] = (unsigned)__popcll(m);
            __syncthreads();
            if (tid < 256) {
                unsigned run = base[tid];
                for (int ww = 0; ww < SEL_WAVES; ++ww) {
                    const unsigned c = wcnt[ww][tid];
                    wcnt[ww][tid] = run;
                    run += c;
                }
                base[tid] = run;
            }
            __syncthreads();
            if (valid) dst[wcnt[w][dg] + rank] = (unsigned short)id;
            __syncthreads();
            if (tid < 256)
                for (int ww = 0; ww < SEL_WAVES; ++ww) wcnt[ww][tid] = 0;
            __syncthreads();
        }
        unsigned short* t = src;
        src = dst;
        dst = t;
        which ^= 1;
    }
    __syncthreads();
    if (tid == 0) {
        p.kept[br] = (int)s_kept;
        p.sel[br] = which;
    }
}

// grid (tgt_r, B): the slice's peaks / intensities at its offset, and its kept points at (kept points of the slices before it)
// in the frame's compacted output; the r = 0 workgroup writes counts[b] (the frame's status on a rejected frame)
__global__ __launch_bounds__(EMIT_THREADS) void pts_emit(PtsArgs p) {
    __shared__ int s_pre, s_all;
    __shared__ unsigned wtot[EMIT_WAVES];
    __shared__ unsigned s_run;
    const int r = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, R = p.tgt_r;
    const int st = p.status[b];
    if (st < 0) {
        if (r == 0 && tid == 0) p.counts[b] = st;
        return;
    }
    if (tid == 0) {
        s_pre = 0;
        s_all = 0;
        s_run = 0;
    }
    __syncthreads();
    const int* kept = p.kept + (size_t)b * R;
    int pre = 0, all = 0;
    for (int q = tid; q < R; q += EMIT_THREADS) {
        const int v = kept[q];
        if (q < r) pre += v;
        all += v;
    }
    if (pre) atomicAdd(&s_pre, pre);
    if (r == 0 && all) atomicAdd(&s_all, all);
    __syncthreads();
    if (r == 0 && tid == 0) p.counts[b] = s_all;
    const size_t br = (size_t)b * R + r;
    const int k = p.cnt[br], E = p.tgt_e;
    const size_t seg = (size_t)b * p.num + p.off[br];
    const unsigned short* src = (p.sel[br] ? p.idx1 : p.idx0) + seg;
    const float* cube = frame_cube(p, b);
    const PtsLerp lr = p.lr[r];
    const bool keep_r = p.keep_r[r] != 0;
    const float cr = p.ax_r[r];
    float* out = p.points + ((size_t)b * p.num + s_pre) * 3;
    for (int t0 = 0; t0 < k; t0 += EMIT_THREADS) {
        const int j = t0 + tid;
        const bool valid = j < k;
        const int id = valid ? src[j] : 0, a = id / E, e = id - a * E;
        if (valid && p.peaks) {
            int* pk = p.peaks + (seg + j) * 3;
            pk[0] = r;
            pk[1] = a;
            pk[2] = e;
        }
        if (valid && p.intens) p.intens[seg + j] = interp(p, cube, lr, a, e);
        const bool keep = valid && keep_r && p.keep_a[a] && p.keep_e[e];
        const unsigned long long bk = __ballot(keep);
        if (lane == 0) wtot[w] = (unsigned)__popcll(bk);
        __syncthreads();
        unsigned pos = s_run, tot = 0;
        for (int q = 0; q < w; ++q) pos += wtot[q];
        if (tid == 0)
            for (int q = 0; q < EMIT_WAVES; ++q) tot += wtot[q];
        pos += (unsigned)__popcll(bk & lanes_below(lane));
        if (keep) {
            float* o = out + (size_t)pos * 3;
            o[0] = cr;
            o[1] = p.ax_a[a];
            o[2] = p.ax_e[e];
        }
        __syncthreads();
        if (tid == 0) s_run += tot;
    }
}

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

// compute_indices_weights_linear of torch's CPU upsampling, in float: src = max(scale * (d + 0.5) - 0.5, 0), scale = in / out
void lerp_table(int in, int out, std::vector<PtsLerp>& t) {
    t.resize(out);
    const float scale = (float)in / (float)out;
    for (int d = 0; d < out; ++d) {
        const float x = scale * ((float)d + 0.5f);
        float src = x - 0.5f;
        if (src < 0.f) src = 0.f;
        const int i0 = std::min((int)std::floor(src), in - 1);
        const float l1 = std::min(std::max(src - (float)i0, 0.f), 1.f);
        t[d] = PtsLerp{i0, i0 + (i0 < in - 1 ? 1 : 0), 1.f - l1, l1};
    }
}

}  // namespace

int radar_points_check_config(const rald_radar_points_config& c) {
    RALD_CHECK(c.in_r >= 1 && c.in_a >= 1 && c.in_e >= 1 && c.in_channels >= 1 && c.tgt_r >= 1 && c.tgt_a >= 1 && c.tgt_e >= 1,
               "radar_points: every input and target dimension must be positive");
    RALD_CHECK((int64_t)c.tgt_a * c.tgt_e <= MAX_SLICE, "radar_points: tgt_a * tgt_e = " + std::to_string((int64_t)c.tgt_a * c.tgt_e) +
                                                           " exceeds " + std::to_string(MAX_SLICE) + " (one range slice must fit in LDS)");
    const int64_t cap = std::min<int64_t>((int64_t)c.tgt_r * c.tgt_a * c.tgt_e, INT32_MAX);
    RALD_CHECK(c.num_points >= 1 && c.num_points <= cap, "radar_points: num_points = " + std::to_string(c.num_points) + " must be in [1, " +
                                                             std::to_string(cap) + "] (tgt_r * tgt_a * tgt_e)");
    return 0;
}

int64_t radar_points_workspace_bytes(const rald_radar_points_config& c, int32_t batch) {
    const int64_t B = batch, R = c.tgt_r;
    return round_up(B * R * 8, 256) + 4 * round_up(B * R * 4, 256) + round_up(B * 4, 256) + 2 * round_up(B * c.num_points * 2, 256);
}

RadarPoints::~RadarPoints() {
    if (dev) (void)hipFree(dev);
}

int radar_points_create(const rald_radar_points_config& cfg, const float* axis_r, const float* axis_a, const float* axis_e,
                        const uint8_t* keep_r, const uint8_t* keep_a, const uint8_t* keep_e, RadarPoints** out) {
    RALD_TRY(radar_points_check_config(cfg));
    RALD_CHECK(axis_r && axis_a && axis_e && keep_r && keep_a && keep_e,
               "radar_points: the three axis tables and keep masks (tgt_r / tgt_a / tgt_e entries each) are required");
    std::vector<PtsLerp> lr, la, le;
    lerp_table(cfg.in_r, cfg.tgt_r, lr);
    lerp_table(cfg.in_a, cfg.tgt_a, la);
    lerp_table(cfg.in_e, cfg.tgt_e, le);
    const int R = cfg.tgt_r, A = cfg.tgt_a, E = cfg.tgt_e;
    size_t off = 0;
    auto place = [&](size_t bytes) { const size_t o = off; off = align16(off + bytes); return o; };
    const size_t o_lr = place(R * sizeof(PtsLerp)), o_la = place(A * sizeof(PtsLerp)), o_le = place(E * sizeof(PtsLerp)),
                 o_ar = place(R * 4), o_aa = place(A * 4), o_ae = place(E * 4), o_kr = place(R), o_ka = place(A), o_ke = place(E);
    std::vector<char> t(off, 0);
    memcpy(t.data() + o_lr, lr.data(), R * sizeof(PtsLerp));
    memcpy(t.data() + o_la, la.data(), A * sizeof(PtsLerp));
    memcpy(t.data() + o_le, le.data(), E * sizeof(PtsLerp));
    memcpy(t.data() + o_ar, axis_r, R * 4);
    memcpy(t.data() + o_aa, axis_a, A * 4);
    memcpy(t.data() + o_ae, axis_e, E * 4);
    for (int i = 0; i < R; ++i) t[o_kr + i] = keep_r[i] ? 1 : 0;
    for (int i = 0; i < A; ++i) t[o_ka + i] = keep_a[i] ? 1 : 0;
    for (int i = 0; i < E; ++i) t[o_ke + i] = keep_e[i] ? 1 : 0;
    RadarPoints* h = new RadarPoints();
    h->cfg = cfg;
    hipError_t e = hipMalloc(&h->dev, t.size());
    if (e == hipSuccess) e = hipMemcpy(h->dev, t.data(), t.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)pts_select, hipFuncAttributeMaxDynamicSharedMemorySize, MAX_SLICE * 4);
    if (e != hipSuccess) {
        set_error(std::string("radar_points_create: ") + hipGetErrorString(e));
        delete h;
        return 2;
    }
    char* base = (char*)h->dev;
    h->lr = (const PtsLerp*)(base + o_lr);
    h->la = (const PtsLerp*)(base + o_la);
    h->le = (const PtsLerp*)(base + o_le);
    h->ax_r = (const float*)(base + o_ar);
    h->ax_a = (const float*)(base + o_aa);
    h->ax_e = (const float*)(base + o_ae);
    h->keep_r = (const uint8_t*)(base + o_kr);
    h->keep_a = (const uint8_t*)(base + o_ka);
    h->keep_e = (const uint8_t*)(base + o_ke);
    *out = h;
    return 0;
}

int radar_points_run(const RadarPoints& h, const float* cubes, int32_t batch, float* points, int32_t* counts, int32_t* peaks, float* intensities,
                     void* workspace, int64_t workspace_bytes, hipStream_t st) {
    const rald_radar_points_config& c = h.cfg;
    RALD_CHECK(cubes && points && counts && workspace && batch >= 1 && batch <= 65535, "radar_points_run: bad argument");
    RALD_CHECK(workspace_bytes >= radar_points_workspace_bytes(c, batch), "radar_points_run: workspace too small (rald_radar_points_workspace_bytes)");
    const int64_t B = batch, R = c.tgt_r;
    char* ws = (char*)workspace;
    size_t o = 0;
    auto take = [&](int64_t bytes) { char* q = ws + o; o += round_up(bytes, 256); return q; };
    PtsArgs p{};
    p.cubes = cubes;
    p.lr = h.lr; p.la = h.la; p.le = h.le;
    p.ax_r = h.ax_r; p.ax_a = h.ax_a; p.ax_e = h.ax_e;
    p.keep_r = h.keep_r; p.keep_a = h.keep_a; p.keep_e = h.keep_e;
    p.sums = (double*)take(B * R * 8);
    p.cnt = (int*)take(B * R * 4);
    p.off = (int*)take(B * R * 4);
    p.kept = (int*)take(B * R * 4);
    p.sel = (int*)take(B * R * 4);
    p.status = (int*)take(B * 4);
    p.idx0 = (unsigned short*)take(B * c.num_points * 2);
    p.idx1 = (unsigned short*)take(B * c.num_points * 2);
    p.points = points;
    p.counts = counts;
    p.peaks = peaks;
    p.intens = intensities;
    p.in_r = c.in_r; p.in_a = c.in_a; p.in_e = c.in_e; p.C = c.in_channels;
    p.tgt_r = c.tgt_r; p.tgt_a = c.tgt_a; p.tgt_e = c.tgt_e;
    p.num = (int)c.num_points;
    const dim3 g(c.tgt_r, batch);
    hipLaunchKernelGGL(pts_slice_sums, g, dim3(SUM_THREADS), 0, st, p);
    hipLaunchKernelGGL(pts_allocate, dim3(batch), dim3(64), 0, st, p);
    hipLaunchKernelGGL(pts_select, g, dim3(SEL_THREADS), (size_t)c.tgt_a * c.tgt_e * 4, st, p);
    hipLaunchKernelGGL(pts_emit, g, dim3(EMIT_THREADS), 0, st, p);
    RALD_HIP(hipGetLastError());
    return 0;
}

}  // namespace rald
