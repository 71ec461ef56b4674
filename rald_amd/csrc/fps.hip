// Farthest-point sampling of a ragged batch: k points per cloud, each the one farthest from those chosen so far.
// The arithmetic is defined to the bit (include/rald_hip.h): p' = fl(p * s) once at load, d2 = fl(fl(fl(dx*dx) + fl(dy*dy)) + fl(dz*dz))
// with no contraction, mind = min(mind, d2), the next choice = the largest mind, the smallest index on equal values.
//   fps_kernel<PER, STREAM, MAXT>   grid (cloud), nt = 64 .. MAXT threads (a power of two): thread t owns the points t, t + nt, t + 2 nt, ...
//     resident (STREAM = false): the scaled coordinates and mind of its PER points stay in registers for the whole run
//     streaming (STREAM = true): mind stays in registers, the scaled coordinates are re-read every iteration from an SoA copy in the
//                                scratch buffer (every thread reads back only what it wrote itself)
// One iteration: every thread knows the last winner's coordinates -> mind update and local arg-max -> wave all-reduce of the 64-bit key
// (mind's bits << 32 | 0xFFFFFFFF - index: mind >= +0, so the unsigned maximum is "largest distance, then smallest index") -> the lane
// that holds the wave's maximum writes key and coordinates into the wave's LDS slot -> ONE barrier -> every thread reads the waves' keys,
// takes the maximum and reads the winning slot's coordinates.  The slots are double-buffered by the iteration's parity: a slot is
// written again two iterations later, behind the barrier of the iteration between.
// The loop runs min(k, n) - 1 times, n <= max_per_sample <= 65536 and k both host arguments; nothing waits on another workgroup.
// Every global index comes from lane and loop counters (i < n), from start mod n, or is a fixed output slot; the LDS slot read is
// masked to the slots that exist.  Non-finite coordinates therefore change the selection (unspecified) but no address.
#include <cmath>

#include "common.h"
#include "kernels.h"

namespace rald {

namespace {

constexpr int FPS_MAX_THREADS = 1024;
constexpr int FPS_RESIDENT_PER = 32;                        // points per thread with coordinates in registers: 4 x 32 VGPRs, at most 512 threads
constexpr int FPS_STREAM_PER = 64;                          // mind values per thread of the streaming form: 64 VGPRs of the 128 at 1024 threads
constexpr int64_t FPS_RESIDENT_MAX = (int64_t)FPS_RESIDENT_PER * 512;                 // 16 384
constexpr int64_t FPS_MAX_POINTS = (int64_t)FPS_STREAM_PER * FPS_MAX_THREADS;         // 65 536

struct FpsArgs {
    const float* points; const int64_t* offsets; const int32_t* counts; const int64_t* start;
    int64_t n_dense, max_per_sample, soa_stride;
    int k;
    float sx, sy, sz;
    int64_t* out_idx; float* out_dist2; float* soa;
};

__device__ __forceinline__ float fps_d2(float ax, float ay, float az, float bx, float by, float bz) {
#pragma clang fp contract(off)                               // three products and two sums, each rounded: what numpy float32 computes
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return (dx * dx + dy * dy) + dz * dz;
}

__device__ __forceinline__ float fps_scale(float p, float s) {
#pragma clang fp contract(off)
    return p * s;
}

template <int CTRL>
__device__ __forceinline__ unsigned long long fps_max_dpp(unsigned long long v) {
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)v, CTRL, 0xF, 0xF, true);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(v >> 32), CTRL, 0xF, 0xF, true);
    const unsigned long long u = ((unsigned long long)hi << 32) | lo;
    return u > v ? u : v;
}

// maximum of the wave's 64 keys in every lane: four DPP steps inside the rows of 16 lanes, then lanes ^ 16 and ^ 32
__device__ __forceinline__ unsigned long long fps_wave_max(unsigned long long v) {
    v = fps_max_dpp<0xB1>(v);                                // quad_perm [1,0,3,2]
    v = fps_max_dpp<0x4E>(v);                                // quad_perm [2,3,0,1]
    v = fps_max_dpp<0x141>(v);                               // row_half_mirror
    v = fps_max_dpp<0x140>(v);                               // row_mirror
    unsigned long long u = __shfl_xor(v, 16, 64);
    v = u > v ? u : v;
    u = __shfl_xor(v, 32, 64);
    return u > v ? u : v;
}

template <int PER, bool STREAM, int MAXT>
__global__ __launch_bounds__(MAXT) void fps_kernel(FpsArgs a) {
    constexpr int WAVES = MAXT / 64;                         // LDS slots per buffer
    __shared__ unsigned long long s_key[2][WAVES];
    __shared__ float4 s_xyz[2][WAVES];
    constexpr int G = PER < 8 ? PER : 8;                     // points per uniform skip test (and per batch of streaming loads)
    const int b = blockIdx.x, t = threadIdx.x, nt = blockDim.x;
    int64_t row0, len;
    if (a.offsets) { row0 = a.offsets[b]; len = a.offsets[b + 1] - row0; }
    else { row0 = (int64_t)b * a.n_dense; len = a.n_dense; }
    if (a.counts) { const int64_t c = a.counts[b]; len = c < len ? c : len; }
    len = len < a.max_per_sample ? len : a.max_per_sample;   // a longer cloud is sampled from its first max_per_sample rows
    const int n = len > 0 ? (int)len : 0;                    // <= 65 536
    const int m = a.k < n ? a.k : n;
    int64_t* oi = a.out_idx + (int64_t)b * a.k;
    float* od = a.out_dist2 ? a.out_dist2 + (int64_t)b * a.k : nullptr;
    for (int j = m + t; j < a.k; j += nt) {                  // slots a short cloud cannot fill
        oi[j] = -1;
        if (od) od[j] = NAN;
    }
    if (n == 0) return;                                      // the whole workgroup, before any barrier
    const float* p = a.points + row0 * 3;
    // the streaming form's scaled copy: x, y, z arrays of soa_stride = PER * 1024 floats, so every slot of every thread exists
    float* soa_x = STREAM ? a.soa + (int64_t)b * 3 * a.soa_stride : nullptr;
    float* soa_y = soa_x + a.soa_stride;
    float* soa_z = soa_y + a.soa_stride;

    float px[STREAM ? 1 : PER], py[STREAM ? 1 : PER], pz[STREAM ? 1 : PER], mind[PER];
    if (STREAM) {
        // every slot of a group the loop reads (zeros behind the cloud), by the thread that reads it back: a plain loop, no registers kept
        const int group = G * nt;
        int end = (n + group - 1) / group * group;
        end = end < PER * nt ? end : PER * nt;
        for (int i = t; i < end; i += nt) {
            const bool in = i < n;
            const unsigned r = in ? (unsigned)i * 3u : 0u;      // a slot behind the cloud reads row 0 (n >= 1): no divergent load
            const float lx = p[r], ly = p[r + 1], lz = p[r + 2];
            soa_x[i] = in ? fps_scale(lx, a.sx) : 0.f; soa_y[i] = in ? fps_scale(ly, a.sy) : 0.f; soa_z[i] = in ? fps_scale(lz, a.sz) : 0.f;
        }
    }
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int i = t + j * nt;
        const bool in = i < n;
        if (!STREAM) {
            const unsigned r = in ? (unsigned)i * 3u : 0u;
            const float lx = p[r], ly = p[r + 1], lz = p[r + 2];
            px[j] = in ? fps_scale(lx, a.sx) : 0.f; py[j] = in ? fps_scale(ly, a.sy) : 0.f; pz[j] = in ? fps_scale(lz, a.sz) : 0.f;
        }
        // a slot behind the cloud: mind 0 at index >= n loses against every point of the cloud (mind >= 0 at a smaller index)
        mind[j] = in ? INFINITY : 0.f;
    }
    // slots of waves that do not exist: below every key of a point (wave 0 writes them before it reaches the first barrier)
    if (t < 2 * WAVES && t % WAVES >= nt / 64) s_key[t / WAVES][t % WAVES] = 0;

    int64_t s = a.start ? a.start[b] : 0;
    s %= n;
    const int c0 = (int)(s < 0 ? s + n : s);
    float cx = fps_scale(p[(int64_t)c0 * 3], a.sx), cy = fps_scale(p[(int64_t)c0 * 3 + 1], a.sy), cz = fps_scale(p[(int64_t)c0 * 3 + 2], a.sz);
    if (t == 0) {
        oi[0] = c0;
        if (od) od[0] = INFINITY;
    }
    const int wave = t >> 6;
    for (int it = 1; it < m; ++it) {
        float best = -1.f, bx = 0.f, by = 0.f, bz = 0.f;
        int bj = 0;                                          // the slot, not the index: a constant per unrolled step, nothing to keep per slot
        unsigned lane_off = (unsigned)t;
        // an empty statement the optimiser cannot see through: without it the 3 x PER load addresses are computed once before the loop
        // and kept in registers, which the streaming form does not have (the resource report showed spills); with it, one add per slot
        if (STREAM) asm volatile("" : "+v"(lane_off));
#pragma unroll
        for (int g = 0; g < PER; g += G) {
            if (g * nt < n) {                                // uniform: no point of this group of slots lies inside the cloud otherwise
                float x[G], y[G], z[G];
#pragma unroll
                for (int j = 0; j < G; ++j) {
                    if (STREAM) {
                        // unconditional loads: the copy holds every slot of a group that reaches into the cloud (zeros behind it)
                        const unsigned i = (unsigned)((g + j) * nt) + lane_off;
                        x[j] = soa_x[i]; y[j] = soa_y[i]; z[j] = soa_z[i];
                    } else {
                        x[j] = px[g + j]; y[j] = py[g + j]; z[j] = pz[g + j];
                    }
                }
#pragma unroll
                for (int j = 0; j < G; ++j) {
                    const float mj = fminf(mind[g + j], fps_d2(x[j], y[j], z[j], cx, cy, cz));
                    mind[g + j] = mj;
                    if (mj > best) { best = mj; bj = g + j; bx = x[j]; by = y[j]; bz = z[j]; }     // strict: ascending indices, the first stays
                }
            }
        }
        const unsigned long long key = ((unsigned long long)__float_as_uint(best) << 32) | (0xFFFFFFFFu - (unsigned)(t + bj * nt));
        const unsigned long long wkey = fps_wave_max(key);
        const int buf = it & 1;
        if (key == wkey) {                                   // one lane: a key carries its point's index
            s_key[buf][wave] = key;
            s_xyz[buf][wave] = make_float4(bx, by, bz, 0.f);
        }
        __syncthreads();
        unsigned long long win = s_key[buf][0];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) { const unsigned long long u = s_key[buf][w]; win = u > win ? u : win; }
        const unsigned idx = 0xFFFFFFFFu - (unsigned)win;
        const float4 c = s_xyz[buf][(idx & (unsigned)(nt - 1)) >> 6];     // the winner's thread is index mod nt (nt a power of two)
        cx = c.x; cy = c.y; cz = c.z;
        if (t == 0) {
            oi[it] = (int64_t)idx;
            if (od) od[it] = __uint_as_float((unsigned)(win >> 32));
        }
    }
}

// threads of the streaming form: the smallest power of two that gives every point a thread, 64 .. 1024
inline int fps_threads(int64_t max_per_sample) {
    int nt = 64;
    while (nt < FPS_MAX_THREADS && nt < max_per_sample) nt *= 2;
    return nt;
}

inline int64_t fps_soa_stride(int64_t max_per_sample) { return (max_per_sample <= 8 * FPS_MAX_THREADS ? 8 : FPS_STREAM_PER) * (int64_t)FPS_MAX_THREADS; }

// 1 resident, 2 streaming; 0 where the request cannot be served
inline int fps_pick_form(int64_t max_per_sample, int form) {
    if (max_per_sample < 1 || max_per_sample > FPS_MAX_POINTS || form < 0 || form > 2) return 0;
    if (form == 0) return max_per_sample <= FPS_RESIDENT_MAX ? 1 : 2;
    return form == 1 && max_per_sample > FPS_RESIDENT_MAX ? 0 : form;
}

template <int PER, bool STREAM, int MAXT>
void fps_launch(const FpsArgs& a, int B, int nt, hipStream_t st) {
    hipLaunchKernelGGL((fps_kernel<PER, STREAM, MAXT>), dim3(B), dim3(nt), 0, st, a);
}

}  // namespace

int64_t fps_scratch_bytes(int B, int64_t max_per_sample, int form) {
    const int f = fps_pick_form(max_per_sample, form);
    if (B < 1 || f == 0) return -1;
    return f == 2 ? (int64_t)B * 3 * fps_soa_stride(max_per_sample) * 4 : 0;
}

int fps_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int B, int64_t n_dense, int64_t max_per_sample, int k,
               const int64_t* start, const float* scale3_host, int64_t* out_idx, float* out_dist2, void* scratch, int64_t scratch_bytes, int form,
               hipStream_t st) {
    RALD_CHECK(points && out_idx, "fps_ragged: null pointer (points, out_idx)");
    RALD_CHECK(B >= 1, "fps_ragged: batch must be >= 1");
    RALD_CHECK(k >= 1, "fps_ragged: k must be >= 1");
    RALD_CHECK(offsets || n_dense >= 0, "fps_ragged: n_dense must be >= 0 without offsets");
    RALD_CHECK(form >= 0 && form <= 2, "fps_ragged: form must be 0 (auto), 1 (resident) or 2 (streaming)");
    RALD_CHECK(max_per_sample >= 1 && max_per_sample <= FPS_MAX_POINTS, "fps_ragged: max_per_sample must be 1 .. 65536");
    const int f = fps_pick_form(max_per_sample, form);
    RALD_CHECK(f != 0, "fps_ragged: the resident form takes max_per_sample up to 16384");
    const int64_t need = fps_scratch_bytes(B, max_per_sample, form);
    RALD_CHECK(scratch_bytes >= need, "fps_ragged: scratch too small");
    RALD_CHECK(need == 0 || (scratch && (uintptr_t)scratch % 16 == 0), "fps_ragged: null or unaligned scratch");
    FpsArgs a;
    a.points = points; a.offsets = offsets; a.counts = counts; a.start = start;
    a.n_dense = n_dense; a.max_per_sample = max_per_sample; a.soa_stride = fps_soa_stride(max_per_sample);
    a.k = k;
    a.sx = scale3_host ? scale3_host[0] : 1.f; a.sy = scale3_host ? scale3_host[1] : 1.f; a.sz = scale3_host ? scale3_host[2] : 1.f;
    a.out_idx = out_idx; a.out_dist2 = out_dist2; a.soa = (float*)scratch;
    if (f == 1) {
        // Few waves: every wave repeats the reduction and the cross-wave step, and a SIMD issues for all of its waves in turn, so one
        // wave per SIMD (256 threads) with more points per thread is the cheapest way to cover a cloud while the registers last
        if (max_per_sample <= 256) fps_launch<1, false, 256>(a, B, fps_threads(max_per_sample), st);
        else if (max_per_sample <= 1024) fps_launch<4, false, 256>(a, B, 256, st);
        else if (max_per_sample <= 2048) fps_launch<8, false, 256>(a, B, 256, st);
        else if (max_per_sample <= 4096) fps_launch<16, false, 256>(a, B, 256, st);
        else if (max_per_sample <= 8192) fps_launch<32, false, 256>(a, B, 256, st);
        else fps_launch<FPS_RESIDENT_PER, false, 512>(a, B, 512, st);
    } else {
        const int nt = fps_threads(max_per_sample);
        if (max_per_sample <= 8 * FPS_MAX_THREADS) fps_launch<8, true, FPS_MAX_THREADS>(a, B, nt, st);
        else fps_launch<FPS_STREAM_PER, true, FPS_MAX_THREADS>(a, B, nt, st);
    }
    RALD_HIP(hipGetLastError());
    return 0;
}

}  // namespace rald
