// First-return beam casting through the decoder field: one launch marches R straight segments per sample through
// the occupancy logit of ae_decode.hip and returns, per segment, the first point at which the logit is > 0.
//
// A lane holds a ray where the streaming decoder holds a query: the sample point is computed in registers from the ray's origin and
// direction, the first-crossing state stays in registers, and HBM sees two vectors in and one range (+ logit, step, point) out per ray
// instead of 12 B in and 4 B out per evaluated point.  The context image, u, the variance factor and the basis are staged exactly as
// ae_decode_stream_kernel stages them (one __syncthreads(), before the loops); the evaluation of a 64-ray chunk at its 64 sample points
// is that kernel's statement sequence - features, var, scores, lazily rescaled online softmax, merge of the lane halves - so a logit
// computed here is bit-identical to rald_ae_decode_queries on the same [R,3] points (the reproducibility unit is the 32-query half with
// its wave-wide __any; a chunk is rays chunk*64 + qb*32 + r, clamped to R-1, as that kernel clamps its queries).
//
// The rule.  Every float operation below is rounded on its own (fp contract(off)), as newton_step is.
//
//   Inputs.   origins, dirs: fp32, in normalised coordinates; the segment runs from o to o + d.  ray_batch_stride (in floats): 0 for one
//             [R,3] table shared by all samples, or 3*R for [B,R,3].  n_steps S in [1, 65535].  n_refine in [0, 30].
//   March.    For k = 0..S in order: t_k = (float)k / (float)S (correctly rounded division) and q_c = o_c + t_k * d_c (multiply, then
//             add).  The ray HITS at the first k whose logit is > 0.  A NaN logit never hits.  On a hit, record k_hit = k, hi = t_k,
//             lo = t_{k-1} (for k = 0: lo = hi = 0) and l_hit = logit.  A lane that has hit keeps computing with its wave, and its later
//             logits are ignored.  A wave leaves the march when all 64 lanes have hit, or after k = S.  This is the only early exit.  It is
//             wave-uniform and there is no barrier in the loop.
//   Refine.   n_refine bisection steps with all 64 lanes taking part: mid = 0.5f * (lo + hi), evaluate at o + mid*d.  Only rays with
//             k_hit >= 1 update their state.  If logit > 0: hi = mid, l_hit = logit.  Otherwise lo = mid.  Other rays evaluate at their
//             own hi (hit at 0) or at t = 1 (miss) and change nothing.  A wave none of whose rays has k_hit >= 1 skips refinement.
//   Outputs.  Written by the h == 0 lanes for rays < R only.  out_t [B,R]: hi, or -1 for a miss.  out_logit [B,R]: l_hit, or NaN for a
//             miss.  out_step int32 [B,R]: k_hit, or -1.  out_points [B,R,3], optional: o + hi*d by the same rounding rule, or NaN for a
//             miss.  The returned point is always one at which this kernel saw logit > 0.  That is the reference's own decision rule
//             (output > 0).
//
// No atomics, no inline assembly, no scratch.  LDS is the plain kernel's (num_latents up to 1024).
#include <cmath>

#include "common.h"
#include "kernels.h"

namespace rald {

typedef _Float16 f16;
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

struct RayArgs {
    const unsigned char* ctx; int64_t ctx_stride;     // per sample: image | u | inv_scale
    const unsigned short* l_img;                      // [64][64] fp16 image of the var factor
    const float* basis;                               // [3][24]
    const float* origins;                             // [R][3] or [B][R][3]
    const float* dirs;
    int64_t ray_batch_stride;                         // 0 or 3 * R floats
    float* out_t;                                     // [B][R]
    float* out_logit;                                 // [B][R]
    int* out_step;                                    // [B][R]
    float* out_points;                                // nullptr or [B][R][3]
    int R, M, n_steps, n_refine;
    float c0, eps;
};

// t_k of the march and the sample point o + t d: one rounding per operation
__device__ __forceinline__ float ray_param(int k, int S) {
#pragma clang fp contract(off)
    return (float)k / (float)S;
}
__device__ __forceinline__ float ray_at(float o, float t, float d) {
#pragma clang fp contract(off)
    const float m = t * d;
    return o + m;
}
__device__ __forceinline__ float ray_mid(float lo, float hi) {
#pragma clang fp contract(off)
    const float s = lo + hi;
    return 0.5f * s;
}

// The logits of one 64-query chunk at the points (px, py, pz)[qb] of lane (r, h): ae_decode_stream_kernel's statements between its query
// load and its store.  Both lane halves return the h = 0 lane's number (the one that kernel stores).
template <bool DIAG>
__device__ __forceinline__ void decode_chunk(const unsigned char* s_h, const unsigned char* s_l, const float* s_u, const float* s_basis, int M,
                                             float inv_scale, float eps, float c0, int r, int h, float quarter, const float* px,
                                             const float* py, const float* pz, float* logit) {
    f16x8 bq[2][4];
    float rq[2];                                              // rstd_q / scale
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
        const float x = px[qb], y = py[qb], z = pz[qb];
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            f16x8 f;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int e = 8 * s + j;
                float p;
                if (DIAG) p = (s == 0 ? x : (s == 1 ? y : z)) * s_basis[24 * s + e];
                else p = fmaf(z, s_basis[48 + e], fmaf(y, s_basis[24 + e], x * s_basis[e]));
                p += quarter;
                p = __builtin_amdgcn_fractf(p);
                f[j] = (f16)__builtin_amdgcn_sinf(p);
            }
            bq[qb][s] = f;
        }
        f16x8 f;
        f[0] = (f16)(h ? 0.f : x); f[1] = (f16)(h ? 0.f : y); f[2] = (f16)(h ? 0.f : z);
        f[3] = (f16)(h ? 0.f : 1.f); f[4] = f[3];
        f[5] = (f16)0.f; f[6] = (f16)0.f; f[7] = (f16)0.f;
        bq[qb][3] = f;
    }
    // ---- LayerNorm statistics of the query embedding: var_q = |L.f~|^2 (two 32-row tiles x 4 k-steps)
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
        float ss = 0.f;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            f32x16 acc;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = 0.f;
            const int row = 32 * t + r;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const f16x8 la = *reinterpret_cast<const f16x8*>(s_l + row * 128 + (((2 * s + h) ^ (row & 7)) << 4));
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(la, bq[qb][s], acc, 0, 0, 0);
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) ss = fmaf(acc[i], acc[i], ss);
        }
        ss += __shfl_xor(ss, 32, 64);
        const float var = ss + eps;
        const float rstd = rsqrtf(var);
        const float sd = var * rstd;                           // sqrt(var + eps)
        const f16 sd_hi = (f16)sd;
        const f16 sd_lo = (f16)(sd - (float)sd_hi);
        f16x8 f = bq[qb][3];
        f[5] = h ? (f16)0.f : sd_hi; f[6] = h ? (f16)0.f : sd_lo; f[7] = h ? (f16)0.f : sd_hi;
        bq[qb][3] = f;
        rq[qb] = rstd * inv_scale;
    }
    // ---- scores + online softmax over the latents
    float m[2] = {-INFINITY, -INFINITY}, den[2] = {0.f, 0.f}, num[2] = {0.f, 0.f};
    const int ntile = M >> 5;
    for (int t = 0; t < ntile; ++t) {
        const int row = 32 * t + r;
        f16x8 fa[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) fa[s] = *reinterpret_cast<const f16x8*>(s_h + row * 128 + (((2 * s + h) ^ (row & 7)) << 4));
        float4 uv[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) uv[g] = *reinterpret_cast<const float4*>(s_u + 32 * t + 8 * g + 4 * h);
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
            f32x16 acc;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
            for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[s], bq[qb][s], acc, 0, 0, 0);
            float tm = fmaxf(fmaxf(acc[0], acc[1]), fmaxf(acc[2], acc[3]));
#pragma unroll
            for (int i = 4; i < 16; i += 4) tm = fmaxf(tm, fmaxf(fmaxf(acc[i], acc[i + 1]), fmaxf(acc[i + 2], acc[i + 3])));
            const float vm = tm * rq[qb];
            if (__any(vm > m[qb] + 8.0f)) {                    // lazy running maximum: p stays <= 2^8
                const float mn = fmaxf(m[qb], vm);
                const float alpha = __builtin_amdgcn_exp2f(m[qb] - mn);
                den[qb] *= alpha; num[qb] *= alpha;
                m[qb] = mn;
            }
            const float nm = -m[qb];
            float d0 = 0.f, d1 = 0.f, n0 = 0.f, n1 = 0.f;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float p0 = __builtin_amdgcn_exp2f(fmaf(acc[4 * g + 0], rq[qb], nm));
                const float p1 = __builtin_amdgcn_exp2f(fmaf(acc[4 * g + 1], rq[qb], nm));
                const float p2 = __builtin_amdgcn_exp2f(fmaf(acc[4 * g + 2], rq[qb], nm));
                const float p3 = __builtin_amdgcn_exp2f(fmaf(acc[4 * g + 3], rq[qb], nm));
                d0 += p0; d1 += p1; d0 += p2; d1 += p3;
                n0 = fmaf(p0, uv[g].x, n0); n1 = fmaf(p1, uv[g].y, n1); n0 = fmaf(p2, uv[g].z, n0); n1 = fmaf(p3, uv[g].w, n1);
            }
            den[qb] += d0 + d1;
            num[qb] += n0 + n1;
        }
    }
    // ---- merge the two lane halves of each query; both halves go on with the h = 0 lane's number (the one that is stored)
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
        const float mo = __shfl_xor(m[qb], 32, 64), dn = __shfl_xor(den[qb], 32, 64), nn = __shfl_xor(num[qb], 32, 64);
        const float mm = fmaxf(m[qb], mo);
        const float wa = __builtin_amdgcn_exp2f(m[qb] - mm), wb = __builtin_amdgcn_exp2f(mo - mm);
        const float dsum = den[qb] * wa + dn * wb, nsum = num[qb] * wa + nn * wb;
        logit[qb] = __shfl(nsum / dsum + c0, r, 64);
    }
}

template <bool DIAG, int NW>
__global__ __launch_bounds__(NW * 64) void ae_decode_rays_kernel(RayArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int M = a.M;
    unsigned char* s_h = smem;                                   // M * 128
    unsigned char* s_l = smem + (size_t)M * 128;                 // 8192
    float* s_u = reinterpret_cast<float*>(s_l + 8192);           // M + 4
    float* s_basis = s_u + M + 4;                                // 72 (+ pad)
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.y;
    {
        const uint4* src = reinterpret_cast<const uint4*>(a.ctx + (int64_t)b * a.ctx_stride);
        uint4* dst = reinterpret_cast<uint4*>(s_h);
        const int n16 = M * 8;                                   // image
        for (int i = tid; i < n16; i += NW * 64) dst[i] = src[i];
        const uint4* su = src + n16;                             // u | inv_scale
        uint4* du = reinterpret_cast<uint4*>(s_u);
        for (int i = tid; i < M / 4 + 1; i += NW * 64) du[i] = su[i];
        const uint4* sl = reinterpret_cast<const uint4*>(a.l_img);
        uint4* dl = reinterpret_cast<uint4*>(s_l);
        for (int i = tid; i < 512; i += NW * 64) dl[i] = sl[i];
        if (tid < 72) s_basis[tid] = a.basis[tid] * 0.15915494309189535f;      // radians -> revolutions (v_sin_f32 takes revolutions)
    }
    __syncthreads();
    const float inv_scale = s_u[M];
    const int r = lane & 31, h = lane >> 5;
    const int R = a.R, S = a.n_steps;
    const float* org = a.origins + (int64_t)b * a.ray_batch_stride;
    const float* dir = a.dirs + (int64_t)b * a.ray_batch_stride;
    const int64_t row0 = (int64_t)b * R;
    const int nchunks = (R + 63) / 64;
    const float quarter = h ? 0.25f : 0.0f;                       // cos(t) = sin(t + 1/4 revolution)

    for (int chunk = blockIdx.x * NW + wave; chunk < nchunks; chunk += gridDim.x * NW) {
        float ox[2], oy[2], oz[2], dx[2], dy[2], dz[2];
        float lo[2] = {0.f, 0.f}, hi[2] = {0.f, 0.f}, lh[2];
        int kh[2] = {-1, -1};
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
            int q = chunk * 64 + qb * 32 + r;
            q = q < R ? q : R - 1;
            ox[qb] = org[q * 3 + 0]; oy[qb] = org[q * 3 + 1]; oz[qb] = org[q * 3 + 2];
            dx[qb] = dir[q * 3 + 0]; dy[qb] = dir[q * 3 + 1]; dz[qb] = dir[q * 3 + 2];
            lh[qb] = __builtin_nanf("");
        }
        float px[2], py[2], pz[2], logit[2];
        // ---- march: the first k with logit > 0
        float t_prev = 0.f;
        for (int k = 0; k <= S; ++k) {
            const float t = ray_param(k, S);
#pragma unroll
            for (int qb = 0; qb < 2; ++qb) { px[qb] = ray_at(ox[qb], t, dx[qb]); py[qb] = ray_at(oy[qb], t, dy[qb]); pz[qb] = ray_at(oz[qb], t, dz[qb]); }
            decode_chunk<DIAG>(s_h, s_l, s_u, s_basis, M, inv_scale, a.eps, a.c0, r, h, quarter, px, py, pz, logit);
#pragma unroll
            for (int qb = 0; qb < 2; ++qb)
                if (kh[qb] < 0 && logit[qb] > 0.f) { kh[qb] = k; hi[qb] = t; lo[qb] = t_prev; lh[qb] = logit[qb]; }
            t_prev = t;
            if (__all(kh[0] >= 0 && kh[1] >= 0)) break;          // wave-uniform: every ray of the chunk has its first return
        }
        // ---- refine: bisection of [lo, hi] (logit(lo) <= 0 < logit(hi)) for the rays that crossed between two samples
        if (a.n_refine > 0 && __any(kh[0] >= 1 || kh[1] >= 1)) {
            for (int it = 0; it < a.n_refine; ++it) {
                float te[2];
#pragma unroll
                for (int qb = 0; qb < 2; ++qb) {
                    te[qb] = kh[qb] >= 1 ? ray_mid(lo[qb], hi[qb]) : (kh[qb] == 0 ? hi[qb] : 1.0f);
                    px[qb] = ray_at(ox[qb], te[qb], dx[qb]); py[qb] = ray_at(oy[qb], te[qb], dy[qb]); pz[qb] = ray_at(oz[qb], te[qb], dz[qb]);
                }
                decode_chunk<DIAG>(s_h, s_l, s_u, s_basis, M, inv_scale, a.eps, a.c0, r, h, quarter, px, py, pz, logit);
#pragma unroll
                for (int qb = 0; qb < 2; ++qb)
                    if (kh[qb] >= 1) {
                        if (logit[qb] > 0.f) { hi[qb] = te[qb]; lh[qb] = logit[qb]; }
                        else lo[qb] = te[qb];
                    }
            }
        }
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
            const int q = chunk * 64 + qb * 32 + r;
            if (h == 0 && q < R) {
                const bool hit = kh[qb] >= 0;
                const float nan = __builtin_nanf("");
                a.out_t[row0 + q] = hit ? hi[qb] : -1.f;
                a.out_logit[row0 + q] = lh[qb];
                a.out_step[row0 + q] = kh[qb];
                if (a.out_points) {
                    float* p = a.out_points + (row0 + q) * 3;
                    p[0] = hit ? ray_at(ox[qb], hi[qb], dx[qb]) : nan;
                    p[1] = hit ? ray_at(oy[qb], hi[qb], dy[qb]) : nan;
                    p[2] = hit ? ray_at(oz[qb], hi[qb], dz[qb]) : nan;
                }
            }
        }
    }
}

template <bool DIAG, int NW>
static int launch_rays(const RayArgs& a, int B, hipStream_t st) {
    auto kern = ae_decode_rays_kernel<DIAG, NW>;
    static bool attr_set = false;
    if (!attr_set) {
        RALD_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 1024 * 128 + 8192 + (1024 + 4 + 76) * 4));
        attr_set = true;
    }
    const int nchunks = (a.R + 63) / 64;
    int per_sample = (nchunks + NW - 1) / NW;                      // workgroups that have at least one chunk per wave
    const int cap = B >= 256 ? 1 : 256 / B;                        // about one workgroup per CU over the whole batch
    if (per_sample > cap) per_sample = cap;
    const size_t smem = (size_t)a.M * 128 + 8192 + (size_t)(a.M + 4 + 76) * 4;
    hipLaunchKernelGGL(kern, dim3((unsigned)per_sample, (unsigned)B), dim3(NW * 64), smem, st, a);
    RALD_HIP(hipGetLastError());
    return 0;
}

// A chunk costs n_steps + 1 + n_refine decodes of 64 points, so a scan of a few thousand chunks is a long launch with few waves: the
// workgroup is as narrow as it takes to put a workgroup on every CU (4 waves while batch * chunks <= 4 * 256, else 8).  The plain
// decoder's 12 waves would leave 168 registers a wave, and the ray state on top of the decoder's does not fit them (the compiler
// spills 74 to 191 registers to scratch there); 8 waves take 222 (block-diagonal basis) and 256 (general), no scratch.  A chunk's
// results do not depend on the choice.
int ae_cast_rays(const void* ctx, const unsigned short* l_img, const float* origins, const float* dirs, int64_t ray_batch_stride,
                 const float* basis, int basis_diag, int B, int R, int M, int n_steps, int n_refine, float c0, float* out_t, float* out_logit,
                 int* out_step, float* out_points, hipStream_t st) {
    RALD_CHECK(M % 32 == 0 && M >= 32 && M <= 1024, "ae_cast_rays: num_latents must be a multiple of 32 in [32,1024]");
    RALD_CHECK(B >= 1 && B <= 65535 && R >= 1 && R <= (1 << 28), "ae_cast_rays: bad batch / ray count");
    RALD_CHECK(ray_batch_stride == 0 || ray_batch_stride == 3 * (int64_t)R, "ae_cast_rays: ray_batch_stride must be 0 or 3 * n_rays");
    RALD_CHECK(n_steps >= 1 && n_steps <= 65535, "ae_cast_rays: n_steps must be in [1,65535]");
    RALD_CHECK(n_refine >= 0 && n_refine <= 30, "ae_cast_rays: n_refine must be in [0,30]");
    RALD_CHECK(ctx && l_img && origins && dirs && basis && out_t && out_logit && out_step, "ae_cast_rays: null pointer");
    RayArgs a;
    a.ctx = (const unsigned char*)ctx; a.ctx_stride = ae_ctx_stride(M); a.l_img = l_img; a.basis = basis; a.origins = origins; a.dirs = dirs;
    a.ray_batch_stride = ray_batch_stride; a.out_t = out_t; a.out_logit = out_logit; a.out_step = out_step; a.out_points = out_points;
    a.R = R; a.M = M; a.n_steps = n_steps; a.n_refine = n_refine; a.c0 = c0; a.eps = 1e-5f;
    const int64_t work = (int64_t)B * ((R + 63) / 64);
    if (work <= 4 * 256) return basis_diag ? launch_rays<true, 4>(a, B, st) : launch_rays<false, 4>(a, B, st);
    return basis_diag ? launch_rays<true, 8>(a, B, st) : launch_rays<false, 8>(a, B, st);
}

}  // namespace rald
