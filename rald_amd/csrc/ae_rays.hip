// First-return beam casting through the decoder field: one launch marches R straight segments per sample through
// the occupancy logit of ae_decode.hip and returns, per segment, the first point at which the logit is > 0.
//
// A lane holds a ray where the streaming decoder holds a query: the sample point is computed in registers from the ray's origin and
// direction, the first-crossing state stays in registers, and HBM sees two vectors in and one range (+ logit, step, point) out per ray
// instead of 12 B in and 4 B out per evaluated point.  The context image, u, the variance factor and the basis are staged by the function
// that stages them for ae_decode_stream_kernel (stage_context; one __syncthreads(), before the loops); the evaluation of a 64-ray chunk at
// its 64 sample points is the same function that kernel calls (chunk_sums of ae_decode_core.h: features, var, scores, lazily rescaled
// online softmax, merge of the lane halves), so a logit
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

#include "ae_decode_core.h"
#include "common.h"
#include "kernels.h"

namespace rald {

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

// The logits of one 64-ray chunk at the points pt[qb] of lane (r, h): chunk_sums, as ae_decode_stream_kernel calls it between its
// query load and its store.  Both lane halves return the h = 0 lane's number (the one that kernel stores).
template <bool DIAG>
__device__ __forceinline__ void decode_chunk(const DecoderLds& c, const DecoderLane& ln, float eps, float inv_scale, float c0,
                                             const float (&pt)[2][3], float* logit) {
    float dsum[2], nsum[2];
    chunk_sums<DIAG>(c, ln, pt, eps, inv_scale, dsum, nsum);
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) logit[qb] = __shfl(nsum[qb] / dsum[qb] + c0, ln.r, 64);
}

template <bool DIAG, int NW>
__global__ __launch_bounds__(NW * 64) void ae_decode_rays_kernel(RayArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const DecoderLds c = decoder_lds(smem, a.M);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.y;
    stage_context<NW * 64>(c, a.ctx + (int64_t)b * a.ctx_stride, a.l_img, a.basis, tid);
    __syncthreads();
    const float inv_scale = c.u[c.M];
    const int r = lane & 31, h = lane >> 5;
    const DecoderLane ln = {r, h, h ? 0.25f : 0.0f};
    const int R = a.R, S = a.n_steps;
    const float* org = a.origins + (int64_t)b * a.ray_batch_stride;
    const float* dir = a.dirs + (int64_t)b * a.ray_batch_stride;
    const int64_t row0 = (int64_t)b * R;
    const int nchunks = (R + 63) / 64;

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
        float pt[2][3], logit[2];
        // ---- march: the first k with logit > 0
        float t_prev = 0.f;
        for (int k = 0; k <= S; ++k) {
            const float t = ray_param(k, S);
#pragma unroll
            for (int qb = 0; qb < 2; ++qb) { pt[qb][0] = ray_at(ox[qb], t, dx[qb]); pt[qb][1] = ray_at(oy[qb], t, dy[qb]); pt[qb][2] = ray_at(oz[qb], t, dz[qb]); }
            decode_chunk<DIAG>(c, ln, a.eps, inv_scale, a.c0, pt, logit);
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
                    pt[qb][0] = ray_at(ox[qb], te[qb], dx[qb]); pt[qb][1] = ray_at(oy[qb], te[qb], dy[qb]); pt[qb][2] = ray_at(oz[qb], te[qb], dz[qb]);
                }
                decode_chunk<DIAG>(c, ln, a.eps, inv_scale, a.c0, pt, logit);
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
        RALD_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)decoder_smem_bytes(DECODER_MAX_LATENTS)));
        attr_set = true;
    }
    hipLaunchKernelGGL(kern, dim3(decoder_grid_x(a.R, NW, B), (unsigned)B), dim3(NW * 64), decoder_smem_bytes(a.M), st, a);
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
