// The forward evaluation of the streaming query decoder (header of ae_decode.hip), once: ae_decode_stream_kernel (ae_decode.hip)
// and ae_decode_rays_kernel (ae_rays.hip) call all of it, so a point's logit has the same bits in both because it is the same
// function, for the same 32-query half and wave-mates.  ae_decode_grad_stream_kernel takes the staging, the feature phase and
// the merge of the lane halves from here and keeps its own text of the stages between (see there).
//
// A chunk is 64 points, two 32-point halves; chunk_sums is its whole evaluation, with the loop over the halves inside every stage
// (the compiler packs fp32 math across the two halves and the score pass shares its operand loads between them):
//
//     build_features -> variance tiles + closing of the std slots -> scores + online softmax -> merge_lane_halves
//
// Only build_features and merge_lane_halves are functions of their own; the two stages between are statements of chunk_sums, and
// its running sums never leave it: either as a function, or the sums handed out through references, moved the compiler's code off
// the parent's.
#pragma once
#include <cmath>

#include "common.h"

namespace rald {

typedef _Float16 f16;
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

constexpr int SLOT_ONE = 51;      // (s=3, h=0, j=3): 1.0 -> h0_hi ; j=4 (slot 52): 1.0 -> h0_lo
constexpr int SLOT_STD = 53;      // j=5,6,7 (slots 53,54,55): std_hi, std_lo, std_hi -> hb_hi, hb_hi, hb_lo
constexpr int SLOT_U = 63;        // column of the projection that carries u (its feature slot is always zero)

// byte offset of element (row, k) in a [rows][64] fp16 image with 128-byte rows, 16-byte chunks XOR-swizzled by the row
__host__ __device__ static inline int img_off(int row, int k) { return row * 128 + (((k >> 3) ^ (row & 7)) << 4) + (k & 7) * 2; }

// ---- host: LDS size and grid of a kernel that holds one sample's context per workgroup
static inline size_t decoder_smem_bytes(int M) { return (size_t)M * 128 + 8192 + (size_t)(M + 4 + 76) * 4; }
constexpr int DECODER_MAX_LATENTS = 1024;

// workgroups per sample for n points a sample (the longest segment, if ragged), NW waves a workgroup
static inline unsigned decoder_grid_x(int64_t n, int NW, int B) {
    const int64_t nchunks = (n + 63) / 64;
    int64_t per_sample = (nchunks + NW - 1) / NW;                  // workgroups that have at least one chunk per wave
    const int64_t cap = B >= 256 ? 1 : 256 / B;                    // about one workgroup per CU over the whole batch
    if (per_sample > cap) per_sample = cap;
    return (unsigned)per_sample;
}

// ---- device: the context in LDS
struct DecoderLds {
    unsigned char* h;             // M * 128: the image H~
    unsigned char* l;             // 8192: the variance factor
    float* u;                     // M + 4: u | inv_scale
    float* basis;                 // 72 (+ 4 pad): revolutions
    int M;
};
__device__ __forceinline__ DecoderLds decoder_lds(unsigned char* smem, int M) {
    DecoderLds s;
    s.h = smem;
    s.l = smem + (size_t)M * 128;
    s.u = reinterpret_cast<float*>(s.l + 8192);
    s.basis = s.u + M + 4;
    s.M = M;
    return s;
}

// Fills s from one sample's context (image | u | inv_scale), the variance factor and the basis; the caller's __syncthreads()
// follows.  s_brad: nullptr, or 72 floats that receive the basis in radians.
template <int NT>
__device__ __forceinline__ void stage_context(const DecoderLds& s, const unsigned char* ctx, const unsigned short* l_img,
                                              const float* basis, int tid, float* s_brad = nullptr) {
    const int M = s.M;
    const uint4* src = reinterpret_cast<const uint4*>(ctx);
    uint4* dst = reinterpret_cast<uint4*>(s.h);
    const int n16 = M * 8;                                   // image
    for (int i = tid; i < n16; i += NT) dst[i] = src[i];
    const uint4* su = src + n16;                             // u | inv_scale
    uint4* du = reinterpret_cast<uint4*>(s.u);
    for (int i = tid; i < M / 4 + 1; i += NT) du[i] = su[i];
    const uint4* sl = reinterpret_cast<const uint4*>(l_img);
    uint4* dl = reinterpret_cast<uint4*>(s.l);
    for (int i = tid; i < 512; i += NT) dl[i] = sl[i];
    if (tid < 72) {
        const float bv = basis[tid];
        s.basis[tid] = bv * 0.15915494309189535f;            // radians -> revolutions (v_sin_f32 takes revolutions)
        if (s_brad) s_brad[tid] = bv;
    }
}

// lane (r, h) of a wave: point r of a 32-point half, lane half h (header of ae_decode.hip)
struct DecoderLane {
    int r, h;                     // lane & 31, lane >> 5
    float quarter;                // h ? 0.25f : 0.0f: cos(t) = sin(t + 1/4 revolution)
};

// phase (in revolutions) of frequency e = 8 s + j of the point (x, y, z)
template <bool DIAG>
__device__ __forceinline__ float feature_phase(const float* s_basis, int s, int e, float x, float y, float z) {
    if (DIAG) return (s == 0 ? x : (s == 1 ? y : z)) * s_basis[24 * s + e];
    return fmaf(z, s_basis[48 + e], fmaf(y, s_basis[24 + e], x * s_basis[e]));
}

// ---- stage 1: the B operands of the points pt[qb] = (x, y, z) of this lane, the std slots still zero
template <bool DIAG, int NH>
__device__ __forceinline__ void build_features(const DecoderLds& c, const DecoderLane& ln, const float (&pt)[NH][3], f16x8 (&bq)[NH][4]) {
    const int h = ln.h;
#pragma unroll
    for (int qb = 0; qb < NH; ++qb) {
        const float x = pt[qb][0], y = pt[qb][1], z = pt[qb][2];
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            f16x8 f;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int e = 8 * s + j;
                float p = feature_phase<DIAG>(c.basis, s, e, x, y, z);
                p += ln.quarter;
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
}

// ---- stage 4, of one half: merge the two lane halves of a point -> its maximum, denominator and numerator; softmax . u = nsum / dsum
__device__ __forceinline__ void merge_lane_halves(float m, float den, float num, float& mm, float& dsum, float& nsum) {
    const float mo = __shfl_xor(m, 32, 64), dn = __shfl_xor(den, 32, 64), nn = __shfl_xor(num, 32, 64);
    mm = fmaxf(m, mo);
    const float wa = __builtin_amdgcn_exp2f(m - mm), wb = __builtin_amdgcn_exp2f(mo - mm);
    dsum = den * wa + dn * wb;
    nsum = num * wa + nn * wb;
}

// ---- one 64-point chunk at the points pt[qb] of this lane (the plain and the ray kernel's): features, LayerNorm statistics of the query
// embedding (which close the std slots of the operands and give rq = rstd_q / scale), score pass, merge -> dsum, nsum per half; the
// h = 0 lane's nsum / dsum + c0 is the point's logit
template <bool DIAG>
__device__ __forceinline__ void chunk_sums(const DecoderLds& c, const DecoderLane& ln, const float (&pt)[2][3], float eps, float inv_scale,
                                           float (&dsum)[2], float (&nsum)[2]) {
    const int r = ln.r, h = ln.h, M = c.M;
    f16x8 bq[2][4];
    float rq[2];                                              // rstd_q / scale
    build_features<DIAG, 2>(c, ln, pt, bq);
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
                const f16x8 la = *reinterpret_cast<const f16x8*>(c.l + row * 128 + (((2 * s + h) ^ (row & 7)) << 4));
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
        for (int s = 0; s < 4; ++s) fa[s] = *reinterpret_cast<const f16x8*>(c.h + row * 128 + (((2 * s + h) ^ (row & 7)) << 4));
        float4 uv[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) uv[g] = *reinterpret_cast<const float4*>(c.u + 32 * t + 8 * g + 4 * h);
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
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
        float mm;
        merge_lane_halves(m[qb], den[qb], num[qb], mm, dsum[qb], nsum[qb]);
    }
}

}  // namespace rald
