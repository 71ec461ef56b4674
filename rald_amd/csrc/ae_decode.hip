// Streaming query decoder of the set-latent autoencoder (KLAutoEncoder.decode, model/models_ae.py:417-424):
//
//     queries [Q,3] -> PointEmbed -> PreNorm(LN q, LN ctx) 1-head d=dim cross-attention over the M latents
//                   -> to_out -> to_outputs -> one logit per query
//
// ONE kernel, 12 bytes in and 4 bytes out per query; nothing else touches HBM.  What makes that possible is that every
// step between the 51 Fourier features of a query and its attention scores is linear except the query LayerNorm, whose
// statistics are themselves a quadratic form of the features:
//
//     qe      = feat.Wpe^T + b_pe                          (PointEmbed :128-138)
//     qe - mu = feat.Wc^T + b_c                            Wc, b_c = Wpe, b_pe centred over the d outputs (mean is linear)
//     var     = |L.[feat;1]|^2                             L^T.L = [Wc|b_c]^T.[Wc|b_c] / d     (52 x 52, weights only)
//     S[q,l]  = rstd_q * (feat.H_l + h0_l) + hb_l          H = LN_ctx(x).T2, h0 = LN_ctx(x).t20, hb = LN_ctx(x).t2b
//     logit   = softmax_l(S[q,:]) . u + c0                 u = LN_ctx(x).w_fold   (value path folded, see ae.hip)
//
// with T2 = Wk^T.(scale.Wq.diag(g).Wc) etc. computed once per weight load on the host in double (Ae::finalize).  Per sample
// the decoder context is therefore H [M x 51] + three vectors instead of K,V [M x d]: 64 KiB in LDS for M = 512, resident
// for the whole launch, and the per-query score GEMM has K = 64 instead of K = d (+ the d x 64 embedding GEMM + LayerNorm
// that it replaces).  Exact in real arithmetic; numerically the 51-term sums run on v_mfma_f32_32x32x16_f16 (fp16 operands:
// 11-bit mantissas; features are in [-1,1], H carries one power-of-two scale per sample) with fp32 accumulation.
//
// Operand layout (k = slot 0..63 of the K = 64 contraction; MFMA 32x32x16 B-operand: lane (q = lane&31, h = lane>>5) holds
// k = 16s + 8h + j of k-step s): the h = 0 lanes hold sin(p_e) (e = 8s + j < 24), x, y, z, 1, 1, std, std_lo, std; the h = 1
// lanes hold cos(p_e) and zeros - every lane computes its own 32 slots from its query's 3 coordinates in registers, no LDS.
// The two 1-slots multiply h0 split in fp16 hi + lo, the three std-slots (std_q = sqrt(var_q + eps) in hi / lo) multiply
// hb (hi, hi, lo), so that rstd_q * acc = S exactly as above with ~22-bit bias terms.
//
// S^T = H~.f~^T puts the latent index on the accumulator registers and the query on the lane: the softmax over the M
// latents is lane-local (online, lazily rescaled), u is read from LDS as a broadcast.  Bound: v_exp_f32 + the 3 VALU per
// score next to 4 MFMA per 32x32 score tile - not HBM (16 B/query) and not the 2.15 MFLOP/query the reference executes.
//
// A query's logit is reproducible for the same 64-query chunk (any batch size, any grid), but not bit for bit in other company: the
// running maximum moves when ANY lane of the wave asks for it (__any), so the steps at which a query's sums are rescaled depend on
// its wave-mates; the last bits follow (measured: 1e-6 on logits of a few units).
//
// Domain: scores (log2 units) below 2^29 in size.  vm = tm * rq is a rounded product while the exponents fmaf(acc, rq, -m) use the exact
// one, so a score can sit half an ulp of itself above the maximum it was compared with: harmless up to 2^29 (8 + 64 < 127), but from
// 2^31 on that half ulp alone is 2^7 and exp2 returns inf (logit NaN).  No fp32 softmax means anything there (the reference's own scores
// carry the same ulp of 2^9); real contexts have scores of 10 .. 100.
#include <cmath>
#include <vector>

#include "ae_decode_core.h"
#include "common.h"
#include "kernels.h"

namespace rald {

// slot of reference feature f (0..23 sin, 24..47 cos, 48..50 xyz), see the header
static inline int slot_of_feature(int f) {
    if (f < 24) return 16 * (f >> 3) + (f & 7);
    if (f < 48) { const int e = f - 24; return 16 * (e >> 3) + 8 + (e & 7); }
    return 48 + (f - 48);
}

// ---------------------------------------------------------------------------------------------------------------
// host: weight-only tables (double precision)
// ---------------------------------------------------------------------------------------------------------------
// t2aug [d][64] fp32 in slot order (cols of features: H; SLOT_ONE: h0; SLOT_STD: hb; SLOT_U: u) and the var factor L
// as a [64][64] fp16 image.  Wq [d][d] (to_q), Wk [d][d] (first half of to_kv), ng / nb [d] (query LayerNorm),
// Wpe [d][51], bpe [d], wfold [d] (value path, ae.hip).
int ae_decode_tables(int d, const float* Wq, const float* Wk, const float* ng, const float* nb, const float* Wpe, const float* bpe,
                     const float* wfold, std::vector<float>& t2aug, std::vector<unsigned short>& l_img) {
    const int F = 51, FA = 52;
    std::vector<double> Wc((size_t)d * FA);                 // [c][f], column 51 = centred bias
    for (int f = 0; f < FA; ++f) {
        double mu = 0.0;
        for (int c = 0; c < d; ++c) mu += f < F ? (double)Wpe[(size_t)c * F + f] : (double)bpe[c];
        mu /= d;
        for (int c = 0; c < d; ++c) Wc[(size_t)c * FA + f] = (f < F ? (double)Wpe[(size_t)c * F + f] : (double)bpe[c]) - mu;
    }
    // ---- var factor: modified Gram-Schmidt on [Wc|bc] / sqrt(d): R [52][52] upper triangular, R^T.R = Gram matrix
    std::vector<double> Qm((size_t)d * FA), R((size_t)FA * FA, 0.0);
    const double inv_sd = 1.0 / std::sqrt((double)d);
    for (int j = 0; j < FA; ++j) {
        std::vector<double> v(d);
        double n0 = 0.0;
        for (int c = 0; c < d; ++c) { v[c] = Wc[(size_t)c * FA + j] * inv_sd; n0 += v[c] * v[c]; }
        for (int i = 0; i < j; ++i) {
            double r = 0.0;
            for (int c = 0; c < d; ++c) r += Qm[(size_t)c * FA + i] * v[c];
            R[(size_t)i * FA + j] = r;
            for (int c = 0; c < d; ++c) v[c] -= r * Qm[(size_t)c * FA + i];
        }
        double nn = 0.0;
        for (int c = 0; c < d; ++c) nn += v[c] * v[c];
        const double rjj = (nn > 1e-24 * (n0 > 0 ? n0 : 1.0)) ? std::sqrt(nn) : 0.0;     // dependent column: contributes nothing new
        R[(size_t)j * FA + j] = rjj;
        for (int c = 0; c < d; ++c) Qm[(size_t)c * FA + j] = rjj > 0 ? v[c] / rjj : 0.0;
    }
    l_img.assign(64 * 64, 0);
    for (int i = 0; i < FA; ++i)
        for (int f = i; f < FA; ++f) {
            const int k = f < F ? slot_of_feature(f) : SLOT_ONE;
            const f16 hv = (f16)(float)R[(size_t)i * FA + f];
            unsigned short bits;
            __builtin_memcpy(&bits, &hv, 2);
            l_img[img_off(i, k) / 2] = bits;
        }
    // ---- T [j][53]: scale*log2e * Wq . diag(g) . [Wc | bc] and scale*log2e * Wq . nb
    const int NC = 53;
    const double s = 1.4426950408889634 / std::sqrt((double)d);
    std::vector<double> T((size_t)d * NC, 0.0);
    for (int j = 0; j < d; ++j) {
        double* tj = &T[(size_t)j * NC];
        for (int c = 0; c < d; ++c) {
            const double wq = (double)Wq[(size_t)j * d + c];
            const double wg = wq * (double)ng[c] * s;
            const double* wc = &Wc[(size_t)c * FA];
            for (int f = 0; f < FA; ++f) tj[f] += wg * wc[f];
            tj[52] += wq * (double)nb[c] * s;
        }
    }
    // ---- T2 [c'][53] = Wk^T . T, scattered into slot order
    t2aug.assign((size_t)d * 64, 0.f);
    std::vector<double> acc(NC);
    for (int cp = 0; cp < d; ++cp) {
        for (int f = 0; f < NC; ++f) acc[f] = 0.0;
        for (int j = 0; j < d; ++j) {
            const double wk = (double)Wk[(size_t)j * d + cp];
            const double* tj = &T[(size_t)j * NC];
            for (int f = 0; f < NC; ++f) acc[f] += wk * tj[f];
        }
        float* o = &t2aug[(size_t)cp * 64];
        for (int f = 0; f < F; ++f) o[slot_of_feature(f)] = (float)acc[f];
        o[SLOT_ONE] = (float)acc[51];
        o[SLOT_STD] = (float)acc[52];
        o[SLOT_U] = wfold[cp];
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// per-sample context: Y = LN_ctx(x) . t2aug  (fp32), then the fp16 LDS image + u + scale
// ---------------------------------------------------------------------------------------------------------------
template <int VPL>     // d = 64 * VPL
__global__ __launch_bounds__(256) void ae_ctx_project_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, const float* __restrict__ t2,
                                                             float* __restrict__ Y, unsigned* __restrict__ absmax, int rows, int M) {
    constexpr int D = 64 * VPL;
    __shared__ float xs[4][D];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int row = blockIdx.x * 4 + w;
    {
        const int r = row < rows ? row : rows - 1;
        float v[VPL];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < VPL; ++i) { v[i] = x[(int64_t)r * D + lane + 64 * i]; s += v[i]; }
        const float mean = wave_sum(s) * (1.0f / D);
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < VPL; ++i) { const float dv = v[i] - mean; q += dv * dv; }
        const float rstd = rsqrtf(wave_sum(q) * (1.0f / D) + 1e-5f);
#pragma unroll
        for (int i = 0; i < VPL; ++i) {
            const int c = lane + 64 * i;
            xs[w][c] = (v[i] - mean) * rstd * gamma[c] + beta[c];
        }
    }
    __syncthreads();
    __shared__ float red[4][4][64];
    const float y = project4_rows<D>(xs, t2, red, lane, w);
    if (row < rows) Y[(int64_t)row * 64 + lane] = y;
    // largest |coefficient| of the sample (the fp16 image's scale): max is order-independent, so the atomic keeps the result
    // reproducible; non-negative floats compare like their bit patterns
    float mx = (row < rows && (lane <= SLOT_ONE || lane == SLOT_STD)) ? fabsf(y) : 0.f;
    mx = wave_max(mx);
    if (lane == 0 && row < rows) atomicMax(absmax + row / M, __float_as_uint(mx));
}

// ctx = [ H~ image: M x 128 B | u: M floats | inv_scale, 3 pad floats ] per sample; 4 latent rows per workgroup
__global__ __launch_bounds__(256) void ae_ctx_pack_kernel(const float* __restrict__ Y, const unsigned* __restrict__ absmax,
                                                          unsigned char* __restrict__ ctx, int M, int64_t ctx_stride) {
    const int b = blockIdx.y;
    const int l = blockIdx.x * 4 + (threadIdx.x >> 6), k = threadIdx.x & 63;
    const float* y = Y + (int64_t)b * M * 64;
    unsigned char* out = ctx + (int64_t)b * ctx_stride;
    const float mx = __uint_as_float(absmax[b]);
    // power-of-two scale that puts the largest entry into [2^13, 2^14): fp16 keeps 11 bits for everything within 2^-27 of it.
    // The exponent stops at 126: a largest entry below 2^-113 would ask for a scale (and 0 * scale = NaN) beyond fp32, and 1 / scale
    // stays a normal number; such a context sits lower in the fp16 range instead (2^-120 -> 2^6, still 11 bits down to 2^-20 of it)
    float scale = 1.0f;
    if (mx > 0.f && mx < 3.0e38f) scale = exp2f((float)min(13 - ilogbf(mx), 126));
    float v = 0.f;
    if (k < SLOT_ONE) v = y[l * 64 + k] * scale;
    else if (k == SLOT_ONE || k == SLOT_ONE + 1) {
        const float t = y[l * 64 + SLOT_ONE] * scale;
        const f16 hi = (f16)t;
        v = k == SLOT_ONE ? (float)hi : t - (float)hi;
    } else if (k >= SLOT_STD && k <= SLOT_STD + 2) {
        const float t = y[l * 64 + SLOT_STD] * scale;
        const f16 hi = (f16)t;
        v = k == SLOT_STD + 2 ? t - (float)hi : (float)hi;
    }
    *reinterpret_cast<f16*>(out + img_off(l, k)) = (f16)v;
    float* u = reinterpret_cast<float*>(out + (int64_t)M * 128);
    if (k == SLOT_U) u[l] = y[l * 64 + SLOT_U];
    if (l == 0 && k == 0) u[M] = 1.0f / scale;
}

int ae_ctx_build(const float* x, const float* gamma, const float* beta, const float* t2aug, float* Yscratch, void* ctx, int B, int M, int d,
                 hipStream_t st) {
    RALD_CHECK(d == 256 || d == 512, "ae_ctx_build: dim must be 256 or 512");
    RALD_CHECK(M % 4 == 0, "ae_ctx_build: num_latents must be a multiple of 4");
    const int rows = B * M;
    unsigned* absmax = reinterpret_cast<unsigned*>(Yscratch + (int64_t)rows * 64);      // B words behind the projection (scratch is sized for them)
    RALD_HIP(hipMemsetAsync(absmax, 0, (size_t)B * 4, st));
    if (d == 256) hipLaunchKernelGGL((ae_ctx_project_kernel<4>), dim3(cdiv(rows, 4)), dim3(256), 0, st, x, gamma, beta, t2aug, Yscratch, absmax, rows, M);
    else hipLaunchKernelGGL((ae_ctx_project_kernel<8>), dim3(cdiv(rows, 4)), dim3(256), 0, st, x, gamma, beta, t2aug, Yscratch, absmax, rows, M);
    RALD_HIP(hipGetLastError());
    hipLaunchKernelGGL(ae_ctx_pack_kernel, dim3(M / 4, B), dim3(256), 0, st, Yscratch, absmax, (unsigned char*)ctx, M, ae_ctx_stride(M));
    RALD_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// the streaming kernel
// ---------------------------------------------------------------------------------------------------------------
struct DecodeArgs {
    const unsigned char* ctx; int64_t ctx_stride;     // per sample: image | u | inv_scale
    const unsigned short* l_img;                      // [64][64] fp16 image of the var factor
    const float* queries;                             // [B][Q][3]
    float* out;                                       // [B][Q]
    const float* basis;                               // [3][24]
    int64_t Q;
    int M;
    float c0, eps;
};

// RAGGED = false: sample b owns queries [b*Q, (b+1)*Q).  RAGGED = true: rows offsets[b] .. offsets[b+1] - 1 of one concatenated array
// (a.Q unused), chunked from the segment's own first row, so a query has the wave-mates it has in a dense launch on that segment alone.
template <bool DIAG, int NW, bool RAGGED>
__global__ __launch_bounds__(NW * 64) void ae_decode_stream_kernel(DecodeArgs a, const int64_t* __restrict__ offsets) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const DecoderLds c = decoder_lds(smem, a.M);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.y;
    int64_t first = 0, seg = 0;
    if constexpr (RAGGED) {
        first = offsets[b];
        seg = offsets[b + 1] - first;
        // an empty or short segment leaves this workgroup without a chunk (the grid is sized by the longest one): it is done before it
        // loads the context; a descending or negative pair of offsets decodes nothing
        if (first < 0 || seg <= 0 || (int64_t)blockIdx.x * NW * 64 >= seg) return;
    }
    stage_context<NW * 64>(c, a.ctx + (int64_t)b * a.ctx_stride, a.l_img, a.basis, tid);
    __syncthreads();
    const float inv_scale = c.u[c.M];
    const int r = lane & 31, h = lane >> 5;
    const DecoderLane ln = {r, h, h ? 0.25f : 0.0f};
    const int64_t Q = RAGGED ? seg : a.Q;
    const float* qin = a.queries + (RAGGED ? first : (int64_t)b * a.Q) * 3;
    float* qout = a.out + (RAGGED ? first : (int64_t)b * a.Q);
    const int64_t nchunks = (Q + 63) / 64;

    for (int64_t chunk = (int64_t)blockIdx.x * NW + wave; chunk < nchunks; chunk += (int64_t)gridDim.x * NW) {
        float pt[2][3];
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
            int64_t q = chunk * 64 + qb * 32 + r;
            q = q < Q ? q : Q - 1;
            pt[qb][0] = qin[q * 3 + 0]; pt[qb][1] = qin[q * 3 + 1]; pt[qb][2] = qin[q * 3 + 2];
        }
        float dsum[2], nsum[2];
        chunk_sums<DIAG>(c, ln, pt, a.eps, inv_scale, dsum, nsum);
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
            const int64_t q = chunk * 64 + qb * 32 + r;
            if (h == 0 && q < Q) qout[q] = nsum[qb] / dsum[qb] + a.c0;
        }
    }
}

// longest = the queries of one sample (dense) or a host upper bound of the longest segment (ragged): it sizes the grid
template <bool DIAG, bool RAGGED>
static int launch_decode(const DecodeArgs& a, const int64_t* offsets, int B, int64_t longest, hipStream_t st) {
    constexpr int NW = 12;                                         // waves per workgroup (the measured best of 8, 12 and 16)
    auto kern = ae_decode_stream_kernel<DIAG, NW, RAGGED>;
    static bool attr_set = false;
    if (!attr_set) {
        RALD_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)decoder_smem_bytes(DECODER_MAX_LATENTS)));
        attr_set = true;
    }
    hipLaunchKernelGGL(kern, dim3(decoder_grid_x(longest, NW, B), (unsigned)B), dim3(NW * 64), decoder_smem_bytes(a.M), st, a, offsets);
    RALD_HIP(hipGetLastError());
    return 0;
}

// one workgroup per CU holds the sample's image in LDS
int ae_decode_stream(const void* ctx, const unsigned short* l_img, const float* queries, float* out, const float* basis, int basis_diag,
                     int B, int64_t Q, int M, float c0, hipStream_t st) {
    RALD_CHECK(M % 32 == 0 && M >= 32 && M <= 1024, "ae_decode_stream: num_latents must be a multiple of 32 in [32,1024]");
    RALD_CHECK(B >= 1 && Q >= 1 && B <= 65535, "ae_decode_stream: bad batch / query count");
    DecodeArgs a;
    a.ctx = (const unsigned char*)ctx; a.ctx_stride = ae_ctx_stride(M); a.l_img = l_img; a.queries = queries; a.out = out; a.basis = basis;
    a.Q = Q; a.M = M; a.c0 = c0; a.eps = 1e-5f;
    return basis_diag ? launch_decode<true, false>(a, nullptr, B, Q, st) : launch_decode<false, false>(a, nullptr, B, Q, st);
}

// the same decoder on ragged query sets: queries [T][3] / out [T] concatenated over the samples, offsets [B + 1] on the device (sample b owns
// rows offsets[b] .. offsets[b+1] - 1; empty segments are fine), max_per_sample a host upper bound of the longest segment (trusted: the
// offsets are on the device, so a bound that is too small leaves the rows behind it undecoded and returns no error).  Nothing is read
// back: a workgroup without a chunk in its sample's segment returns at once.
int ae_decode_stream_ragged(const void* ctx, const unsigned short* l_img, const float* queries, const int64_t* offsets, float* out,
                            const float* basis, int basis_diag, int B, int64_t max_per_sample, int M, float c0, hipStream_t st) {
    RALD_CHECK(M % 32 == 0 && M >= 32 && M <= 1024, "ae_decode_stream_ragged: num_latents must be a multiple of 32 in [32,1024]");
    RALD_CHECK(B >= 1 && B <= 65535 && max_per_sample >= 0, "ae_decode_stream_ragged: bad batch / query count");
    RALD_CHECK(offsets, "ae_decode_stream_ragged: null offsets");
    if (max_per_sample == 0) return 0;
    RALD_CHECK(queries && out, "ae_decode_stream_ragged: null pointer");
    DecodeArgs a;
    a.ctx = (const unsigned char*)ctx; a.ctx_stride = ae_ctx_stride(M); a.l_img = l_img; a.queries = queries; a.out = out; a.basis = basis;
    a.Q = 0; a.M = M; a.c0 = c0; a.eps = 1e-5f;
    return basis_diag ? launch_decode<true, true>(a, offsets, B, max_per_sample, st) : launch_decode<false, true>(a, offsets, B, max_per_sample, st);
}

// ---------------------------------------------------------------------------------------------------------------
// logit + gradient with respect to the query point
// ---------------------------------------------------------------------------------------------------------------
// The logit is a closed form of the query's 51 features, so its gradient is one too.  With D = d f / d q (51 x 3: cos(p_e) basis[:,e],
// -sin(p_e) basis[:,e], identity), ubar = p.u, a_l = p_l (u_l - ubar), A_l = f.H_l + h0_l:
//
//     grad = ln2 [ rstd D^T G  -  rstd^3 (sum_l a_l A_l) D~^T L^T L f~ ],      G = sum_l a_l H_l
//
// Two passes over the score tiles per 64-query chunk.  Pass 1 is ae_decode_stream_kernel's statement sequence on one 32-query
// half (same features, same variance, same lazily rescaled softmax), written out here: staging, the feature phase and the merge of the
// lane halves are the same functions that kernel calls (ae_decode_core.h), but as calls to its feature, variance and score stages, or
// to the score tile alone, pass 1 and pass 2 cost this kernel registers.  The logit is that kernel's, bit for bit,
// for the same segment (tested, and recorded in tests/golden/g2x_decode_bits.npz).
// Pass 2 recomputes each score tile, forms a_l from the final maximum, denominator and ubar, and feeds it - the latents sit on the
// accumulator registers, the queries on the lanes, which is the MFMA B-operand layout up to a fixed order of the contraction index -
// into a second product G^T[k,q] += H~^T[k,l] a[l,q].  Its A operand is a transposed copy of the image, built once per workgroup in
// LDS in exactly that order: row k holds, for tile t, k-step s, lane half h, the 8 latents 32t + 8(2s + (j>>2)) + 4h + (j&3), j = 0..7,
// i.e. the rows that accumulator registers 8s .. 8s+7 of a lane of half h carry.  Rows are 2M + 16 bytes apart (an odd number of
// 16-byte chunks: the 32 rows of an operand read fall into different banks).  a_l is rounded to fp16 after a per-sample power-of-two
// scale (2^12 / 2^ilogb(max |u|), so |a_l| < 2^14); what falls below fp16's range is below 2^-37 max|u| per term, under the 2^-24
// max|u| that ubar's own fp32 rounding leaves in every a_l.  sum_l a_l A_l is f~.G over the slots <= 52; d var / d q is three more
// B operands (the columns of D~ in fp16) against the resident variance factor, dotted lane-locally with the L f~ accumulators.
//
// LDS: the plain layout + 72 floats of the basis in radians + the transposed image 64 (2M + 16) bytes: 139.6 KiB at M = 512, the
// largest M taken (M = 1024 would need 269 KiB).  8 waves per workgroup (two per SIMD, up to 256 registers each: the kernel takes 190
// with the block-diagonal basis, 219 with a general one, and spills with the 168 that 12 waves would leave).
struct DecodeGradArgs {
    DecodeArgs d;
    float* grad;                                      // [B][Q][3]
    float* proj;                                      // nullptr or [B][Q][3]
    float max_step;
};

// One clamped Newton step towards logit = 0.  Contraction is off: the float64 replay of the tests states this operation sequence
// (products, sums, one division per quotient), and an fma here would be a different sequence.
__device__ __forceinline__ void newton_step(float x, float y, float z, float logit, float gx, float gy, float gz, float max_step, float* o) {
#pragma clang fp contract(off)
    const float g2 = gx * gx + gy * gy + gz * gz;
    float sx = 0.f, sy = 0.f, sz = 0.f;
    if (g2 > 1e-20f) {
        const float t = -logit / g2;
        sx = t * gx; sy = t * gy; sz = t * gz;
        const float n = sqrtf(sx * sx + sy * sy + sz * sz);
        if (n > max_step) {
            const float c = max_step / n;
            sx *= c; sy *= c; sz *= c;
        }
        if (!(isfinite(sx) && isfinite(sy) && isfinite(sz))) { sx = 0.f; sy = 0.f; sz = 0.f; }
    }
    o[0] = fminf(fmaxf(x + sx, -1.f), 1.f);
    o[1] = fminf(fmaxf(y + sy, -1.f), 1.f);
    o[2] = fminf(fmaxf(z + sz, -1.f), 1.f);
}

constexpr int GRAD_NW = 8;
__host__ __device__ static inline int ht_row_bytes(int M) { return 2 * M + 16; }
static inline size_t grad_smem_bytes(int M) { return decoder_smem_bytes(M) + 76 * 4 + (size_t)64 * ht_row_bytes(M); }

template <bool DIAG, int NW, bool RAGGED>
__global__ __launch_bounds__(NW * 64) void ae_decode_grad_stream_kernel(DecodeGradArgs ga, const int64_t* __restrict__ offsets) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const DecodeArgs& a = ga.d;
    const int M = a.M;
    const DecoderLds lds = decoder_lds(smem, M);                 // the plain layout, then what this kernel adds
    unsigned char *s_h = lds.h, *s_l = lds.l;
    float *s_u = lds.u, *s_basis = lds.basis;                    // basis in revolutions
    float* s_brad = s_basis + 76;                                // 72 (+ pad): radians, the factor of D
    unsigned char* s_ht = reinterpret_cast<unsigned char*>(s_brad + 76);     // 64 rows of 2M + 16 bytes
    const int RS = ht_row_bytes(M);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.y;
    int64_t first = 0, seg = 0;
    if constexpr (RAGGED) {
        first = offsets[b];
        seg = offsets[b + 1] - first;
        if (first < 0 || seg <= 0 || (int64_t)blockIdx.x * NW * 64 >= seg) return;
    }
    stage_context<NW * 64>(lds, a.ctx + (int64_t)b * a.ctx_stride, a.l_img, a.basis, tid, s_brad);
    __syncthreads();
    {
        // transposed image in the second product's contraction order (see above)
        const int cpr = M >> 3;                                  // 16-byte chunks per row
        for (int idx = tid; idx < 64 * cpr; idx += NW * 64) {
            const int k = idx / cpr, c = idx - k * cpr;
            const int base = 32 * (c >> 2) + 16 * ((c >> 1) & 1) + 4 * (c & 1);
            f16x8 v;
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = *reinterpret_cast<const f16*>(s_h + img_off(base + 8 * (j >> 2) + (j & 3), k));
            *reinterpret_cast<f16x8*>(s_ht + k * RS + c * 16) = v;
        }
    }
    // power-of-two scale of a_l = p_l (u_l - ubar) for its fp16 rounding: |u_l - ubar| <= 2 max|u| < 2^(ilogb + 2)
    float a_scale = 1.0f, inv_a_scale = 1.0f;
    {
        float um = 0.f;
        for (int i = lane; i < M; i += 64) um = fmaxf(um, fabsf(s_u[i]));
        um = wave_max(um);
        if (um > 0.f && um < 3.0e38f) {
            const int e = max(min(12 - ilogbf(um), 100), -100);
            a_scale = exp2f((float)e);
            inv_a_scale = exp2f((float)-e);
        }
    }
    __syncthreads();
    const float inv_scale = s_u[M];
    const int r = lane & 31, h = lane >> 5;
    const int64_t Q = RAGGED ? seg : a.Q;
    const int64_t row0 = RAGGED ? first : (int64_t)b * a.Q;
    const float* qin = a.queries + row0 * 3;
    float* qout = a.out + row0;
    float* gout = ga.grad + row0 * 3;
    float* pout = ga.proj ? ga.proj + row0 * 3 : nullptr;
    const int64_t nchunks = (Q + 63) / 64;
    const float quarter = h ? 0.25f : 0.0f;                       // cos(t) = sin(t + 1/4 revolution)
    const float gk = inv_scale * inv_a_scale;                     // G and f~.G carry the image's scale and a_scale

    // One 32-query half of a 64-query chunk at a time (the halves of ae_decode_stream_kernel share only their operand loads: each has
    // its own running maximum), so the state of one half - 16 registers of features, 32 of G - is what a wave holds.
    for (int64_t chunk = (int64_t)blockIdx.x * NW + wave; chunk < nchunks; chunk += (int64_t)gridDim.x * NW) {
#pragma unroll 1
        for (int qb = 0; qb < 2; ++qb) {
            if (chunk * 64 + qb * 32 >= Q) break;                 // wave-uniform: a half without a query
            f16x8 bq[4];
            int64_t q = chunk * 64 + qb * 32 + r;
            const bool live = h == 0 && q < Q;
            q = q < Q ? q : Q - 1;
            const float x = qin[q * 3 + 0], y = qin[q * 3 + 1], z = qin[q * 3 + 2];
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                f16x8 f;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int e = 8 * s + j;
                    float p = feature_phase<DIAG>(s_basis, s, e, x, y, z);
                    p += quarter;
                    p = __builtin_amdgcn_fractf(p);
                    f[j] = (f16)__builtin_amdgcn_sinf(p);
                }
                bq[s] = f;
            }
            {
                f16x8 f;
                f[0] = (f16)(h ? 0.f : x); f[1] = (f16)(h ? 0.f : y); f[2] = (f16)(h ? 0.f : z);
                f[3] = (f16)(h ? 0.f : 1.f); f[4] = f[3];
                f[5] = (f16)0.f; f[6] = (f16)0.f; f[7] = (f16)0.f;
                bq[3] = f;
            }
            // ---- LayerNorm statistics of the query embedding: var_q = |L.f~|^2 (two 32-row tiles x 4 k-steps) ...
            f32x16 lf[2];
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
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(la, bq[s], acc, 0, 0, 0);
                }
#pragma unroll
                for (int i = 0; i < 16; ++i) ss = fmaf(acc[i], acc[i], ss);
                lf[t] = acc;
            }
            ss += __shfl_xor(ss, 32, 64);
            // ... and its derivative, one axis at a time: the column of D~ in the B-operand layout (the h = 0 lanes hold d sin(p_e) =
            // cos(p_e) b, the h = 1 lanes d cos(p_e) = -sin(p_e) b, both sin(p + quarter + 1/4 revolution) b; the last k-step is the
            // identity on the axis' own slot) against the resident factor, dotted with the L.f~ accumulators
            float vd[3];
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                f16x8 dq[4];
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                    if (DIAG && s != ax) continue;
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int e = 8 * s + j;
                        float p = feature_phase<DIAG>(s_basis, s, e, x, y, z);
                        p += quarter + 0.25f;
                        dq[s][j] = (f16)(__builtin_amdgcn_sinf(__builtin_amdgcn_fractf(p)) * s_brad[24 * ax + e]);
                    }
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) dq[3][j] = (f16)((j == ax && h == 0) ? 1.f : 0.f);
                float dd = 0.f;
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    f32x16 ad;
#pragma unroll
                    for (int i = 0; i < 16; ++i) ad[i] = 0.f;
                    const int row = 32 * t + r;
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        if (DIAG && s != 3 && s != ax) continue;
                        const f16x8 la = *reinterpret_cast<const f16x8*>(s_l + row * 128 + (((2 * s + h) ^ (row & 7)) << 4));
                        ad = __builtin_amdgcn_mfma_f32_32x32x16_f16(la, dq[s], ad, 0, 0, 0);
                    }
#pragma unroll
                    for (int i = 0; i < 16; ++i) dd = fmaf(lf[t][i], ad[i], dd);
                }
                vd[ax] = dd + __shfl_xor(dd, 32, 64);
            }
            const float var = ss + a.eps;
            const float rstd = rsqrtf(var);
            const float sd = var * rstd;                           // sqrt(var + eps)
            const f16 sd_hi = (f16)sd;
            const f16 sd_lo = (f16)(sd - (float)sd_hi);
            {
                f16x8 f = bq[3];
                f[5] = h ? (f16)0.f : sd_hi; f[6] = h ? (f16)0.f : sd_lo; f[7] = h ? (f16)0.f : sd_hi;
                bq[3] = f;
            }
            const float rq = rstd * inv_scale;                     // rstd_q / scale
            // ---- pass 1: scores + online softmax over the latents (the statements of ae_decode_stream_kernel)
            float m = -INFINITY, den = 0.f, num = 0.f;
            const int ntile = M >> 5;
            for (int t = 0; t < ntile; ++t) {
                const int row = 32 * t + r;
                f16x8 fa[4];
#pragma unroll
                for (int s = 0; s < 4; ++s) fa[s] = *reinterpret_cast<const f16x8*>(s_h + row * 128 + (((2 * s + h) ^ (row & 7)) << 4));
                float4 uv[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) uv[g] = *reinterpret_cast<const float4*>(s_u + 32 * t + 8 * g + 4 * h);
                f32x16 acc;
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
                for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[s], bq[s], acc, 0, 0, 0);
                float tm = fmaxf(fmaxf(acc[0], acc[1]), fmaxf(acc[2], acc[3]));
#pragma unroll
                for (int i = 4; i < 16; i += 4) tm = fmaxf(tm, fmaxf(fmaxf(acc[i], acc[i + 1]), fmaxf(acc[i + 2], acc[i + 3])));
                const float vm = tm * rq;
                if (__any(vm > m + 8.0f)) {                        // lazy running maximum: p stays <= 2^8
                    const float mn = fmaxf(m, vm);
                    const float alpha = __builtin_amdgcn_exp2f(m - mn);
                    den *= alpha; num *= alpha;
                    m = mn;
                }
                const float nm = -m;
                float d0 = 0.f, d1 = 0.f, n0 = 0.f, n1 = 0.f;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float p0 = __builtin_amdgcn_exp2f(fmaf(acc[4 * g + 0], rq, nm));
                    const float p1 = __builtin_amdgcn_exp2f(fmaf(acc[4 * g + 1], rq, nm));
                    const float p2 = __builtin_amdgcn_exp2f(fmaf(acc[4 * g + 2], rq, nm));
                    const float p3 = __builtin_amdgcn_exp2f(fmaf(acc[4 * g + 3], rq, nm));
                    d0 += p0; d1 += p1; d0 += p2; d1 += p3;
                    n0 = fmaf(p0, uv[g].x, n0); n1 = fmaf(p1, uv[g].y, n1); n0 = fmaf(p2, uv[g].z, n0); n1 = fmaf(p3, uv[g].w, n1);
                }
                den += d0 + d1;
                num += n0 + n1;
            }
            // ---- merge the two lane halves of the query; both halves go on with the h = 0 lane's numbers (the ones that are stored)
            float mm, dsum, nsum;
            merge_lane_halves(m, den, num, mm, dsum, nsum);
            const float logit = nsum / dsum + a.c0;
            const float ub = __shfl(nsum / dsum, r, 64);
            const float cs = a_scale / __shfl(dsum, r, 64);
            const float nm2 = -mm;
            // ---- pass 2: a_l = p_l (u_l - ubar) and G^T += H~^T . a (two 32-slot tiles)
            f32x16 G[2];
#pragma unroll
            for (int T = 0; T < 2; ++T)
#pragma unroll
                for (int i = 0; i < 16; ++i) G[T][i] = 0.f;
            for (int t = 0; t < ntile; ++t) {
                const int row = 32 * t + r;
                f16x8 fa[4];
#pragma unroll
                for (int s = 0; s < 4; ++s) fa[s] = *reinterpret_cast<const f16x8*>(s_h + row * 128 + (((2 * s + h) ^ (row & 7)) << 4));
                float4 uv[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) uv[g] = *reinterpret_cast<const float4*>(s_u + 32 * t + 8 * g + 4 * h);
                f16x8 ht[2][2];
#pragma unroll
                for (int T = 0; T < 2; ++T)
#pragma unroll
                    for (int s = 0; s < 2; ++s) ht[T][s] = *reinterpret_cast<const f16x8*>(s_ht + (32 * T + r) * RS + t * 64 + s * 32 + h * 16);
                f32x16 acc;
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
                for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[s], bq[s], acc, 0, 0, 0);
                f16x8 ab[2];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float p0 = __builtin_amdgcn_exp2f(fmaf(acc[4 * g + 0], rq, nm2));
                    const float p1 = __builtin_amdgcn_exp2f(fmaf(acc[4 * g + 1], rq, nm2));
                    const float p2 = __builtin_amdgcn_exp2f(fmaf(acc[4 * g + 2], rq, nm2));
                    const float p3 = __builtin_amdgcn_exp2f(fmaf(acc[4 * g + 3], rq, nm2));
                    ab[g >> 1][4 * (g & 1) + 0] = (f16)(p0 * ((uv[g].x - ub) * cs));
                    ab[g >> 1][4 * (g & 1) + 1] = (f16)(p1 * ((uv[g].y - ub) * cs));
                    ab[g >> 1][4 * (g & 1) + 2] = (f16)(p2 * ((uv[g].z - ub) * cs));
                    ab[g >> 1][4 * (g & 1) + 3] = (f16)(p3 * ((uv[g].w - ub) * cs));
                }
#pragma unroll
                for (int T = 0; T < 2; ++T)
#pragma unroll
                    for (int s = 0; s < 2; ++s) G[T] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ht[T][s], ab[s], G[T], 0, 0, 0);
            }
            // ---- epilogue: register i of tile T of a lane of half h holds slot 32T + 8(i>>2) + 4h + (i&3) of its query's G, i.e. k-step
            // 2T + (i>>3), sin (i&4 == 0) or cos, frequency 4h + (i&3); the last k-step holds x, y, z, 1 (h = 0) and the second 1 (h = 1)
            float sa = 0.f, gt[3] = {0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < 3; ++s) {
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const int e = 8 * s + 4 * h + jj;
                    float p = feature_phase<DIAG>(s_basis, s, e, x, y, z);
                    const float sn = __builtin_amdgcn_sinf(__builtin_amdgcn_fractf(p));
                    const float cn = __builtin_amdgcn_sinf(__builtin_amdgcn_fractf(p + 0.25f));
                    const float Gs = G[s >> 1][8 * (s & 1) + jj], Gc = G[s >> 1][8 * (s & 1) + 4 + jj];
                    sa = fmaf(Gs, (float)(f16)sn, sa);             // the fp16 features that the scores were made of
                    sa = fmaf(Gc, (float)(f16)cn, sa);
                    const float w = Gs * cn - Gc * sn;
                    if (DIAG) gt[s] = fmaf(w, s_brad[24 * s + e], gt[s]);
                    else {
#pragma unroll
                        for (int ax = 0; ax < 3; ++ax) gt[ax] = fmaf(w, s_brad[24 * ax + e], gt[ax]);
                    }
                }
            }
            if (h == 0) {
                sa = fmaf(G[1][8], (float)(f16)x, sa);
                sa = fmaf(G[1][9], (float)(f16)y, sa);
                sa = fmaf(G[1][10], (float)(f16)z, sa);
                sa += G[1][11];
                gt[0] += G[1][8]; gt[1] += G[1][9]; gt[2] += G[1][10];
            } else {
                sa += G[1][8];
            }
            sa += __shfl_xor(sa, 32, 64);
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) gt[ax] += __shfl_xor(gt[ax], 32, 64);
            const float c1 = 0.6931471805599453f * rstd * gk;
            const float c2 = c1 * rstd * rstd * sa;
            const float gx = c1 * gt[0] - c2 * vd[0], gy = c1 * gt[1] - c2 * vd[1], gz = c1 * gt[2] - c2 * vd[2];
            if (live) {
                qout[q] = logit;
                gout[q * 3 + 0] = gx; gout[q * 3 + 1] = gy; gout[q * 3 + 2] = gz;
                if (pout) newton_step(x, y, z, logit, gx, gy, gz, ga.max_step, pout + q * 3);
            }
        }
    }
}

template <bool DIAG, bool RAGGED>
static int launch_decode_grad(const DecodeGradArgs& a, const int64_t* offsets, int B, int64_t longest, hipStream_t st) {
    constexpr int NW = GRAD_NW;
    auto kern = ae_decode_grad_stream_kernel<DIAG, NW, RAGGED>;
    static bool attr_set = false;
    if (!attr_set) {
        RALD_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)grad_smem_bytes(AE_DECODE_GRAD_MAX_LATENTS)));
        attr_set = true;
    }
    hipLaunchKernelGGL(kern, dim3(decoder_grid_x(longest, NW, B), (unsigned)B), dim3(NW * 64), grad_smem_bytes(a.d.M), st, a, offsets);
    RALD_HIP(hipGetLastError());
    return 0;
}

// offsets == nullptr: dense, n = the queries of one sample; else ragged, n = the host upper bound of the longest segment.
// out_proj may be null (then max_step is not read)
int ae_decode_grad_stream(const void* ctx, const unsigned short* l_img, const float* queries, const int64_t* offsets, float* out, float* grad,
                          float* proj, float max_step, const float* basis, int basis_diag, int B, int64_t n, int M, float c0, hipStream_t st) {
    RALD_CHECK(M % 32 == 0 && M >= 32 && M <= AE_DECODE_GRAD_MAX_LATENTS,
               "ae_decode_grad_stream: num_latents must be a multiple of 32 in [32,512] (the transposed image has to fit in LDS)");
    RALD_CHECK(B >= 1 && B <= 65535 && (offsets ? n >= 0 : n >= 1), "ae_decode_grad_stream: bad batch / query count");
    RALD_CHECK(!proj || (std::isfinite(max_step) && max_step > 0.f), "ae_decode_grad_stream: max_step must be finite and > 0");
    if (offsets && n == 0) return 0;
    RALD_CHECK(queries && out && grad, "ae_decode_grad_stream: null pointer");
    DecodeGradArgs a;
    a.d.ctx = (const unsigned char*)ctx; a.d.ctx_stride = ae_ctx_stride(M); a.d.l_img = l_img; a.d.queries = queries; a.d.out = out;
    a.d.basis = basis; a.d.Q = offsets ? 0 : n; a.d.M = M; a.d.c0 = c0; a.d.eps = 1e-5f;
    a.grad = grad; a.proj = proj; a.max_step = proj ? max_step : 0.f;
    if (offsets) return basis_diag ? launch_decode_grad<true, true>(a, offsets, B, n, st) : launch_decode_grad<false, true>(a, offsets, B, n, st);
    return basis_diag ? launch_decode_grad<true, false>(a, nullptr, B, n, st) : launch_decode_grad<false, false>(a, nullptr, B, n, st);
}

}  // namespace rald
