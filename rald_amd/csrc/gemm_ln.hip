// Residual GEMM with the NEXT LayerNorm fused into its epilogue (N = 512 = one full row per tile):
//
//     x[m][:]  += A[m][:] . W^T + bias                      (x = f(x) + x, fp32 residual stream)
//     h[m][:]   = LN(x[m][:]) * (add_one + g[s][:]) + b[s][:]    (bf16, the next GEMM's A operand)
//
// i.e. `to_out(...) + x` followed by AdaLayerNorm / PreNorm-LayerNorm of the following sub-block
// (models_radar_generation.py:166-168 + :127-131; models_ae.py:413-414 + :41-42).  Unfused, the
// LayerNorm is a separate HBM-bound pass that re-reads the 4-byte stream; fused, x is read once
// and written once per sub-block and three launches per transformer block disappear.
//
// Tile BM x 512 x 64, 8 waves as WM x WN, LDS-DMA staged double buffer (the engine of gemm_tile.h, as in
// gemm_nt_glds_kernel and gemm_mx8_kernel; at BM = 128 the two stages take exactly the CU's 160 KiB).  Epilogue:
//   0. (group-uniform form) bias, g, b of the 512 columns -> LDS, once per workgroup, before any store;
//   1. v = acc + bias + x_old in the accumulator layout (lane: 4 columns of 16 rows per m-tile);
//   2. per-row sum / sum-of-squares: 32 in-lane values, 2 cross-lane steps, then across the WN waves
//      through a 4 KiB LDS table and ONE workgroup barrier (single-pass variance in fp32: 512 terms);
//   3. x_new and h leave through the wave-private LDS transpose as whole rows (16 B per lane).
#include <cstdlib>
#include <type_traits>
#include <utility>

#include "common.h"
#include "kernels.h"
#include "gemm_tile.h"
#include "mx8.h"

namespace rald {

// LDS layout of the epilogue (it reuses the staging buffers): per-wave transpose patches of 16 rows, the row-sum table, then bias | g | b
template <int BM, int WM, int WN>
struct LnEpiLds {
    static constexpr int NT = 512 / (16 * WN);
    static constexpr int ROWB_F = NT * 16 * 4, STRIDE_F = ROWB_F + 16;      // fp32 patch row (x_new)
    static constexpr int ROWB_H = NT * 16 * 2, STRIDE_H = ROWB_H + 16;      // bf16 patch row (h)
    static constexpr int PATCH = 16 * STRIDE_F;
    static constexpr int RED_OFF = WM * WN * PATCH;                         // float2 red[BM][WN]
    static constexpr int VEC_OFF = RED_OFF + BM * WN * 8;                   // GU: float vec[3][512] = bias | g | b
    static constexpr int BYTES = VEC_OFF + 3 * 512 * 4;
};

// the calls f(0), ..., f(N - 1) with the index as a compile-time constant
template <int... Q, typename F>
__device__ __forceinline__ void unrolled(std::integer_sequence<int, Q...>, F&& f) { (f(std::integral_constant<int, Q>{}), ...); }
template <int N, typename F>
__device__ __forceinline__ void unrolled(F&& f) { unrolled(std::make_integer_sequence<int, N>{}, f); }

// ---- epilogue shared by the main-loop forms: acc (+ x_old already inside unless XEPI) -> x_new, h ---------------------------------
// GU (group-uniform, chosen on the host): all BM rows of a tile share one modulation row (gstride == 0 or rows_per_group % BM == 0).
// bias, g and b of the tile's 512 columns are then fetched ONCE per workgroup, before any store, into 6 KiB of LDS behind `red`
// and read from there in both phases.  The per-row form (GU = false) is for tiles that straddle modulation groups: every
// m-tile of phase 2 loads its 16 g / b vectors behind the x_new stores it has just issued, and - vmcnt being one in-order counter for loads and stores on gfx950 - waits for
// those stores and the previous m-tile's h stores to be acknowledged before it can compute (gemm_epilogue.h states the rule).
// DEAD: every wave's last read of the staging buffers already lies behind a barrier (the pipelined main loop).
template <int BM, int WM, int WN, bool XEPI, bool GU, bool DEAD>
__device__ __forceinline__ void resid_ln_epilogue(const GemmLnArgs& a, f32x4 (&acc)[BM / (16 * WM)][512 / (16 * WN)], unsigned char* smem, int m0) {
    constexpr int BN = 512;
    constexpr int WAVES = WM * WN;
    constexpr int MT = BM / (16 * WM);
    constexpr int NT = BN / (16 * WN);
    using L = LnEpiLds<BM, WM, WN>;
    typedef float nt_f32x4 __attribute__((ext_vector_type(4)));
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int fr = lane & 15, fq = lane >> 4;
    const bool nt_io = (a.nt_io & 1) != 0;
    const float* vec = reinterpret_cast<const float*>(smem + L::VEC_OFF);
    if constexpr (GU) {
        static_assert(WAVES * 64 >= 3 * BN / 4, "one float4 per thread covers bias, g and b");
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        const int which = tid / (BN / 4), col = (tid % (BN / 4)) * 4;          // uniform per wave: 0 bias, 1 g, 2 b
        if (which < 3) {
            const int64_t goff = (int64_t)(m0 / a.rows_per_group) * a.gstride;
            const float* src = which == 0 ? a.bias : (which == 1 ? a.g : a.b) + goff;
            t = *reinterpret_cast<const float4*>(src + col);
        }
        if constexpr (!DEAD) {
            asm volatile("" ::: "memory");
            __builtin_amdgcn_s_barrier();         // staging buffers are dead: reuse them (vec, then patches + red)
            asm volatile("" ::: "memory");
        }
        if (which < 3) *reinterpret_cast<float4*>(smem + L::VEC_OFF + (which * BN + col) * 4) = t;
        __syncthreads();
    }
    // ---- 1. v = acc + bias + x_old (accumulator layout), row partial sums -------------------------
    const int mb = m0 + wm * (BM / WM);
    const int nb = wn * (BN / WN);
    float s1[MT], s2[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        int m = mb + i * 16 + fr;
        m = m < a.M ? m : a.M - 1;
        s1[i] = 0.f; s2[i] = 0.f;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int n = nb + j * 16 + 4 * fq;
            const float4 b = GU ? *reinterpret_cast<const float4*>(vec + n) : *reinterpret_cast<const float4*>(a.bias + n);
            // (bf16 operands: x_old is already in the accumulators, see the main loop)
            float4 xo = make_float4(0.f, 0.f, 0.f, 0.f);
            if constexpr (XEPI) {
                const nt_f32x4 xv = nt_io ? __builtin_nontemporal_load(reinterpret_cast<const nt_f32x4*>(a.x + (int64_t)m * BN + n))
                                          : *reinterpret_cast<const nt_f32x4*>(a.x + (int64_t)m * BN + n);
                xo = make_float4(xv[0], xv[1], xv[2], xv[3]);
            }
            f32x4 v = acc[i][j];
            v[0] += b.x + xo.x; v[1] += b.y + xo.y; v[2] += b.z + xo.z; v[3] += b.w + xo.w;
            acc[i][j] = v;
            s1[i] += (v[0] + v[1]) + (v[2] + v[3]);
            s2[i] += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
        }
        s1[i] += __shfl_xor(s1[i], 16, 64); s2[i] += __shfl_xor(s2[i], 16, 64);
        s1[i] += __shfl_xor(s1[i], 32, 64); s2[i] += __shfl_xor(s2[i], 32, 64);
        asm volatile("" ::: "memory");            // keep only one m-tile's x_old loads in flight (register pressure)
    }
    if constexpr (!GU) {
        asm volatile("" ::: "memory");
        __builtin_amdgcn_s_barrier();             // staging buffers are dead: reuse them (patches + red)
        asm volatile("" ::: "memory");
    }
    float2* red = reinterpret_cast<float2*>(smem + L::RED_OFF);
    if (fq == 0) {
#pragma unroll
        for (int i = 0; i < MT; ++i) red[(wm * (BM / WM) + i * 16 + fr) * WN + wn] = make_float2(s1[i], s2[i]);
    }
    __syncthreads();
    float mean[MT], rstd[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        float t1 = 0.f, t2 = 0.f;
#pragma unroll
        for (int w = 0; w < WN; ++w) {
            const float2 p = red[(wm * (BM / WM) + i * 16 + fr) * WN + w];
            t1 += p.x; t2 += p.y;
        }
        mean[i] = t1 * (1.0f / BN);
        const float var = fmaxf(t2 * (1.0f / BN) - mean[i] * mean[i], 0.f);
        rstd[i] = rsqrtf(var + a.eps);
    }

    // ---- 2. x_new (fp32) and h (bf16) out as whole rows through the wave-private patch -------------
    unsigned char* patch = smem + wave * L::PATCH;
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        // x_new
#pragma unroll
        for (int j = 0; j < NT; ++j)
            *reinterpret_cast<float4*>(patch + fr * L::STRIDE_F + (16 * j + 4 * fq) * 4) = make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
        {
            constexpr int LPR = L::ROWB_F / 16, RPI = 64 / LPR;
#pragma unroll
            for (int r0 = 0; r0 < 16; r0 += RPI) {
                const int r = r0 + lane / LPR, pc = lane % LPR;
                const int m = mb + i * 16 + r;
                const uint4 v = *reinterpret_cast<const uint4*>(patch + r * L::STRIDE_F + pc * 16);
                if (m < a.M) {
                    typedef unsigned int nt_u32x4 __attribute__((ext_vector_type(4)));
                    if (nt_io) __builtin_nontemporal_store(nt_u32x4{v.x, v.y, v.z, v.w}, reinterpret_cast<nt_u32x4*>(a.x + (int64_t)m * BN + nb + pc * 4));
                    else *reinterpret_cast<uint4*>(a.x + (int64_t)m * BN + nb + pc * 4) = v;
                }
            }
        }
        // h = (v - mean) * rstd * (add_one + g) + b ; modulation row of this row's sample
        int m = mb + i * 16 + fr;
        m = m < a.M ? m : a.M - 1;
        const int64_t goff = (int64_t)(m / a.rows_per_group) * a.gstride;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int n = nb + j * 16 + 4 * fq;
            const float4 gg = GU ? *reinterpret_cast<const float4*>(vec + BN + n) : *reinterpret_cast<const float4*>(a.g + goff + n);
            const float4 bb = GU ? *reinterpret_cast<const float4*>(vec + 2 * BN + n) : *reinterpret_cast<const float4*>(a.b + goff + n);
            const f32x4 v = acc[i][j];
            *reinterpret_cast<bf16x4*>(patch + fr * L::STRIDE_H + (16 * j + 4 * fq) * 2) =
                pack4((v[0] - mean[i]) * rstd[i] * (a.add_one + gg.x) + bb.x, (v[1] - mean[i]) * rstd[i] * (a.add_one + gg.y) + bb.y,
                      (v[2] - mean[i]) * rstd[i] * (a.add_one + gg.z) + bb.z, (v[3] - mean[i]) * rstd[i] * (a.add_one + gg.w) + bb.w);
        }
        {
            constexpr int LPR = L::ROWB_H / 16, RPI = 64 / LPR;
#pragma unroll
            for (int r0 = 0; r0 < 16; r0 += RPI) {
                const int r = r0 + lane / LPR, pc = lane % LPR;
                const int mm = mb + i * 16 + r;
                const uint4 v = *reinterpret_cast<const uint4*>(patch + r * L::STRIDE_H + pc * 16);
                if (a.h8) {
                    // MXFP8 output: this lane's 16-byte piece is 8 consecutive columns, 4 consecutive lanes = one 32-column
                    // block (nb and the pieces are 32-column aligned); every lane of the wave takes part in the shuffles
                    const bf16x8 hv = *reinterpret_cast<const bf16x8*>(&v);
                    float f[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) f[e] = (float)hv[e];
                    const int64_t mc = mm < a.M ? mm : a.M - 1;
                    const int col = nb + pc * 8;
                    unsigned char q8[8] __attribute__((aligned(8)));
                    unsigned char sc;
                    mx8_block(f, q8, &sc, true);
                    if (mm < a.M) {
                        *reinterpret_cast<uint2*>(a.h8 + mc * BN + col) = *reinterpret_cast<const uint2*>(q8);
                        if ((pc & 3) == 0) a.hs[mc * (BN / 32) + col / 32] = sc;
                    }
                } else if (mm < a.M) {
                    typedef unsigned int nt_u32x4 __attribute__((ext_vector_type(4)));
                    if (nt_io) __builtin_nontemporal_store(nt_u32x4{v.x, v.y, v.z, v.w}, reinterpret_cast<nt_u32x4*>(a.h + (int64_t)mm * BN + nb + pc * 8));
                    else *reinterpret_cast<uint4*>(a.h + (int64_t)mm * BN + nb + pc * 8) = v;
                }
            }
        }
    }
}

// Staging, swizzle and the MXFP8 loop body are gemm_tile.h's; the pipelined 128-row bf16 loop keeps its own scalar-base DMA addressing.
template <int BM, int WM, int WN, bool MX, bool GU>
__device__ __forceinline__ void gemm_resid_ln_body(const GemmLnArgs& a) {
    constexpr int BN = 512, NSTAGE = 2, BK = 64;
    constexpr int WAVES = WM * WN;
    constexpr int MT = BM / (16 * WM);
    constexpr int NT = BN / (16 * WN);
    constexpr int ROWB = 128;                                    // bytes per LDS row
    constexpr int RPP = 1024 / ROWB;                             // rows per DMA piece (one wave instruction = 1 KiB)
    constexpr int CA = BM / RPP / WAVES;                         // pieces per stage and wave
    constexpr int CB = BN / RPP / WAVES;
    static_assert(CA >= 1 && CB >= 1 && BM % (RPP * WAVES) == 0 && BN % (RPP * WAVES) == 0 && MT >= 1 && NT >= 1, "tile/wave split");
    constexpr int STAGE_BYTES = (BM + BN) * ROWB;
    static_assert(LnEpiLds<BM, WM, WN>::BYTES <= NSTAGE * STAGE_BYTES, "epilogue scratch (patches, red, bias | g | b) must fit in the staging buffers");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    int mtile = blockIdx.x;
    if (a.strideW != 0) {
        // per-group weights: keep a group's tiles on one XCD (launch index g -> XCD g & 7), so its weights cross the fabric once
        const int tg = a.w_rows / BM, ngroups = (int)gridDim.x / (tg > 0 ? tg : 1);
        if (tg >= 1 && tg < 8 && ngroups * tg == (int)gridDim.x && (ngroups & 7) == 0) {
            const int slot = (int)blockIdx.x >> 3;
            mtile = ((slot / tg) * 8 + ((int)blockIdx.x & 7)) * tg + slot % tg;
        }
    }
    const int m0 = mtile * BM;
    // operand rows per k-step: 128 bytes = 64 bf16 or 128 e4m3 (MX: e4m3 + e8m0 per 32, see gemm_fp8.hip)
    constexpr int ESZ = MX ? 1 : 2;
    const unsigned char* A0 = MX ? a.A8 : reinterpret_cast<const unsigned char*>(a.A);
    const unsigned char* W0 = MX ? a.W8 : reinterpret_cast<const unsigned char*>(a.W + (int64_t)(m0 / a.w_rows) * a.strideW);

    typedef float nt_f32x4 __attribute__((ext_vector_type(4)));
    const bool nt_io_ = (a.nt_io & 1) != 0;
    f32x4 acc[MT][NT];
    const int nk = MX ? a.K / 128 : a.K / BK;
    const int fr = lane & 15, fq = lane >> 4;
    if constexpr (MX) {
        Mx8Loop<BM, BN, WM, WN> L;
        L.begin(acc, A0, a.lda, a.SA, m0, a.M, W0, a.ldw, a.SW, 0, BN, a.K, smem, wave, lane);
        for (int kt = 0; kt < nk; ++kt) L.step(acc, kt, kt & 1, (kt + 1) & 1, smem, wave, lane);
    } else {
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // The residual x_old rides into the accumulators DURING the main loop: k-step q < 8 loads one eighth of this wave's x
    // tile (MT*NT/8 float4 per lane) right after the next stage's DMA is issued, and k-step q+1 adds it to the accumulators.
    // With one 160-KiB workgroup per CU every CU is in the same phase at the same time, so an epilogue that first READS
    // 67 MB of x leaves the MFMA pipe idle chip-wide while HBM streams, and HBM idle while the MFMAs run; spreading the read
    // over the k-loop overlaps the two (K = 512 at M = 32768: 47 -> 45 us; the rest of the epilogue is the 100 MB of stores, ~10 us,
    // and a main loop whose k-steps each wait one HBM latency for the A panel at prefetch distance 1).
    constexpr int XP = MT * NT / 8;                                   // float4 pieces per k-step
    static_assert(MT * NT % 8 == 0, "x pieces per k-step");
    nt_f32x4 xt[XP];
    const int mb_ = m0 + wm * (BM / WM), nb_ = wn * (BN / WN);
    // x_old addresses as uniform base + one 32-bit lane offset per m-tile + immediates (64-bit lane pointers per piece were hoisted out of
    // the k-loop by the compiler: 64 registers of loop-invariant addresses next to 128 accumulators)
    const unsigned char* xbase = reinterpret_cast<const unsigned char*>(a.x) + (int64_t)mb_ * BN * 4;      // uniform
    unsigned xoff[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        int r = i * 16 + fr;
        r = mb_ + r < a.M ? r : a.M - 1 - mb_;
        xoff[i] = (unsigned)r * (BN * 4) + (unsigned)(nb_ + 4 * fq) * 4;
    }
    auto x_load = [&](auto QC) {
        constexpr int q = decltype(QC)::value;
#pragma unroll
        for (int e = 0; e < XP; ++e) {
            const int idx = q * XP + e, i = idx / NT, j = idx % NT;
            const unsigned char* sp = xbase;
            asm volatile("" : "+s"(sp));                               // (keeps the address in the saddr + lane offset + immediate form)
            const nt_f32x4* px = reinterpret_cast<const nt_f32x4*>(sp + xoff[i] + j * 64);
            xt[e] = nt_io_ ? __builtin_nontemporal_load(px) : *px;
        }
    };
    auto x_add = [&](auto QC) {
        constexpr int q = decltype(QC)::value;
#pragma unroll
        for (int e = 0; e < XP; ++e) {
            const int idx = q * XP + e, i = idx / NT, j = idx % NT;
            acc[i][j][0] += xt[e][0]; acc[i][j][1] += xt[e][1]; acc[i][j][2] += xt[e][2]; acc[i][j][3] += xt[e][3];
        }
    };
    const unsigned char* gA[CA];
    const unsigned char* gB[CB];
    dma_sources<WAVES>(gA, A0, a.lda * ESZ, m0, a.M, wave, lane);
    dma_sources<WAVES>(gB, W0, a.ldw * ESZ, 0, BN, wave, lane);
    // (dma_stage's issue order, written out: in the unrolled k-steps below `buf` and `kt` are constants, and through the shared helper the
    //  LDS destinations of the ten pieces fold differently - two more scalar adds in each 800-instruction block of the 64-row form)
    auto stage = [&](int kt, int buf) {
        unsigned char* base = smem + buf * STAGE_BYTES;
#pragma unroll
        for (int p = 0; p < CA; ++p)
            __builtin_amdgcn_global_load_lds((glb_void*)(gA[p] + kt * ROWB), (lds_void*)(base + (wave + WAVES * p) * 1024), 16, 0, 0);
#pragma unroll
        for (int p = 0; p < CB; ++p)
            __builtin_amdgcn_global_load_lds((glb_void*)(gB[p] + kt * ROWB), (lds_void*)(base + BM * ROWB + (wave + WAVES * p) * 1024), 16, 0, 0);
    };
    // piece q of x_old loads in k-step q and is added in k-step q + 1
    auto kstep = [&](int kt, auto QC) {
        constexpr int q = decltype(QC)::value;                        // 0..7: x piece of this k-step; 8: add the last piece; 9: none
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (kt + 1 < nk) stage(kt + 1, (kt + 1) & 1);
        if constexpr (q >= 1 && q <= 8) x_add(std::integral_constant<int, q - 1>{});
        if constexpr (q <= 7) x_load(QC);
        const bf16x8* sA = reinterpret_cast<const bf16x8*>(smem + (kt & 1) * STAGE_BYTES);
        const bf16x8* sB = sA + BM * 8;
#pragma unroll
        for (int kk = 0; kk < BK / 32; ++kk) {
            bf16x8 fa[MT], fb[NT];
            const int chunk = kk * 4 + fq;
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                const int r = wm * (BM / WM) + i * 16 + fr;
                fa[i] = sA[r * 8 + RALD_SWZ(r, chunk)];
            }
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int r = wn * (BN / WN) + j * 16 + fr;
                fb[j] = sB[r * 8 + RALD_SWZ(r, chunk)];
            }
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[j], fa[i], acc[i][j], 0, 0, 0);
        }
    };
    if constexpr (MT == 4 && NT == 8 && CA + CB == 10) {
        // ---- pipelined main loop of the 128-row form (round 3) ----------------------------------------------------------------------
        // An iteration starts right AFTER a tile hand-over (barrier), so no LDS read is pending at the loop head and the compiler's
        // waits inside are exact counts.  Fragments: the A side (4 m-tiles) is double-buffered per 32-deep sub-step, the B side (8
        // n-tiles) is refreshed IN PLACE: the read of n-tile j for the next sub-step goes out right behind the 4 MFMAs that consumed
        // the current one (LDS returns in order; the register hazard is the hardware's).  The 10 DMA pieces of the next tile and the
        // 12 reads are spread between the MFMAs instead of standing in front of them (round 2: wait - barrier - 10 DMA issues - 12
        // reads - wait - 32 MFMAs - 12 reads - wait - 32 MFMAs, i.e. ~1300 idle matrix-pipe cycles per 2048-cycle k-step).
        constexpr int W_ALL = 0x0070;                                  // vmcnt(0) lgkmcnt(0)
        constexpr int W_ST1 = ((CA + CB) & 15) | (((CA + CB) >> 4) << 14) | 0x0f70;
        bf16x8 fa[MT], fb[NT];
        // DMA sources as scalar base + 32-bit lane offset (the saddr form of global_load_lds): 3 VGPRs instead of the 20 that ten
        // 64-bit lane pointers take - the register file has 128 accumulators, 48 fragment registers and 16 of x_old to hold
        const unsigned char* sbA = A0 + (int64_t)m0 * a.lda * ESZ;                    // uniform
        const int lr = lane >> 3;                                                     // row inside a DMA piece
        const int lc = RALD_SWZ(lr, lane & 7);                                        // source chunk that lands in physical chunk lane & 7
        unsigned voA[CA];
#pragma unroll
        for (int p = 0; p < CA; ++p) {
            int r = RPP * (wave + WAVES * p) + lr;
            r = m0 + r < a.M ? r : a.M - 1 - m0;
            voA[p] = (unsigned)r * (unsigned)(a.lda * ESZ) + (unsigned)lc * 16u;
        }
        const unsigned voB = (unsigned)(RPP * wave + lr) * (unsigned)(a.ldw * ESZ) + (unsigned)lc * 16u;
        const unsigned stepB = (unsigned)(RPP * WAVES) * (unsigned)(a.ldw * ESZ);     // uniform: bytes between this wave's W pieces
        // k-steps run in ascending order from 0 in every tile, so a sample's sums do not depend on its tile or batch size (a per-tile
        // rotated start measured +0.8 % and was not shipped: DESIGN §5).  The no-op koff / wrap stays: removing it changes the compiled code.
        const int koff = 0;
        auto ksrc = [&](int kt) { const int k = kt + koff; return k >= nk ? k - nk : k; };
        auto stage2 = [&](int kt, int buf) {
            unsigned char* base = smem + buf * STAGE_BYTES;
            const unsigned char* ka = sbA + ksrc(kt) * ROWB;
            const unsigned char* kb = W0 + ksrc(kt) * ROWB;
#pragma unroll
            for (int p = 0; p < CA; ++p)
                __builtin_amdgcn_global_load_lds((glb_void*)(ka + voA[p]), (lds_void*)(base + (wave + WAVES * p) * 1024), 16, 0, 0);
#pragma unroll
            for (int p = 0; p < CB; ++p)
                __builtin_amdgcn_global_load_lds((glb_void*)(kb + (size_t)p * stepB + voB), (lds_void*)(base + BM * ROWB + (wave + WAVES * p) * 1024), 16, 0, 0);
        };
        auto rdA = [&](int buf, int kk, int i) -> bf16x8 {
            const bf16x8* sA = reinterpret_cast<const bf16x8*>(smem + buf * STAGE_BYTES);
            const int r = wm * (BM / WM) + i * 16 + fr;
            return sA[r * 8 + RALD_SWZ(r, kk * 4 + fq)];
        };
        auto rdB = [&](int buf, int kk, int j) -> bf16x8 {
            const bf16x8* sB = reinterpret_cast<const bf16x8*>(smem + buf * STAGE_BYTES) + BM * 8;
            const int r = wn * (BN / WN) + j * 16 + fr;
            return sB[r * 8 + RALD_SWZ(r, kk * 4 + fq)];
        };
        // One 32-deep sub-step = 32 MFMAs on the fragments in registers, with the 12 fragment reads of the NEXT sub-step (buffer nbuf,
        // half nkk) going out in place as soon as a fragment's last MFMA has been issued:
        //   head   (i,0) (i,1) for i = 0..3        then fb[0], fb[1] are re-read
        //   middle (i,j) for j = 2..5              fb[j] re-read behind its 4 MFMAs
        //   tail   (i,6) (i,7) for i = 0..3        fa[i] re-read behind its 2 MFMAs, fb[6], fb[7] at the end
        // so every A fragment is re-read >= 6 MFMAs (~100 clocks, an LDS latency) before the next sub-step's head needs it and no
        // fragment is double-buffered.  The DMA pieces of the next tile (first sub-step of an iteration) go between the head's MFMAs.
        // sched_barrier(0) after every group pins the order (hipcc otherwise pulls the reads to the front and waits for all of them).
        auto mm = [&](int i, int j) { acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[j], fa[i], acc[i][j], 0, 0, 0); };
        auto substep = [&](int nbuf, int nkk, auto DMA, int kt_next) {
            constexpr bool dma = decltype(DMA)::value;
            unsigned char* dbase = smem + (kt_next & 1) * STAGE_BYTES;
            const unsigned char* ka = sbA + ksrc(kt_next) * ROWB;
            const unsigned char* kb = W0 + ksrc(kt_next) * ROWB;
            // (the scalar bases pass through an empty asm: otherwise loop strength reduction turns every piece's address into a 64-bit
            //  lane pointer carried around the loop - the 20 registers this addressing form is here to save)
            auto dmaA = [&](int p) {
                const unsigned char* sp = ka;
                asm volatile("" : "+s"(sp));
                __builtin_amdgcn_global_load_lds((glb_void*)(sp + voA[p]), (lds_void*)(dbase + (wave + WAVES * p) * 1024), 16, 0, 0);
            };
            auto dmaB = [&](int p) {
                const unsigned char* sp = kb + (size_t)p * stepB;
                asm volatile("" : "+s"(sp));
                __builtin_amdgcn_global_load_lds((glb_void*)(sp + voB), (lds_void*)(dbase + BM * ROWB + (wave + WAVES * p) * 1024), 16, 0, 0);
            };
#pragma unroll
            for (int i = 0; i < MT; ++i) {                              // head
                mm(i, 0);
                if constexpr (dma) { if (i < CA) dmaA(i); else dmaB(i - CA); }
                __builtin_amdgcn_sched_barrier(0);
                mm(i, 1);
                if constexpr (dma) dmaB(i + MT - CA);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (nbuf >= 0) { fb[0] = rdB(nbuf, nkk, 0); fb[1] = rdB(nbuf, nkk, 1); }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 2; j < NT - 2; ++j) {                          // middle
                mm(0, j); mm(1, j);
                if constexpr (dma) { if (j - 2 + 2 * MT - CA < CB) dmaB(j - 2 + 2 * MT - CA); }
                __builtin_amdgcn_sched_barrier(0);
                mm(2, j); mm(3, j);
                if (nbuf >= 0) fb[j] = rdB(nbuf, nkk, j);
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int i = 0; i < MT; ++i) {                              // tail
                mm(i, NT - 2); mm(i, NT - 1);
                if (nbuf >= 0) fa[i] = rdA(nbuf, nkk, i);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (nbuf >= 0) { fb[NT - 2] = rdB(nbuf, nkk, NT - 2); fb[NT - 1] = rdB(nbuf, nkk, NT - 1); }
            __builtin_amdgcn_sched_barrier(0);
        };
        static_assert(2 * MT - CA + (NT - 4) >= CB, "all DMA pieces of a stage find a slot in the first sub-step");
        auto hand_over = [&]() {
            __builtin_amdgcn_s_waitcnt(W_ALL);                         // the next tile has landed; my reads of this one are done
            __builtin_amdgcn_s_barrier();
        };
        stage2(0, 0);
        if (nk > 1) { stage2(1, 1); __builtin_amdgcn_s_waitcnt(W_ST1); } else __builtin_amdgcn_s_waitcnt(W_ALL);
        __builtin_amdgcn_s_barrier();
        // tile 0, sub-step 0: its fragments have nothing to hide behind
#pragma unroll
        for (int j = 0; j < NT; ++j) fb[j] = rdB(0, 0, j);
#pragma unroll
        for (int i = 0; i < MT; ++i) fa[i] = rdA(0, 0, i);
        substep(0, 1, std::false_type{}, 0);                           // MFMAs (tile 0, kk 0); reads (tile 0, kk 1)
        hand_over();
        // iteration kt >= 1: [DMA tile kt+1] MFMAs (kt-1, kk 1) + reads (kt, kk 0) | MFMAs (kt, kk 0) + reads (kt, kk 1) | hand-over.
        // (x_old is added in the epilogue on this path: riding along in the loop - a uniform switch over the piece index - cost the
        //  register allocator PHI copies of all 128 accumulators and 140 spills)
        auto iter = [&](int kt, auto DMA) {
            substep(kt & 1, 0, DMA, kt + 1);                           // MFMAs (kt-1, kk 1) + DMA of tile kt+1 + reads (kt, kk 0)
            substep(kt & 1, 1, std::false_type{}, 0);                  // MFMAs (kt, kk 0) + reads (kt, kk 1)
            hand_over();
        };
        for (int kt = 1; kt + 1 < nk; ++kt) iter(kt, std::true_type{});
        if (nk > 1) iter(nk - 1, std::false_type{});
        substep(-1, 0, std::false_type{}, 0);                          // MFMAs (last tile, kk 1)
    } else {
    stage(0, 0);
    if (nk >= 9) {                                                    // K >= 576: pieces over the first eight k-steps
        unrolled<9>([&](auto q) { kstep(q, q); });
        for (int kt = 9; kt < nk; ++kt) kstep(kt, std::integral_constant<int, 9>{});
    } else if (nk == 8) {                                             // K = 512: the last piece is added after the loop
        unrolled<8>([&](auto q) { kstep(q, q); });
        x_add(std::integral_constant<int, 7>{});
    } else {                                                          // short K: all of x after the loop
        for (int kt = 0; kt < nk; ++kt) kstep(kt, std::integral_constant<int, 9>{});
        unrolled<8>([&](auto q) { x_load(q); x_add(q); });
    }
    }

    }
    constexpr bool PIPE = !MX && MT == 4 && NT == 8 && CA + CB == 10;     // the pipelined loop adds x_old in the epilogue
    resid_ln_epilogue<BM, WM, WN, (MX || PIPE), GU, PIPE>(a, acc, smem, m0);
}

template <int BM, int WM, int WN, bool MX, bool GU>
__global__ __launch_bounds__(WM * WN * 64) void gemm_resid_ln_kernel(GemmLnArgs a) { gemm_resid_ln_body<BM, WM, WN, MX, GU>(a); }

template <int BM, int WM, int WN, bool MX, bool GU>
static int launch_ln_gu(const GemmLnArgs& a, hipStream_t st) {
    constexpr int smem = 2 * (BM + 512) * 64 * 2;                 // (always above 64 KiB)
    static bool raised = false;
    return launch_dyn_lds(gemm_resid_ln_kernel<BM, WM, WN, MX, GU>, raised, dim3(cdiv(a.M, BM)), WM * WN * 64, smem, st, a);
}

// group-uniform form when a tile's BM rows all share one modulation row (the denoiser: 512 rows per sample; the AE stack: gstride 0)
template <int BM, int WM, int WN, bool MX>
static int launch_ln(const GemmLnArgs& a, hipStream_t st) {
    if (a.gstride == 0 || a.rows_per_group % BM == 0) return launch_ln_gu<BM, WM, WN, MX, true>(a, st);
    return launch_ln_gu<BM, WM, WN, MX, false>(a, st);
}

int gemm_resid_ln(const GemmLnArgs& a, hipStream_t st) {
    const bool mx = a.A8 != nullptr;                         // MXFP8 operands: A8/SA and W8/SW instead of A and W
    RALD_CHECK(a.M > 0 && a.K > 0 && a.K % (mx ? 128 : 64) == 0, "gemm_resid_ln: bad shape");
    RALD_CHECK(a.lda % 16 == 0 && a.ldw % 16 == 0 && a.lda >= a.K && a.ldw >= a.K, "gemm_resid_ln: leading dimensions");
    RALD_CHECK((mx ? (a.SA && a.W8 && a.SW) : (a.A && a.W)) && a.bias && a.x && (a.h || (a.h8 && a.hs)) && a.g && a.b && a.rows_per_group > 0,
               "gemm_resid_ln: null argument");
    RALD_CHECK(((uintptr_t)a.A % 16 == 0) && ((uintptr_t)a.W % 16 == 0) && ((uintptr_t)a.A8 % 16 == 0) && ((uintptr_t)a.W8 % 16 == 0) &&
               ((uintptr_t)a.x % 16 == 0) && ((uintptr_t)a.h % 16 == 0) && ((uintptr_t)a.g % 16 == 0) && ((uintptr_t)a.b % 16 == 0) &&
               a.gstride % 4 == 0, "gemm_resid_ln: 16-byte alignment");
    RALD_CHECK(!mx || (int64_t)a.M * (a.K / 32) < ((int64_t)1 << 31), "gemm_resid_ln: scale index overflow");
    RALD_CHECK(a.strideW == 0 || (!mx && a.w_rows % 128 == 0 && a.strideW % 8 == 0), "gemm_resid_ln: per-group weights need bf16 operands and groups of whole 128-row tiles");
    // 128-row tiles (all 160 KiB of LDS) when they cover the chip, 64-row tiles for smaller M
    if (cdiv(a.M, 128) >= 192) return mx ? launch_ln<128, 2, 4, true>(a, st) : launch_ln<128, 2, 4, false>(a, st);
    return mx ? launch_ln<64, 1, 8, true>(a, st) : launch_ln<64, 1, 8, false>(a, st);
}

int resid_gemm_ln(const GemmLnArgs& a, int n, float* scratch, hipStream_t st) {
    // (the batched fallback below runs M / w_rows whole groups; the product has M = B * n_latents)
    RALD_CHECK(a.strideW == 0 || (a.w_rows > 0 && a.M % a.w_rows == 0), "resid_gemm_ln: per-group weights need M to be a multiple of w_rows");
    const int splits = splitk_for(a.M, a.K);
    if (n == 512 && splits && !a.A8 && !a.h8 && a.strideW == 0)
        return resid_splitk_ln(a.A, a.lda, a.W, a.ldw, a.bias, a.x, a.g ? a.h : nullptr, a.g, a.b, a.gstride, a.rows_per_group, a.add_one, a.eps,
                               a.M, a.K, splits, scratch, st);
    if (n == 512 && a.g && gemm_resid_ln_pays(a.M, a.K)) return gemm_resid_ln(a, st);
    RALD_CHECK(!a.A8, "resid_gemm_ln: MXFP8 operands need the fused kernel");
    GemmArgs o = gemm_args(a.A, a.lda, a.W, a.ldw, a.x, n, a.bias, a.M, n, a.K);
    if (a.strideW) { o.M = a.w_rows; o.batch = a.M / a.w_rows; o.strideA = a.w_rows * a.lda; o.strideB = a.strideW; o.strideC = (int64_t)a.w_rows * n; }
    RALD_TRY(gemm_nt(o, EPI_RESID, st));
    if (!a.g) return 0;
    if (a.h8) return layernorm_mod_mx8(a.x, a.h8, a.hs, a.M, n, a.g, a.b, a.gstride, a.rows_per_group, a.add_one, a.eps, st);
    return layernorm_mod(a.x, a.h, a.M, n, a.g, a.b, a.gstride, a.rows_per_group, a.add_one, a.eps, st);
}

}  // namespace rald
