// NT bf16 GEMM on MFMA (v_mfma_f32_16x16x32_bf16), fp32 accumulate, fused epilogues.
//
//   C[b][m][n] = sum_k A[b][m][k] * B[b][n][k]      A: activations, B: weights ([out,in] as
//   torch.nn.Linear stores them) - both K-contiguous, which is exactly the MFMA fragment
//   order, so neither operand is ever transposed in memory.
//
// Two staging engines share one tile/epilogue design (BM x BN x 64, waves in a 2 x (WAVES/2) grid,
// 16x16 MFMA tiles, LDS rows of 128 B whose 16-byte chunks are XOR-swizzled by (row & 7) so every
// ds_read_b128 lane group is bank-conflict free; the swizzled read, the LDS-DMA staging and the tile
// walk are gemm_tile.h's, shared with the MXFP8 and residual+LayerNorm GEMMs):
//   * gemm_nt_kernel      register staging: global_load_dwordx4 -> VGPR -> ds_write_b128.  At 2
//                         workgroups/CU the ds_write path (~79 B/clk/CU) makes this LDS-bound.
//   * gemm_nt_glds_kernel LDS-DMA staging: global_load_lds_dwordx4 writes the tile straight into
//                         LDS (lane-linear destination; the swizzle is applied to each lane's
//                         SOURCE address and again on the read - CDNA guide rule 21), freeing the
//                         ds_write bandwidth and 32 staging VGPRs.
// The MFMA is issued with the weight fragment as the "A" operand so each lane ends up owning
// 4 CONSECUTIVE output columns of one row (D[i=n][j=m]: j = lane&15, i = 4*(lane>>4)+reg):
// the epilogue stores 8-byte (bf16) / 16-byte (f32) pieces instead of 2-byte scatters.
//
// Epilogues (what the reference does between two Linears, fused):
//   EPI_BF16   C_bf16 = alpha*acc + bias
//   EPI_F32    C_f32  = alpha*acc + bias
//   EPI_RESID  C_f32 += acc + bias                         (x = f(x) + x, residual stream in fp32)
//   EPI_GEGLU  C_bf16[m][c] = (acc_x + b_x) * gelu_erf(acc_g + b_g)   weights pre-packed so that
//              packed rows [32t,32t+16) are the 'x' half and [32t+16,32t+32) the 'gate' half of
//              output columns [16t,16t+16)  (models_radar_generation.py:93-95, models_ae.py:52-54)
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "common.h"
#include "kernels.h"
#include "gemm_epilogue.h"
#include "gemm_tile.h"

namespace rald {

// ---- epilogue: lane owns row m = mb + 16i + fr, 4 consecutive columns n = nb + 16j + 4*fq + {0..3}
template <int MT, int NT, int EPI>
__device__ __forceinline__ void gemm_epilogue(f32x4 (&acc)[MT][NT], const GemmArgs& a, int mb, int nb, int64_t coff, int fr, int fq) {
    if constexpr (EPI == EPI_GEGLU) {
        bf16* C = reinterpret_cast<bf16*>(a.C) + coff;
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const int m = mb + i * 16 + fr;
            if (m >= a.M) continue;
#pragma unroll
            for (int p = 0; p < NT / 2; ++p) {
                const int nx = nb + 32 * p + 4 * fq;           // packed row of the 'x' half
                const int ng = nx + 16;                        // packed row of the gate half
                float4 bx = *reinterpret_cast<const float4*>(a.bias + nx);
                float4 bg = *reinterpret_cast<const float4*>(a.bias + ng);
                f32x4 x = acc[i][2 * p], g = acc[i][2 * p + 1];
                bf16x4 o = pack4((x[0] + bx.x) * gelu_erf(g[0] + bg.x), (x[1] + bx.y) * gelu_erf(g[1] + bg.y),
                                 (x[2] + bx.z) * gelu_erf(g[2] + bg.z), (x[3] + bx.w) * gelu_erf(g[3] + bg.w));
                const int c = nb / 2 + 16 * p + 4 * fq;
                *reinterpret_cast<bf16x4*>(C + (int64_t)m * a.ldc + c) = o;
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const int m = mb + i * 16 + fr;
            if (m >= a.M) continue;
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int n = nb + j * 16 + 4 * fq;
                if (n >= a.N) continue;                        // N is a multiple of 4
                f32x4 v = acc[i][j];
                float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
                if (a.bias) b = *reinterpret_cast<const float4*>(a.bias + n);
                const float al = n < a.alpha_ncols ? a.alpha : 1.0f;
                if constexpr (EPI == EPI_BF16) {
                    bf16* C = reinterpret_cast<bf16*>(a.C) + coff;
                    *reinterpret_cast<bf16x4*>(C + (int64_t)m * a.ldc + n) =
                        pack4(al * v[0] + b.x, al * v[1] + b.y, al * v[2] + b.z, al * v[3] + b.w);
                } else if constexpr (EPI == EPI_F32) {
                    float* C = reinterpret_cast<float*>(a.C) + coff;
                    *reinterpret_cast<float4*>(C + (int64_t)m * a.ldc + n) =
                        make_float4(al * v[0] + b.x, al * v[1] + b.y, al * v[2] + b.z, al * v[3] + b.w);
                } else {  // EPI_RESID
                    float* C = reinterpret_cast<float*>(a.C) + coff;
                    float4* p = reinterpret_cast<float4*>(C + (int64_t)m * a.ldc + n);
                    float4 r = *p;
                    *p = make_float4(r.x + v[0] + b.x, r.y + v[1] + b.y, r.z + v[2] + b.z, r.w + v[3] + b.w);
                }
            }
        }
    }
}


// =================================================================================================
// register-staged engine (4 waves, 2x2)
// =================================================================================================
template <int BM, int BN, int EPI>
__global__ __launch_bounds__(256) void gemm_nt_kernel(GemmArgs a) {
    constexpr int BK = 64;
    constexpr int MT = BM / 32;   // 16-row m-tiles per wave
    constexpr int NT = BN / 32;   // 16-col n-tiles per wave
    constexpr int PA = BM / 32;   // staging passes (32 rows x 128 B per pass)
    constexpr int PB = BN / 32;
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * (BM + BN) * BK * 2];
    bf16x8* sA = reinterpret_cast<bf16x8*>(smem);                       // [2][BM][8 chunks]
    bf16x8* sB = reinterpret_cast<bf16x8*>(smem + 2 * BM * BK * 2);     // [2][BN][8 chunks]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
    int64_t oa, ob, coff;
    gemm_batch_offsets(a, blockIdx.z, oa, ob, coff);
    const bf16* A = a.A + oa;
    const bf16* B = a.B + ob;

    // staging coordinates: thread -> (row within pass, 16-byte chunk)
    const int srow = tid >> 3, schunk = tid & 7;
    const bf16* gA[PA];
    const bf16* gB[PB];
#pragma unroll
    for (int p = 0; p < PA; ++p) {
        int r = m0 + srow + 32 * p;
        r = r < a.M ? r : a.M - 1;                       // clamp: tail rows read valid memory
        gA[p] = A + (int64_t)r * a.lda + schunk * 8;
    }
#pragma unroll
    for (int p = 0; p < PB; ++p) {
        int r = n0 + srow + 32 * p;
        r = r < a.N ? r : a.N - 1;
        gB[p] = B + (int64_t)r * a.ldb + schunk * 8;
    }
    bf16x8 rA[PA], rB[PB];
    auto load_tile = [&](int kt) {
#pragma unroll
        for (int p = 0; p < PA; ++p) rA[p] = *reinterpret_cast<const bf16x8*>(gA[p] + kt * BK);
#pragma unroll
        for (int p = 0; p < PB; ++p) rB[p] = *reinterpret_cast<const bf16x8*>(gB[p] + kt * BK);
    };
    auto store_tile = [&](int buf) {
#pragma unroll
        for (int p = 0; p < PA; ++p) {
            int r = srow + 32 * p;
            sA[(buf * BM + r) * 8 + RALD_SWZ(r, schunk)] = rA[p];
        }
#pragma unroll
        for (int p = 0; p < PB; ++p) {
            int r = srow + 32 * p;
            sB[(buf * BN + r) * 8 + RALD_SWZ(r, schunk)] = rB[p];
        }
    };

    f32x4 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nk = a.K / BK;
    load_tile(0);
    store_tile(0);
    __syncthreads();
    const int fr = lane & 15, fq = lane >> 4;
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) load_tile(kt + 1);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            bf16x8 fa[MT], fb[NT];
            const int chunk = kk * 4 + fq;
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                int r = wm * (BM / 2) + i * 16 + fr;
                fa[i] = sA[(buf * BM + r) * 8 + RALD_SWZ(r, chunk)];
            }
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                int r = wn * (BN / 2) + j * 16 + fr;
                fb[j] = sB[(buf * BN + r) * 8 + RALD_SWZ(r, chunk)];
            }
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[j], fa[i], acc[i][j], 0, 0, 0);
        }
        if (kt + 1 < nk) store_tile(buf ^ 1);
        __syncthreads();
    }
    gemm_epilogue<MT, NT, EPI>(acc, a, m0 + wm * (BM / 2), n0 + wn * (BN / 2), coff, fr, fq);
}

// =================================================================================================
// LDS-DMA engine: WM x WN waves; NSTAGE LDS buffers
// =================================================================================================
template <int BM, int BN, int WM, int WN, int NSTAGE, int EPI>
__global__ __launch_bounds__(WM * WN * 64) void gemm_nt_glds_kernel(GemmArgs a) {
    constexpr int BK = 64;
    constexpr int WAVES = WM * WN;
    constexpr int MT = BM / (16 * WM);       // m-tiles per wave
    constexpr int NT = BN / (16 * WN);       // n-tiles per wave
    constexpr int CA = BM / 8 / WAVES;       // 1-KiB DMA pieces (8 rows x 128 B) per wave for A
    constexpr int CB = BN / 8 / WAVES;
    constexpr int STAGE_BYTES = (BM + BN) * BK * 2;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // [NSTAGE][A tile | B tile]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    int tm, tn;
    xcd_strip_tile(tm, tn);
    const int ntn = gridDim.x, nt = ntn * gridDim.y;
    int bz = blockIdx.z;
    if (nt < 8 && (gridDim.z & 7) == 0) {
        // batched problems of a few tiles each (the folded cross-attention: 2 x 2 tiles per sample, per-sample B operand): in launch order
        // a batch entry's tiles land on different XCDs and each re-reads the entry's operands from HBM.  Deal whole batch entries to the
        // XCDs instead: launch index g -> XCD g & 7, slot g >> 3 -> entry (slot / nt) * 8 + XCD, tile slot % nt.
        const int g = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        const int slot = g >> 3;
        bz = (slot / nt) * 8 + (g & 7);
        const int tl = slot % nt;
        tm = tl / ntn;
        tn = tl % ntn;
    }
    const int m0 = tm * BM, n0 = tn * BN;
    int64_t oa, ob, coff;
    gemm_batch_offsets(a, bz, oa, ob, coff);
    const bf16* A = a.A + oa;
    const bf16* B = a.B + ob;

    const int nk = a.K / BK;
    const bf16* gA[CA];
    const bf16* gB[CB];
    dma_sources<WAVES>(gA, A, a.lda, m0, a.M, wave, lane);
    dma_sources<WAVES>(gB, B, a.ldb, n0, a.N, wave, lane);
    auto stage = [&](int kt, int buf) { dma_stage<BM, WAVES>(gA, gB, kt, nk, smem + buf * STAGE_BYTES, wave); };

    f32x4 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int fr = lane & 15, fq = lane >> 4;
    // fragment reads of one 32-deep k sub-step (kk) of the tile in LDS buffer `buf`
    auto read_frags = [&](int buf, int kk, bf16x8 (&fa)[MT], bf16x8 (&fb)[NT]) {
        const bf16x8* sA = reinterpret_cast<const bf16x8*>(smem + buf * STAGE_BYTES);
        const bf16x8* sB = sA + BM * 8;
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
    };
    auto mfma_all = [&](const bf16x8 (&fa)[MT], const bf16x8 (&fb)[NT]) {
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[j], fa[i], acc[i][j], 0, 0, 0);
    };
    // Measured (round 3): the loop is matrix-pipe-bound at the power-limited clock - without any DMA after the prologue a k-step
    // still takes 1.25 us against 1.54 - and the same loop on v_mfma_f32_32x32x16_bf16 is 5-8 % slower.
    if constexpr (NSTAGE == 2) {
        // Software-pipelined main loop, rotated so that an iteration starts right AFTER a tile hand-over (barrier): nothing is
        // pending on the LDS counter at the loop head, so the compiler's waits inside the iteration are exact counts (round 2: the
        // loop head carried pending fragment reads and hipcc answered with lgkmcnt(0) in front of every first MFMA burst, i.e. the
        // 12 reads just issued were waited for before any MFMA could go - a third of a k-step with the matrix pipe idle).
        // The fragment registers are double-buffered: F0 = 32-deep sub-step 0 of a tile, F1 = sub-step 1.  An iteration:
        //   DMA of tile kt+1 into the buffer that tile kt-1 has just left | reads F0(kt) under the MFMAs of F1(kt-1) |
        //   reads F1(kt) under the MFMAs of F0(kt) | wait (tile kt+1 landed, my reads of tile kt done) + barrier.
        // The DMA issues and the LDS reads are spread between the MFMAs (sched_group_barrier) instead of in front of them.
        bf16x8 fa0[MT], fb0[NT], fa1[MT], fb1[NT];
        constexpr int W_ALL = 0x0070;                                                  // vmcnt(0) lgkmcnt(0), expcnt untouched
        constexpr int W_ST1 = ((CA + CB) & 15) | (((CA + CB) >> 4) << 14) | 0x0f70;    // vmcnt(CA+CB): the older stage has landed
        stage(0, 0);
        if (nk > 1) { stage(1, 1); __builtin_amdgcn_s_waitcnt(W_ST1); }
        else __builtin_amdgcn_s_waitcnt(W_ALL);
        __builtin_amdgcn_s_barrier();
        read_frags(0, 0, fa0, fb0);
        read_frags(0, 1, fa1, fb1);
        mfma_all(fa0, fb0);
        __builtin_amdgcn_s_waitcnt(W_ALL);
        __builtin_amdgcn_s_barrier();
        auto body = [&](int kt, auto with_dma) {
            const int cur = kt & 1;
            if constexpr (decltype(with_dma)::value) stage(kt + 1, cur ^ 1);
            read_frags(cur, 0, fa0, fb0);
            mfma_all(fa1, fb1);                                  // sub-step 1 of tile kt-1
            if constexpr (MT + NT == 12 && MT * NT == 32) {
                if constexpr (decltype(with_dma)::value) {
#pragma unroll
                    for (int g = 0; g < CA + CB; ++g) {          // 1 MFMA, then one DMA piece (8 x): the DMA goes out first, its latency is the long one
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                        __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);
                    }
#pragma unroll
                    for (int g = 0; g < 12; ++g) {               // 2 MFMAs, then one fragment read (12 x)
                        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
                        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                    }
                } else {
#pragma unroll
                    for (int g = 0; g < 12; ++g) {
                        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
                        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                    }
                    __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            read_frags(cur, 1, fa1, fb1);
            mfma_all(fa0, fb0);                                  // sub-step 0 of tile kt
            if constexpr (MT + NT == 12 && MT * NT == 32) {
#pragma unroll
                for (int g = 0; g < 12; ++g) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                }
                __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_waitcnt(W_ALL);                   // tile kt+1 landed; my reads of tile kt are done
            __builtin_amdgcn_s_barrier();
        };
        for (int kt = 1; kt + 1 < nk; ++kt) body(kt, std::true_type{});
        if (nk > 1) body(nk - 1, std::false_type{});
        mfma_all(fa1, fb1);                                      // sub-step 1 of the last tile
    } else {
#pragma unroll
        for (int s = 0; s < NSTAGE - 1; ++s)
            if (s < nk) stage(s, s);
        for (int kt = 0; kt < nk; ++kt) {
            // tile kt must have landed: allow the NSTAGE-2 younger tiles to stay in flight
            if (kt + NSTAGE - 2 < nk) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NSTAGE - 2) * (CA + CB)) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            asm volatile("" ::: "memory");
            __builtin_amdgcn_s_barrier();          // everyone's pieces of tile kt are in LDS; buffer (kt-1)%NSTAGE is free
            asm volatile("" ::: "memory");
            if (kt + NSTAGE - 1 < nk) stage(kt + NSTAGE - 1, (kt + NSTAGE - 1) % NSTAGE);
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                bf16x8 fa[MT], fb[NT];
                read_frags(kt % NSTAGE, kk, fa, fb);
                mfma_all(fa, fb);
            }
        }
    }
    if constexpr (NSTAGE != 2) {              // (the 2-stage loop ends on a barrier behind its last fragment reads)
        asm volatile("" ::: "memory");
        __builtin_amdgcn_s_barrier();         // every wave is done reading the staging buffers: reuse them as patches
        asm volatile("" ::: "memory");
    }
    gemm_epilogue_lds<MT, NT, EPI>(acc, a, m0 + wm * (BM / WM), n0 + wn * (BN / WN), coff, lane, smem + wave * EPI_PATCH_BYTES,
                                   reinterpret_cast<float*>(smem + WAVES * EPI_PATCH_BYTES) + wave * NT * 16);
}

// =================================================================================================
// persistent LDS-DMA engine: 256 x 256 x 64 tiles, 8 waves (4 x 2), 2 stages; one workgroup per CU walks its tiles
// =================================================================================================
// The one-tile kernel above spends a third of a K = 512 tile outside its k-loop (first stage, epilogue, dispatch), with every CU in the
// same phase at the same time.  Here workgroup w runs tiles w, w + grid, ... (through the same XCD strip walk, so each round of tiles is
// the set a plain launch runs together) and the next tile's stages 0 and 1 are issued BEFORE the epilogue's stores.  vmcnt is one
// in-order counter per wave for loads and stores, so the two duties go to different waves, fixed for the whole kernel:
//   waves 0-3  DMA waves:   every LDS-DMA piece of every stage (8 A + 8 B pieces per k-step) and the tile's bias row; no global store
//   waves 4-7  store waves: every global store of the epilogue; no VMEM load, and no vmcnt wait inside the tile loop
// (wave i and wave i + 4 share SIMD i & 3 if waves are placed round-robin: one of each kind per SIMD; speed only).  All eight waves run
// the MFMAs of the one-tile kernel on the same fragments, k-steps ascending from 0: every element's arithmetic is that kernel's.
// The stage buffers belong to the next tile during the epilogue, so the transpose patches live in the 31 KiB behind them.  One epilogue
// step = one 16-row m-tile (bf16 outputs: one 8-row half, a 16-row patch of 128 columns x 12 slots does not fit): every wave writes its
// patch, ONE workgroup barrier, each store wave writes out its own patch and that of DMA wave (wave - 4) as whole rows.  Twelve slots:
//   slots 4-7          a store wave's own patch: written and read by that wave alone (LDS operations of one wave execute in order), so no
//                      barrier orders it
//   slots 0-3, 8-11    DMA wave d's patch of step s in slot d + 8 (s & 1): the slot of step s + 1 was last read at step s - 1, i.e. before
//                      its readers arrived at barrier s, so behind barrier s the DMA waves go straight on to step s + 1 (arithmetic and
//                      patch write) while the store waves read and store step s
// Every barrier stands outside the role branch: all eight waves execute 4 (GEGLU) / 8 (bf16 outputs) per tile's epilogue.
// EPI_SOFTMAX64 (the folded cross-attention's scores) runs BATCHED: the tile index counts (batch entry, m-tile, n-tile) through
// batched_tile_at, each entry with its own operand bases; no bias.  The bf16 and GEGLU forms take one problem.
// Host contract (gemm_nt / the test entries): M % 256 == 0, N % 256 == 0, batch2 == 1, no out8; batch == 1 unless EPI_SOFTMAX64.
constexpr int PERSIST_LDS_BYTES = 160 * 1024;
// Launch-order index g of a one-tile launch's workgroup (grid ntn x ntm x nbatch) -> batch entry and tile: the mapping of
// gemm_nt_glds_kernel, restated on an index instead of blockIdx so that persistent workgroup w, taking g = w, w + grid, ..., runs round by
// round the tile sets that launch runs together (a batch entry's few tiles on one XCD, its operands crossing the fabric once).
__device__ __forceinline__ void batched_tile_at(int g, int ntn, int ntm, int nbatch, int& bz, int& tm, int& tn) {
    const int nt = ntn * ntm;
    if (nt < 8 && (nbatch & 7) == 0) {
        const int slot = g >> 3;
        bz = (slot / nt) * 8 + (g & 7);
        const int tl = slot % nt;
        tm = tl / ntn;
        tn = tl % ntn;
    } else {
        bz = g / nt;
        xcd_strip_tile_at(g - bz * nt, ntn, ntm, tm, tn);
    }
}
template <int EPI>
__global__ __launch_bounds__(512) void gemm_nt_persist_kernel(GemmArgs a) {
    static_assert(EPI == EPI_BF16 || EPI == EPI_GEGLU || EPI == EPI_SOFTMAX64, "the persistent engine is built for the three bf16-output epilogues");
    constexpr bool BATCHED = EPI == EPI_SOFTMAX64, BIAS = EPI != EPI_SOFTMAX64;
    constexpr int BM = 256, BN = 256, BK = 64, WN = 2, MT = 4, NT = 8;
    constexpr int DW = 4;                             // DMA waves
    constexpr int CP = BM / 8 / DW;                   // 1-KiB DMA pieces per operand per DMA wave and k-step
    constexpr int STAGE_BYTES = (BM + BN) * BK * 2;
    constexpr int OC = (EPI == EPI_GEGLU) ? NT * 8 : NT * 16;            // output columns of a wave
    constexpr int ROWB = OC * 2, STRIDE = ROWB + 16, LPR = ROWB / 16;    // as gemm_epilogue_lds
    constexpr int PR = (EPI == EPI_GEGLU) ? 16 : 8;                      // rows of a patch
    constexpr int PATCH = PR * STRIDE;
    constexpr int NSLOT = 12;                                            // 4 own + 2 x 4 partner patches
    constexpr int RPI = 64 / LPR;                                        // rows per store instruction
    constexpr int BIAS_OFF = 2 * STAGE_BYTES + 31 * 1024;                // the tile's 256 bias values
    static_assert(2 * STAGE_BYTES + NSLOT * PATCH <= BIAS_OFF && BIAS_OFF + BN * 4 <= PERSIST_LDS_BYTES && PR % RPI == 0 && (MT * 16 / PR) % 2 == 0,
                  "LDS plan; an even number of steps per tile keeps the slot parity across tiles");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // [2][A tile | B tile] [12 patch slots] ... [bias]
    float* tbias = reinterpret_cast<float*>(smem + BIAS_OFF);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const bool dma = wave < DW;
    const int ntm = a.M / BM, ntn = a.N / BN, nt = ntm * ntn * (BATCHED ? a.batch : 1);
    const int nk = a.K / BK;
    const int fr = lane & 15, fq = lane >> 4;

    // lane part of every DMA source address (bytes): row lane >> 3 of the piece, swizzled chunk; the piece and k-step parts are uniform
    const unsigned voA = (unsigned)((lane >> 3) * (int)a.lda + RALD_SWZ(lane >> 3, lane & 7) * 8) * 2u;
    const unsigned voB = (unsigned)((lane >> 3) * (int)a.ldb + RALD_SWZ(lane >> 3, lane & 7) * 8) * 2u;
    // One 1-KiB LDS-DMA piece: lane l's 16 bytes at base + voff go to LDS byte lds + 16 l.  Written as assembly so that the compiler's
    // wait-count pass does not see it: the roles are a run-time branch, and the pass - which merges both sides of a branch - would put a
    // vmcnt(0) in front of the LDS reads of ALL waves, the store waves' wait for their own stores included.  Every wait for a DMA in this
    // kernel is written out (W_ST1, hand_over).
    const unsigned lds0 = (unsigned)(uintptr_t)(lds_void*)smem;
    auto dma_piece = [&](const char* base, unsigned voff, unsigned lds) {
        asm volatile("s_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(base), "{m0}"(lds) : "memory");
    };
    // One tile: its batch entry's operand offsets (elements; 0 for the one-problem forms) and its first row and column
    struct Tile { int64_t oa, ob, oc; int m0, n0; };
    auto tile_at = [&](int t) {
        int bz = 0, tm, tn;
        if constexpr (BATCHED) batched_tile_at(t, ntn, ntm, a.batch, bz, tm, tn);
        else xcd_strip_tile_at(t, ntn, ntm, tm, tn);
        return Tile{bz * a.strideA, bz * a.strideB, bz * a.strideC, tm * BM, tn * BN};
    };
    // DMA wave d issues pieces d, d + 4, ... (tile rows 8 * piece .. + 7) of both operands
    auto stage = [&](const Tile& T, int kt, int buf) {
        const char* pa = reinterpret_cast<const char*>(a.A) + (T.oa + (int64_t)(T.m0 + 8 * wave) * a.lda + kt * BK) * 2;
        const char* pb = reinterpret_cast<const char*>(a.B) + (T.ob + (int64_t)(T.n0 + 8 * wave) * a.ldb + kt * BK) * 2;
        const unsigned s = lds0 + buf * STAGE_BYTES + wave * 1024;
#pragma unroll
        for (int p = 0; p < CP; ++p) dma_piece(pa + (int64_t)p * (8 * DW * 2) * a.lda, voA, s + p * DW * 1024);
#pragma unroll
        for (int p = 0; p < CP; ++p) dma_piece(pb + (int64_t)p * (8 * DW * 2) * a.ldb, voB, s + BM * 128 + p * DW * 1024);
    };
    auto read_frags = [&](int buf, int kk, bf16x8 (&fa)[MT], bf16x8 (&fb)[NT]) {
        const bf16x8* sA = reinterpret_cast<const bf16x8*>(smem + buf * STAGE_BYTES);
        const bf16x8* sB = sA + BM * 8;
        const int chunk = kk * 4 + fq;
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const int r = wm * (MT * 16) + i * 16 + fr;
            fa[i] = sA[r * 8 + RALD_SWZ(r, chunk)];
        }
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int r = wn * (NT * 16) + j * 16 + fr;
            fb[j] = sB[r * 8 + RALD_SWZ(r, chunk)];
        }
    };
    f32x4 acc[MT][NT];
    auto mfma_all = [&](const bf16x8 (&fa)[MT], const bf16x8 (&fb)[NT]) {
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[j], fa[i], acc[i][j], 0, 0, 0);
    };
    constexpr int W_ALL = 0x0070;                                        // vmcnt(0) lgkmcnt(0), expcnt untouched
    constexpr int W_LGKM = 0xc07f;                                       // lgkmcnt(0) only
    constexpr int W_ST1 = ((2 * CP) & 15) | (((2 * CP) >> 4) << 14) | 0x0070;   // vmcnt(2 CP) lgkmcnt(0): the older of two stages has landed
    // tile hand-over: the DMA waves' pieces have landed, everybody's fragment reads are done.  The store waves have nothing but their own
    // output stores on vmcnt and never wait for them.
    auto hand_over = [&]() {
        if (dma) __builtin_amdgcn_s_waitcnt(W_ALL);
        else __builtin_amdgcn_s_waitcnt(W_LGKM);
        __builtin_amdgcn_s_barrier();
    };
    // one k-step of the one-tile kernel's rotated loop (see there); the DMA waves issue the next stage first
    bf16x8 fa0[MT], fb0[NT], fa1[MT], fb1[NT];
    auto body = [&](const Tile& T, int kt, bool with_dma) {
        const int cur = kt & 1;
        if (with_dma && dma) stage(T, kt + 1, cur ^ 1);
        __builtin_amdgcn_sched_barrier(0);
        read_frags(cur, 0, fa0, fb0);
        mfma_all(fa1, fb1);                                  // sub-step 1 of k-step kt-1
#pragma unroll
        for (int g = 0; g < 12; ++g) {                       // 2 MFMAs, then one fragment read (12 x)
            __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);
        __builtin_amdgcn_sched_barrier(0);
        read_frags(cur, 1, fa1, fb1);
        mfma_all(fa0, fb0);                                  // sub-step 0 of k-step kt
#pragma unroll
        for (int g = 0; g < 12; ++g) {
            __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);
        __builtin_amdgcn_sched_barrier(0);
        hand_over();
    };

    if constexpr (BIAS)
        if (!a.bias && tid < BN / 4) *reinterpret_cast<float4*>(tbias + 4 * tid) = make_float4(0.f, 0.f, 0.f, 0.f);
    int t = blockIdx.x;                                      // launch-order index of the tile in the virtual ntn x ntm (x batch) grid
    Tile T = tile_at(t);
    if (dma) {
        stage(T, 0, 0);
        if (nk > 1) stage(T, 1, 1);
    }
    for (;;) {
        // stages 0 and 1 of this tile are in flight (DMA waves), issued under the previous tile's epilogue
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (dma) {
            if (nk > 1) __builtin_amdgcn_s_waitcnt(W_ST1);
            else __builtin_amdgcn_s_waitcnt(W_ALL);
        } else __builtin_amdgcn_s_waitcnt(W_LGKM);
        __builtin_amdgcn_s_barrier();
        // the tile's bias row, one 1-KiB piece: behind the barrier nobody reads the previous tile's any more, and the DMA waves' next
        // hand-over wait covers it
        if constexpr (BIAS)
            if (wave == 0 && a.bias) dma_piece(reinterpret_cast<const char*>(a.bias + T.n0), 16u * lane, lds0 + BIAS_OFF);
        read_frags(0, 0, fa0, fb0);
        read_frags(0, 1, fa1, fb1);
        mfma_all(fa0, fb0);
        hand_over();
        for (int kt = 1; kt + 1 < nk; ++kt) body(T, kt, true);
        if (nk > 1) body(T, nk - 1, false);
        // both stage buffers are free (the loop ends on a barrier behind its last fragment reads): the next tile's first two stages go
        // out before any store of this one
        const int tnext = t + gridDim.x;
        Tile Tn = T;
        if (tnext < nt) {
            Tn = tile_at(tnext);
            if (dma) {
                stage(Tn, 0, 0);
                if (nk > 1) stage(Tn, 1, 1);
            }
        }
        mfma_all(fa1, fb1);                                  // sub-step 1 of the last k-step

        // ---- epilogue: the arithmetic and rounding of gemm_epilogue_lds.  Its first patch write lies behind this tile's k-loop barriers and
        // so behind the store waves' last patch reads of the previous tile (which they finished before they came to that tile loop's first
        // barrier): no barrier of its own orders it.
        {
            int lane_e = lane;                                // opaque: the epilogue's lane addresses are made here, not kept across the k-loops
            asm volatile("" : "+v"(lane_e));
            const int fr = lane_e & 15, fq = lane_e >> 4;
            unsigned char* slot0 = smem + 2 * STAGE_BYTES + wave * PATCH;      // even steps (and every step of a store wave): slot `wave`
            unsigned char* slot1 = slot0 + (dma ? 8 * PATCH : 0);              // odd steps of a DMA wave: slot wave + 8
            const int mb = T.m0 + wm * (MT * 16), nb = T.n0 + wn * (NT * 16);
            const int oc0 = (EPI == EPI_GEGLU) ? nb / 2 : nb;
            const float* wbias = tbias + wn * (NT * 16);
            bf16* C = reinterpret_cast<bf16*>(a.C) + T.oc;
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                bf16x4 sm[EPI == EPI_SOFTMAX64 ? NT : 1];
                if constexpr (EPI == EPI_SOFTMAX64) {
                    // all 16 rows of the m-tile at once (the cross-lane steps want every lane): row fr's 64 columns of a group = 4 n-tiles x
                    // the 4 lanes fr, fr + 16, fr + 32, fr + 48; the two 8-row steps below only write their half
#pragma unroll
                    for (int g = 0; g < NT / 4; ++g) {
                        float e[16];
                        float mx = -3.0e38f;
#pragma unroll
                        for (int q = 0; q < 4; ++q)
#pragma unroll
                            for (int c = 0; c < 4; ++c) { e[4 * q + c] = a.alpha * acc[i][4 * g + q][c]; mx = fmaxf(mx, e[4 * q + c]); }
                        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
                        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
                        float su = 0.f;
#pragma unroll
                        for (int q = 0; q < 16; ++q) { e[q] = __builtin_amdgcn_exp2f(e[q] - mx); su += e[q]; }
                        su += __shfl_xor(su, 16, 64);
                        su += __shfl_xor(su, 32, 64);
                        const float inv = 1.0f / su;
#pragma unroll
                        for (int q = 0; q < 4; ++q) sm[4 * g + q] = pack4(e[4 * q] * inv, e[4 * q + 1] * inv, e[4 * q + 2] * inv, e[4 * q + 3] * inv);
                    }
                }
#pragma unroll
                for (int h = 0; h < 16 / PR; ++h) {
                    const int odd = (i * (16 / PR) + h) & 1;    // parity of the step within the tile
                    unsigned char* patch = odd ? slot1 : slot0;
                    asm volatile("" ::: "memory");
                    if (PR == 16 || (fr >> 3) == h) {
                        const int pr = fr & (PR - 1);
                        if constexpr (EPI == EPI_GEGLU) {
#pragma unroll
                            for (int p = 0; p < NT / 2; ++p) {
                                const float4 bx = *reinterpret_cast<const float4*>(wbias + 32 * p + 4 * fq);
                                const float4 bg = *reinterpret_cast<const float4*>(wbias + 32 * p + 4 * fq + 16);
                                const f32x4 x = acc[i][2 * p], g = acc[i][2 * p + 1];
                                const f32x2 g01 = gelu_poly2(f32x2{g[0] + bg.x, g[1] + bg.y});
                                const f32x2 g23 = gelu_poly2(f32x2{g[2] + bg.z, g[3] + bg.w});
                                const f32x2 o01 = f32x2{x[0] + bx.x, x[1] + bx.y} * g01;
                                const f32x2 o23 = f32x2{x[2] + bx.z, x[3] + bx.w} * g23;
                                *reinterpret_cast<bf16x4*>(patch + pr * STRIDE + (16 * p + 4 * fq) * 2) = pack4(o01[0], o01[1], o23[0], o23[1]);
                            }
                        } else if constexpr (EPI == EPI_SOFTMAX64) {
#pragma unroll
                            for (int j = 0; j < NT; ++j) *reinterpret_cast<bf16x4*>(patch + pr * STRIDE + (16 * j + 4 * fq) * 2) = sm[j];
                        } else {
#pragma unroll
                            for (int j = 0; j < NT; ++j) {
                                const int n = nb + j * 16 + 4 * fq;
                                const float4 b = *reinterpret_cast<const float4*>(wbias + 16 * j + 4 * fq);
                                const f32x4 v = acc[i][j];
                                const float al = n < a.alpha_ncols ? a.alpha : 1.0f;
                                const float o0 = al * v[0] + b.x, o1 = al * v[1] + b.y, o2 = al * v[2] + b.z, o3 = al * v[3] + b.w;
                                *reinterpret_cast<bf16x4*>(patch + pr * STRIDE + (16 * j + 4 * fq) * 2) = pack4(o0, o1, o2, o3);
                            }
                        }
                    }
                    asm volatile("" ::: "memory");
                    __builtin_amdgcn_s_waitcnt(W_LGKM);        // my patch is in LDS
                    asm volatile("" ::: "memory");
                    // lane -> (row lane / LPR, 16-byte piece lane % LPR) of the rows going out
                    const int r = lane_e / LPR, pc = lane_e % LPR;
                    uint4 v[2][PR / RPI];
                    if (!dma) {
                        // a store wave's own patch: private to the wave, read back with no workgroup barrier in between
#pragma unroll
                        for (int q = 0; q < PR / RPI; ++q) v[0][q] = *reinterpret_cast<const uint4*>(slot0 + (q * RPI + r) * STRIDE + pc * 16);
                    }
                    asm volatile("" ::: "memory");
                    __builtin_amdgcn_s_barrier();              // the step's one barrier: the DMA waves' patches of this step are written
                    asm volatile("" ::: "memory");
                    if (!dma) {
                        // DMA wave (wave - 4)'s patch of this step: 128 rows up, same columns.  All reads first, then the stores.
                        const unsigned char* partner = slot0 - DW * PATCH + (odd ? 8 * PATCH : 0);
#pragma unroll
                        for (int q = 0; q < PR / RPI; ++q) v[1][q] = *reinterpret_cast<const uint4*>(partner + (q * RPI + r) * STRIDE + pc * 16);
#pragma unroll
                        for (int w2 = 0; w2 < 2; ++w2)
#pragma unroll
                            for (int q = 0; q < PR / RPI; ++q) {
                                const int m = mb - w2 * (BM / 2) + i * 16 + h * PR + q * RPI + r;
                                bf16* Cp = C + (int64_t)m * a.ldc + oc0 + pc * 8;
                                typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
                                const u32x4 vv = u32x4{v[w2][q].x, v[w2][q].y, v[w2][q].z, v[w2][q].w};
                                // streamed output, the policy of gemm_epilogue_lds under GEMM_NT_STORE (which gemm_nt always sets).  The s_nop
                                // is the hazard the compiler cannot see through the asm: a VALU write to the data registers of a store of
                                // more than 8 bytes needs two wait states behind it (without it the next row's address arithmetic, placed in
                                // v[data] directly behind the store, reached memory in 16 lanes of the row: found by the bit-equality test)
                                asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1 nt\n\ts_nop 1" ::"v"(Cp), "v"(vv) : "memory");
                            }
                    }
                    // no second barrier: the next step's patches go to the other partner slots, and a store wave's own slot is its own
                    asm volatile("" ::: "memory");
                }
            }
        }
        if (tnext >= nt) break;
        t = tnext;
        T = Tn;
    }
}

// -------------------------------------------------------------------------------------------------
template <int BM, int BN>
static int launch_tile(const GemmArgs& a, int epi, hipStream_t st) {
    dim3 grid(cdiv(a.N, BN), cdiv(a.M, BM), a.batch * a.batch2);
    switch (epi) {
        case EPI_BF16:  hipLaunchKernelGGL((gemm_nt_kernel<BM, BN, EPI_BF16>), grid, dim3(256), 0, st, a); break;
        case EPI_F32:   hipLaunchKernelGGL((gemm_nt_kernel<BM, BN, EPI_F32>), grid, dim3(256), 0, st, a); break;
        case EPI_RESID: hipLaunchKernelGGL((gemm_nt_kernel<BM, BN, EPI_RESID>), grid, dim3(256), 0, st, a); break;
        case EPI_GEGLU: hipLaunchKernelGGL((gemm_nt_kernel<BM, BN, EPI_GEGLU>), grid, dim3(256), 0, st, a); break;
        default: set_error("gemm: bad epilogue"); return 1;
    }
    RALD_HIP(hipGetLastError());
    return 0;
}

template <int BM, int BN, int WM, int WN, int NSTAGE, int EPI>
static int launch_glds_epi(const GemmArgs& a, hipStream_t st) {
    constexpr int WAVES = WM * WN;
    constexpr int smem = NSTAGE * (BM + BN) * 64 * 2;
    static_assert(smem >= epi_lds_bytes<BN / (16 * WN)>(WAVES), "epilogue patches and bias slots must fit in the staging buffers");
    static bool raised = false;
    return launch_dyn_lds(gemm_nt_glds_kernel<BM, BN, WM, WN, NSTAGE, EPI>, raised, dim3(cdiv(a.N, BN), cdiv(a.M, BM), a.batch * a.batch2), WAVES * 64, smem, st, a);
}
template <int BM, int BN, int WM, int WN, int NSTAGE>
static int launch_glds(const GemmArgs& a, int epi, hipStream_t st) {
    switch (epi) {
        case EPI_BF16:  return launch_glds_epi<BM, BN, WM, WN, NSTAGE, EPI_BF16>(a, st);
        case EPI_F32:   return launch_glds_epi<BM, BN, WM, WN, NSTAGE, EPI_F32>(a, st);
        case EPI_RESID: return launch_glds_epi<BM, BN, WM, WN, NSTAGE, EPI_RESID>(a, st);
        case EPI_GEGLU: return launch_glds_epi<BM, BN, WM, WN, NSTAGE, EPI_GEGLU>(a, st);
        case EPI_F16S:
            if constexpr ((BM == 64 && BN == 64) || (BM == 128 && BN == 128 && NSTAGE == 2)) return launch_glds_epi<BM, BN, WM, WN, NSTAGE, EPI_F16S>(a, st);
            else { set_error("gemm: the fp16-slab epilogue is built for the 64x64 ring and the 128x128 LDS-DMA engines"); return 1; }
        case EPI_SOFTMAX64:
            if constexpr ((BN / WN) % 64 == 0 && BM >= 128) return launch_glds_epi<BM, BN, WM, WN, NSTAGE, EPI_SOFTMAX64>(a, st);
            else { set_error("gemm: the softmax epilogue needs waves of 64-column groups"); return 1; }
        default: set_error("gemm: bad epilogue"); return 1;
    }
}

// CUs of the current device, asked once per device and cached: launches inside a stream capture find the value there
static int cu_count(int& cus) {
    static int cached[64] = {};
    int dev = 0;
    RALD_HIP(hipGetDevice(&dev));
    RALD_CHECK(dev >= 0 && dev < 64, "gemm: device index out of range");
    if (cached[dev] == 0) RALD_HIP(hipDeviceGetAttribute(&cached[dev], hipDeviceAttributeMultiprocessorCount, dev));
    cus = cached[dev];
    return 0;
}
// one workgroup per CU (at most max_workgroups), each walking its tiles
static int launch_persist(const GemmArgs& a, int epi, int max_workgroups, hipStream_t st) {
    int cus = 0;
    if (int rc = cu_count(cus)) return rc;
    const int64_t tiles = (int64_t)(a.M / 256) * (a.N / 256) * a.batch;
    RALD_CHECK(tiles < (1ll << 30), "gemm: too many tiles for the persistent engine's tile index");
    const int grid = (int)std::min<int64_t>(tiles, std::min(cus, max_workgroups));
    RALD_CHECK(grid >= 1, "gemm: the persistent engine needs at least one workgroup");
    static bool raised_bf16 = false, raised_geglu = false, raised_softmax = false;
    switch (epi) {
        case EPI_SOFTMAX64: return launch_dyn_lds(gemm_nt_persist_kernel<EPI_SOFTMAX64>, raised_softmax, dim3(grid), 512, PERSIST_LDS_BYTES, st, a);
        case EPI_BF16:  return launch_dyn_lds(gemm_nt_persist_kernel<EPI_BF16>, raised_bf16, dim3(grid), 512, PERSIST_LDS_BYTES, st, a);
        case EPI_GEGLU: return launch_dyn_lds(gemm_nt_persist_kernel<EPI_GEGLU>, raised_geglu, dim3(grid), 512, PERSIST_LDS_BYTES, st, a);
        default: set_error("gemm: the persistent engine has the bf16, GEGLU and softmax epilogues"); return 1;
    }
}

int f16_saturation_gemm(unsigned* count, bool reset) {
    RALD_HIP(hipMemcpyFromSymbol(count, HIP_SYMBOL(g_f16_sat_gemm), sizeof(unsigned)));
    if (reset) { const unsigned z = 0; RALD_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_f16_sat_gemm), &z, sizeof(unsigned))); }
    return 0;
}

// Host-side shape contract is checked here, before any launch (an out-of-bounds MFMA tile
// can take the whole node down, so nothing is left to the kernel).
int gemm_nt(const GemmArgs& a0, int epi, hipStream_t st) {
    // bf16 outputs are streamed (written once, read by the next kernel after the whole tensor has
    // passed through): non-temporal stores keep them from evicting the weight panels out of L2.
    GemmArgs a = a0;
    a.flags |= GEMM_NT_STORE;
    RALD_CHECK(a.M > 0 && a.N > 0 && a.K > 0 && a.batch > 0 && a.batch2 > 0, "gemm: empty problem");
    const int64_t nbatch = (int64_t)a.batch * a.batch2;
    RALD_CHECK(nbatch <= 65535, "gemm: batch * batch2 exceeds the grid z limit");
    RALD_CHECK(a.K % 64 == 0, "gemm: K must be a multiple of 64 (pad with zeros)");
    RALD_CHECK(a.N % 4 == 0, "gemm: N must be a multiple of 4");
    RALD_CHECK(a.lda % 8 == 0 && a.ldb % 8 == 0, "gemm: lda/ldb must be multiples of 8 elements (16-byte rows)");
    RALD_CHECK(a.lda >= a.K && a.ldb >= a.K, "gemm: leading dimension smaller than K");
    RALD_CHECK(((uintptr_t)a.A % 16 == 0) && ((uintptr_t)a.B % 16 == 0) && ((uintptr_t)a.C % 16 == 0), "gemm: pointers must be 16-byte aligned");
    RALD_CHECK(a.ldc % 4 == 0, "gemm: ldc must be a multiple of 4");
    if (epi == EPI_GEGLU) {
        RALD_CHECK(a.N % 128 == 0 && a.bias != nullptr, "gemm: GEGLU needs N % 128 == 0 and a packed bias");
        RALD_CHECK(a.ldc >= a.N / 2, "gemm: GEGLU ldc < N/2");
    } else {
        RALD_CHECK(a.ldc >= a.N, "gemm: ldc < N");
    }
    if (epi == EPI_F16S) {                                        // split-K slabs (resid_splitk_ln): the 64x64 ring or 128x128 tiles, as EPI_F32 would get
        RALD_CHECK(!a.out8 && a.N % 8 == 0, "gemm: the fp16-slab epilogue needs N % 8 == 0");
        const int64_t w128 = (int64_t)cdiv(a.M, 128) * cdiv(a.N, 128) * nbatch, w64 = (int64_t)cdiv(a.M, 64) * cdiv(a.N, 64) * nbatch;
        RALD_CHECK(w128 >= 192 || w64 <= 256, "gemm: fp16 slabs are not built for the register-staged engine (ask gemm_f16s_ok first)");
        if (w128 >= 192) return launch_glds<128, 128, 2, 2, 2>(a, epi, st);
        return launch_glds<64, 64, 2, 2, 8>(a, epi, st);
    }
    if (epi == EPI_SOFTMAX64) {
        // whole tiles only: every wave normalises complete 64-column groups of complete rows
        RALD_CHECK(a.M % 128 == 0 && a.N % 128 == 0 && !a.bias && !a.out8 && a.alpha_ncols >= a.N, "gemm: the softmax epilogue needs M, N % 128 == 0 and no bias");
        if (a.M % 256 == 0 && a.N % 256 == 0) {
            const int64_t wg256 = (int64_t)(a.M / 256) * (a.N / 256) * nbatch;
            if (a.batch2 == 1) {
                // two or more tiles per CU, batch entries included: the persistent tile loop, batched
                int cus = 0;
                if (int rc = cu_count(cus)) return rc;
                if (wg256 >= 2 * (int64_t)cus) return launch_persist(a, epi, 1 << 30, st);
            }
            if (wg256 >= 256) return launch_glds<256, 256, 4, 2, 2>(a, epi, st);
        }
        return launch_glds<128, 128, 2, 2, 2>(a, epi, st);
    }
    if (a.out8) {
        RALD_CHECK(epi == EPI_GEGLU && a.outs && a.batch * a.batch2 == 1 && a.M % 256 == 0 && a.N % 256 == 0 && (a.N / 2) % 32 == 0 &&
                   (int64_t)(a.M / 256) * (a.N / 256) >= 256, "gemm: the MXFP8 output form needs the GEGLU epilogue on full 256x256 tiles");
        return launch_glds<256, 256, 4, 2, 2>(a, epi, st);
    }
    // engine selection: register-staged 64x64 tiles or the 64x64 LDS-DMA ring for the small-M (batch-1) regime, LDS-DMA 256x256 tiles
    // (8 waves) when they give every CU at least one tile, LDS-DMA 64x128 (3 stages) for 192-320 tiles of 128x128, LDS-DMA 128x128
    // (4 waves, 2 workgroups/CU) otherwise.
    const int64_t wg128 = (int64_t)cdiv(a.M, 128) * cdiv(a.N, 128) * nbatch;
    if (wg128 < 192) {
        // small-M (batch-1) regime: too few tiles to hide memory latency behind other workgroups, so put
        // (up to) the whole K extent in flight at once: 64x64 tiles, 8-stage LDS-DMA ring (128 KB).
        const int64_t wg64 = (int64_t)cdiv(a.M, 64) * cdiv(a.N, 64) * nbatch;
        if (wg64 > 256) return launch_tile<64, 64>(a, epi, st);   // more than one tile per CU: 5 small workgroups/CU hide latency
        return launch_glds<64, 64, 2, 2, 8>(a, epi, st);
    }
    const int64_t wg256 = (int64_t)(a.M / 256) * (a.N / 256) * nbatch;
    if (a.M % 256 == 0 && a.N % 256 == 0 && wg256 >= 256) {
        // two or more tiles per CU: the persistent tile loop
        if (nbatch == 1 && (epi == EPI_BF16 || epi == EPI_GEGLU)) {
            int cus = 0;
            if (int rc = cu_count(cus)) return rc;
            if (wg256 >= 2 * (int64_t)cus) return launch_persist(a, epi, 1 << 30, st);
        }
        return launch_glds<256, 256, 4, 2, 2>(a, epi, st);
    }
    // 192-320 tiles of 128 x 128 = about one 4-wave workgroup per CU, walking its k-steps as a latency chain (N = 512 projections at
    // M = 8192: 19-21 us for 4.3 GFLOP).  64 x 128 tiles with 3 stages give two workgroups per CU and a deeper prefetch: NFE at
    // B = 16 4.63 -> 4.36 ms, B = 8 2.94 -> 2.90 ms against 128 x 128 tiles.
    if (epi != EPI_GEGLU && wg128 <= 320 && a.M % 64 == 0) return launch_glds<64, 128, 2, 2, 3>(a, epi, st);
    return launch_glds<128, 128, 2, 2, 2>(a, epi, st);
}

// Test entry: one full-tile bf16 problem on the 256 x 256 LDS-DMA tiles whatever the tile count - the persistent engine with a grid cap,
// or the one-tile kernel (persistent == 0) - so that tests reach both at small shapes.
int gemm_nt_256_test(const GemmArgs& a0, int epi, int persistent, int max_workgroups, hipStream_t st) {
    GemmArgs a = a0;
    a.flags |= GEMM_NT_STORE;
    RALD_CHECK(epi == EPI_BF16 || epi == EPI_GEGLU, "gemm_nt_256_test: EPI_BF16 or EPI_GEGLU");
    RALD_CHECK(a.M > 0 && a.N > 0 && a.K > 0 && a.M % 256 == 0 && a.N % 256 == 0 && a.K % 64 == 0, "gemm_nt_256_test: M, N % 256 == 0 and K % 64 == 0");
    RALD_CHECK(a.batch == 1 && a.batch2 == 1 && !a.out8, "gemm_nt_256_test: one problem, bf16 output");
    RALD_CHECK(a.lda % 8 == 0 && a.ldb % 8 == 0 && a.lda >= a.K && a.ldb >= a.K, "gemm_nt_256_test: lda/ldb must be multiples of 8 and at least K");
    RALD_CHECK(((uintptr_t)a.A % 16 == 0) && ((uintptr_t)a.B % 16 == 0) && ((uintptr_t)a.C % 16 == 0) && ((uintptr_t)a.bias % 16 == 0),
               "gemm_nt_256_test: pointers must be 16-byte aligned");
    RALD_CHECK(a.ldc % 8 == 0 && a.ldc >= (epi == EPI_GEGLU ? a.N / 2 : a.N), "gemm_nt_256_test: ldc");
    RALD_CHECK(epi != EPI_GEGLU || a.bias, "gemm_nt_256_test: GEGLU needs a packed bias");
    RALD_CHECK(max_workgroups >= 1, "gemm_nt_256_test: max_workgroups must be at least 1");
    if (persistent) return launch_persist(a, epi, max_workgroups, st);
    return launch_glds<256, 256, 4, 2, 2>(a, epi, st);
}

// Test entry with a batch: gemm_nt_256_test's problem `batch` times over (entry b at A + b strideA, B + b strideB, C + b strideC; strideA or
// strideB 0 = shared), and EPI_SOFTMAX64 beside the two others.  The persistent engine is batched for EPI_SOFTMAX64 only: a batch of the
// other two runs on the one-tile kernel (persistent == 0).  Every argument is checked here, before the first HIP call.
int gemm_nt_256_batched_test(const GemmArgs& a0, int epi, int persistent, int max_workgroups, hipStream_t st) {
    GemmArgs a = a0;
    a.flags |= GEMM_NT_STORE;
    RALD_CHECK(epi == EPI_BF16 || epi == EPI_GEGLU || epi == EPI_SOFTMAX64, "gemm_nt_256_batched_test: EPI_BF16, EPI_GEGLU or EPI_SOFTMAX64");
    RALD_CHECK(a.M > 0 && a.N > 0 && a.K > 0 && a.M % 256 == 0 && a.N % 256 == 0 && a.K % 64 == 0,
               "gemm_nt_256_batched_test: M, N % 256 == 0 and K % 64 == 0 (full tiles only)");
    RALD_CHECK(a.batch >= 1 && a.batch <= 65535 && !a.out8, "gemm_nt_256_batched_test: 1 <= batch <= 65535, bf16 output");
    RALD_CHECK(a.batch2 == 1, "gemm_nt_256_batched_test: batch2 must be 1 (the engine has no inner batch)");
    RALD_CHECK(a.lda % 8 == 0 && a.ldb % 8 == 0 && a.lda >= a.K && a.ldb >= a.K, "gemm_nt_256_batched_test: lda/ldb must be multiples of 8 and at least K");
    RALD_CHECK(((uintptr_t)a.A % 16 == 0) && ((uintptr_t)a.B % 16 == 0) && ((uintptr_t)a.C % 16 == 0) && ((uintptr_t)a.bias % 16 == 0),
               "gemm_nt_256_batched_test: pointers must be 16-byte aligned");
    const int ncols = epi == EPI_GEGLU ? a.N / 2 : a.N;
    RALD_CHECK(a.ldc % 8 == 0 && a.ldc >= ncols, "gemm_nt_256_batched_test: ldc");
    RALD_CHECK(a.strideA >= 0 && a.strideB >= 0 && a.strideA % 8 == 0 && a.strideB % 8 == 0 && a.strideC % 8 == 0,
               "gemm_nt_256_batched_test: strides must be non-negative multiples of 8 elements");
    RALD_CHECK(a.batch == 1 || a.strideC >= (int64_t)(a.M - 1) * a.ldc + ncols, "gemm_nt_256_batched_test: strideC lets the outputs of two entries overlap");
    RALD_CHECK(epi != EPI_GEGLU || a.bias, "gemm_nt_256_batched_test: GEGLU needs a packed bias");
    RALD_CHECK(epi != EPI_SOFTMAX64 || (!a.bias && a.alpha_ncols >= a.N), "gemm_nt_256_batched_test: the softmax epilogue takes no bias and one alpha");
    RALD_CHECK(max_workgroups >= 1, "gemm_nt_256_batched_test: max_workgroups must be at least 1");
    RALD_CHECK(!persistent || a.batch == 1 || epi == EPI_SOFTMAX64, "gemm_nt_256_batched_test: the persistent engine is batched for EPI_SOFTMAX64 only");
    if (persistent) return launch_persist(a, epi, max_workgroups, st);
    return launch_glds<256, 256, 4, 2, 2>(a, epi, st);
}

}  // namespace rald
