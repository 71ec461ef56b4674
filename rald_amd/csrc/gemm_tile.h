// The LDS-DMA tile engine of the bf16 (gemm.hip), MXFP8 (gemm_fp8.hip) and residual+LayerNorm (gemm_ln.hip) GEMMs: device helpers only.
//
// One k-step of one operand row is 128 BYTES (64 bf16 or 128 e4m3), so the LDS layout and the piece mapping are the same for both
// element types and the helpers serve both.
// An LDS stage is [A tile | B tile], rows of 128 B = 8 chunks of 16 B; logical chunk c of row r lives in physical chunk c ^ (r & 7), so
// every ds_read_b128 lane group is bank-conflict free.  global_load_lds writes lane-linear (one wave instruction = 1 KiB = 8 rows), so
// the XOR goes on each lane's SOURCE address and again on the fragment read (CDNA guide rule 21).
#pragma once
#include "common.h"

namespace rald {

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

// The swizzle: physical 16-byte chunk of logical chunk `chunk` in LDS row `row`.  A macro, not a function: the bf16 loops keep their
// registers and instruction selection only when the expression is optimised inside its caller (as a helper function, a swizzled read
// cost the 128x128 bf16 loop 5 VGPRs and two VALU address adds per sub-step).  A bf16 fragment is tile[row * 8 + RALD_SWZ(row, chunk)].
#define RALD_SWZ(row, chunk) ((chunk) ^ ((row) & 7))

// ---- tile walk ---------------------------------------------------------------------------------------------------------------------
// XCD-aware tile order (speed only): workgroups are dealt round-robin over the 8 XCDs, so the blocks with equal id%8 share an L2.  Give
// each of those 8 groups a CONTIGUOUS span of the tile walk (bijective for any grid size, guide 5 q/r form), and walk the tiles in column
// STRIPS of GN n-tiles (n fastest inside a strip, then m, then the next strip): the 32 tiles an XCD runs at once then share <= GN weight
// panels (2 MB at GN = 8, 256-row tiles, K = 512) that stay in its 4 MB L2 while the A panels stream through.  Row-major order re-fetched
// the whole 4 MB FF1 weight matrix for every round of tiles (measured: 296 MB fetched vs 37.5 MB algorithmic).
// `lin` is the workgroup's launch-order index in a grid of ntn x ntm tiles (the persistent GEMM passes virtual ones: its workgroup w takes
// lin = w, w + grid, ... and so runs, round by round, the tile sets a one-tile-per-workgroup launch runs).
__device__ __forceinline__ void xcd_strip_tile_at(int lin, int ntn, int ntm, int& tm, int& tn) {
    const int nt = ntn * ntm;
    const int xcd = lin & 7, q = nt >> 3, rr = nt & 7;
    const int tile = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + (lin >> 3);
    constexpr int GN = 8;
    if (ntn % GN == 0) {
        const int strip = tile / (ntm * GN), within = tile % (ntm * GN);
        tm = within / GN;
        tn = strip * GN + within % GN;
    } else {
        tm = tile / ntn;
        tn = tile % ntn;
    }
}
__device__ __forceinline__ void xcd_strip_tile(int& tm, int& tn) {
    xcd_strip_tile_at(blockIdx.y * gridDim.x + blockIdx.x, gridDim.x, gridDim.y, tm, tn);
}

// ---- staging -----------------------------------------------------------------------------------------------------------------------
// T is the operand's element type (bf16, or unsigned char for e4m3); pointers and leading dimensions are in elements so that the address
// arithmetic compiles as it did in each kernel (a k-step is 128 / sizeof(T) elements, a chunk 16 / sizeof(T)).
// DMA source addresses of one operand.  Piece p of this wave covers tile rows 8*(wave + WAVES*p) .. +7; lane l lands in LDS at
// piece_base + 16*l = (row r = l>>3, physical chunk l&7), which must hold the LOGICAL chunk (l&7) ^ (r&7).  Rows past `rows` are
// clamped: tail rows read valid memory.
template <int WAVES, typename T, int C>
__device__ __forceinline__ void dma_sources(const T* (&g)[C], const T* base, int64_t ld, int row0, int rows, int wave, int lane) {
    const int lr = lane >> 3;
    const int lc = RALD_SWZ(lr, lane & 7);
#pragma unroll
    for (int p = 0; p < C; ++p) {
        int r = row0 + 8 * (wave + WAVES * p) + lr;
        r = r < rows ? r : rows - 1;
        g[p] = base + (int64_t)r * ld + lc * (16 / (int)sizeof(T));
    }
}
// One stage: k-step kt (of nk) of both operands into `stage` = [A tile of BM rows | B tile].
// k-steps run in ascending order from 0 in every tile, so a sample's sums do not depend on its tile or batch size (a per-tile rotated
// start was measured and not shipped: DESIGN §5).  The no-op koff / wrap stays: removing it changes the compiled code.
template <int BM, int WAVES, typename T, int CA, int CB>
__device__ __forceinline__ void dma_stage(const T* const (&gA)[CA], const T* const (&gB)[CB], int kt, int nk, unsigned char* stage, int wave) {
    constexpr int BK = 128 / (int)sizeof(T);
    const int koff = 0;
    int ks = kt + koff;
    ks = ks >= nk ? ks - nk : ks;
#pragma unroll
    for (int p = 0; p < CA; ++p)
        __builtin_amdgcn_global_load_lds((glb_void*)(gA[p] + ks * BK), (lds_void*)(stage + (wave + WAVES * p) * 1024), 16, 0, 0);
#pragma unroll
    for (int p = 0; p < CB; ++p)
        __builtin_amdgcn_global_load_lds((glb_void*)(gB[p] + ks * BK), (lds_void*)(stage + BM * 128 + (wave + WAVES * p) * 1024), 16, 0, 0);
}

// ---- fragment reads ----------------------------------------------------------------------------------------------------------------
// bf16: tile[row * 8 + RALD_SWZ(row, chunk)] on a bf16x8 pointer (see RALD_SWZ for why that is not a function).
// MXFP8: chunks fq and fq + 4 of tile row `row` (the operand layout of v_mfma_scale_f32_16x16x128_f8f6f4, see gemm_fp8.hip)
__device__ __forceinline__ i32x8 frag_mx8(const unsigned char* tile, int row, int fq) {
    const i32x4* s = reinterpret_cast<const i32x4*>(tile) + row * 8;
    const i32x4 lo = s[RALD_SWZ(row, fq)], hi = s[RALD_SWZ(row, fq + 4)];
    return i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// ---- MXFP8 main loop ---------------------------------------------------------------------------------------------------------------
// acc = A[m0.., :K] . B[n0.., :K]^T for this wave's (BM/WM) x (BN/WN) part of the tile, e4m3 operands (ld in bytes) with e8m0 scales
// S[row][K/32]; rows are clamped to M / N.  Two LDS stages at `smem`; scales are one byte per lane per tile row per k-step, fetched a
// k-step ahead with plain byte loads (they stay in L2).  The kernel writes the loop itself,
//     Mx8Loop<BM, BN, WM, WN> L;  L.begin(acc, ...);  for (int kt = 0; kt < L.nk; ++kt) L.step(acc, kt, <buffer of kt>, <the other>, ...);
// because a `for` inside an inlined helper compiles to another latch (the inliner puts the caller's continuation behind the loop's blocks
// and instruction selection inverts compare and branch).  The staging buffers are still being read by other waves after the last step.
template <int BM, int BN, int WM, int WN>
struct Mx8Loop {
    static constexpr int WAVES = WM * WN;
    static constexpr int MT = BM / (16 * WM);
    static constexpr int NT = BN / (16 * WN);
    static constexpr int CA = BM / 8 / WAVES;       // 1-KiB DMA pieces (8 rows x 128 B) per wave
    static constexpr int CB = BN / 8 / WAVES;
    static constexpr int STAGE_BYTES = (BM + BN) * 128;
    const unsigned char* gA[CA];
    const unsigned char* gB[CB];
    const unsigned char *SA, *SB;
    int offA[MT], offB[NT];                         // scale byte of this lane's (tile row, K-block fq) for k-step kt: S[row * kb + kt * 4 + fq]
    int sa_next[MT], sb_next[NT];
    int nk;

    __device__ __forceinline__ void load_scales(int kt) {
#pragma unroll
        for (int i = 0; i < MT; ++i) sa_next[i] = SA[offA[i] + kt * 4];
#pragma unroll
        for (int j = 0; j < NT; ++j) sb_next[j] = SB[offB[j] + kt * 4];
    }
    // zero acc, set the addresses up, put k-step 0 in flight
    __device__ __forceinline__ void begin(f32x4 (&acc)[MT][NT], const unsigned char* A, int64_t lda, const unsigned char* SA_, int m0, int M,
                                          const unsigned char* B, int64_t ldb, const unsigned char* SB_, int n0, int N, int K, unsigned char* smem, int wave, int lane) {
        SA = SA_; SB = SB_;
        const int wm = wave / WN, wn = wave % WN;
        const int kb = K / 32;                      // scale bytes per row
        dma_sources<WAVES>(gA, A, lda, m0, M, wave, lane);
        dma_sources<WAVES>(gB, B, ldb, n0, N, wave, lane);
        const int fr = lane & 15, fq = lane >> 4;
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            int r = m0 + wm * (BM / WM) + i * 16 + fr;
            r = r < M ? r : M - 1;
            offA[i] = r * kb + fq;
        }
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            int r = n0 + wn * (BN / WN) + j * 16 + fr;
            r = r < N ? r : N - 1;
            offB[j] = r * kb + fq;
        }
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        nk = K / 128;
        dma_stage<BM, WAVES>(gA, gB, 0, nk, smem, wave);
        load_scales(0);
    }
    // k-step kt out of LDS buffer `cur`, k-step kt + 1 into buffer `nxt`
    __device__ __forceinline__ void step(f32x4 (&acc)[MT][NT], int kt, int cur, int nxt, unsigned char* smem, int wave, int lane) {
        const int wm = wave / WN, wn = wave % WN;
        const int fr = lane & 15, fq = lane >> 4;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // tile kt and its scales have landed
        __builtin_amdgcn_s_barrier();                          // ... for every wave; buffer nxt is free
        asm volatile("" ::: "memory");
        int sa[MT], sb[NT];
#pragma unroll
        for (int i = 0; i < MT; ++i) sa[i] = sa_next[i];
#pragma unroll
        for (int j = 0; j < NT; ++j) sb[j] = sb_next[j];
        if (kt + 1 < nk) {
            dma_stage<BM, WAVES>(gA, gB, kt + 1, nk, smem + nxt * STAGE_BYTES, wave);
            load_scales(kt + 1);
        }
        const unsigned char* tA = smem + cur * STAGE_BYTES;
        const unsigned char* tB = tA + BM * 128;
        i32x8 fa[MT];
#pragma unroll
        for (int i = 0; i < MT; ++i) fa[i] = frag_mx8(tA, wm * (BM / WM) + i * 16 + fr, fq);
        // weight fragments one n-tile ahead of the MFMAs that consume them (an LDS round trip per n-tile otherwise)
        i32x8 fb = frag_mx8(tB, wn * (BN / WN) + fr, fq);
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            i32x8 fb_next = fb;
            if (j + 1 < NT) fb_next = frag_mx8(tB, wn * (BN / WN) + (j + 1) * 16 + fr, fq);
#pragma unroll
            for (int i = 0; i < MT; ++i)
                acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fb, fa[i], acc[i][j], 0, 0, 0, sb[j], 0, sa[i]);
            fb = fb_next;
        }
    }
};

}  // namespace rald
