// Conv3d k3 of the radar encoder and decoder (radar.hip holds the model, model/models_radar_encoder.py): the four implicit-GEMM engines
// (igemm, line, plane, persistent plane), their epilogue, the split-K reduce pass, the route function that picks an engine from the shape,
// the launch, and the op-level entries conv3d_full / conv3d_igemm - the only way in for the model, the training path and the tests.
//
// Layout as in radar.hip: activations channels-LAST ([b][d][h][w][c]: one voxel's channels are an MFMA A-fragment row), every conv input the
// bf16 tensor another pass wrote, so a convolution is a pure implicit GEMM
//     M = output voxels, N = Cout, K = 27*Cin  (weights packed [Cout][tap][Cin], K-contiguous).
// Zero padding: out-of-range taps contribute exact zeros (register zero-fill, no padded copy).  Downsample = F.pad(0,1) + conv k3 s2 p0 is
// the igemm kernel with stride 2 and left pad 0.  LDS tiles are rows of 128 B = 8 chunks with the GEMMs' swizzle (RALD_SWZ, gemm_tile.h).
#include <type_traits>

#include "gemm_tile.h"
#include "kernels.h"

namespace rald {

// The kernels' argument block (private to this file; conv3d_full fills it).
struct ConvArgs {
    const bf16* in;      // [B][ID][IH][IW][Cin]
    const bf16* w;       // [Cout][27][Cin]
    const float* bias;   // [Cout]
    const float* resid;  // [M][Cout] or nullptr
    float* out;          // [M][Cout]
    int B, ID, IH, IW, Cin, OD, OH, OW, Cout, stride, pad;
    // optional: GroupNorm(32) partial statistics of the OUTPUT, one slot per 128-voxel tile (requires OD*OH*OW % 128 == 0 so that
    // no tile straddles two samples): gn_part[tile][32 groups][2] doubles = {sum, sumsq}; saves the statistics pass over the fp32
    // activation (537 MB at full resolution, B = 8) that the next GroupNorm would otherwise make
    double* gn_part = nullptr;
    // optional split-K (few tiles, long K: the 64- and 512-voxel levels): gridDim.z workgroups share a tile, each takes a contiguous
    // range of k-steps and writes its raw accumulators to split_part[z][M][Cout]; conv_split_reduce_kernel adds them in order
    float* split_part = nullptr;
    // optional: the result as bf16 INSTEAD of fp32 (training: a data gradient whose only reader is the GroupNorm backward - half the bytes
    // written here and read twice there); no residual, no split-K
    bf16* out16 = nullptr;
};

// Epilogue shared by the four convolution kernels: bias (+ fp32 residual), fp32 store, optional GroupNorm partials of the output.
// acc[i][j][e] <-> voxel m0 + wm*64 + i*16 + fr, channel n0 + wn*32 + j*16 + 4*fq + e.  Must be reached by the whole workgroup
// after the K-loop's last barrier (it reuses the staging LDS when a.gn_part is set).
__device__ __forceinline__ void conv_epilogue(f32x4 (&acc)[4][2], const ConvArgs& a, int64_t M, int64_t m0, int n0, int wm, int wn, int fr,
                                              int fq, int tid, unsigned char* smem, int64_t tile128 = -1, const float4* pre_bias = nullptr,
                                              const float4* pre_resid = nullptr) {   // pre_*: this lane's bias [NT] / residual [MT][NT] values, loaded earlier
    constexpr int BM = 128, BN = 64, MT = 4, NT = 2;
    float cs[NT][4], cq[NT][4];                 // per-lane channel sums over this lane's MT voxels (GroupNorm partials)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) { cs[j][e] = 0.f; cq[j][e] = 0.f; }
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const int64_t m = m0 + wm * (BM / 2) + i * 16 + fr;
        if (m >= M) continue;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int n = n0 + wn * (BN / 2) + j * 16 + 4 * fq;
            if (n >= a.Cout) continue;
            const float4 b = pre_bias ? pre_bias[j] : *reinterpret_cast<const float4*>(a.bias + n);
            f32x4 v = acc[i][j];
            float4 o = make_float4(v[0] + b.x, v[1] + b.y, v[2] + b.z, v[3] + b.w);
            if (a.resid) {
                const float4 r = pre_resid ? pre_resid[i * NT + j] : *reinterpret_cast<const float4*>(a.resid + m * a.Cout + n);
                o.x += r.x; o.y += r.y; o.z += r.z; o.w += r.w;
            }
            if (a.out16) *reinterpret_cast<bf16x4*>(a.out16 + m * a.Cout + n) = pack4(o.x, o.y, o.z, o.w);
            else *reinterpret_cast<float4*>(a.out + m * a.Cout + n) = o;
            cs[j][0] += o.x; cs[j][1] += o.y; cs[j][2] += o.z; cs[j][3] += o.w;
            cq[j][0] += o.x * o.x; cq[j][1] += o.y * o.y; cq[j][2] += o.z * o.z; cq[j][3] += o.w * o.w;
        }
    }
    if (a.gn_part) {
        // fixed-shape reduction (bit-reproducible): 16 voxel lanes by butterfly, the two voxel halves (wm) and the channels of a
        // group in index order.  Host contract: full tiles (M % 128 == 0, Cout % 64 == 0), the K-loop's last barrier has passed.
        float2* sc = reinterpret_cast<float2*>(smem);                       // [wm][64 channels of this n-tile]
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                // the 16 voxel lanes of one fq share a DPP row: four row-local adds (quad swaps, half-mirror, mirror) leave the row's total in every
                // lane at VALU rate (the ds_bpermute butterfly this replaces was 2.3 us of a 24 us tile: 128 LDS-crossbar ops and their waits)
                float s1 = cs[j][e], s2 = cq[j][e];
                s1 += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s1), 0xB1, 0xf, 0xf, true));
                s2 += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s2), 0xB1, 0xf, 0xf, true));
                s1 += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s1), 0x4E, 0xf, 0xf, true));
                s2 += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s2), 0x4E, 0xf, 0xf, true));
                s1 += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s1), 0x141, 0xf, 0xf, true));
                s2 += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s2), 0x141, 0xf, 0xf, true));
                s1 += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s1), 0x140, 0xf, 0xf, true));
                s2 += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s2), 0x140, 0xf, 0xf, true));
                if (fr == 0) sc[wm * 64 + wn * 32 + j * 16 + 4 * fq + e] = make_float2(s1, s2);
            }
        __syncthreads();
        const int cpg = a.Cout / 32, gpt = 64 / cpg;                         // channels per group, groups in this 64-channel tile
        if (tid < gpt) {
            double su = 0.0, sq = 0.0;
            for (int w = 0; w < 2; ++w)
                for (int c = tid * cpg; c < (tid + 1) * cpg; ++c) { su += (double)sc[w * 64 + c].x; sq += (double)sc[w * 64 + c].y; }
            double* o = a.gn_part + ((tile128 >= 0 ? tile128 : (int64_t)blockIdx.y) * 32 + n0 / cpg + tid) * 2;
            o[0] = su; o[1] = sq;
        }
    }
}

// ---- pieces the engines share ---------------------------------------------------------------------------------------------------------
// All four engines compute 128 x 64 (voxels x couts) per four waves with the fragment layout of conv_epilogue: MT = 4 m-tiles and NT = 2
// n-tiles of 16 per wave.  A piece is shared here only where the kernels compile to the same instructions with it as with the text written
// out (tools/isa_audit.py --against): the fragment reads, the staged-row index `ebase`, the plane kernels' weight ring load, their accumulator
// zeroing and their bias / residual pre-fetch do not and stay written out in each kernel.
// (igemm and line kernels)
__device__ __forceinline__ void zero_acc(f32x4 (&acc)[4][2]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
}
// this thread's 16-byte chunk of row `row` of the packed weights [Cout][27][cin]; rows past Cout are clamped (tail rows read valid memory)
__device__ __forceinline__ const bf16* weight_row(const ConvArgs& a, int row, int cin, int schunk) {
    row = row < a.Cout ? row : a.Cout - 1;
    return a.w + (int64_t)row * 27 * cin + schunk * 8;
}
// channels c0 + 8 schunk .. + 7 of input voxel (b, id, ih, iw); exact zeros outside the volume (Conv3d's zero padding).  (c0 and schunk apart:
// with their sum as one argument the address arithmetic compiles differently)
__device__ __forceinline__ bf16x8 gather_row(const ConvArgs& a, int b, int id, int ih, int iw, int c0, int schunk) {
    bf16x8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (bf16)0.f;
    if ((unsigned)id < (unsigned)a.ID && (unsigned)ih < (unsigned)a.IH && (unsigned)iw < (unsigned)a.IW)
        v = *reinterpret_cast<const bf16x8*>(a.in + ((((int64_t)b * a.ID + id) * a.IH + ih) * a.IW + iw) * a.Cin + c0 + schunk * 8);
    return v;
}
// one 32-deep sub-step: acc[i][j] += fa[i] . fb[j]
__device__ __forceinline__ void mfma_sweep(f32x4 (&acc)[4][2], const bf16x8 (&fa)[4], const bf16x8 (&fb)[2]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[j], fa[i], acc[i][j], 0, 0, 0);
}

// Implicit-GEMM Conv3d k3: same tile machinery as gemm_nt_kernel (128 voxels x 64 couts x 64 K,
// 4 waves 2x2, XOR-swizzled double-buffered LDS); the A rows are gathered per tap.
__global__ __launch_bounds__(256) void conv3d_igemm_kernel(ConvArgs a) {
    constexpr int BM = 128, BN = 64, BK = 64;
    constexpr int MT = BM / 32, NT = BN / 32, PA = BM / 32, PB = BN / 32;
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * (BM + BN) * BK * 2];
    bf16x8* sA = reinterpret_cast<bf16x8*>(smem);
    bf16x8* sB = reinterpret_cast<bf16x8*>(smem + 2 * BM * BK * 2);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int64_t M = (int64_t)a.B * a.OD * a.OH * a.OW;
    const int64_t m0 = (int64_t)blockIdx.y * BM;
    const int n0 = blockIdx.x * BN;
    const int srow = tid >> 3, schunk = tid & 7;

    // per staged row: base voxel coordinates of the receptive field
    int rb[PA], rd[PA], rh[PA], rw[PA];
#pragma unroll
    for (int p = 0; p < PA; ++p) {
        int64_t m = m0 + srow + 32 * p;
        if (m >= M) m = M - 1;
        const int ow = (int)(m % a.OW);
        int64_t r = m / a.OW;
        const int oh = (int)(r % a.OH); r /= a.OH;
        const int od = (int)(r % a.OD);
        rb[p] = (int)(r / a.OD);
        rd[p] = od * a.stride - a.pad; rh[p] = oh * a.stride - a.pad; rw[p] = ow * a.stride - a.pad;
    }
    const bf16* gB[PB];
#pragma unroll
    for (int p = 0; p < PB; ++p) gB[p] = weight_row(a, n0 + srow + 32 * p, a.Cin, schunk);
    const int cpk = a.Cin / BK;                 // K-steps per tap
    const int nk = 27 * cpk;
    bf16x8 rA[PA], rB[PB];
    auto load_tile = [&](int kt) {
        const int tap = kt / cpk, c0 = (kt - tap * cpk) * BK;
        const int kd = tap / 9, kh = (tap / 3) % 3, kw = tap % 3;
#pragma unroll
        for (int p = 0; p < PA; ++p) rA[p] = gather_row(a, rb[p], rd[p] + kd, rh[p] + kh, rw[p] + kw, c0, schunk);
#pragma unroll
        for (int p = 0; p < PB; ++p) rB[p] = *reinterpret_cast<const bf16x8*>(gB[p] + (int64_t)kt * BK);
    };
    auto store_tile = [&](int buf) {
#pragma unroll
        for (int p = 0; p < PA; ++p) {
            const int r = srow + 32 * p;
            sA[(buf * BM + r) * 8 + RALD_SWZ(r, schunk)] = rA[p];
        }
#pragma unroll
        for (int p = 0; p < PB; ++p) {
            const int r = srow + 32 * p;
            sB[(buf * BN + r) * 8 + RALD_SWZ(r, schunk)] = rB[p];
        }
    };
    f32x4 acc[MT][NT];
    zero_acc(acc);
    const int k_begin = (int)((int64_t)nk * blockIdx.z / gridDim.z), k_end = (int)((int64_t)nk * (blockIdx.z + 1) / gridDim.z);
    load_tile(k_begin);
    store_tile(k_begin & 1);
    __syncthreads();
    const int fr = lane & 15, fq = lane >> 4;
    for (int kt = k_begin; kt < k_end; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < k_end) load_tile(kt + 1);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            bf16x8 fa[MT], fb[NT];
            const int chunk = kk * 4 + fq;
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                const int r = wm * (BM / 2) + i * 16 + fr;
                fa[i] = sA[(buf * BM + r) * 8 + RALD_SWZ(r, chunk)];
            }
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int r = wn * (BN / 2) + j * 16 + fr;
                fb[j] = sB[(buf * BN + r) * 8 + RALD_SWZ(r, chunk)];
            }
            mfma_sweep(acc, fa, fb);
        }
        if (kt + 1 < k_end) store_tile(buf ^ 1);
        __syncthreads();
    }
    if (a.split_part) {                          // raw partial sums of this k-range (bias / residual are added by the reduce pass)
        float* part = a.split_part + (int64_t)blockIdx.z * M * a.Cout;
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const int64_t m = m0 + wm * (BM / 2) + i * 16 + fr;
            if (m >= M) continue;
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int n = n0 + wn * (BN / 2) + j * 16 + 4 * fq;
                if (n >= a.Cout) continue;
                *reinterpret_cast<float4*>(part + m * a.Cout + n) = make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
            }
        }
        return;
    }
    conv_epilogue(acc, a, M, m0, n0, wm, wn, fr, fq, tid, smem);
}
// out = bias + sum_z part[z] (+ resid), z in order; one float4 per thread.  Aliasing contract: resid == out is allowed (resblock's in-place
// residual) although both are __restrict__ - the one thread that writes out[i .. i+3] is the only one that reads resid[i .. i+3], and its
// store depends on that load, so no reordering the qualifier permits can change the result; `part` must not overlap either
// (tests/test_gpu_radar_encoder_ops.py runs every split shape in place and compares bit for bit).
__global__ __launch_bounds__(256) void conv_split_reduce_kernel(const float* __restrict__ part, int splits, int64_t MC, int Cout,
                                                                const float* __restrict__ bias, const float* __restrict__ resid,
                                                                float* __restrict__ out) {
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= MC) return;
    const float4 b = *reinterpret_cast<const float4*>(bias + (int)(i % Cout));
    float4 acc = *reinterpret_cast<const float4*>(part + i);
    for (int z = 1; z < splits; ++z) {
        const float4 p = *reinterpret_cast<const float4*>(part + (int64_t)z * MC + i);
        acc.x += p.x; acc.y += p.y; acc.z += p.z; acc.w += p.w;
    }
    acc.x += b.x; acc.y += b.y; acc.z += b.z; acc.w += b.w;
    if (resid) {
        const float4 r = *reinterpret_cast<const float4*>(resid + i);
        acc.x += r.x; acc.y += r.y; acc.z += r.z; acc.w += r.w;
    }
    *reinterpret_cast<float4*>(out + i) = acc;
}

// Stride-1, pad-1 variant that stages whole input LINES.  A tile is 128 consecutive output voxels = L = 128/OW complete w-lines
// (OW = 2^lw in {8, 16, 32}); for a fixed (kd, kh) the three kw taps read the same L input lines shifted by one voxel, so the
// lines are staged ONCE with a one-voxel apron (L x (OW+2) rows of 128 B) and the taps index into them: a third of the gathers of
// conv3d_igemm_kernel, whose full-resolution launches run at the L2 -> CU rate of those gathers.  Same MFMA fragment layout
// and epilogue.  Host contract: stride 1, pad 1, M % 128 == 0, Cin % 64 == 0.
__global__ __launch_bounds__(256) void conv3d_line_kernel(ConvArgs a, int lw) {
    constexpr int BM = 128, BN = 64, BK = 64, MT = 4, NT = 2, PB = 2, RE_MAX = 160, PAX = RE_MAX / 32;
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * RE_MAX * 128 + 2 * BN * 128];
    bf16x8* sA = reinterpret_cast<bf16x8*>(smem);                         // [2][RE_MAX rows][8 chunks]
    bf16x8* sB = reinterpret_cast<bf16x8*>(smem + 2 * RE_MAX * 128);      // [2][64 couts][8 chunks]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int64_t M = (int64_t)a.B * a.OD * a.OH * a.OW;
    const int64_t m0 = (int64_t)blockIdx.y * BM;
    const int n0 = blockIdx.x * BN;
    const int srow = tid >> 3, schunk = tid & 7;
    const int OW = 1 << lw, EW = OW + 2, RE = (BM >> lw) * EW;
    // staged row e = srow + 32p -> (line l, apron column we): the line's (b, od, oh) and the input column iw = we - 1
    int eb[PAX], ed[PAX], eh[PAX], ewi[PAX];
    const int64_t ln0 = m0 >> lw;
#pragma unroll
    for (int p = 0; p < PAX; ++p) {
        const int e = srow + 32 * p;
        const int l = e / EW;
        ewi[p] = e < RE ? e - l * EW - 1 : -2;                               // -2: no such row (never valid)
        int64_t ln = ln0 + l;
        const int64_t nlines = (int64_t)a.B * a.OD * a.OH;
        if (ln >= nlines) ln = nlines - 1;
        eh[p] = (int)(ln % a.OH);
        const int64_t r = ln / a.OH;
        ed[p] = (int)(r % a.OD);
        eb[p] = (int)(r / a.OD);
    }
    const bf16* gB[PB];
#pragma unroll
    for (int p = 0; p < PB; ++p) gB[p] = weight_row(a, n0 + srow + 32 * p, a.Cin, schunk);
    const int cpk = a.Cin / BK;
    const int nsteps = 27 * cpk;                                             // step s = (pair * cpk + c) * 3 + kw, pair = kd*3 + kh
    // Global loads run TWO k-steps ahead of their first use (a k-step is only 16 MFMAs per wave, far less than one memory
    // latency): weights in two register sets that alternate by step parity, input lines loaded at kw = 0 of the previous
    // (kd, kh) pair and written to LDS at its kw = 2.
    bf16x8 rA[PAX], rB[2][PB];
    auto load_A = [&](int pc) {                                              // pc = pair * cpk + c
        const int pair = pc / cpk, c0 = (pc - pair * cpk) * BK;
        const int kd = pair / 3, kh = pair - 3 * kd;
#pragma unroll
        for (int p = 0; p < PAX; ++p) rA[p] = gather_row(a, eb[p], ed[p] + kd - 1, eh[p] + kh - 1, ewi[p], c0, schunk);
    };
    auto store_A = [&](int buf) {
#pragma unroll
        for (int p = 0; p < PAX; ++p) {
            const int e = srow + 32 * p;
            if (e < RE) sA[(buf * RE_MAX + e) * 8 + RALD_SWZ(e, schunk)] = rA[p];
        }
    };
    auto load_B = [&](int s, auto PAR) {
        constexpr int par = decltype(PAR)::value;
        const int pc = s / 3, kw = s - 3 * pc;
        const int pair = pc / cpk, c = pc - pair * cpk;
        const int kt = (pair * 3 + kw) * cpk + c;                            // weight K index: tap-major, then the Cin chunk
#pragma unroll
        for (int p = 0; p < PB; ++p) rB[par][p] = *reinterpret_cast<const bf16x8*>(gB[p] + (int64_t)kt * BK);
    };
    auto store_B = [&](int buf, auto PAR) {
        constexpr int par = decltype(PAR)::value;
#pragma unroll
        for (int p = 0; p < PB; ++p) {
            const int r = srow + 32 * p;
            sB[(buf * BN + r) * 8 + RALD_SWZ(r, schunk)] = rB[par][p];
        }
    };
    f32x4 acc[MT][NT];
    zero_acc(acc);
    const int fr = lane & 15, fq = lane >> 4;
    int ebase[MT];                                                           // staged row of this lane's voxel at kw = 0
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const int r = wm * (BM / 2) + i * 16 + fr;
        ebase[i] = (r >> lw) * EW + (r & (OW - 1));
    }
    using P0 = std::integral_constant<int, 0>;
    using P1 = std::integral_constant<int, 1>;
    const int npc = 9 * cpk;
    load_A(0); load_B(0, P0{});
    store_A(0); store_B(0, P0{});
    if (nsteps > 1) load_B(1, P1{});
    if (npc > 1) load_A(1);
    __syncthreads();
    // one k-step; KW = s % 3, PAR = s & 1 (compile-time so that the register sets are not indexed dynamically)
    auto step = [&](int pc, auto KWC, auto PARC) {
        constexpr int kw = decltype(KWC)::value, par = decltype(PARC)::value;
        const int s = 3 * pc + kw;
        const int abuf = pc & 1;
        if (s + 2 < nsteps) load_B(s + 2, PARC);                             // set `par` held B(s), already in LDS
        if (kw == 0 && pc >= 1 && pc + 1 < npc) load_A(pc + 1);               // (pc = 0: issued in the prologue)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            bf16x8 fa[MT], fb[NT];
            const int chunk = kk * 4 + fq;
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                const int e = ebase[i] + kw;
                fa[i] = sA[(abuf * RE_MAX + e) * 8 + RALD_SWZ(e, chunk)];
            }
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int r = wn * (BN / 2) + j * 16 + fr;
                fb[j] = sB[(par * BN + r) * 8 + RALD_SWZ(r, chunk)];
            }
            mfma_sweep(acc, fa, fb);
        }
        if (s + 1 < nsteps) store_B(par ^ 1, std::integral_constant<int, par ^ 1>{});   // B(s+1), loaded one step ago
        if (kw == 2 && pc + 1 < npc) store_A(abuf ^ 1);                       // lines of the next pair, loaded at its kw = 0
        __syncthreads();
    };
    using K0 = std::integral_constant<int, 0>;
    using K1 = std::integral_constant<int, 1>;
    using K2 = std::integral_constant<int, 2>;
    for (int pc = 0; pc < npc; pc += 2) {                                    // s = 3 pc + kw: parity (pc + kw) & 1
        step(pc, K0{}, P0{}); step(pc, K1{}, P1{}); step(pc, K2{}, P0{});
        if (pc + 1 < npc) { step(pc + 1, K0{}, P1{}); step(pc + 1, K1{}, P0{}); step(pc + 1, K2{}, P1{}); }
    }
    conv_epilogue(acc, a, M, m0, n0, wm, wn, fr, fq, tid, smem);
}

// ---- parts of the two plane-staged kernels (conv3d_plane_kernel, conv3d_pplane_kernel) ------------------------------------------------
// Register arrays (the weight ring rB, the fragment buffers fa / fb) are only ever indexed by compile-time constants: a slot or buffer
// number travels as a template argument or as an IC<N> tag.
template <int N>
using IC = std::integral_constant<int, N>;
// slot SL (compile-time: the ring is never indexed dynamically) of the weight register ring rB into the weights' LDS area sB [3 taps][64 couts][8 chunks]
template <int SL>
__device__ __forceinline__ void plane_store_w(bf16x8* sB, const bf16x8 (&rB)[3][3], int srow, int schunk) {
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) sB[(kw * 64 + srow) * 8 + RALD_SWZ(srow, schunk)] = rB[SL][kw];
}
// the MFMAs of one tap (both 32-deep halves) out of fragment buffer BB: the MFMA sweep of the plane kernels
template <int BB>
__device__ __forceinline__ void plane_mm(f32x4 (&acc)[4][2], const bf16x8 (&fa)[2][2][4], const bf16x8 (&fb)[2][2][2]) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) mfma_sweep(acc, fa[BB][kk], fb[BB][kk]);
}
// The three taps of one (kd, kh) pair, up to the barrier behind the pair's last read of the weights: tap kw + 1 is read (rd(poff, kw + 1, buffer),
// the kernel's fragment read into fa / fb) under the MFMAs of tap kw, one ds_read per MFMA.
template <class RD>
__device__ __forceinline__ void plane_pair_taps(f32x4 (&acc)[4][2], const bf16x8 (&fa)[2][2][4], const bf16x8 (&fb)[2][2][2], RD& rd, int poff) {
    rd(poff, 0, IC<0>{});
    __builtin_amdgcn_sched_barrier(0);
    rd(poff, 1, IC<1>{});
    plane_mm<0>(acc, fa, fb);
#pragma unroll
    for (int g = 0; g < 12; ++g) { __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x100, 1, 0); }
    __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
    __builtin_amdgcn_sched_barrier(0);
    rd(poff, 2, IC<0>{});
    plane_mm<1>(acc, fa, fb);
#pragma unroll
    for (int g = 0; g < 12; ++g) { __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x100, 1, 0); }
    __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
    __builtin_amdgcn_sched_barrier(0);
    plane_mm<0>(acc, fa, fb);
    __syncthreads();                                                          // every wave has read this pair's weights
}

// Plane-staged form for the 64-channel levels: a workgroup of 8 waves takes 256 output voxels = L = 256 / OW whole w-lines of ONE (b, d) plane
// and stages everything those voxels ever read - the three d-planes x (L + 2) h-lines x (OW + 2) columns, <= 1 024 rows of 128 B = 128 KiB -
// ONCE; the 27 taps then only index into that image, and the only traffic of the main loop is the weights of one (kd, kh) pair at a time
// (3 taps, 24 KiB, from L2).  conv3d_line_kernel re-stages its lines for each of the nine (kd, kh) pairs (360 KB per 256 voxels instead of
// 130 KB) and, worse, WAITS for them: with one or two k-steps of prefetch in registers a step lasts as long as a trip to memory - 3.6 us per
// pair for 0.7 us of MFMA work, 18 GB/s per CU, whatever the inner loop looks like (a 3-taps-per-barrier form of that kernel with
// software-pipelined fragment reads measured exactly the same 515 us per full-resolution convolution of 4 samples).  Here a tile pays the trip
// once.  Measured (radar-condition encode at B = 8, eight full-resolution launches): 7.72 -> 7.06 ms, 515 -> ~455 us per launch; with the
// staging loads redirected to one address (compile-time variant) 7.05 ms, without the epilogue 6.06 ms - what is left of a 28 us tile is ~7 us of
// prologue (16 rows of address arithmetic, loads and LDS stores per thread, one exposed trip to memory), ~12 us of main loop (6.6 us of MFMA work:
// two barriers and one exposed fragment-read latency per pair, one workgroup per CU) and 8.5 us of epilogue (residual read, GroupNorm partial
// sums, fp32 stores) that nothing overlaps.  Host contract: stride 1, pad 1, Cin = 64, Cout % 64 == 0, OW in {16, 32}, OH % L == 0 (a tile never leaves its plane), M % 256 == 0.
// LDS (dynamic): 128 KiB of lines + 24 KiB of weights; the epilogue's scratch reuses the weights' 24 KiB.
__global__ __launch_bounds__(512) void conv3d_plane_kernel(ConvArgs a, int lw) {
    constexpr int BN = 64, MT = 4, NT = 2, RE_MAX = 1024, PAX = RE_MAX / 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem3[];
    bf16x8* sA = reinterpret_cast<bf16x8*>(smem3);                        // [RE rows][8 chunks], row e = ((kd * (L + 2)) + l) * (OW + 2) + we
    bf16x8* sB = reinterpret_cast<bf16x8*>(smem3 + RE_MAX * 128);         // [3 taps][64 couts][8 chunks]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int64_t M = (int64_t)a.B * a.OD * a.OH * a.OW;
    const int64_t m0 = (int64_t)blockIdx.y * 256;
    const int n0 = blockIdx.x * BN;
    const int srow = tid >> 3, schunk = tid & 7;
    const int OW = 1 << lw, EW = OW + 2, L = 256 >> lw, LH = L + 2, PL = LH * EW, RE = 3 * PL;
    const int64_t ln0 = m0 >> lw;
    const int oh0 = (int)(ln0 % a.OH);
    const int64_t pl = ln0 / a.OH;
    const int od = (int)(pl % a.OD), b = (int)(pl / a.OD);
    const bf16* gW = weight_row(a, n0 + srow, 64, schunk);                   // (Cin = 64: tap t of output channel rw at element t * 64)
    // the weights run THREE pairs ahead of their use in a register ring (12 VGPRs per pair): with one pair of prefetch every pair waited for its
    // weights - all 256 CUs ask the L2 for the same 24 KiB at the same moment, ~3 us a trip - and a tile took 30 us for 6.6 us of MFMA work
    bf16x8 rB[3][3];
    auto loadW = [&](int pair, auto SLOT) {                                  // (written out in both plane kernels: DESIGN section 16)
        constexpr int sl = decltype(SLOT)::value;
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) rB[sl][kw] = *reinterpret_cast<const bf16x8*>(gW + (pair * 3 + kw) * 64);
    };
    {   // the tile's whole input image, once: unconditional loads from clamped addresses, zeros selected at the LDS store
        bf16x8 rA[PAX];
        unsigned rvalid = 0;
#pragma unroll
        for (int p = 0; p < PAX; ++p) {
            const int e = srow + 64 * p;
            const int kd = e / PL, rem = e - kd * PL;
            const int l = rem / EW, we = rem - l * EW;
            const int id = od + kd - 1, ih = oh0 - 1 + l, iw = we - 1;
            const bool ok = e < RE && (unsigned)id < (unsigned)a.ID && (unsigned)ih < (unsigned)a.IH && (unsigned)iw < (unsigned)a.IW;
            const int64_t off = ok ? ((((int64_t)b * a.ID + id) * a.IH + ih) * a.IW + iw) * 64 + schunk * 8 : (int64_t)schunk * 8;
            rA[p] = *reinterpret_cast<const bf16x8*>(a.in + off);
            rvalid |= ok ? (1u << p) : 0u;
        }
        loadW(0, IC<0>{});
        loadW(1, IC<1>{});
        loadW(2, IC<2>{});
        bf16x8 zero;
#pragma unroll
        for (int j = 0; j < 8; ++j) zero[j] = (bf16)0.f;
#pragma unroll
        for (int p = 0; p < PAX; ++p) {
            const int e = srow + 64 * p;
            if (e < RE) sA[e * 8 + RALD_SWZ(e, schunk)] = (rvalid >> p) & 1 ? rA[p] : zero;
        }
        plane_store_w<0>(sB, rB, srow, schunk);
        loadW(3, IC<0>{});
    }
    f32x4 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int fr = lane & 15, fq = lane >> 4;
    int ebase[MT];                                                           // staged row of this lane's voxel for tap (0, 0, 0)
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const int r = wm * 64 + i * 16 + fr;
        ebase[i] = (r >> lw) * EW + (r & (OW - 1));
    }
    // fragments of one tap (both 32-deep halves), double-buffered: tap kw + 1 is read under the MFMAs of tap kw
    bf16x8 fa[2][2][MT], fb[2][2][NT];
    auto rd = [&](int poff, int kw, auto BUF) {
        constexpr int bb = decltype(BUF)::value;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const int chunk = kk * 4 + fq;
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                const int e = ebase[i] + poff + kw;
                fa[bb][kk][i] = sA[e * 8 + RALD_SWZ(e, chunk)];
            }
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int r = wn * (BN / 2) + j * 16 + fr;
                fb[bb][kk][j] = sB[(kw * BN + r) * 8 + RALD_SWZ(r, chunk)];
            }
        }
    };
    __syncthreads();
    auto step = [&](auto PAIR) {
        constexpr int pair = decltype(PAIR)::value;
        constexpr int kd = pair / 3, kh = pair - 3 * kd;
        plane_pair_taps(acc, fa, fb, rd, (kd * LH + kh) * EW);
        if constexpr (pair + 1 < 9) {
            plane_store_w<(pair + 1) % 3>(sB, rB, srow, schunk);              // pair + 1, loaded three pairs ago
            if constexpr (pair + 4 < 9) loadW(pair + 4, IC<(pair + 1) % 3>{});
            __syncthreads();
        }
    };
    step(IC<0>{}); step(IC<1>{}); step(IC<2>{});
    step(IC<3>{}); step(IC<4>{}); step(IC<5>{});
    // what the epilogue adds - bias and fp32 residual of this lane's outputs - is fetched under the last three pairs (one workgroup per CU:
    // nothing else would hide that trip to memory; M % 256 == 0 and Cout % 64 == 0, so every index exists)
    float4 pb[NT], pr[MT * NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) pb[j] = *reinterpret_cast<const float4*>(a.bias + n0 + wn * (BN / 2) + j * 16 + 4 * fq);
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
            pr[i * NT + j] = a.resid ? *reinterpret_cast<const float4*>(a.resid + (m0 + wm * 64 + i * 16 + fr) * a.Cout + n0 + wn * (BN / 2) + j * 16 + 4 * fq)
                                     : make_float4(0.f, 0.f, 0.f, 0.f);
    step(IC<6>{}); step(IC<7>{}); step(IC<8>{});
    // the epilogue is the 128-voxel one, once per half of the tile (waves 0-3 / 4-7); its scratch lies in the weights' area
    conv_epilogue(acc, a, M, m0 + (wm >> 1) * 128, n0, wm & 1, wn, fr, fq, tid & 255, smem3 + RE_MAX * 128 + (wm >> 1) * 2048,
                  2 * (int64_t)blockIdx.y + (wm >> 1), pb, pr);
}

// The plane-staged form made persistent along d: a workgroup walks `ds` consecutive d-planes of one (b, 256-voxel h-block) column with a rolling window of
// three input planes in LDS (plane id lives in slot id mod 3).  Per output tile it stages ONE new plane instead of three - loaded into registers at the start
// of the tile, stored over the plane that leaves the window as soon as the kd = 0 pairs have read it - the weights' register ring runs on across tiles (pair (p + 4) mod 9 is
// fetched under pair p, whatever tile that belongs to), and the next tile's first fragment reads follow this tile's output stores directly: the prologue
// of conv3d_plane_kernel (address arithmetic, one exposed trip to memory, 16 LDS stores per thread) is paid once per `ds` tiles.
// grid.y = columns x segments: column = (b, oh0 / L), segment = ds planes.  Host contract: conv3d_plane_kernel's, and OD % ds == 0.
__global__ __launch_bounds__(512) void conv3d_pplane_kernel(ConvArgs a, int lw, int ds) {
    constexpr int BN = 64, MT = 4, NT = 2, RE_MAX = 1024, PPX = 6;                 // a plane image is <= 340 rows: 6 staging rows per thread
    extern __shared__ __attribute__((aligned(16))) unsigned char smem3[];
    bf16x8* sA = reinterpret_cast<bf16x8*>(smem3);                        // [3 slots][PL rows][8 chunks]; swizzle by the absolute row index
    bf16x8* sB = reinterpret_cast<bf16x8*>(smem3 + RE_MAX * 128);         // [3 taps][64 couts][8 chunks]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int64_t M = (int64_t)a.B * a.OD * a.OH * a.OW;
    const int n0 = blockIdx.x * BN;
    const int srow = tid >> 3, schunk = tid & 7;
    const int OW = 1 << lw, EW = OW + 2, L = 256 >> lw, LH = L + 2, PL = LH * EW;
    const int nseg = a.OD / ds, nhb = a.OH / L;
    const int seg = blockIdx.y % nseg, col = blockIdx.y / nseg;
    const int hb = col % nhb, b = col / nhb;
    const int oh0 = hb * L, d_lo = seg * ds;
    // this thread's staging rows of a plane image: row e = l * EW + we <-> input (ih = oh0 - 1 + l, iw = we - 1); the same for every plane
    int rowoff[PPX];                                                         // element offset inside a plane, or -1
#pragma unroll
    for (int p = 0; p < PPX; ++p) {
        const int e = srow + 64 * p;
        const int l = e / EW, we = e - l * EW;
        const int ih = oh0 - 1 + l, iw = we - 1;
        rowoff[p] = (e < PL && (unsigned)ih < (unsigned)a.IH && (unsigned)iw < (unsigned)a.IW) ? (ih * a.IW + iw) * 64 + schunk * 8 : -1;
    }
    const int64_t plane_elems = (int64_t)a.IH * a.IW * 64;
    const bf16* inb = a.in + (int64_t)b * a.ID * plane_elems;
    bf16x8 zero;
#pragma unroll
    for (int j = 0; j < 8; ++j) zero[j] = (bf16)0.f;
    auto loadP = [&](int id, bf16x8 (&r)[PPX]) {                              // plane id (may lie outside the volume: zeros at the store)
        const bool inside = (unsigned)id < (unsigned)a.ID;
        const bf16* pb_ = inb + (int64_t)(inside ? id : 0) * plane_elems;
#pragma unroll
        for (int p = 0; p < PPX; ++p) r[p] = *reinterpret_cast<const bf16x8*>(pb_ + (rowoff[p] >= 0 ? rowoff[p] : schunk * 8));
    };
    auto storeP = [&](int id, const bf16x8 (&r)[PPX]) {
        const bool inside = (unsigned)id < (unsigned)a.ID;
        const int slot = (id + 3) % 3;
#pragma unroll
        for (int p = 0; p < PPX; ++p) {
            const int e = srow + 64 * p;
            if (e < PL) { const int ea = slot * PL + e; sA[ea * 8 + RALD_SWZ(ea, schunk)] = (inside && rowoff[p] >= 0) ? r[p] : zero; }
        }
    };
    const bf16* gW = weight_row(a, n0 + srow, 64, schunk);
    bf16x8 rB[3][3];
    auto loadW = [&](int pair, auto SLOT) {                                  // (written out in both plane kernels: DESIGN section 16)
        constexpr int sl = decltype(SLOT)::value;
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) rB[sl][kw] = *reinterpret_cast<const bf16x8*>(gW + (pair * 3 + kw) * 64);
    };
    bf16x8 rP[PPX];
    {   // the first window: planes d_lo - 1, d_lo, d_lo + 1
        bf16x8 r0[PPX], r1[PPX];
        loadP(d_lo - 1, r0); loadP(d_lo, r1); loadP(d_lo + 1, rP);
        loadW(0, IC<0>{}); loadW(1, IC<1>{}); loadW(2, IC<2>{});
        storeP(d_lo - 1, r0); storeP(d_lo, r1); storeP(d_lo + 1, rP);
        plane_store_w<0>(sB, rB, srow, schunk);
        loadW(3, IC<0>{});
    }
    const int fr = lane & 15, fq = lane >> 4;
    int ebase[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const int r = wm * 64 + i * 16 + fr;
        ebase[i] = (r >> lw) * EW + (r & (OW - 1));
    }
    float4 pb[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) pb[j] = *reinterpret_cast<const float4*>(a.bias + n0 + wn * (BN / 2) + j * 16 + 4 * fq);
    f32x4 acc[MT][NT];
    bf16x8 fa[2][2][MT], fb[2][2][NT];
    auto rd = [&](int poff, int kw, auto BUF) {
        constexpr int bb = decltype(BUF)::value;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const int chunk = kk * 4 + fq;
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                const int e = ebase[i] + poff + kw;
                fa[bb][kk][i] = sA[e * 8 + RALD_SWZ(e, chunk)];
            }
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int r = wn * (BN / 2) + j * 16 + fr;
                fb[bb][kk][j] = sB[(kw * BN + r) * 8 + RALD_SWZ(r, chunk)];
            }
        }
    };
    __syncthreads();
    for (int d = d_lo; d < d_lo + ds; ++d) {
        const bool more = d + 1 < d_lo + ds;
        if (more) loadP(d + 2, rP);                                          // the plane the NEXT tile adds to the window: a whole tile ahead
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int64_t m0 = (((int64_t)b * a.OD + d) * a.OH + oh0) * OW;
        const int sl0 = (d + 2) % 3;                                          // slot of plane d - 1; d -> (sl0 + 1) % 3, d + 1 -> (sl0 + 2) % 3
        float4 pr[MT * NT];
        auto step = [&](auto PAIR) {
            constexpr int pair = decltype(PAIR)::value;
            constexpr int kd = pair / 3, kh = pair - 3 * kd;
            int slot = sl0 + kd;
            slot = slot >= 3 ? slot - 3 : slot;
            plane_pair_taps(acc, fa, fb, rd, slot * PL + kh * EW);
            if constexpr (pair < 8) {
                plane_store_w<(pair + 1) % 3>(sB, rB, srow, schunk);          // pair + 1, loaded three pairs ago
                loadW((pair + 4) % 9, IC<(pair + 1) % 3>{});                  // (wraps into the next tile: the weights do not depend on the tile)
                if constexpr (pair == 2) { if (more) storeP(d + 2, rP); }     // over plane d - 1, whose last readers were pairs 0-2 (frees rP's registers)
                __syncthreads();
            }
        };
        step(IC<0>{}); step(IC<1>{}); step(IC<2>{});
        step(IC<3>{}); step(IC<4>{}); step(IC<5>{});
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j)
                pr[i * NT + j] = a.resid ? *reinterpret_cast<const float4*>(a.resid + (m0 + wm * 64 + i * 16 + fr) * a.Cout + n0 + wn * (BN / 2) + j * 16 + 4 * fq)
                                         : make_float4(0.f, 0.f, 0.f, 0.f);
        step(IC<6>{}); step(IC<7>{}); step(IC<8>{});
        // (after pair 8's barrier nobody reads the weights' area: the epilogue's scratch lies there)
        conv_epilogue(acc, a, M, m0 + (wm >> 1) * 128, n0, wm & 1, wn, fr, fq, tid & 255, smem3 + RE_MAX * 128 + (wm >> 1) * 2048, m0 / 128 + (wm >> 1), pb, pr);
        if (more) {
            __syncthreads();                                                  // the epilogue's scratch has been read
            plane_store_w<0>(sB, rB, srow, schunk);                           // pair 0 of the next tile (fetched under pair 5)
            loadW(3, IC<0>{});
            __syncthreads();
        }
    }
}

// Engine choice for one convolution: THE one place that decides it (pure host arithmetic, no HIP call; exported as
// rald_op_conv3d_route so that a test can ask which engine a shape runs on).  In order:
//   CONV_IGEMM_SPLIT  allow_split, not a line shape, few tiles x long K (<= 64 tiles, >= 12 k-steps: the 512- and 64-voxel levels, every
//                     downsample below full resolution): conv3d_igemm_kernel with gridDim.z = splits k-ranges + conv_split_reduce_kernel
//   line shapes (stride 1, pad 1, W in {8, 16, 32}, M % 128 == 0):
//     CONV_PPLANE     Cin = 64, Cout % 64 == 0, W >= 16, H a multiple of the 256 / W lines of a tile, D % 8 == 0 and >= 256 workgroups
//     CONV_PLANE      the same without the D condition, M / 256 >= 256 tiles
//     CONV_LINE       every other line shape
//   CONV_IGEMM        everything else (stride 2, W not a power of two in range, M % 128 != 0, pad != 1)
// The route also carries what the launch of a line shape needs (lw, pds), so that launch_conv derives nothing.
ConvRoute conv3d_route(int B, int ID, int IH, int IW, int Cin, int Cout, int stride, int pad, int allow_split) {
    ConvRoute r{CONV_IGEMM, 1};
    if (B <= 0 || ID <= 0 || IH <= 0 || IW <= 0 || Cin <= 0 || Cout <= 0 || (stride != 1 && stride != 2)) return r;
    const int OD = ID / stride, OH = IH / stride, OW = IW / stride;
    const int64_t M = (int64_t)B * OD * OH * OW;
    const bool line_shape = stride == 1 && pad == 1 && (OW == 8 || OW == 16 || OW == 32) && M % 128 == 0 && Cin % 64 == 0;
    if (line_shape) {
        const int lw = OW == 8 ? 3 : OW == 16 ? 4 : 5;
        constexpr int pds = 8;                                                // planes per persistent workgroup
        const int Lp = 256 >> lw;
        const bool plane_shape = Cin == 64 && Cout % 64 == 0 && lw >= 4 && OH % Lp == 0 && 3 * (Lp + 2) * (OW + 2) <= 1024;
        r.lw = lw;
        if (plane_shape && OD % pds == 0 && (int64_t)B * (OH / Lp) * (OD / pds) >= 256) { r.engine = CONV_PPLANE; r.pds = pds; }
        else if (plane_shape && M % 256 == 0 && M / 256 >= 256) r.engine = CONV_PLANE;
        else r.engine = CONV_LINE;
        return r;
    }
    // few tiles x long K (the 512- and 64-voxel levels: 8-64 workgroups looping over 54-108 k-steps): split K over gridDim.z
    const int64_t tiles = (int64_t)cdiv(Cout, 64) * ((M + 127) / 128);
    const int nk = 27 * (Cin / 64);
    if (allow_split && tiles >= 1 && tiles <= 64 && nk >= 12 && Cout % 4 == 0) {
        int splits = (int)(256 / tiles);
        if (splits > 16) splits = 16;
        if (splits > nk / 3) splits = nk / 3;
        if (splits >= 2) { r.engine = CONV_IGEMM_SPLIT; r.splits = splits; }   // (splits * tiles <= 256: at most 8 MiB of partial sums)
    }
    return r;
}

// The plane kernels' dynamic LDS: the tile's input image (1 024 rows of 128 B) + one (kd, kh) pair of weights.  More than the 64 KiB a kernel
// gets by default, so each kernel is opted in once.
constexpr int LDSP = 1024 * 128 + 3 * 64 * 128;
template <class K>
static void allow_plane_lds(K kernel) {
    static bool attr_set = false;                                             // (one per kernel: K differs)
    if (!attr_set) { (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDSP); attr_set = true; }
}

// One convolution on the engine `r` names.  split_ws: r.splits * M * Cout floats when r splits (bias / residual are added by the reduce pass;
// a.resid == a.out, the in-place residual of resblock, is fine on every route: each output element is read and then written by one thread).
static void launch_conv(ConvArgs a, const ConvRoute& r, float* split_ws, hipStream_t st) {
    const int64_t M = (int64_t)a.B * a.OD * a.OH * a.OW;
    const dim3 grid(cdiv(a.Cout, 64), (unsigned)((M + 127) / 128));
    switch (r.engine) {
        case CONV_PPLANE:                                                     // a workgroup per (b, 256-voxel h-block, r.pds planes)
            allow_plane_lds(conv3d_pplane_kernel);
            hipLaunchKernelGGL(conv3d_pplane_kernel, dim3(grid.x, (unsigned)(a.B * (a.OH / (256 >> r.lw)) * (a.OD / r.pds))), dim3(512), LDSP, st, a, r.lw, r.pds);
            break;
        case CONV_PLANE:
            allow_plane_lds(conv3d_plane_kernel);
            hipLaunchKernelGGL(conv3d_plane_kernel, dim3(grid.x, (unsigned)(M / 256)), dim3(512), LDSP, st, a, r.lw);
            break;
        case CONV_LINE:
            hipLaunchKernelGGL(conv3d_line_kernel, grid, dim3(256), 0, st, a, r.lw);
            break;
        case CONV_IGEMM_SPLIT: {
            float* out = a.out;
            a.split_part = split_ws;
            hipLaunchKernelGGL(conv3d_igemm_kernel, dim3(grid.x, grid.y, r.splits), dim3(256), 0, st, a);
            const int64_t MC = M * a.Cout;
            hipLaunchKernelGGL(conv_split_reduce_kernel, dim3((unsigned)((MC / 4 + 255) / 256)), dim3(256), 0, st, split_ws, r.splits, MC, a.Cout,
                               a.bias, a.resid, out);
            break;
        }
        default:
            hipLaunchKernelGGL(conv3d_igemm_kernel, grid, dim3(256), 0, st, a);
    }
}

// ---- op level (the model in radar.hip, the training path and the tests) ------------------------------------------------------------
// The complete ConvArgs at op level.  allow_split = 1: the route the model (RadarEncoder::Impl::run_conv) takes (split-K through the caller's
// workspace where conv3d_route says so); 0: never split.  gn_part (nullable): [B*So/128][32][2] doubles, the GroupNorm partials of the output.
// resid == out (in place) is allowed.  Every check comes before the first HIP call.
int conv3d_full(const bf16* in, const bf16* w_packed, const float* bias, const float* resid, float* out, bf16* out_bf16, double* gn_part,
                float* split_ws, int64_t split_ws_bytes, int allow_split, int B, int ID, int IH, int IW, int Cin, int Cout, int stride, int pad,
                hipStream_t st) {
    RALD_CHECK(in && w_packed && bias && (out || out_bf16), "conv3d: null pointer");
    RALD_CHECK(!out_bf16 || (!out && !resid && (uintptr_t)out_bf16 % 8 == 0), "conv3d: the bf16 result replaces the fp32 one and takes no residual");
    RALD_CHECK(B > 0 && ID > 0 && IH > 0 && IW > 0 && (stride == 1 || stride == 2), "conv3d: bad geometry");
    RALD_CHECK(Cin % 64 == 0 && Cout % 4 == 0, "conv3d: Cin must be a multiple of 64 and Cout of 4");
    RALD_CHECK(Cin > 0 && Cout > 0 && ID >= stride && IH >= stride && IW >= stride && pad >= 0 && pad <= 2, "conv3d: bad geometry");
    RALD_CHECK(allow_split == 0 || allow_split == 1, "conv3d: allow_split is 0 (never split K) or 1 (the encoder's route)");
    ConvArgs a;
    a.in = in; a.w = w_packed; a.bias = bias; a.resid = resid; a.out = out; a.out16 = out_bf16;
    a.B = B; a.ID = ID; a.IH = IH; a.IW = IW; a.Cin = Cin; a.Cout = Cout; a.stride = stride; a.pad = pad;
    a.OD = ID / stride; a.OH = IH / stride; a.OW = IW / stride;
    const int64_t M = (int64_t)B * a.OD * a.OH * a.OW;
    const int64_t So = (int64_t)a.OD * a.OH * a.OW;
    const ConvRoute r = conv3d_route(B, ID, IH, IW, Cin, Cout, stride, pad, allow_split);
    if (r.engine == CONV_IGEMM_SPLIT) {
        RALD_CHECK(!out_bf16, "conv3d: the bf16 result is not available where the route splits K (allow_split = 0 keeps one pass)");
        RALD_CHECK(!gn_part, "conv3d: no GroupNorm partials (gn_part) where the route splits K");
        RALD_CHECK(split_ws && (uintptr_t)split_ws % 16 == 0, "conv3d: split-K needs a 16-byte aligned workspace");
        RALD_CHECK(split_ws_bytes >= (int64_t)r.splits * M * Cout * 4, "conv3d: split-K workspace too small (splits * M * Cout * 4 bytes)");
    }
    if (gn_part) {
        RALD_CHECK(So % 128 == 0, "conv3d: gn_part needs output voxels per sample (So) % 128 == 0, so that no tile straddles two samples");
        RALD_CHECK(Cout == 64 || Cout == 128 || Cout == 256, "conv3d: gn_part needs Cout of 64, 128 or 256");
        RALD_CHECK((uintptr_t)gn_part % 8 == 0, "conv3d: gn_part must be 8-byte aligned");
        a.gn_part = gn_part;
    }
    launch_conv(a, r, split_ws, st);
    RALD_HIP(hipGetLastError());
    return 0;
}

int conv3d_igemm(const bf16* in, const bf16* w_packed, const float* bias, const float* resid, float* out, int B, int ID, int IH, int IW,
                 int Cin, int Cout, int stride, int pad, hipStream_t st, bf16* out_bf16) {
    return conv3d_full(in, w_packed, bias, resid, out, out_bf16, nullptr, nullptr, 0, 0, B, ID, IH, IW, Cin, Cout, stride, pad, st);
}

}  // namespace rald
