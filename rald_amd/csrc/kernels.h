// Internal launch interface of the kernel files (not part of the C-ABI; include/rald_hip.h is).
#pragma once
#include <cstdlib>
#include <vector>

#include "common.h"

namespace rald {

// ---------------------------------------------------------------- gemm.hip
enum { GEMM_NT_STORE = 64 };  // GemmArgs::flags: streamed (system-scope, non-temporal) bf16 output stores of the LDS-DMA engines
enum { EPI_BF16 = 0, EPI_F32 = 1, EPI_RESID = 2, EPI_GEGLU = 3,
       EPI_SOFTMAX64 = 4,
       EPI_F16S = 5 };        // C_fp16 = 2^-6 (alpha*acc + bias), saturating: split-K slabs for reduce_resid_ln(part_f16) (norm.hip)   // C_bf16 = softmax over every aligned group of 64 output columns of alpha*acc, in exp2 units (folded cross-attention, dit.hip)
struct GemmArgs {
    const bf16* A; int64_t lda; int64_t strideA;   // [batch][M][K] activations (K contiguous)
    const bf16* B; int64_t ldb; int64_t strideB;   // [batch][N][K] weights     (K contiguous)
    void* C;       int64_t ldc; int64_t strideC;   // bf16 or f32, see epilogue
    const float* bias;                             // [N] or nullptr
    int M, N, K, batch;
    float alpha;
    int alpha_ncols;                               // alpha applies to output columns n < alpha_ncols only (others use 1)
    int flags;                                     // GEMM_NT_STORE or 0 (gemm_nt and the MXFP8 GEMM set it on every launch)
    // optional inner batch (attention heads): grid z = batch * batch2, blockIdx.z = b1 * batch2 + b2,
    // operand offset = b1 * stride + b2 * stride2
    int batch2 = 1;
    int64_t strideA2 = 0, strideB2 = 0, strideC2 = 0;
    // optional MXFP8 form of a bf16 / GEGLU output INSTEAD of C: e4m3 [M][ldc] + e8m0 scales [M][ncols/32] (batch 1 only)
    unsigned char *out8 = nullptr, *outs = nullptr;
};
#ifdef __HIPCC__
__device__ __forceinline__ void gemm_batch_offsets(const GemmArgs& a, int bz, int64_t& oa, int64_t& ob, int64_t& oc) {
    const int b1 = bz / a.batch2, b2 = bz - b1 * a.batch2;
    oa = (int64_t)b1 * a.strideA + (int64_t)b2 * a.strideA2;
    ob = (int64_t)b1 * a.strideB + (int64_t)b2 * a.strideB2;
    oc = (int64_t)b1 * a.strideC + (int64_t)b2 * a.strideC2;
}
#endif
int gemm_nt(const GemmArgs& a, int epi, hipStream_t st);
// test entry: a full-tile bf16 problem (EPI_BF16 / EPI_GEGLU, batch 1) on 256 x 256 tiles at any tile count: the persistent engine on at most
// max_workgroups workgroups, or with persistent == 0 the one-tile LDS-DMA kernel
int gemm_nt_256_test(const GemmArgs& a, int epi, int persistent, int max_workgroups, hipStream_t st);
// the same with a.batch entries (strideA / strideB / strideC; batch2 must be 1) and EPI_SOFTMAX64 as a third epilogue; the persistent engine
// takes a batch for EPI_SOFTMAX64 only
int gemm_nt_256_batched_test(const GemmArgs& a, int epi, int persistent, int max_workgroups, hipStream_t st);
// diagnostic: lanes that clamped an fp16 slab value since the last reset (EPI_F16S here, the per-head slabs in attn_small.hip); blocking
int f16_saturation_gemm(unsigned* count, bool reset);
int f16_saturation_attn(unsigned* count, bool reset);
// EPI_F16S exists on the LDS-DMA engines only: true when gemm_nt would run this shape on one of them (else use EPI_F32)
inline bool gemm_f16s_ok(int M, int N, int batch) {
    const int64_t w128 = (int64_t)((M + 127) / 128) * ((N + 127) / 128) * batch, w64 = (int64_t)((M + 63) / 64) * ((N + 63) / 64) * batch;
    return w128 >= 192 || w64 <= 256;
}
inline GemmArgs gemm_args(const bf16* A, int64_t lda, const bf16* B, int64_t ldb, void* C, int64_t ldc,
                          const float* bias, int M, int N, int K) {
    GemmArgs g;
    g.A = A; g.lda = lda; g.strideA = 0; g.B = B; g.ldb = ldb; g.strideB = 0;
    g.C = C; g.ldc = ldc; g.strideC = 0; g.bias = bias; g.M = M; g.N = N; g.K = K; g.batch = 1; g.alpha = 1.f; g.alpha_ncols = 1 << 30; g.flags = 0;
    return g;
}

// ---------------------------------------------------------------- gemm_ln.hip
// x[M][512] += A[M][K].W[512][K]^T + bias ;  h = LN(x) * (add_one + g[s]) + b[s]  (s = row / rows_per_group * gstride)
struct GemmLnArgs {
    const bf16* A; int64_t lda;
    const bf16* W; int64_t ldw;
    const float* bias;
    float* x;                 // [M][512] fp32, updated in place
    bf16* h;                  // [M][512] bf16 out (skipped when h8 is set)
    unsigned char* h8 = nullptr;   // optional MXFP8 form of h instead: e4m3 [M][512] ...
    unsigned char* hs = nullptr;   // ... + e8m0 scales [M][16]
    int nt_io = 1;                 // non-temporal residual / output traffic
    // MXFP8 operands instead of A / W when A8 is set: e4m3 [M][K], [512][K] + e8m0 scales [..][K/32]; lda/ldw in elements
    const unsigned char *A8 = nullptr, *SA = nullptr, *W8 = nullptr, *SW = nullptr;
    const float* g; const float* b; int64_t gstride; int rows_per_group; float add_one, eps;
    int M, K;
    // optional per-group weights (bf16 operands): rows [i*w_rows, (i+1)*w_rows) multiply W + i*strideW (w_rows a multiple of 128)
    int64_t strideW = 0; int w_rows = 1 << 30;
};
int gemm_resid_ln(const GemmLnArgs& a, hipStream_t st);
// true when the fused kernel beats GEMM + separate LayerNorm (measured on MI355X, tools/bench_resid_ln.py and
// whole-NFE sweeps: wins from M = 16384 on for K = 512 and K = 2048, +1 % per NFE at B = 32; at M = 8192 it loses)
inline bool gemm_resid_ln_pays(int M, int K = 512) { (void)K; return M >= 16384; }
// bf16 operands, h in bf16 (set h8 / hs for MXFP8, A8 / SA / W8 / SW for MXFP8 operands); eps = 1e-5 (nn.LayerNorm's default)
inline GemmLnArgs gemm_ln_args(const bf16* A, int64_t lda, const bf16* W, int64_t ldw, const float* bias, float* x, bf16* h,
                               const float* g, const float* b, int64_t gstride, int rows_per_group, float add_one, int M, int K) {
    GemmLnArgs a;
    a.A = A; a.lda = lda; a.W = W; a.ldw = ldw; a.bias = bias; a.x = x; a.h = h;
    a.g = g; a.b = b; a.gstride = gstride; a.rows_per_group = rows_per_group; a.add_one = add_one; a.eps = 1e-5f; a.M = M; a.K = K;
    return a;
}
// x[M][n] += A.W^T + bias, then (a.g set) the LayerNorm of GemmLnArgs: the engine choice of every residual projection of the latent stacks.
// Split-K (resid_splitk_ln through `scratch`, splitk_for) when the operands are bf16 and the LN output is not MXFP8; else the fused
// gemm_resid_ln where it pays; else gemm_nt (EPI_RESID; batched over the weight groups of a.strideW) + a separate LayerNorm.  The first
// two own whole 512-wide rows (n = 512 only); MXFP8 operands need the fused kernel.
int resid_gemm_ln(const GemmLnArgs& a, int n, float* scratch, hipStream_t st);

// radar_train.hip: out [B*D*H*W][32] bf16 = the 27-neighbourhood (zero outside the volume) of channel 0 of cube [B][D][H][W][cube_ch], 5 zero pads
int patches27(const float* cube, int cube_ch, bf16* out, int B, int D, int H, int Wd, hipStream_t st);
// ---------------------------------------------------------------- gemm_tn.hip
// C[n1][n2] += sum_m A[m][n1] . B[m][n2] (fp32, atomics); colsum (optional) [n1] += sum_m A[m][n1].  Weight / bias gradient of a Linear.
int gemm_tn(const bf16* A, int64_t lda, const bf16* B, int64_t ldb, float* C, int64_t ldc, float* colsum, int M, int N1, int N2, hipStream_t st,
            float* workspace = nullptr, int64_t workspace_floats = 0);
int64_t gemm_tn_workspace_floats(int M, int N1, int N2);
// the same with B = the virtual patch matrix of a 3x3x3 Conv3d over channels-last x: dW [Cout][Cin][27] += ..., dbias += column sums of dy
int conv3d_wgrad_tn(const bf16* dy, const bf16* x, float* dW, float* dbias, int B, int ID, int IH, int IW, int Cin, int Cout, int stride, int pad,
                    hipStream_t st, float* workspace = nullptr, int64_t workspace_floats = 0);
int64_t conv3d_wgrad_workspace_floats(int B, int ID, int IH, int IW, int Cin, int Cout, int stride, int pad);
// the plan conv3d_wgrad_tn launches with (pure host arithmetic): 1 line kernel, 0 generic kernel, -1 a refused shape
int conv3d_wgrad_route(int B, int ID, int IH, int IW, int Cin, int Cout, int stride, int pad, int* ranges, int* per_range);

// ---------------------------------------------------------------- norm.hip
// out_bf16[m][c] = LN(x[m])[c] * (add_one + g[s][c]) + b[s][c],  s = (m / rows_per_group) * gstride
int layernorm_mod(const float* x, bf16* out, int M, int D, const float* g, const float* b,
                  int64_t gstride, int rows_per_group, float add_one, float eps, hipStream_t st);
// x_f32[m][n] = coef[s].c_in * sum_k xin[m][k] * W[n][k]      (proj_in fused with EDM c_in)
int proj_in(const float* xin, const float* W, float* x, int M, int C, int D, const float* coef,
            int coef_stride, int rows_per_group, hipStream_t st);
// D_x[m][c] = c_skip * xin[m][c] + c_out * sum_k LN_affine(x[m])[k] * Wout[c][k]
int final_norm_proj(const float* x, const float* gamma, const float* beta, const float* Wout,
                    const float* xin, float* out, int M, int D, int C, const float* coef,
                    int coef_stride, int rows_per_group, hipStream_t st, const bf16* Whl = nullptr);
// out [hi | lo][n] bf16 with w = hi + lo (to ~2^-17): the pre-split proj_out weight that final_norm_proj's large-M form takes as Whl
int split_hi_lo(const float* w, bf16* out, int n, hipStream_t st);

// ---------------------------------------------------------------- attention.hip
struct AttnArgs {
    const bf16* Q;  int64_t ldq,  strideQ;     // Q [b][i][h*64+d]
    const bf16* K;  int64_t ldk,  strideK;     // K [b][j][h*64+d]
    const bf16* Vt; int64_t ldvt, strideVt;    // Vt[b][h*hsk+d][j]  (keys contiguous; columns nk .. round_up(nk,64)-1 finite)
    // alternative V operand, row-major like K (V[b][j][h*64+d]): set V and leave Vt null; needs nk % 64 == 0.  Read through
    // ds_read_b64_tr_b16, so a fused q|k|v projection can feed the kernel without a transposed copy of V.
    const bf16* V = nullptr; int64_t ldv = 0, strideV = 0;
    // key split (few queries x many keys, e.g. 512 latents x 10 000 points at batch 1): ksplit > 1 workgroups share a query block,
    // each takes a contiguous range of key tiles and writes unnormalised partials to `part` (attention_split_scratch_bytes),
    // a second kernel combines them.  0 / 1 = off; attention_pick_ksplit() suggests a value.
    int ksplit = 1; float* part = nullptr;
    bf16* O;        int64_t ldo,  strideO;     // O [b][i][h*64+d]
    int nq, nk, heads, batch;
    int k_rows;                                // rows allocated per batch in K (>= round_up(nk,64): the tail tile reads them)
    float scale;                               // softmax scale; ignored when q_prescaled
    int q_prescaled;                           // Q already multiplied by scale*log2(e) (done for free in the producing GEMM's epilogue)
    // fp16 form (the folded set-encoder attention, ae_encode.hip): K and V point at fp16 data, the queries are fp32 in Qf (same
    // ldq / strideQ, in elements), converted on load.  Needs q_prescaled and the row-major V.
    int f16 = 0; const float* Qf = nullptr;
    int hsk = 64;                              // column offset between the heads' K / V slices; 0 = every head reads the same 64 columns
    int v_padded = 0;                          // row-major V: rows nk .. k_rows-1 are ZERO (the caller's contract), so nk need not be a multiple of 64
};
int attention_d64(const AttnArgs& a, hipStream_t st);
// self-attention of n tokens per sample over a fused projection qkv [batch][n][q | k | v of `inner` columns each] (q prescaled,
// V row-major) into O [batch][n][inner]
inline AttnArgs self_attn_args(const bf16* qkv, bf16* O, int n, int inner, int heads, int batch, float scale) {
    AttnArgs a;
    a.Q = qkv; a.ldq = 3 * inner; a.strideQ = (int64_t)n * 3 * inner;
    a.K = qkv + inner; a.ldk = 3 * inner; a.strideK = (int64_t)n * 3 * inner;
    a.Vt = nullptr; a.ldvt = 0; a.strideVt = 0;
    a.V = qkv + 2 * inner; a.ldv = 3 * inner; a.strideV = (int64_t)n * 3 * inner;
    a.O = O; a.ldo = inner; a.strideO = (int64_t)n * inner;
    a.nq = n; a.nk = n; a.k_rows = n; a.heads = heads; a.batch = batch; a.scale = scale; a.q_prescaled = 1;
    return a;
}
int attention_pick_ksplit(int nq, int nk, int heads, int batch);
inline int64_t attention_split_scratch_bytes(int ksplit, int nq, int heads, int batch) { return (int64_t)ksplit * batch * heads * nq * 66 * 4; }

// ---------------------------------------------------------------- attn_bwd.hip (training: gradients of the attention above)
// dQ, dK, dV of O = softmax(Q K^T scale) V per head; every operand bf16 [b][row][h*64 + d] with its row and batch strides (column
// slices of fused buffers are fine).  lse / delta: fp32 scratch of batch*heads*nq elements each (written, then read).
struct AttnBwdArgs {
    const bf16 *Q, *K, *V, *O, *dO;
    int64_t ldq, sq, ldk, sk, ldv, sv, ldo, so, lddo, sdo;
    bf16 *dQ, *dK, *dV;
    int64_t lddq, sdq, lddk, sdk, lddv, sdv;
    float *lse, *delta;
    int nq, nk, heads, batch;
    float scale;
};
int attention_bwd_d64(const AttnBwdArgs& a, hipStream_t st);

// ---------------------------------------------------------------- ae_train.hip (autoencoder training: no float atomics)
int64_t ln_affine_bwd_scratch_bytes(int64_t rows);
int ln_affine_bwd(const float* x, const float* dh, const float* g, float eps, int64_t rows, float* dx, bf16* dx_bf16, float* dgamma, float* dbeta,
                  float* scratch, int64_t scratch_bytes, hipStream_t st);
int64_t pe_wgrad_scratch_bytes(int64_t rows);
int pe_wgrad(const float* dY, const float* pts, const float* basis, int64_t rows, float* dW, float* db, float* scratch, int64_t scratch_bytes,
             hipStream_t st);
int posterior_bwd(const float* dz, const float* dkl, const float* ml, const float* eps, float* dml, int B, int rows, int L, hipStream_t st);
int scale_rows(const float* in, const float* s, float* x_accum, bf16* out_bf16, int64_t rows, int cols, int64_t rows_per_sample, hipStream_t st);
int64_t ae_loss_scratch_bytes(int batch, int64_t n_queries);
int ae_loss(const float* logits, const float* labels, const float* kl, const int32_t* n_dev, int batch, int64_t Q, float vol_w, float near_w,
            float kl_w, float grad_scale, double* losses4, int32_t* counts3, float* dlogits, float* dkl, void* scratch, int64_t scratch_bytes,
            hipStream_t st);
int softmax_bwd_rows(const float* S, const float* dP, const float* delta, int64_t rows, int64_t ld, int n, float scale, bf16* P, bf16* dS,
                     hipStream_t st);

// ---------------------------------------------------------------- attn_small.hip (<= 2048 rows: fused per-head sub-blocks)
// part[h][row][512] = (softmax(q_h k_h^T) v_h) . Wo[:, 64h:64h+64]^T  for the fused q|k|v buffer of a self-attention
int attn_self_proj(const bf16* qkv, int64_t ld, const bf16* Wo, float* part, int NL, int heads, int batch, hipStream_t st, bool part_f16 = false);
// part[h][row][512] = (softmax(to_q(hin)_h Kc_h^T) Vc_h) . Wo[:, 64h:64h+64]^T against 64 cached condition tokens
int xattn_q2_proj(const bf16* hin, const bf16* Wq, const bf16* Kc, int64_t ldk, int64_t strideK, const bf16* Vt, int64_t ldvt, int64_t strideVt,
                  const bf16* Wo, float* part, int M, int NL, int heads, int n_keys, float qscale, hipStream_t st, bool part_f16 = false);
// x[M][512] += bias + sum_s part[s]; optionally h = LN(x) * (add_one + g) + b  (norm.hip; deterministic order)
// (part_f16: the slabs are fp16 scaled by 2^-6, as attn_self_proj / xattn_q2_proj write them with part_f16; S = 8 only)
int reduce_resid_ln(const float* part, int S, int64_t part_stride, const float* bias, float* x, bf16* h, int M, const float* g, const float* b,
                    int64_t gstride, int rows_per_group, float add_one, float eps, hipStream_t st, bool part_f16 = false);
// row count up to which the fused small-batch sub-blocks are used (measured on MI355X, tools/sweep_nfe.py: per NFE at B = 1 / 2 / 4
// 1.41 / 1.70 / 2.59 ms fused against 1.64 / 1.89 / 2.27 ms unfused - from 2048 rows on the plain kernels fill the chip)
inline bool small_m_fused(int M, int NL, int heads, int D, int n_keys) { return M <= 1024 && NL == 512 && heads == 8 && D == 512 && n_keys == 64; }

// ---------------------------------------------------------------- small.hip
enum { ACT_NONE = 0, ACT_SILU = 1 };
// out[s][n] = act(sum_k in[s][k] * W[n][k] + bias[n]); fp32 throughout, S small (t-embed path)
int skinny_linear(const float* in, const float* W, const float* bias, float* out, int S, int N, int K,
                  int act, hipStream_t st);
// pe[s][0:128] = cos(c_noise[s]*f_i), pe[s][128:256] = sin(..)   (PositionalEmbedding)
int positional_embedding(const float* c_noise, float* pe, int S, int channels, hipStream_t st);
int cast_f32_bf16(const float* in, bf16* out, int64_t n, hipStream_t st);
// diagnostic: fills the LDS of every CU with NaN patterns (see small.hip)
int poison_lds(hipStream_t st);
// dst_bf16[map(r)][c] = src_f32[r][c] ; map==nullptr -> identity; ld_dst >= cols (pad zero-filled by caller)
int pack_rows_bf16(const float* src, bf16* dst, int rows, int cols, int64_t ld_dst, const int* rowmap, hipStream_t st);
int scale_f32(const float* in, float* out, float s, int64_t n, hipStream_t st);
// Heun/Euler updates of edm_sampler (models_radar_generation.py:265-273)
int heun_euler(const float* x_hat, const float* denoised, float t_hat, float t_next, float* d_cur,
               float* x_next, int64_t n, hipStream_t st);
int heun_correct(const float* x_hat, const float* x_euler, const float* denoised, const float* d_cur,
                 float t_hat, float t_next, float* x_next, int64_t n, hipStream_t st);

// ---------------------------------------------------------------- rng.hip
// out[b][0:n_per_sample] = N(0,1) from Philox4x32-10, key (seeds[b] mod 2^32, tag), counter (element / 4, step, 0, 0); seeds on the device
int philox_normal(const int64_t* seeds, int B, int64_t n_per_sample, int tag, int step, float* out, hipStream_t st);
// the churn step of edm_sampler (:260) in place: x[b] += scale * n[b], n = noise [B][n_per_sample] or generated from seeds (tag 1, `step`)
int churn_noise(float* x, const float* noise, const int64_t* seeds, int B, int64_t n_per_sample, int step, float scale, hipStream_t st);
// host: Karras levels t [num_steps + 1] (t_N = 0) and churned levels t_hat [num_steps] (:246-249, :258-259)
int edm_schedule(int num_steps, double smin, double smax, double rho, double S_churn, double S_min, double S_max, float* t, float* t_hat);

// ---------------------------------------------------------------- ae_kernels.hip
int point_features(const float* pts, const float* basis, bf16* feat, int64_t n, hipStream_t st);
int softmax_rows(const float* S, int64_t ld_s, bf16* P, int64_t ld_p, int rows, int n, hipStream_t st);
int softmax_dot(const float* S, const float* u, float* out, int64_t rows, int nkeys, int rows_per_batch, float c0, hipStream_t st);
int ln_dot(const float* x, const float* gamma, const float* beta, const float* w, float* out, int M, int D, hipStream_t st);
int add_bcast_cast(const float* a, const float* d, bf16* out, int64_t per_batch, int batch, hipStream_t st);
int posterior(const float* ml, const float* eps, float* mean_o, float* logvar_o, float* z, float* kl, int B, int rows, int L, hipStream_t st);
int small_k_linear(const float* in, const float* W, const float* bias, float* out, int M, int K, int N, hipStream_t st);

#ifdef __HIPCC__
// y[r][lane] = sum_c xs[r][c] * T[c*64 + lane] for the 4 rows a 4-wave workgroup holds (normalised) in LDS: wave w sums the K-quarter
// [w*D/4, (w+1)*D/4) for ALL 4 rows - each table element is fetched once per workgroup instead of once per row (one wave per row read the
// whole 128-KiB table per row: 64 MB of L2 traffic for 512 rows) - and the partials meet in LDS.  Returns row w's 64 outputs on wave w.
template <int D>
__device__ __forceinline__ float project4_rows(const float (*xs)[D], const float* __restrict__ T, float (*red)[4][64], int lane, int w) {
    constexpr int KQ = D / 4;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int c = w * KQ; c < (w + 1) * KQ; c += 32) {
        float t[32];
#pragma unroll
        for (int j = 0; j < 32; ++j) t[j] = T[(c + j) * 64 + lane];
#pragma unroll
        for (int j = 0; j < 32; ++j) {
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] = fmaf(xs[r][c + j], t[j], acc[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) red[w][r][lane] = acc[r];
    __syncthreads();
    return (red[0][w][lane] + red[1][w][lane]) + (red[2][w][lane] + red[3][w][lane]);
}
#endif

// ---------------------------------------------------------------- ae_encode.hip (folded encoder attentions)
int ae_embed_factor(int d, const float* Wpe, const float* bpe, std::vector<double>& Wc, std::vector<double>& R);
int ae_encode_tables(int d, int I, int M, int heads, bool mixq, const float* Wpe, const float* bpe, const float* d_lat, const float* mng,
                     const float* mnb, const float* mWq, const float* mWkv, const float* mWo, const float* mbo, const float* lat,
                     const float* Wqp, const float* bqp, const float* cg, const float* cb, const float* cWq, const float* cWkv,
                     const float* cWo, const float* cbo, std::vector<float>& Rf, std::vector<float>& Q1, std::vector<float>& T4,
                     std::vector<float>& X0, std::vector<float>& T1, std::vector<float>& T3, std::vector<float>& c3);
int ae_enc_features(const float* pc, const float* basis, const float* Rf, void* F, void* G, int B, int P, int Pp, hipStream_t st);
int ae_enc_qproj(const float* xin, const float* X0, float* x, const float* gamma, const float* beta, const float* T1, float* Qo, int rows, int M,
                 int d, hipStream_t st);
// ---------------------------------------------------------------- ae_decode.hip (streaming query decoder)
// per-sample decoder context: [ fp16 image M x 128 B | u: M floats | inv_scale + 3 pad floats ]
inline int64_t ae_ctx_stride(int M) { return (int64_t)M * 128 + (int64_t)M * 4 + 16; }
int ae_decode_tables(int d, const float* Wq, const float* Wk, const float* ng, const float* nb, const float* Wpe, const float* bpe,
                     const float* wfold, std::vector<float>& t2aug, std::vector<unsigned short>& l_img);   // host, double precision
int ae_ctx_build(const float* x, const float* gamma, const float* beta, const float* t2aug, float* Yscratch, void* ctx, int B, int M, int d,
                 hipStream_t st);
int ae_decode_stream(const void* ctx, const unsigned short* l_img, const float* queries, float* out, const float* basis, int basis_diag,
                     int B, int64_t Q, int M, float c0, hipStream_t st);
// ragged query sets: queries [T][3] / out [T], device offsets [B + 1], max_per_sample = host upper bound of the longest segment
int ae_decode_stream_ragged(const void* ctx, const unsigned short* l_img, const float* queries, const int64_t* offsets, float* out,
                            const float* basis, int basis_diag, int B, int64_t max_per_sample, int M, float c0, hipStream_t st);
// logit + gradient with respect to the query point (+ one clamped Newton step when proj is given): offsets == nullptr -> dense, n queries per
// sample; else ragged with n = the host upper bound of the longest segment.  The logits are ae_decode_stream[_ragged]'s bit for bit.
constexpr int AE_DECODE_GRAD_MAX_LATENTS = 512;     // the second product's transposed image must fit in LDS next to the plain layout
int ae_decode_grad_stream(const void* ctx, const unsigned short* l_img, const float* queries, const int64_t* offsets, float* out, float* grad,
                          float* proj, float max_step, const float* basis, int basis_diag, int B, int64_t n, int M, float c0, hipStream_t st);
// ae_rays.hip: first-return beam casting through the decoder field.  origins / dirs [R][3] (ray_batch_stride 0) or
// [B][R][3] (3 * R); every logit is ae_decode_stream's on the same points, bit for bit.  out_points may be null.
int ae_cast_rays(const void* ctx, const unsigned short* l_img, const float* origins, const float* dirs, int64_t ray_batch_stride,
                 const float* basis, int basis_diag, int B, int R, int M, int n_steps, int n_refine, float c0, float* out_t, float* out_logit,
                 int* out_step, float* out_points, hipStream_t st);
// basis_diag of a host copy of point_embed.basis [3][24]: 1 when it is block-diagonal (x -> columns 0-7, y -> 8-15, z -> 16-23), which
// makes a projection one multiply instead of three; the one rule by which every caller picks the streaming kernel's form
inline int ae_basis_is_block_diagonal(const float* basis_host) {
    for (int a = 0; a < 3; ++a)
        for (int e = 0; e < 24; ++e)
            if (e / 8 != a && basis_host[a * 24 + e] != 0.f) return 0;
    return 1;
}
// scratch of one rald_op_ae_decode call: projection [B*M][64] fp32 + one |max| word per sample, then the B contexts (16-byte aligned)
inline int64_t ae_decode_op_ctx_offset(int B, int M) { return ((int64_t)B * M * 64 * 4 + (int64_t)B * 4 + 15) / 16 * 16; }
inline int64_t ae_decode_op_scratch_bytes(int B, int M) { return ae_decode_op_ctx_offset(B, M) + (int64_t)B * ae_ctx_stride(M); }

// ---------------------------------------------------------------- post.hip
int post_scratch_ints(int64_t Q);
void post_scan_counts(int* counts, int nblocks, int64_t* total, hipStream_t st);   // exclusive scan of per-block counts
int post_occupied_points(const float* logits, const float* queries, int64_t Q, const double* pc_range_host, int aniso, int iso,
                         int view_cone, float thr, float* out_pts, int64_t* out_idx, int64_t* out_count, int* scratch, hipStream_t st);
int post_transform_points(const float* in, int64_t n, const double* pc_range_host, int aniso, int iso, int view_cone, float* out, hipStream_t st);
// post_transform_points + unit normals -J^-T g / |.| of the gradients g taken in normalised coordinates (J = d metric / d normalised)
// (offsets: nullptr, or the device [B + 1] row offsets of a ragged batch of worst-case size n: rows from offsets[B] on are not written)
int post_oriented_points(const float* in, const float* grad, int64_t n, const int64_t* offsets, int B, const double* pc_range_host, int aniso,
                         int iso, int view_cone, float* out_pts, float* out_normals, hipStream_t st);
int post_chamfer_sums(const float* a, int64_t na, const float* b, int64_t nb, double* sums, hipStream_t st);
// ragged batches: concatenated rows + device int64 offsets [B + 1]; no host read
int post_occupied_points_ragged(const float* logits, const float* queries, const int64_t* in_offsets, int B, int64_t T,
                                const double* pc_range_host, int aniso, int iso, int view_cone, float thr, float* out_pts, int64_t* out_idx,
                                int64_t* out_offsets, int* scratch, hipStream_t st);
int post_chamfer_sums_ragged(const float* a, const int64_t* a_off, const float* b, const int64_t* b_off, int B, int64_t max_a, int64_t max_b,
                             double* sums, hipStream_t st);
int post_iou(const float* logits, const float* labels, int B, int64_t Q, float* acc, float* iou, hipStream_t st);
int radar_cube_prepare(const float* raw, int B, int R, int A, int E, int Craw, int tA, int tE, int norm_i, float max_i, int norm_d,
                       float max_d, float* out, hipStream_t st);

// ---------------------------------------------------------------- cloud_metrics.hip
// exact nearest neighbours (fp64) of ragged batches, per row and reduced per frame; scratch: the *_scratch_bytes of the same arguments
int64_t cloud_metrics_scratch_bytes(int B, int64_t max_pred, int64_t max_gt);
int64_t cloud_nn_scratch_bytes(int B, int64_t max_a, int64_t max_b, int64_t b_chunk);     // b_chunk 0: the automatic chunk length
int cloud_nn_ragged(const float* a, const int64_t* a_off, const float* b, const int64_t* b_off, int B, int64_t max_a, int64_t max_b, int64_t b_chunk,
                    double* out_dist, int64_t* out_idx, void* scratch, int64_t scratch_bytes, hipStream_t st);
int cloud_metrics_ragged(const float* pred, const int64_t* pred_off, const float* gt, const int64_t* gt_off, int B, int64_t max_pred, int64_t max_gt,
                         const double* thresholds_host, int n_thr, double* out_raw, double* out_dist_pred, int64_t* out_idx_pred,
                         double* out_dist_gt, int64_t* out_idx_gt, void* scratch, hipStream_t st);

// ---------------------------------------------------------------- fps.hip
// farthest-point sampling of a ragged batch, one workgroup per cloud; form 0 auto, 1 resident, 2 streaming (scratch: fps_scratch_bytes)
int64_t fps_scratch_bytes(int B, int64_t max_per_sample, int form);
int fps_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int B, int64_t n_dense, int64_t max_per_sample, int k,
               const int64_t* start, const float* scale3_host, int64_t* out_idx, float* out_dist2, void* scratch, int64_t scratch_bytes, int form,
               hipStream_t st);

// ---------------------------------------------------------------- voxel_reduce.hip, radius_search.hip, knn_search.hip
// the grid-indexed operations on ragged clouds (include/rald_hip.h, DESIGN.md sections 21 - 23).  The layout and the grid come as the
// two structs of cloud_index.h, which also holds the index, the compaction and the device helpers they share; chunk 0 = automatic, else
// a multiple of 1024; every *_scratch_bytes is -1 for sizes the calls refuse
struct RaggedCloud;
struct GridSpec;
int voxel_passes(int64_t cells);                   // radix passes of 8 bits for keys 0 .. cells; -1 outside 1 .. 2^31 - 1
// voxel-grid down-sampling: one centroid per occupied cell, ascending key
int64_t voxel_scratch_bytes(int B, int64_t n_total, int64_t max_per_sample, int64_t chunk);
int voxel_downsample_ragged(const RaggedCloud& c, const GridSpec& grid, float* out_points, int64_t* out_offsets, int32_t* out_count,
                            int64_t* out_first, int32_t* out_cells, int64_t* out_inverse, void* scratch, int64_t scratch_bytes, int64_t chunk,
                            hipStream_t st);
// fixed-radius neighbour counts (and the nearest other row) inside each cloud, and the radius outlier filter on them
int64_t radius_scratch_bytes(int B, int64_t n_total, int64_t max_per_sample, int64_t chunk);
int radius_count_ragged(const RaggedCloud& c, const GridSpec& grid, float radius, int max_count, int32_t* out_count, int64_t* out_nn_idx,
                        float* out_nn_dist2, void* scratch, int64_t scratch_bytes, int64_t chunk, hipStream_t st);
int radius_filter_ragged(const RaggedCloud& c, const GridSpec& grid, float radius, int min_neighbors, float* out_points, int64_t* out_offsets,
                         int64_t* out_index, int32_t* out_count, void* scratch, int64_t scratch_bytes, int64_t chunk, hipStream_t st);
// k nearest other rows inside each cloud, and the statistical outlier filter on their mean distance
int64_t knn_scratch_bytes(int B, int64_t n_total, int64_t max_per_sample, int64_t chunk);
int knn_ragged(const RaggedCloud& c, const GridSpec& grid, int k, float max_radius, int64_t* out_idx, float* out_dist2, int32_t* out_found,
               void* scratch, int64_t scratch_bytes, int64_t chunk, hipStream_t st);
int64_t statistical_scratch_bytes(int B, int64_t n_total, int64_t max_per_sample, int64_t chunk);
int statistical_filter_ragged(const RaggedCloud& c, const GridSpec& grid, int k, float max_radius, double std_ratio, float* out_points,
                              int64_t* out_offsets, int64_t* out_index, double* out_mean, double* out_stats, void* scratch,
                              int64_t scratch_bytes, int64_t chunk, hipStream_t st);

// ---------------------------------------------------------------- cloud_normals.hip
// PCA normals, surface variation and covariance eigenvalues from the k nearest other rows (the search of knn_search.h, no [n, k] table),
// and the normal consistency of two ragged batches with normals on cloud_nn_ragged's neighbours
int64_t normals_scratch_bytes(int B, int64_t n_total, int64_t max_per_sample, int64_t chunk);
int normals_ragged(const RaggedCloud& c, const GridSpec& grid, int k, float max_radius, const float* view3_host, float* out_normals,
                   float* out_curvature, float* out_eigenvalues, int32_t* out_found, void* scratch, int64_t scratch_bytes, int64_t chunk,
                   hipStream_t st);
int64_t normal_consistency_scratch_bytes(int B, int64_t n_pred_total, int64_t n_gt_total, int64_t max_pred, int64_t max_gt);
int normal_consistency_ragged(const float* pred, const float* pred_normals, const int64_t* pred_off, int64_t n_pred_total, const float* gt,
                              const float* gt_normals, const int64_t* gt_off, int64_t n_gt_total, int B, int64_t max_pred, int64_t max_gt,
                              double* out_nc, int64_t* out_counts, void* scratch, int64_t scratch_bytes, hipStream_t st);

// ---------------------------------------------------------------- cloud_cluster.hip
// density clustering (DBSCAN) on the radius search's neighbourhoods: labels in a canonical numbering, and the filter that keeps the
// clusters of at least min_cluster_size rows or the largest one
int64_t cluster_scratch_bytes(int B, int64_t n_total, int64_t max_per_sample, int64_t chunk);
int cluster_labels_ragged(const RaggedCloud& c, const GridSpec& grid, float eps, int min_points, int32_t* out_labels, int32_t* out_num_clusters,
                          int32_t* out_sizes, int32_t* out_count, void* scratch, int64_t scratch_bytes, int64_t chunk, hipStream_t st);
int cluster_filter_ragged(const RaggedCloud& c, const GridSpec& grid, float eps, int min_points, int min_cluster_size, int largest_only,
                          float* out_points, int64_t* out_offsets, int64_t* out_index, int32_t* out_labels, int32_t* out_num_clusters,
                          void* scratch, int64_t scratch_bytes, int64_t chunk, hipStream_t st);

// ---------------------------------------------------------------- cloud_plane.hip
// RANSAC plane segmentation with a fixed number of counter-based hypotheses, up to max_planes planes peeled in turn, and the filter that
// keeps the planes' rows or everything else
int64_t plane_scratch_bytes(int B, int64_t n_total, int64_t max_per_sample, int num_hypotheses, int max_planes);
int plane_segment_ragged(const RaggedCloud& c, float threshold, int num_hypotheses, int max_planes, int min_inliers, int refine, int64_t seed,
                         const float* view3_host, int32_t* out_labels, double* out_planes, int32_t* out_num_planes, int32_t* out_inliers,
                         int32_t* out_best, void* scratch, int64_t scratch_bytes, hipStream_t st);
int plane_filter_ragged(const RaggedCloud& c, float threshold, int num_hypotheses, int max_planes, int min_inliers, int refine, int64_t seed,
                        const float* view3_host, int keep_planes, float* out_points, int64_t* out_offsets, int64_t* out_index,
                        int32_t* out_labels, double* out_planes, int32_t* out_num_planes, void* scratch, int64_t scratch_bytes, hipStream_t st);

// ---------------------------------------------------------------- cloud_icp.hip
// ICP registration of every source cloud onto the target cloud of the same batch position, point-to-point (mode 0) or point-to-plane
// (mode 1), iterated on the device, and the rigid transform of a ragged batch by per-cloud float64 transforms
int64_t icp_scratch_bytes(int B, int64_t n_src_total, int64_t max_src, int64_t n_tgt_total, int64_t max_tgt, int64_t chunk);
int icp_ragged(const RaggedCloud& src, const RaggedCloud& tgt, const float* target_normals, const GridSpec& grid, int mode, float max_dist,
               int max_iterations, double tolerance, int min_correspondences, const double* init, double* out_transform, double* out_stats,
               int32_t* out_info, int64_t* out_corr, float* out_moved, void* scratch, int64_t scratch_bytes, int64_t chunk, hipStream_t st);
int rigid_transform_ragged(const RaggedCloud& c, const double* transforms, int stride, const float* normals, float* out_points,
                           float* out_normals, hipStream_t st);

// ---------------------------------------------------------------- surface_nets.hip
// naive surface nets on a batch of dense volumes: one vertex per sign-changing cell, two triangles per sign-changing grid edge with four
// cells around it, counted and ordered on 64-bit sign words
int64_t surface_scratch_bytes(int B, int nx, int ny, int nz);
int surface_nets(const float* volume, int B, const int32_t* dims3_host, const float* lo3_host, const float* spacing3_host, float iso,
                 float* out_vertices, int64_t* out_v_offsets, int64_t max_vertices, int32_t* out_faces, int64_t* out_f_offsets,
                 int64_t max_faces, int32_t* out_cells, void* scratch, int64_t scratch_bytes, hipStream_t st);

// ---------------------------------------------------------------- query.hip
// the nodes of x-planes i0 .. i0 + ni - 1 of a regular grid, [ni * ny * nz, 3], z fastest
int query_grid(const float* lo3_host, const float* spacing3_host, const int32_t* dims3_host, int i0, int ni, float* out, hipStream_t st);
int query_uniform(const double* u, int64_t n, const double* pc_range, int aniso, int iso, float* out, hipStream_t st);
int query_uniform_cart(const double* u, int64_t n, const double* range_cart, const double* range_polar, int aniso, int iso, float* out,
                       int64_t* out_count, int* scratch, hipStream_t st);
int query_norm_points(const float* in, int64_t n, const double* pc_range, int aniso, int iso, float* out, hipStream_t st);
int query_refine(const float* pred, int64_t n_pred, int64_t aug_num, const int64_t* sel, const int64_t* scales, const double* u,
                 const double* pc_range, const double* voxel, int aniso, int iso, int normalise, float* out, hipStream_t st);
int query_refine_ragged(const float* points, const int64_t* offsets, int B, int64_t aug_num, const int64_t* sel, const double* u_sel,
                        const int64_t* scales, const double* u, const double* pc_range, const double* voxel, int aniso, int iso, int normalise,
                        float* out, int64_t* out_offsets, hipStream_t st);

// ---------------------------------------------------------------- gemm_fp8.hip (MXFP8: e4m3 + e8m0 per 32 K-elements)
struct Mx8Args {
    GemmArgs g;                                    // shapes / C / bias / alpha as for gemm_nt; g.A, g.B unused; lda/ldb/strides in bytes
    const unsigned char *A8, *B8;                  // [batch][M][K], [batch][N][K] e4m3
    const unsigned char *SA, *SB;                  // [batch][M][K/32], [batch][N][K/32] e8m0
    int64_t strideSA, strideSB;
};
int gemm_mx8(const Mx8Args& a, int epi, hipStream_t st);
int gemm_mx8_tile(int M, int N, int batch);        // 256 or 128: the tile gemm_mx8 runs such a problem on
int quantize_mx8(const void* in, int in_is_bf16, int64_t ld_in, unsigned char* q, int64_t ld_q, unsigned char* scales, int64_t rows, int K,
                 hipStream_t st);
// small-M split-K residual GEMM + (optional) LayerNorm: see norm.hip.  splitk_for() = 0 when it does not pay.
int resid_splitk_ln(const bf16* A, int64_t lda, const bf16* W, int64_t ldw, const float* bias, float* x, bf16* h, const float* g, const float* b,
                    int64_t gstride, int rows_per_group, float add_one, float eps, int M, int K, int splits, float* scratch, hipStream_t st);
constexpr int splitk_max_rows() { return 4096; }   // the row count up to which split-K pays
inline int splitk_for(int M, int K) { return (K >= 2048 && M <= splitk_max_rows()) ? 4 : 0; }   // [M,512] outputs: few 128x128 tiles
int layernorm_mod_mx8(const float* x, unsigned char* q, unsigned char* scales, int64_t rows, int D, const float* gam, const float* bet,
                      int64_t gstride, int rows_per_group, float add_one, float eps, hipStream_t st);

// ---------------------------------------------------------------- train_kernels.hip (backward building blocks)
struct TransposeArgs {
    const void* in; int64_t ld_in, stride_in, stride_in2;     // [batch][batch2][rows][cols] f32 or bf16
    bf16* out;      int64_t ld_out, stride_out, stride_out2;  // [batch][batch2][cols][rows] bf16
    int rows, cols, batch, batch2;
};
int transpose_rows(const TransposeArgs& a, int in_is_bf16, hipStream_t st);
int ln_mod_bwd(const float* x, const float* dh, const float* s, int64_t gstride, int rows_per_group, float add_one, float eps, int64_t rows,
               int D, float* dx, float* ds, float* dt, hipStream_t st, bf16* dx_bf16 = nullptr);
int geglu_fwd(const bf16* u, bf16* hid, int64_t M, int I, hipStream_t st);
int geglu_bwd(const bf16* u, const bf16* dhid, bf16* du, int64_t M, int I, hipStream_t st);
int colsum(const void* X, int is_bf16, int64_t ld, int64_t M, int N, float* out, hipStream_t st);
int row_lse(const float* S, int64_t rows, int cols, float scale, float* lse, hipStream_t st);
int rowdot_heads(const bf16* dO, const bf16* O, int64_t M, int heads, int nq, float* delta, hipStream_t st);
int attn_bwd_elem(const float* S, const float* dP, const float* lse, const float* delta, int64_t batch, int R, int Cc, int64_t vbatch_stride,
                  int vstride, float scale, int by_col, bf16* P, bf16* dS, hipStream_t st);

int sgemm_acc(const float* A, int64_t lda, int trans_a, const float* B, int64_t ldb, int trans_b, float* Cm, int64_t ldc, int M, int N, int K,
              float alpha, hipStream_t st);
int silu_fwd(const float* x, float* y, int64_t n, hipStream_t st);
int silu_bwd(const float* x, const float* dy, float* dx, int64_t n, hipStream_t st);
int edm_loss_grad(const float* F, const float* xn, const float* y, const float* coef, int64_t per_sample, int64_t total, float* dF, float* D_out,
                  double* loss, hipStream_t st);

// ---------------------------------------------------------------- conv3d.hip (Conv3d k3 of the radar encoder / decoder, op level)
int conv3d_igemm(const bf16* in, const bf16* w_packed, const float* bias, const float* resid, float* out, int B, int ID, int IH, int IW,
                 int Cin, int Cout, int stride, int pad, hipStream_t st, bf16* out_bf16 = nullptr);
// the engine one Conv3d k3 runs on and its split-K count (1 = no split): conv3d_route is the ONE place that decides it, pure host arithmetic
enum ConvEngine { CONV_IGEMM = 0, CONV_LINE = 1, CONV_PLANE = 2, CONV_PPLANE = 3, CONV_IGEMM_SPLIT = 4 };
struct ConvRoute {
    int engine, splits;
    int lw = 0, pds = 0;    // internal, for the launch: log2 of the output line width (line shapes), planes per workgroup (CONV_PPLANE)
};
ConvRoute conv3d_route(int B, int ID, int IH, int IW, int Cin, int Cout, int stride, int pad, int allow_split);
// conv3d_igemm with every field of the kernels' argument block: GroupNorm partials of the output from the epilogue (gn_part), and the
// encoder's split-K route through a caller-owned workspace (allow_split = 1)
int conv3d_full(const bf16* in, const bf16* w_packed, const float* bias, const float* resid, float* out, bf16* out_bf16, double* gn_part,
                float* split_ws, int64_t split_ws_bytes, int allow_split, int B, int ID, int IH, int IW, int Cin, int Cout, int stride, int pad,
                hipStream_t st);
// ---------------------------------------------------------------- radar.hip / radar_train.hip (encoder, op level)
int gn_finish(const double* part, double* stats, int B, int nblk, hipStream_t st);
int upsample2_cast(const float* x, bf16* y, int B, int D, int H, int W, int C, hipStream_t st);
int pad_cast64(const float* z, bf16* y, int64_t rows, int zc, hipStream_t st);
int radar_tokens(const float* z, const float* Wp, const float* bp, const float* re, const float* ae, const float* ee, float* tok, int B, int R, int A,
                 int E, int zc, int C, hipStream_t st);
int groupnorm_fwd(const float* x, const float* gamma, const float* beta, bf16* y, double* stats, int B, int S, int C, int swish, hipStream_t st);
int conv_in_fwd(const float* cube, int cube_ch, int Cin, const float* W, const float* bias, float* out, int B, int D, int H, int Wd, int Cout,
                hipStream_t st);
int conv_pack_weights(const float* W, bf16* out, int Cout, int Cin, int pad_to, int dgrad, hipStream_t st);
int pad_channels(const float* x, bf16* out, int64_t M, int C, int Cpad, hipStream_t st);
int zero_insert2(const float* dy, bf16* out, int B, int OD, int OH, int OW, int C, hipStream_t st);
int groupnorm_bwd(const float* x, const double* stats, const float* gamma, const float* beta, const float* da, float* dx, float* dgamma, float* dbeta,
                  double* gsum_scratch, int B, int S, int C, int swish, int accumulate, hipStream_t st, bf16* dx_bf16 = nullptr, int da_is_bf16 = 0);
int64_t groupnorm_bwd_scratch_bytes(int B, int S, int C);   // what gsum_scratch of groupnorm_bwd must hold
int groupnorm_apply(const float* x, const double* stats, const float* gamma, const float* beta, bf16* y, int B, int S, int C, int swish, hipStream_t st);
int rowdot(const bf16* a, const bf16* b, int64_t M, int C, float* out, hipStream_t st);

// ---------------------------------------------------------------- optim.hip
int optim_grad_sumsq(const float* g, int64_t n, double* out, hipStream_t st);
int optim_clip_coef(const double* sumsq, float pre_scale, float max_norm, float* out2, hipStream_t st);
int optim_adamw_ema(float* p, const float* g, float* m, float* v, float* ema, int64_t n, const float* gscale, double lr, double beta1,
                    double beta2, double eps, double wd, int64_t step, double ema_rate, int write_grad, hipStream_t st);
int optim_ema(float* ema, const float* p, int64_t n, double rate, hipStream_t st);

}  // namespace rald
