// Backward pieces specific to training the set-latent autoencoder (model/models_ae.py: KLAutoEncoder under autograd, the stage-1
// loop engine_ae.py:33-104).  The products run on gemm.hip / gemm_tn.hip and the head-64 attention on attention.hip / attn_bwd.hip;
// this file holds what the AE adds on top of the denoiser's training kernels.  No float atomics anywhere: every reduction over rows
// goes through a workspace of per-workgroup partial sums that a second launch adds in a fixed order, so the gradients of one batch
// are bit-identical run to run.
//
//   ln_affine_bwd     nn.LayerNorm(512) backward with gamma / beta shared by all rows: dx += dLN (fp32, optional bf16 copy),
//                     dgamma += sum dh * xhat, dbeta += sum dh (partials per workgroup of LN_ROWS rows, then ordered column sums)
//   pe_wgrad          PointEmbed.mlp weight gradient (:128-138): dW[o][f] += sum_r dY[r][o] feat_f(p_r), db[o] += sum_r dY[r][o] with the
//                     51 sin / cos / xyz features recomputed from the raw points in LDS (no R x 51 buffer)
//   posterior_bwd     DiagonalGaussianDistribution (:141-163) backward: d[mean | logvar] from dz and dkl[b]; the clamp passes the gradient
//                     where -30 <= logvar <= 20 (torch.clamp's rule); kl is a mean over M * L per sample
//   scale_rows_add    drop-path residual forward: x[r] += s[r / rows_per_sample] * y[r]       (timm DropPath, scale_by_keep)
//   scale_rows_bf16   its backward: out_bf16[r] = s[r / rows_per_sample] * dx[r]               (the branch's gradient)
//   softmax_bwd_rows  the single-head dim-512 attentions' softmax backward on stored fp32 scores: P = softmax(S[r][:n]),
//                     dS = P (dP - delta[r]) * scale as bf16, columns n .. ld zero (keys padded to a multiple of 64 for the GEMMs)
//   ae_loss           the stage-1 loss (engine_ae.py:70-101): BCE-with-logits means over [:, :n] and [:, n:] with n read on the device,
//                     sum(kl) / B, the accuracy / IoU counts per sample, dlogits and dkl; sums in double through ordered partials
#include "common.h"
#include "kernels.h"

namespace rald {

// ------------------------------------------------------------------------------------------------ LayerNorm, affine, D = 512
constexpr int LN_ROWS = 64;                                    // rows per workgroup (4 waves x 16 rows)

__global__ __launch_bounds__(256) void ln_affine_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dh, const float* __restrict__ g,
                                                            float eps, int64_t rows, float* __restrict__ dx, bf16* __restrict__ dx_bf16,
                                                            float* __restrict__ part) {
    __shared__ float red[4][2][512];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c0 = lane * 8;                                   // this lane's 8 columns
    float gv[8], pg[8], pb[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { gv[i] = g[c0 + i]; pg[i] = 0.f; pb[i] = 0.f; }
    const int64_t r0 = (int64_t)blockIdx.x * LN_ROWS;
    for (int k = wave; k < LN_ROWS; k += 4) {
        const int64_t row = r0 + k;
        if (row >= rows) break;
        const float4* xp = reinterpret_cast<const float4*>(x + row * 512 + c0);
        const float4* hp = reinterpret_cast<const float4*>(dh + row * 512 + c0);
        const float4 xa = xp[0], xb = xp[1], ha = hp[0], hb = hp[1];
        const float xv[8] = {xa.x, xa.y, xa.z, xa.w, xb.x, xb.y, xb.z, xb.w};
        const float hv[8] = {ha.x, ha.y, ha.z, ha.w, hb.x, hb.y, hb.z, hb.w};
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) s += xv[i];
        const float mean = wave_sum(s) * (1.0f / 512);
        float v = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) { const float d = xv[i] - mean; v += d * d; }
        const float rstd = rsqrtf(wave_sum(v) * (1.0f / 512) + eps);
        float xh[8], gh[8], s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            xh[i] = (xv[i] - mean) * rstd;
            gh[i] = hv[i] * gv[i];
            s1 += gh[i];
            s2 += gh[i] * xh[i];
            pg[i] += hv[i] * xh[i];
            pb[i] += hv[i];
        }
        const float m1 = wave_sum(s1) * (1.0f / 512), m2 = wave_sum(s2) * (1.0f / 512);
        float4* dp = reinterpret_cast<float4*>(dx + row * 512 + c0);
        float o[8];
        const float4 da = dp[0], db = dp[1];
        const float dv[8] = {da.x, da.y, da.z, da.w, db.x, db.y, db.z, db.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = dv[i] + rstd * (gh[i] - m1 - xh[i] * m2);
        dp[0] = make_float4(o[0], o[1], o[2], o[3]);
        dp[1] = make_float4(o[4], o[5], o[6], o[7]);
        if (dx_bf16) {
            bf16x8 ob;
#pragma unroll
            for (int i = 0; i < 8; ++i) ob[i] = (bf16)o[i];
            *reinterpret_cast<bf16x8*>(dx_bf16 + row * 512 + c0) = ob;
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) { red[wave][0][c0 + i] = pg[i]; red[wave][1][c0 + i] = pb[i]; }
    __syncthreads();
    float* out = part + (int64_t)blockIdx.x * 1024;
    for (int c = threadIdx.x; c < 1024; c += 256) {
        const int j = c >> 9, cc = c & 511;
        out[c] = ((red[0][j][cc] + red[1][j][cc]) + red[2][j][cc]) + red[3][j][cc];
    }
}

// out[c] += sum_{w < nparts} part[w][c] in order of w (c < ncols); one thread per column, coalesced over c
__global__ __launch_bounds__(256) void ordered_colsum_kernel(const float* __restrict__ part, int nparts, int ncols, float* __restrict__ out0,
                                                             float* __restrict__ out1, int split) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= ncols) return;
    float s = 0.f;
    for (int w = 0; w < nparts; ++w) s += part[(int64_t)w * ncols + c];
    if (c < split) out0[c] += s;
    else out1[c - split] += s;
}

int64_t ln_affine_bwd_scratch_bytes(int64_t rows) { return rows > 0 ? (rows + LN_ROWS - 1) / LN_ROWS * 1024 * 4 : 0; }

int ln_affine_bwd(const float* x, const float* dh, const float* g, float eps, int64_t rows, float* dx, bf16* dx_bf16, float* dgamma, float* dbeta,
                  float* scratch, int64_t scratch_bytes, hipStream_t st) {
    RALD_CHECK(rows > 0, "ln_affine_bwd: empty");
    const int64_t nwg = (rows + LN_ROWS - 1) / LN_ROWS;
    RALD_CHECK(nwg < (1ll << 31), "ln_affine_bwd: too many rows");
    RALD_CHECK(scratch && scratch_bytes >= ln_affine_bwd_scratch_bytes(rows), "ln_affine_bwd: scratch too small");
    RALD_CHECK((uintptr_t)scratch % 16 == 0, "ln_affine_bwd: scratch must be 16-byte aligned");
    RALD_CHECK((uintptr_t)x % 16 == 0 && (uintptr_t)dh % 16 == 0 && (uintptr_t)dx % 16 == 0 && (uintptr_t)dx_bf16 % 16 == 0,
               "ln_affine_bwd: 16-byte alignment");
    hipLaunchKernelGGL(ln_affine_bwd_kernel, dim3((unsigned)nwg), dim3(256), 0, st, x, dh, g, eps, rows, dx, dx_bf16, scratch);
    hipLaunchKernelGGL(ordered_colsum_kernel, dim3(4), dim3(256), 0, st, scratch, (int)nwg, 1024, dgamma, dbeta, 512);
    RALD_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------ PointEmbed weight gradient
constexpr int PE_ROWS = 512;                                   // rows per workgroup
constexpr int PE_SUB = 64;                                     // rows staged in LDS at a time
constexpr int PE_F = 52;                                       // 51 features + the bias column (feature 1)

__global__ __launch_bounds__(256) void pe_wgrad_kernel(const float* __restrict__ dY, const float* __restrict__ pts, const float* __restrict__ basis,
                                                       int64_t rows, float* __restrict__ part) {
    __shared__ float sb[72];
    __shared__ float feat[PE_SUB][PE_F];
    if (threadIdx.x < 72) sb[threadIdx.x] = basis[threadIdx.x];
    float acc0[PE_F], acc1[PE_F];                              // output channels threadIdx.x and threadIdx.x + 256
#pragma unroll
    for (int f = 0; f < PE_F; ++f) { acc0[f] = 0.f; acc1[f] = 0.f; }
    const int64_t r0 = (int64_t)blockIdx.x * PE_ROWS;
    for (int sub = 0; sub < PE_ROWS; sub += PE_SUB) {
        const int64_t rs = r0 + sub;
        if (rs >= rows) break;
        const int nr = (int)min((int64_t)PE_SUB, rows - rs);
        __syncthreads();
        for (int i = threadIdx.x; i < PE_SUB * PE_F; i += 256) {
            const int r = i / PE_F, f = i % PE_F;
            float v = 0.f;
            if (r < nr) {
                const float* p = pts + (rs + r) * 3;
                if (f < 48) {
                    const int e = f < 24 ? f : f - 24;
                    const float pr = p[0] * sb[e] + p[1] * sb[24 + e] + p[2] * sb[48 + e];
                    v = f < 24 ? sinf(pr) : cosf(pr);
                } else {
                    v = f < 51 ? p[f - 48] : 1.f;
                }
            }
            feat[r][f] = v;
        }
        __syncthreads();
        for (int r = 0; r < nr; ++r) {
            const float d0 = dY[(rs + r) * 512 + threadIdx.x], d1 = dY[(rs + r) * 512 + 256 + threadIdx.x];
#pragma unroll
            for (int f = 0; f < PE_F; ++f) {
                acc0[f] = fmaf(d0, feat[r][f], acc0[f]);
                acc1[f] = fmaf(d1, feat[r][f], acc1[f]);
            }
        }
    }
    // part[wg][o][52]
    float* out = part + (int64_t)blockIdx.x * 512 * PE_F;
#pragma unroll
    for (int f = 0; f < PE_F; ++f) {
        out[threadIdx.x * PE_F + f] = acc0[f];
        out[(threadIdx.x + 256) * PE_F + f] = acc1[f];
    }
}

// dW[o][f] += sum_w part[w][o][f] (f < 51), db[o] += sum_w part[w][o][51]
__global__ __launch_bounds__(256) void pe_wgrad_reduce_kernel(const float* __restrict__ part, int nparts, float* __restrict__ dW, float* __restrict__ db) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 512 * PE_F) return;
    float s = 0.f;
    for (int w = 0; w < nparts; ++w) s += part[(int64_t)w * 512 * PE_F + i];
    const int o = i / PE_F, f = i % PE_F;
    if (f < 51) dW[o * 51 + f] += s;
    else db[o] += s;
}

int64_t pe_wgrad_scratch_bytes(int64_t rows) { return rows > 0 ? (rows + PE_ROWS - 1) / PE_ROWS * 512 * PE_F * 4 : 0; }

int pe_wgrad(const float* dY, const float* pts, const float* basis, int64_t rows, float* dW, float* db, float* scratch, int64_t scratch_bytes,
             hipStream_t st) {
    RALD_CHECK(rows > 0, "pe_wgrad: empty");
    const int64_t nwg = (rows + PE_ROWS - 1) / PE_ROWS;
    RALD_CHECK(nwg < (1ll << 31), "pe_wgrad: too many rows");
    RALD_CHECK(scratch && scratch_bytes >= pe_wgrad_scratch_bytes(rows), "pe_wgrad: scratch too small");
    RALD_CHECK((uintptr_t)scratch % 16 == 0, "pe_wgrad: scratch must be 16-byte aligned");
    hipLaunchKernelGGL(pe_wgrad_kernel, dim3((unsigned)nwg), dim3(256), 0, st, dY, pts, basis, rows, scratch);
    hipLaunchKernelGGL(pe_wgrad_reduce_kernel, dim3(cdiv(512 * PE_F, 256)), dim3(256), 0, st, scratch, (int)nwg, dW, db);
    RALD_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------ posterior backward
__global__ __launch_bounds__(256) void posterior_bwd_kernel(const float* __restrict__ dz, const float* __restrict__ dkl, const float* __restrict__ ml,
                                                            const float* __restrict__ eps, float* __restrict__ dml, int64_t total, int rows, int L) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t row = i / L;
    const int c = (int)(i - row * L);
    const int b = (int)(row / rows);
    const float inv = 1.0f / ((float)rows * (float)L);
    const float mu = ml[row * 2 * L + c], lv_raw = ml[row * 2 * L + L + c];
    const float lv = fminf(fmaxf(lv_raw, -30.f), 20.f);
    const float g = dz ? dz[i] : 0.f, k = dkl ? dkl[b] : 0.f;
    const float e = eps[i];
    dml[row * 2 * L + c] = g + k * mu * inv;                                              // d/dmean of mean + std*eps and 0.5*mean(mean^2)
    const float dlv = g * e * 0.5f * expf(0.5f * lv) + k * 0.5f * (expf(lv) - 1.0f) * inv;   // through the clamped logvar
    dml[row * 2 * L + L + c] = (lv_raw >= -30.f && lv_raw <= 20.f) ? dlv : 0.f;
}

int posterior_bwd(const float* dz, const float* dkl, const float* ml, const float* eps, float* dml, int B, int rows, int L, hipStream_t st) {
    RALD_CHECK(B > 0 && rows > 0 && L > 0 && ml && eps && dml, "posterior_bwd: bad arguments");
    const int64_t total = (int64_t)B * rows * L;
    hipLaunchKernelGGL(posterior_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, dz, dkl, ml, eps, dml, total, rows, L);
    RALD_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------ drop-path residual
__global__ __launch_bounds__(256) void scale_rows_add_kernel(const float* __restrict__ y, const float* __restrict__ s, float* __restrict__ x,
                                                             int64_t rows_per_sample, int cols, int64_t total4) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    const float sc = s[(i * 4 / cols) / rows_per_sample];
    const float4 a = reinterpret_cast<const float4*>(y)[i];
    float4 o = reinterpret_cast<float4*>(x)[i];
    o.x = fmaf(sc, a.x, o.x); o.y = fmaf(sc, a.y, o.y); o.z = fmaf(sc, a.z, o.z); o.w = fmaf(sc, a.w, o.w);
    reinterpret_cast<float4*>(x)[i] = o;
}
__global__ __launch_bounds__(256) void scale_rows_bf16_kernel(const float* __restrict__ dx, const float* __restrict__ s, bf16* __restrict__ out,
                                                              int64_t rows_per_sample, int cols, int64_t total4) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    const float sc = s[(i * 4 / cols) / rows_per_sample];
    const float4 a = reinterpret_cast<const float4*>(dx)[i];
    reinterpret_cast<bf16x4*>(out)[i] = pack4(sc * a.x, sc * a.y, sc * a.z, sc * a.w);
}

int scale_rows(const float* in, const float* s, float* x_accum, bf16* out_bf16, int64_t rows, int cols, int64_t rows_per_sample, hipStream_t st) {
    RALD_CHECK(in && s && (x_accum || out_bf16) && rows > 0 && cols > 0 && rows_per_sample > 0, "scale_rows: bad arguments");
    RALD_CHECK(cols % 4 == 0, "scale_rows: cols must be a multiple of 4");
    const int64_t total4 = rows * cols / 4;
    const dim3 grid((unsigned)((total4 + 255) / 256));
    if (x_accum) hipLaunchKernelGGL(scale_rows_add_kernel, grid, dim3(256), 0, st, in, s, x_accum, rows_per_sample, cols, total4);
    else hipLaunchKernelGGL(scale_rows_bf16_kernel, grid, dim3(256), 0, st, in, s, out_bf16, rows_per_sample, cols, total4);
    RALD_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------ softmax backward on stored scores
__global__ __launch_bounds__(256) void softmax_bwd_rows_kernel(const float* __restrict__ S, const float* __restrict__ dP, const float* __restrict__ delta,
                                                               int64_t ld, int n, float scale, bf16* __restrict__ P, bf16* __restrict__ dS) {
    __shared__ float red[4];
    const int64_t row = blockIdx.x;
    const float* s = S + row * ld;
    const float* d = dP + row * ld;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float mx = -1e30f;
    for (int i = threadIdx.x; i < n; i += 256) mx = fmaxf(mx, s[i]);
    mx = wave_max(mx);
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float sum = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) sum += __expf(s[i] - mx);
    sum = wave_sum(sum);
    if (lane == 0) red[wave] = sum;
    __syncthreads();
    const float inv = 1.0f / (red[0] + red[1] + red[2] + red[3]);
    const float dl = delta[row];
    for (int i = threadIdx.x; i < (int)ld; i += 256) {
        const float p = i < n ? __expf(s[i] - mx) * inv : 0.f;
        if (P) P[row * ld + i] = (bf16)p;
        dS[row * ld + i] = (bf16)(i < n ? p * (d[i] - dl) * scale : 0.f);
    }
}

int softmax_bwd_rows(const float* S, const float* dP, const float* delta, int64_t rows, int64_t ld, int n, float scale, bf16* P, bf16* dS,
                     hipStream_t st) {
    RALD_CHECK(S && dP && delta && dS && rows > 0 && n > 0, "softmax_bwd_rows: bad arguments");
    RALD_CHECK(ld >= n, "softmax_bwd_rows: ld must be >= n");
    RALD_CHECK(rows < (1ll << 31), "softmax_bwd_rows: too many rows");
    hipLaunchKernelGGL(softmax_bwd_rows_kernel, dim3((unsigned)rows), dim3(256), 0, st, S, dP, delta, ld, n, scale, P, dS);
    RALD_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------ the stage-1 loss
// engine_ae.py:70-101 in two launches.  ae_loss_kernel: one workgroup per AL_CHUNK queries of one sample; every thread loads its AL_ITEMS
// logits and labels before the first dependent operation, writes dlogits, and the workgroup leaves one partial (two double sums, three
// counts) in scratch[b][chunk].  ae_loss_finish_kernel (one workgroup) adds the partials in (b, chunk) order.  The split point n is read
// from device memory, so a captured graph serves any in_voxel_num.  A sample's counts, partials and dlogits row depend on its own row
// only: the same bits in any batch.
constexpr int AL_ITEMS = 4;
constexpr int AL_CHUNK = 256 * AL_ITEMS;

struct AeLossPart { double vol, near; int32_t eq, inter, uni, pad; };
static_assert(sizeof(AeLossPart) == 32, "AeLossPart layout");

__device__ __forceinline__ float sigmoidf_acc(float x) {                       // no cancellation on either side
    const float e = expf(-fabsf(x));
    return (x >= 0.f ? 1.0f : e) / (1.0f + e);
}

__global__ __launch_bounds__(256) void ae_loss_kernel(const float* __restrict__ logits, const float* __restrict__ labels,
                                                      const int32_t* __restrict__ n_dev, int batch, int64_t Q, float vol_w, float near_w,
                                                      float grad_scale, float* __restrict__ dlogits, AeLossPart* __restrict__ part) {
    __shared__ double shv[4], shn[4];
    __shared__ int shc[4][3];
    const int b = blockIdx.y;
    const int64_t j0 = (int64_t)blockIdx.x * AL_CHUNK + threadIdx.x;
    const float* xr = logits + (int64_t)b * Q;
    const float* yr = labels + (int64_t)b * Q;
    float x[AL_ITEMS], y[AL_ITEMS];
#pragma unroll
    for (int i = 0; i < AL_ITEMS; ++i) {
        const int64_t j = j0 + i * 256;
        const bool in = j < Q;
        x[i] = in ? xr[j] : 0.f;
        y[i] = in ? yr[j] : 0.f;
    }
    int64_t n = *n_dev;
    n = n < 0 ? 0 : (n > Q ? Q : n);
    // grad_scale * w / (B * n_span) in double, rounded once: (3 w) / (3 n) and w / n are the same real number, hence the same float
    const float cv = (float)((double)grad_scale * (double)vol_w / ((double)batch * (double)n));
    const float cn = (float)((double)grad_scale * (double)near_w / ((double)batch * (double)(Q - n)));
    double sv = 0.0, sn = 0.0;
    int eq = 0, inter = 0, uni = 0;
#pragma unroll
    for (int i = 0; i < AL_ITEMS; ++i) {
        const int64_t j = j0 + i * 256;
        if (j >= Q) continue;
        const float xv = x[i], yv = y[i];
        const float term = fmaxf(xv, 0.f) - xv * yv + log1pf(expf(-fabsf(xv)));
        const bool vol = j < n;
        if (vol) sv += (double)term;
        else sn += (double)term;
        const bool pred = xv >= 0.f, lab = yv != 0.f;
        eq += pred == lab;
        inter += pred && lab;
        uni += pred || lab;
        if (dlogits) {
            const float d = yv == 1.0f ? -sigmoidf_acc(-xv) : sigmoidf_acc(xv) - yv;
            dlogits[(int64_t)b * Q + j] = (vol ? cv : cn) * d;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        sv += __shfl_xor(sv, o, 64);
        sn += __shfl_xor(sn, o, 64);
        eq += __shfl_xor(eq, o, 64);
        inter += __shfl_xor(inter, o, 64);
        uni += __shfl_xor(uni, o, 64);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { shv[wave] = sv; shn[wave] = sn; shc[wave][0] = eq; shc[wave][1] = inter; shc[wave][2] = uni; }
    __syncthreads();
    if (threadIdx.x == 0) {
        AeLossPart p;
        p.vol = ((shv[0] + shv[1]) + shv[2]) + shv[3];
        p.near = ((shn[0] + shn[1]) + shn[2]) + shn[3];
        p.eq = shc[0][0] + shc[1][0] + shc[2][0] + shc[3][0];
        p.inter = shc[0][1] + shc[1][1] + shc[2][1] + shc[3][1];
        p.uni = shc[0][2] + shc[1][2] + shc[2][2] + shc[3][2];
        p.pad = 0;
        part[(int64_t)b * gridDim.x + blockIdx.x] = p;
    }
}

__global__ __launch_bounds__(256) void ae_loss_finish_kernel(const AeLossPart* __restrict__ part, int nchunk, const float* __restrict__ kl,
                                                             const int32_t* __restrict__ n_dev, int batch, int64_t Q, float vol_w, float near_w,
                                                             float kl_w, float grad_scale, double* __restrict__ losses, int32_t* __restrict__ counts,
                                                             float* __restrict__ dkl) {
    __shared__ double shv[256], shn[256], shk[256];
    const int t = threadIdx.x;
    const int64_t total = (int64_t)batch * nchunk;
    double sv = 0.0, sn = 0.0, sk = 0.0;
    for (int64_t i = t; i < total; i += 256) { sv += part[i].vol; sn += part[i].near; }
    for (int b = t; b < batch; b += 256) {
        sk += (double)kl[b];
        int eq = 0, inter = 0, uni = 0;
        for (int c = 0; c < nchunk; ++c) {
            const AeLossPart p = part[(int64_t)b * nchunk + c];
            eq += p.eq; inter += p.inter; uni += p.uni;
        }
        counts[b * 3 + 0] = eq; counts[b * 3 + 1] = inter; counts[b * 3 + 2] = uni;
        if (dkl) dkl[b] = (float)((double)grad_scale * (double)kl_w / (double)batch);
    }
    shv[t] = sv; shn[t] = sn; shk[t] = sk;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {                                       // a fixed tree: thread t adds slot t + o
        if (t < o) { shv[t] += shv[t + o]; shn[t] += shn[t + o]; shk[t] += shk[t + o]; }
        __syncthreads();
    }
    if (t == 0) {
        int64_t n = *n_dev;
        n = n < 0 ? 0 : (n > Q ? Q : n);
        const double vol = shv[0] / ((double)batch * (double)n);              // 0 / 0 = NaN for an empty span, as torch's mean gives
        const double near = shn[0] / ((double)batch * (double)(Q - n));
        const double klm = shk[0] / (double)batch;
        losses[0] = (double)vol_w * vol + (double)near_w * near + (double)kl_w * klm;
        losses[1] = vol; losses[2] = near; losses[3] = klm;
    }
}

int64_t ae_loss_scratch_bytes(int batch, int64_t n_queries) {
    return batch > 0 && n_queries > 0 ? (int64_t)batch * ((n_queries + AL_CHUNK - 1) / AL_CHUNK) * (int64_t)sizeof(AeLossPart) : 0;
}

int ae_loss(const float* logits, const float* labels, const float* kl, const int32_t* n_dev, int batch, int64_t Q, float vol_w, float near_w,
            float kl_w, float grad_scale, double* losses4, int32_t* counts3, float* dlogits, float* dkl, void* scratch, int64_t scratch_bytes,
            hipStream_t st) {
    RALD_CHECK(batch > 0 && Q > 0, "ae_loss: empty");
    RALD_CHECK(batch <= 65535, "ae_loss: at most 65535 samples");
    const int64_t nchunk = (Q + AL_CHUNK - 1) / AL_CHUNK;
    RALD_CHECK(nchunk < (1ll << 31) && (int64_t)batch * nchunk < (1ll << 31), "ae_loss: too many queries");
    RALD_CHECK(scratch && scratch_bytes >= ae_loss_scratch_bytes(batch, Q), "ae_loss: scratch too small");
    RALD_CHECK((uintptr_t)scratch % 16 == 0 && (uintptr_t)losses4 % 8 == 0, "ae_loss: scratch must be 16-byte, out_losses4 8-byte aligned");
    hipLaunchKernelGGL(ae_loss_kernel, dim3((unsigned)nchunk, (unsigned)batch), dim3(256), 0, st, logits, labels, n_dev, batch, Q, vol_w, near_w,
                       grad_scale, dlogits, (AeLossPart*)scratch);
    hipLaunchKernelGGL(ae_loss_finish_kernel, dim3(1), dim3(256), 0, st, (const AeLossPart*)scratch, (int)nchunk, kl, n_dev, batch, Q, vol_w,
                       near_w, kl_w, grad_scale, losses4, counts3, dkl);
    RALD_HIP(hipGetLastError());
    return 0;
}

}  // namespace rald
