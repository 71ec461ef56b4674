// Radar-spectrum encoder (model/models_radar_encoder.py Encoder :137-241) and the tokeniser half of
// EDMPrecond.process_radar_cond (models_radar_generation.py:363-407).
//
// Data layout (MI355X-first): activations are channels-LAST (NDHWC = [b][r][a][e][c]) so that one
// voxel's channels are contiguous - exactly an MFMA A-fragment row - and the encoder's output
// [B,8,4,2,16] is already in the `permute(0,2,3,4,1)` order the tokeniser wants (:387).  The
// residual trunk stays fp32; every conv input is the bf16 tensor swish(GroupNorm(x)) written by
// one HBM-bound pass (gn_apply), so the conv kernel is a pure implicit GEMM:
//     M = output voxels, N = Cout, K = 27*Cin  (weights packed [Cout][tap][Cin], K-contiguous).
// Conv3d zero padding applies to the normalised+activated tensor, i.e. out-of-range taps
// contribute exact zeros (register zero-fill, no padded copy).  Downsample = F.pad(0,1) + conv
// k3 s2 p0 (:37-41) is the same kernel with stride 2 and left pad 0.
//
// This file: conv_in, GroupNorm, the upsample / pad / token kernels, the model (weights, workspace, forward, decode, tokeniser) and the
// op-level launchers of those kernels.  The 3x3x3 convolution engines, their route and conv3d_full are in conv3d.hip.
#include "dit.h"

#include <cmath>
#include <cstdio>
#include <map>

namespace rald {

// ------------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------------
// conv_in: Cin = 1 -> ch (64); the cube's channel 0 is read in place ([B,R,A,E,cube_ch], :378).
__global__ __launch_bounds__(256) void conv_in_kernel(const float* __restrict__ cube, int cube_ch, int Cin, const float* __restrict__ W,
                                                      const float* __restrict__ bias, float* __restrict__ out, int B, int D,
                                                      int H, int Wd, int Cout) {
    extern __shared__ float sw[];            // [Cin][27][Cout] (tap-major so 8 consecutive co are contiguous)
    for (int i = threadIdx.x; i < Cin * 27 * Cout; i += 256) {
        const int co = i % Cout, t = (i / Cout) % 27, ci = i / (27 * Cout);
        sw[i] = W[(co * Cin + ci) * 27 + t];
    }
    __syncthreads();
    const int groups = Cout / 8;                          // threads per voxel
    const int vpb = 256 / groups;                         // voxels per block
    const int64_t v = (int64_t)blockIdx.x * vpb + threadIdx.x / groups;
    const int cg = threadIdx.x % groups;
    const int64_t nvox = (int64_t)B * D * H * Wd;
    if (v >= nvox) return;
    int w = (int)(v % Wd);
    int64_t r = v / Wd;
    int h = (int)(r % H); r /= H;
    int d = (int)(r % D);
    int b = (int)(r / D);
    float acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = bias[cg * 8 + i];
    for (int kd = 0; kd < 3; ++kd)
        for (int kh = 0; kh < 3; ++kh)
            for (int kw = 0; kw < 3; ++kw) {
                const int id = d + kd - 1, ih = h + kh - 1, iw = w + kw - 1;
                if ((unsigned)id >= (unsigned)D || (unsigned)ih >= (unsigned)H || (unsigned)iw >= (unsigned)Wd) continue;
                const float* xp = cube + ((((int64_t)b * D + id) * H + ih) * Wd + iw) * cube_ch;
                for (int ci = 0; ci < Cin; ++ci) {
                    const float x = xp[ci];
                    const float* wt = sw + (ci * 27 + (kd * 3 + kh) * 3 + kw) * Cout + cg * 8;
#pragma unroll
                    for (int i = 0; i < 8; ++i) acc[i] += x * wt[i];
                }
            }
    float4* o = reinterpret_cast<float4*>(out + v * Cout + cg * 8);
    o[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
    o[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
}

// GroupNorm statistics (32 groups), x [B][S][C] fp32 -> stats[b][g] = {sum, sumsq} in double.  Deterministic (no atomics: the
// radar condition - and with it every sample drawn from it - is bit-reproducible run to run): each block reduces its
// voxels in a fixed order and writes one partial per group, gn_finish_kernel adds the partials in block order.
// part[b][blk][g] = {sum, sumsq}, blk < gridDim.x.
__global__ __launch_bounds__(256) void gn_stats_kernel(const float* __restrict__ x, double* __restrict__ part, int S, int C,
                                                       int vox_per_block) {
    __shared__ float4 sp[256];
    const int b = blockIdx.y;
    const int quads = C / 4;                               // float4 pieces per voxel
    const int q = threadIdx.x % quads;
    const int vstep = 256 / quads;
    const int v0 = blockIdx.x * vox_per_block;
    const int v1 = min(S, v0 + vox_per_block);
    float s0 = 0.f, q0 = 0.f, s1 = 0.f, q1 = 0.f;         // channel pairs (4q,4q+1) and (4q+2,4q+3)
    int v = v0 + threadIdx.x / quads;
    for (; v + 3 * vstep < v1; v += 4 * vstep) {           // four loads in flight per lane (the loop is latency-bound otherwise)
        float4 t[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) t[u] = reinterpret_cast<const float4*>(x + ((int64_t)b * S + v + u * vstep) * C)[q];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            s0 += t[u].x + t[u].y; q0 += t[u].x * t[u].x + t[u].y * t[u].y;
            s1 += t[u].z + t[u].w; q1 += t[u].z * t[u].z + t[u].w * t[u].w;
        }
    }
    for (; v < v1; v += vstep) {
        const float4 t = reinterpret_cast<const float4*>(x + ((int64_t)b * S + v) * C)[q];
        s0 += t.x + t.y; q0 += t.x * t.x + t.y * t.y;
        s1 += t.z + t.w; q1 += t.z * t.z + t.w * t.w;
    }
    sp[threadIdx.x] = make_float4(s0, q0, s1, q1);
    __syncthreads();
    if (threadIdx.x < 32) {
        // C is 64 * 2^k (host-checked): channels per group cpg = 2^lcpg >= 2.  Group g owns quads [g*cpg/4, (g+1)*cpg/4) of every
        // voxel row of the block (cpg = 2: one half of quad g/2); visit exactly those, rows then quads, in a fixed order
        const int g = threadIdx.x, lcpg = 31 - __clz(C / 32), rows = 256 / quads;
        const int tq0 = lcpg >= 2 ? g << (lcpg - 2) : g >> 1, tq1 = lcpg >= 2 ? (g + 1) << (lcpg - 2) : tq0 + 1;
        double su = 0.0, sq = 0.0;
        for (int r = 0; r < rows; ++r)
            for (int tq = tq0; tq < tq1; ++tq) {
                const float4 p = sp[r * quads + tq];
                if (lcpg >= 2 || !(g & 1)) { su += (double)p.x; sq += (double)p.y; }
                if (lcpg >= 2 || (g & 1)) { su += (double)p.z; sq += (double)p.w; }
            }
        double* o = part + (((int64_t)b * gridDim.x + blockIdx.x) * 32 + g) * 2;
        o[0] = su; o[1] = sq;
    }
}
// stats[b][g] = sum over the sample's partial slots part[b*nblk + k][g] (statistics blocks or conv tiles) in a fixed order:
// sixteen contiguous ranges in parallel (threads 64q .. 64q+63), then the ranges in order
__global__ __launch_bounds__(1024) void gn_finish_kernel(const double* __restrict__ part, double* __restrict__ stats, int nblk) {
    __shared__ double sq[16][64];
    const int b = blockIdx.x, gw = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int k0 = (int)((int64_t)nblk * q / 16), k1 = (int)((int64_t)nblk * (q + 1) / 16);
    double acc = 0.0;
#pragma unroll 4
    for (int k = k0; k < k1; ++k) acc += part[((int64_t)b * nblk + k) * 64 + gw];
    sq[q][gw] = acc;
    __syncthreads();
    if (q == 0) {
        double t = sq[0][gw];
#pragma unroll
        for (int i = 1; i < 16; ++i) t += sq[i][gw];
        stats[(int64_t)b * 64 + gw] = t;
    }
}
constexpr int GN_VPB = 512;                                // voxels per statistics block
static inline int gn_blocks(int S) { return (S + GN_VPB - 1) / GN_VPB; }

// y_bf16 = act(GroupNorm(x)) with per-channel affine; act = swish (x*sigmoid(x), :5-7) or identity.
__global__ __launch_bounds__(256) void gn_apply_kernel(const float* __restrict__ x, const double* __restrict__ stats,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       bf16* __restrict__ y, int S, int C, float eps, int do_swish) {
    __shared__ float smean[32], srstd[32];
    const int b = blockIdx.y;
    const int quads = C / 4;
    const int cpg = C / 32;
    if (threadIdx.x < 32) {
        const double n = (double)S * cpg;
        const double su = stats[((int64_t)b * 32 + threadIdx.x) * 2], sq = stats[((int64_t)b * 32 + threadIdx.x) * 2 + 1];
        const double mean = su / n;
        const double var = sq / n - mean * mean;               // biased variance, as torch GroupNorm
        smean[threadIdx.x] = (float)mean;
        srstd[threadIdx.x] = (float)(1.0 / sqrt((var > 0.0 ? var : 0.0) + (double)eps));
    }
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < (int64_t)S * quads; i += (int64_t)gridDim.x * 256) {
        const int q = (int)(i % quads);
        const int64_t idx = (int64_t)b * S * quads + i;
        const float4 t = reinterpret_cast<const float4*>(x)[idx];
        const float4 gm = reinterpret_cast<const float4*>(gamma)[q];
        const float4 bt = reinterpret_cast<const float4*>(beta)[q];
        const float v[4] = {t.x, t.y, t.z, t.w};
        const float gg[4] = {gm.x, gm.y, gm.z, gm.w};
        const float bb[4] = {bt.x, bt.y, bt.z, bt.w};
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int g = (4 * q + j) / cpg;
            float yv = (v[j] - smean[g]) * srstd[g] * gg[j] + bb[j];
            if (do_swish) yv = yv / (1.0f + __expf(-yv));
            o[j] = yv;
        }
        reinterpret_cast<bf16x4*>(y)[idx] = pack4(o[0], o[1], o[2], o[3]);
    }
}

// tokens[b][t][c] = z[b][t][:].Wp[c][:] + bp[c] + r_emb[r][c] + a_emb[a][c] + e_emb[e][c], t = (r*A + a)*E + e
__global__ void radar_token_kernel(const float* __restrict__ z, const float* __restrict__ Wp, const float* __restrict__ bp,
                                   const float* __restrict__ re, const float* __restrict__ ae, const float* __restrict__ ee,
                                   float* __restrict__ tok, int R, int A, int E, int zc, int C) {
    const int t = blockIdx.x;                 // token within the batch
    const int b = blockIdx.y;
    const int e = t % E, aa = (t / E) % A, r = t / (E * A);
    const float* zz = z + ((int64_t)b * R * A * E + t) * zc;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        float acc = bp[c];
        for (int k = 0; k < zc; ++k) acc += zz[k] * Wp[c * zc + k];
        tok[((int64_t)b * R * A * E + t) * C + c] = acc + re[r * C + c] + ae[aa * C + c] + ee[e * C + c];
    }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// ---- decoder helpers --------------------------------------------------------------------------------------------------------
// Upsample (:18-27): nearest-neighbour x2 of the fp32 trunk [B][D][H][W][C] (channels last) -> bf16 [B][2D][2H][2W][C], the input of
// the 3x3x3 convolution that follows.  One thread per 4 channels of an OUTPUT voxel.
__global__ __launch_bounds__(256) void upsample2_cast_kernel(const float* __restrict__ x, bf16* __restrict__ y, int B, int D, int H, int W, int C) {
    const int64_t quads = (int64_t)B * 8 * D * H * W * (C / 4);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < quads; i += (int64_t)gridDim.x * 256) {
        const int c4 = (int)(i % (C / 4));
        int64_t v = i / (C / 4);
        const int ow = (int)(v % (2 * W)); v /= 2 * W;
        const int oh = (int)(v % (2 * H)); v /= 2 * H;
        const int od = (int)(v % (2 * D));
        const int b = (int)(v / (2 * D));
        const float4 s = *reinterpret_cast<const float4*>(x + ((((int64_t)b * D + od / 2) * H + oh / 2) * W + ow / 2) * C + 4 * c4);
        *reinterpret_cast<bf16x4*>(y + i * 4) = pack4(s.x, s.y, s.z, s.w);
    }
}
// z [rows][zc] fp32 -> bf16 [rows][64], zero beyond zc (the decoder's conv_in reads 64-channel rows)
__global__ __launch_bounds__(256) void pad_cast64_kernel(const float* __restrict__ z, bf16* __restrict__ y, int64_t rows, int zc) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * 64) return;
    const int c = (int)(i & 63);
    y[i] = (bf16)(c < zc ? z[(i >> 6) * zc + c] : 0.f);
}

struct RadarEncoder::Impl {
    int ch = 64, zc = 16, R = 128, A = 64, E = 32, token_ch = 512, cin = 1;
    DeviceArena* arena = nullptr;
    enum Kind { CONV3, CONV1, VEC, CONVIN };
    struct Tensor { Kind kind; int cout, cin; void* ptr = nullptr; bool loaded = false; int cin_pad = 0, cout_pad = 0; };   // pads: decoder conv_in / conv_out
    std::map<std::string, Tensor> tensors;
    // tokeniser
    float *w_tok = nullptr, *b_tok = nullptr, *emb_r = nullptr, *emb_a = nullptr, *emb_e = nullptr;
    bool tok_loaded[5] = {false, false, false, false, false};
    // workspace (for `sub` samples at a time)
    int sub = 0;
    float *f0 = nullptr, *f1 = nullptr, *f2 = nullptr, *z = nullptr, *tok = nullptr, *sbuf = nullptr;
    bf16 *n16 = nullptr, *q16 = nullptr, *k16 = nullptr, *vt16 = nullptr, *p16 = nullptr, *o16 = nullptr;
    double* stats = nullptr;
    int gn_part_blocks = 0;
    double* cpart = nullptr;            // per-tile GroupNorm partials written by the conv epilogue
    size_t cpart_bytes = 0;
    float* spart = nullptr;             // split-K partial accumulators of the small-level convolutions
    size_t spart_bytes = 0;
    const float* fused_src = nullptr;   // activation whose partials sit in cpart (nullptr: none)
    int fused_B = 0, fused_S = 0, fused_C = 0;
    int tok_batch = 0;

    void add(const std::string& name, Kind k, int cout, int cin) { Tensor t{k, cout, cin}; t.cin_pad = cin; t.cout_pad = cout; tensors[name] = t; }
    // 3x3x3 convolution whose channel counts are padded up for the implicit-GEMM kernel (Cin to 64, Cout to 4): zero weights / bias in the pad
    void add_conv3_padded(const std::string& n, int cout, int cin, int cout_pad, int cin_pad) {
        add_conv3(n, cout, cin);
        tensors[n + ".weight"].cin_pad = cin_pad; tensors[n + ".weight"].cout_pad = cout_pad; tensors[n + ".bias"].cout_pad = cout_pad;
    }
    bool is_decoder = false;
    int out_ch = 2;
    void add_conv3(const std::string& n, int cout, int cin) { add(n + ".weight", CONV3, cout, cin); add(n + ".bias", VEC, cout, 0); }
    void add_conv1(const std::string& n, int cout, int cin) { add(n + ".weight", CONV1, cout, cin); add(n + ".bias", VEC, cout, 0); }
    void add_norm(const std::string& n, int c) { add(n + ".weight", VEC, c, 0); add(n + ".bias", VEC, c, 0); }
    void add_res(const std::string& n, int cin, int cout) {
        add_norm(n + ".norm1", cin); add_conv3(n + ".conv1", cout, cin); add_norm(n + ".norm2", cout); add_conv3(n + ".conv2", cout, cout);
        if (cin != cout) add_conv1(n + ".nin_shortcut", cout, cin);
    }
    void add_attn(const std::string& n, int c) {
        add_norm(n + ".norm", c);
        for (const char* p : {".q", ".k", ".v", ".proj_out"}) add_conv1(n + p, c, c);
    }
    template <class T> T* P(const std::string& n) { return (T*)tensors.at(n).ptr; }

    int ensure_ws(int nsub);
    int run_conv(const bf16* in, const std::string& name, const float* resid, float* out, int B, int ID, int IH, int IW, int cin,
                 int cout, int stride, int pad, hipStream_t st);
    int gn(const float* x, const std::string& name, bf16* y, int B, int S, int C, bool swish, hipStream_t st);
    int resblock(float*& x, float*& t1, float*& t2, const std::string& name, int B, int Dd, int Hh, int Ww, int cin, int cout, hipStream_t st);
    int attnblock(float* x, const std::string& name, int B, int S, int C, hipStream_t st);
    int forward(const float* cube, int cube_ch, int B, float* zout, hipStream_t st);
    int decode(const float* z, int B, float* out, hipStream_t st);     // Decoder.forward (:333-359), nsub samples
};

static const int kChMult[5] = {1, 1, 2, 2, 4};

static int radar_alloc_tensors(RadarEncoder::Impl& m, DeviceArena* arena) {
    for (auto& kv : m.tensors) {
        auto& t = kv.second;
        size_t bytes = 0;
        switch (t.kind) {
            case RadarEncoder::Impl::CONV3: bytes = (size_t)t.cout_pad * 27 * t.cin_pad * 2; break;
            case RadarEncoder::Impl::CONV1: bytes = (size_t)t.cout * t.cin * 2; break;
            case RadarEncoder::Impl::VEC: bytes = (size_t)t.cout_pad * 4; break;
            case RadarEncoder::Impl::CONVIN: bytes = (size_t)t.cout * t.cin * 27 * 4; break;
        }
        t.ptr = arena->alloc(bytes < 64 ? 64 : bytes, true);       // >= 16 floats so float4 bias reads of a 16-ch tail stay in bounds; pads stay zero
        RALD_CHECK(t.ptr, "radar encoder: weight allocation failed");
    }
    return 0;
}

int RadarEncoder::create(int ch, int z_ch, int R, int A, int E, int token_ch, DeviceArena* arena, int in_channels) {
    RALD_CHECK(in_channels == 1 || in_channels == 2, "radar encoder: in_channels must be 1 or 2");
    RALD_CHECK(ch % 64 == 0 && ch >= 64, "radar encoder: hidden channels must be a multiple of 64");
    RALD_CHECK(R % 16 == 0 && A % 16 == 0 && E % 16 == 0, "radar encoder: cube dims must be multiples of 16");
    RALD_CHECK(z_ch % 4 == 0 && z_ch <= 64, "radar encoder: z channels must be a multiple of 4, <= 64");
    impl = new Impl();
    Impl& m = *impl;
    m.ch = ch; m.zc = z_ch; m.R = R; m.A = A; m.E = E; m.token_ch = token_ch; m.arena = arena; m.cin = in_channels;
    m.add("conv_in.weight", Impl::CONVIN, ch, in_channels);
    m.add("conv_in.bias", Impl::VEC, ch, 0);
    int block_in = ch;
    for (int l = 0; l < 5; ++l) {
        const int block_out = ch * kChMult[l];
        block_in = ch * (l == 0 ? 1 : kChMult[l - 1]);
        for (int b = 0; b < 2; ++b) {
            m.add_res("down." + std::to_string(l) + ".block." + std::to_string(b), block_in, block_out);
            block_in = block_out;
        }
        if (l == 4)
            for (int b = 0; b < 2; ++b) m.add_attn("down.4.attn." + std::to_string(b), block_in);
        if (l != 4) m.add_conv3("down." + std::to_string(l) + ".downsample.conv", block_in, block_in);
    }
    m.add_res("mid.block_1", block_in, block_in);
    m.add_attn("mid.attn_1", block_in);
    m.add_res("mid.block_2", block_in, block_in);
    m.add_norm("norm_out", block_in);
    m.add_conv3("conv_out", z_ch, block_in);
    RALD_TRY(radar_alloc_tensors(m, arena));
    const int nt_r = R / 16, nt_a = A / 16, nt_e = E / 16;
    m.w_tok = (float*)arena->alloc((size_t)token_ch * z_ch * 4, true);
    m.b_tok = (float*)arena->alloc((size_t)token_ch * 4, true);
    m.emb_r = (float*)arena->alloc((size_t)nt_r * token_ch * 4, true);
    m.emb_a = (float*)arena->alloc((size_t)nt_a * token_ch * 4, true);
    m.emb_e = (float*)arena->alloc((size_t)nt_e * token_ch * 4, true);
    RALD_CHECK(m.w_tok && m.b_tok && m.emb_r && m.emb_a && m.emb_e, "radar encoder: allocation failed");
    return 0;
}

// Decoder of the RadarAutoencoder (models_radar_encoder.py:243-359): conv_in z_ch -> 4ch, mid (ResnetBlock, AttnBlock, ResnetBlock), five
// levels from the coarsest up - three ResnetBlocks each, nearest-neighbour x2 + conv3x3 between levels -, GroupNorm + swish + conv_out.
// Same kernels as the encoder; conv_in's z_ch inputs are zero-padded to 64 channels and conv_out's out_ch outputs to 4.
int RadarEncoder::create_decoder(int ch, int z_ch, int out_ch, int R, int A, int E, DeviceArena* arena) {
    RALD_CHECK(ch % 64 == 0 && ch >= 64, "radar decoder: hidden channels must be a multiple of 64");
    RALD_CHECK(R % 16 == 0 && A % 16 == 0 && E % 16 == 0, "radar decoder: cube dims must be multiples of 16");
    RALD_CHECK(z_ch >= 1 && z_ch <= 64 && out_ch >= 1 && out_ch <= 4, "radar decoder: z channels <= 64, output channels <= 4");
    impl = new Impl();
    Impl& m = *impl;
    m.ch = ch; m.zc = z_ch; m.R = R; m.A = A; m.E = E; m.arena = arena; m.is_decoder = true; m.out_ch = out_ch;
    int block_in = ch * kChMult[4];
    m.add_conv3_padded("conv_in", block_in, z_ch, block_in, 64);
    m.add_res("mid.block_1", block_in, block_in);
    m.add_attn("mid.attn_1", block_in);
    m.add_res("mid.block_2", block_in, block_in);
    for (int l = 4; l >= 0; --l) {
        const int block_out = ch * kChMult[l];
        for (int b = 0; b < 3; ++b) {
            m.add_res("up." + std::to_string(l) + ".block." + std::to_string(b), block_in, block_out);
            block_in = block_out;
        }
        if (l != 0) m.add_conv3("up." + std::to_string(l) + ".upsample.conv", block_in, block_in);
    }
    m.add_norm("norm_out", block_in);
    m.add_conv3_padded("conv_out", out_ch, block_in, 4, block_in);
    RALD_TRY(radar_alloc_tensors(m, arena));
    return 0;
}

bool RadarEncoder::all_loaded(std::string* missing) const {
    if (!impl) return false;
    for (const auto& kv : impl->tensors)
        if (!kv.second.loaded) { if (missing) *missing = kv.first; return false; }
    return true;
}

void RadarEncoder::expected_keys(const std::string& prefix, std::set<std::string>& out) const {
    if (!impl) return;
    for (const auto& kv : impl->tensors) out.insert(prefix + kv.first);
}

int RadarEncoder::load_weight(const std::string& name, const float* data, int64_t nelem, Stager& st) {
    RALD_CHECK(impl, "radar encoder: not created");
    auto it = impl->tensors.find(name);
    RALD_CHECK(it != impl->tensors.end(), "radar encoder: unknown key '" + name + "'");
    auto& t = it->second;
    switch (t.kind) {
        case Impl::VEC:
            RALD_CHECK(nelem == t.cout, "radar encoder: size mismatch for '" + name + "'");
            RALD_TRY(st.to_f32(data, (float*)t.ptr, 1, t.cout, t.cout, nullptr));      // (a padded tail stays zero)
            break;
        case Impl::CONVIN:
            RALD_CHECK(nelem == (int64_t)t.cout * t.cin * 27, "radar encoder: size mismatch for '" + name + "'");
            RALD_TRY(st.to_f32(data, (float*)t.ptr, t.cout, t.cin * 27, t.cin * 27, nullptr));
            break;
        case Impl::CONV1:
            RALD_CHECK(nelem == (int64_t)t.cout * t.cin, "radar encoder: size mismatch for '" + name + "'");
            RALD_TRY(st.to_bf16(data, (bf16*)t.ptr, t.cout, t.cin, t.cin, nullptr));
            break;
        case Impl::CONV3: {
            RALD_CHECK(nelem == (int64_t)t.cout * t.cin * 27, "radar encoder: size mismatch for '" + name + "'");
            // torch [Cout][Cin][3][3][3] -> [Cout][tap][Cin] (host permute, then bf16 upload)
            std::vector<float> src((size_t)nelem), dst((size_t)nelem);
            RALD_HIP(hipMemcpy(src.data(), data, (size_t)nelem * 4, hipMemcpyDefault));
            for (int co = 0; co < t.cout; ++co)
                for (int ci = 0; ci < t.cin; ++ci)
                    for (int tp = 0; tp < 27; ++tp)
                        dst[((size_t)co * 27 + tp) * t.cin + ci] = src[((size_t)co * t.cin + ci) * 27 + tp];
            RALD_TRY(st.to_bf16(dst.data(), (bf16*)t.ptr, t.cout * 27, t.cin, t.cin_pad, nullptr));   // rows of cin_pad, zero beyond cin
            break;
        }
    }
    t.loaded = true;
    return 0;
}

int RadarEncoder::load_token_weight(const std::string& name, const float* data, int64_t nelem, Stager& st) {
    RALD_CHECK(impl, "radar encoder: not created");
    Impl& m = *impl;
    const int C = m.token_ch;
    if (name == "radar_token_project.weight") { RALD_CHECK(nelem == (int64_t)C * m.zc, "size mismatch: " + name); m.tok_loaded[0] = true; return st.to_f32(data, m.w_tok, C, m.zc, m.zc, nullptr); }
    if (name == "radar_token_project.bias") { RALD_CHECK(nelem == C, "size mismatch: " + name); m.tok_loaded[1] = true; return st.to_f32(data, m.b_tok, 1, C, C, nullptr); }
    if (name == "radar_r_emb.weight") { RALD_CHECK(nelem == (int64_t)(m.R / 16) * C, "size mismatch: " + name); m.tok_loaded[2] = true; return st.to_f32(data, m.emb_r, m.R / 16, C, C, nullptr); }
    if (name == "radar_a_emb.weight") { RALD_CHECK(nelem == (int64_t)(m.A / 16) * C, "size mismatch: " + name); m.tok_loaded[3] = true; return st.to_f32(data, m.emb_a, m.A / 16, C, C, nullptr); }
    if (name == "radar_e_emb.weight") { RALD_CHECK(nelem == (int64_t)(m.E / 16) * C, "size mismatch: " + name); m.tok_loaded[4] = true; return st.to_f32(data, m.emb_e, m.E / 16, C, C, nullptr); }
    RALD_CHECK(false, "radar encoder: unknown key '" + name + "'");
}

int RadarEncoder::Impl::ensure_ws(int nsub) {
    if (nsub <= sub) return 0;
    RALD_HIP(hipDeviceSynchronize());
    for (void* p : {(void*)f0, (void*)f1, (void*)f2, (void*)n16, (void*)stats, (void*)cpart, (void*)spart, (void*)q16, (void*)k16, (void*)vt16, (void*)p16, (void*)o16, (void*)sbuf})
        if (p) arena->release(p);
    const size_t vox = (size_t)R * A * E;
    const size_t act = (size_t)nsub * vox * ch;                 // level-0 activation (the largest)
    const int ntok = (R / 16) * (A / 16) * (E / 16), cl = ch * 4;
    f0 = (float*)arena->alloc(act * 4, true);
    f1 = (float*)arena->alloc(act * 4, true);
    f2 = (float*)arena->alloc(act * 4, true);
    n16 = (bf16*)arena->alloc(act * 2, true);
    gn_part_blocks = gn_blocks((int)vox);
    stats = (double*)arena->alloc((size_t)nsub * 64 * (1 + gn_part_blocks) * 8, true);   // final {sum, sumsq} + per-block partials
    spart_bytes = (size_t)8 << 20;                              // splits * tiles <= 256 tiles of 128 x 64 fp32
    spart = (float*)arena->alloc(spart_bytes, true);
    cpart_bytes = (size_t)nsub * (vox / 128) * 64 * 8;
    cpart = (double*)arena->alloc(cpart_bytes, true);
    q16 = (bf16*)arena->alloc((size_t)nsub * ntok * cl * 2, true);
    k16 = (bf16*)arena->alloc((size_t)nsub * ntok * cl * 2, true);
    vt16 = (bf16*)arena->alloc((size_t)nsub * cl * ntok * 2, true);
    p16 = (bf16*)arena->alloc((size_t)nsub * ntok * ntok * 2, true);
    o16 = (bf16*)arena->alloc((size_t)nsub * ntok * cl * 2, true);
    sbuf = (float*)arena->alloc((size_t)nsub * ntok * ntok * 4, true);
    RALD_CHECK(f0 && f1 && f2 && n16 && stats && cpart && spart && q16 && k16 && vt16 && p16 && o16 && sbuf, "radar encoder: workspace allocation failed");
    sub = nsub;
    return 0;
}

int RadarEncoder::Impl::gn(const float* x, const std::string& name, bf16* y, int B, int S, int C, bool swish, hipStream_t st) {
    RALD_CHECK(gn_blocks(S) <= gn_part_blocks, "radar encoder: GroupNorm partial buffer too small");
    const float *gamma = P<float>(name + ".weight"), *beta = P<float>(name + ".bias");
    if (x == fused_src && B == fused_B && S == fused_S && C == fused_C) {
        // the convolution that produced x left per-tile partials: no statistics pass over x
        RALD_TRY(gn_finish(cpart, stats, B, S / 128, st));
        return groupnorm_apply(x, stats, gamma, beta, y, B, S, C, swish ? 1 : 0, st);
    }
    return groupnorm_fwd(x, gamma, beta, y, stats, B, S, C, swish ? 1 : 0, st);
}

// One 3x3x3 convolution of the model through conv3d_full (its checks, the route, split-K through spart).  What stays here is the
// bookkeeping of the GroupNorm partials: a convolution into a trunk buffer leaves them in cpart where the shape allows, and fused_src
// names the activation they belong to until something else writes that buffer.
int RadarEncoder::Impl::run_conv(const bf16* in, const std::string& name, const float* resid, float* out, int B, int ID, int IH,
                                 int IW, int cin, int cout, int stride, int pad, hipStream_t st) {
    const int So = (ID / stride) * (IH / stride) * (IW / stride);
    double* part = nullptr;
    if (conv3d_route(B, ID, IH, IW, cin, cout, stride, pad, 1).engine == CONV_IGEMM_SPLIT) {
        if (out == fused_src) fused_src = nullptr;             // no GroupNorm partials from this path
    } else if (out == f0 || out == f1 || out == f2) {
        if (So % 128 == 0 && cout % 64 == 0 && (cout == 64 || cout == 128 || cout == 256) && (size_t)B * (So / 128) * 64 * 8 <= cpart_bytes) {
            part = cpart;
            fused_src = out; fused_B = B; fused_S = So; fused_C = cout;
        } else if (out == fused_src) fused_src = nullptr;      // this buffer is being overwritten without new partials
    }
    return conv3d_full(in, P<bf16>(name + ".weight"), P<float>(name + ".bias"), resid, out, nullptr, part, spart, (int64_t)spart_bytes, 1, B, ID,
                       IH, IW, cin, cout, stride, pad, st);
}

// ResnetBlock.forward (:82-100): x -> x + conv2(swish(GN(conv1(swish(GN(x)))))), 1x1 shortcut if channels change.
int RadarEncoder::Impl::resblock(float*& x, float*& t1, float*& t2, const std::string& name, int B, int Dd, int Hh, int Ww, int cin,
                                 int cout, hipStream_t st) {
    const int S = Dd * Hh * Ww;
    RALD_TRY(gn(x, name + ".norm1", n16, B, S, cin, true, st));
    RALD_TRY(run_conv(n16, name + ".conv1", nullptr, t1, B, Dd, Hh, Ww, cin, cout, 1, 1, st));
    const float* res = x;
    if (cin != cout) {
        RALD_TRY(cast_f32_bf16(x, n16, (int64_t)B * S * cin, st));
        GemmArgs g = gemm_args(n16, cin, P<bf16>(name + ".nin_shortcut.weight"), cin, t2, cout, P<float>(name + ".nin_shortcut.bias"), B * S, cout, cin);
        RALD_TRY(gemm_nt(g, EPI_F32, st));
        if (t2 == fused_src) fused_src = nullptr;
        res = t2;
    }
    RALD_TRY(gn(t1, name + ".norm2", n16, B, S, cout, true, st));
    float* dst = (cin != cout) ? t2 : x;                       // in-place residual add (same index read then written)
    RALD_TRY(run_conv(n16, name + ".conv2", res, dst, B, Dd, Hh, Ww, cout, cout, 1, 1, st));
    if (cin != cout) std::swap(x, t2);
    return 0;
}

// AttnBlock.forward (:112-135): single head over the S tokens, scale C^-1/2, residual.
int RadarEncoder::Impl::attnblock(float* x, const std::string& name, int B, int S, int C, hipStream_t st) {
    RALD_CHECK(S % 64 == 0, "radar attention: token count must be a multiple of 64");
    RALD_TRY(gn(x, name + ".norm", n16, B, S, C, false, st));
    GemmArgs q = gemm_args(n16, C, P<bf16>(name + ".q.weight"), C, q16, C, P<float>(name + ".q.bias"), B * S, C, C);
    RALD_TRY(gemm_nt(q, EPI_BF16, st));
    GemmArgs k = gemm_args(n16, C, P<bf16>(name + ".k.weight"), C, k16, C, P<float>(name + ".k.bias"), B * S, C, C);
    RALD_TRY(gemm_nt(k, EPI_BF16, st));
    GemmArgs v = gemm_args(P<bf16>(name + ".v.weight"), C, n16, C, vt16, S, nullptr, C, S, C);   // V^T (bias folded below)
    v.batch = B; v.strideB = (int64_t)S * C; v.strideC = (int64_t)C * S;
    RALD_TRY(gemm_nt(v, EPI_BF16, st));
    GemmArgs s = gemm_args(q16, C, k16, C, sbuf, S, nullptr, S, S, C);
    s.batch = B; s.strideA = (int64_t)S * C; s.strideB = (int64_t)S * C; s.strideC = (int64_t)S * S; s.alpha = 1.0f / sqrtf((float)C);
    RALD_TRY(gemm_nt(s, EPI_F32, st));
    RALD_TRY(softmax_rows(sbuf, S, p16, S, B * S, S, st));
    // rows of P sum to 1, so P.(v + 1.b_v^T) = P.v + b_v: the v bias becomes the epilogue bias
    GemmArgs pv = gemm_args(p16, S, vt16, S, o16, C, P<float>(name + ".v.bias"), S, C, S);
    pv.batch = B; pv.strideA = (int64_t)S * S; pv.strideB = (int64_t)C * S; pv.strideC = (int64_t)S * C;
    RALD_TRY(gemm_nt(pv, EPI_BF16, st));
    GemmArgs o = gemm_args(o16, C, P<bf16>(name + ".proj_out.weight"), C, x, C, P<float>(name + ".proj_out.bias"), B * S, C, C);
    RALD_TRY(gemm_nt(o, EPI_RESID, st));
    if (x == fused_src) fused_src = nullptr;                  // x changed in place: its conv partials are stale
    return 0;
}

int RadarEncoder::Impl::forward(const float* cube, int cube_ch, int B, float* zout, hipStream_t st) {
    for (const auto& kv : tensors) RALD_CHECK(kv.second.loaded, "radar encoder: missing key '" + kv.first + "'");
    RALD_TRY(ensure_ws(B));
    float *x = f0, *t1 = f1, *t2 = f2;
    fused_src = nullptr;
    int Dd = R, Hh = A, Ww = E;
    RALD_CHECK(cube_ch >= cin, "radar encoder: cube has fewer channels than conv_in expects");
    RALD_TRY(conv_in_fwd(cube, cube_ch, cin, P<float>("conv_in.weight"), P<float>("conv_in.bias"), x, B, Dd, Hh, Ww, ch, st));
    int cin = ch;
    for (int l = 0; l < 5; ++l) {
        const int cout = ch * kChMult[l];
        for (int b = 0; b < 2; ++b) {
            const std::string nm = "down." + std::to_string(l) + ".block." + std::to_string(b);
            RALD_TRY(resblock(x, t1, t2, nm, B, Dd, Hh, Ww, cin, cout, st));
            cin = cout;
            if (l == 4) RALD_TRY(attnblock(x, "down.4.attn." + std::to_string(b), B, Dd * Hh * Ww, cin, st));
        }
        if (l != 4) {
            // Downsample (:37-41): input is the raw trunk (no norm/activation), cast to bf16
            RALD_TRY(cast_f32_bf16(x, n16, (int64_t)B * Dd * Hh * Ww * cin, st));
            RALD_TRY(run_conv(n16, "down." + std::to_string(l) + ".downsample.conv", nullptr, t1, B, Dd, Hh, Ww, cin, cin, 2, 0, st));
            std::swap(x, t1);
            Dd /= 2; Hh /= 2; Ww /= 2;
        }
    }
    RALD_TRY(resblock(x, t1, t2, "mid.block_1", B, Dd, Hh, Ww, cin, cin, st));
    RALD_TRY(attnblock(x, "mid.attn_1", B, Dd * Hh * Ww, cin, st));
    RALD_TRY(resblock(x, t1, t2, "mid.block_2", B, Dd, Hh, Ww, cin, cin, st));
    RALD_TRY(gn(x, "norm_out", n16, B, Dd * Hh * Ww, cin, true, st));
    RALD_TRY(run_conv(n16, "conv_out", nullptr, zout, B, Dd, Hh, Ww, cin, zc, 1, 1, st));
    return 0;
}

int RadarEncoder::Impl::decode(const float* zin, int B, float* out, hipStream_t st) {
    for (const auto& kv : tensors) RALD_CHECK(kv.second.loaded, "radar decoder: missing key '" + kv.first + "'");
    RALD_TRY(ensure_ws(B));
    float *x = f0, *t1 = f1, *t2 = f2;
    fused_src = nullptr;
    int Dd = R / 16, Hh = A / 16, Ww = E / 16;
    int cin = ch * kChMult[4];
    RALD_TRY(pad_cast64(zin, n16, (int64_t)B * Dd * Hh * Ww, zc, st));
    RALD_TRY(run_conv(n16, "conv_in", nullptr, x, B, Dd, Hh, Ww, 64, cin, 1, 1, st));
    RALD_TRY(resblock(x, t1, t2, "mid.block_1", B, Dd, Hh, Ww, cin, cin, st));
    RALD_TRY(attnblock(x, "mid.attn_1", B, Dd * Hh * Ww, cin, st));
    RALD_TRY(resblock(x, t1, t2, "mid.block_2", B, Dd, Hh, Ww, cin, cin, st));
    for (int l = 4; l >= 0; --l) {
        const int cout = ch * kChMult[l];
        for (int b = 0; b < 3; ++b) {
            RALD_TRY(resblock(x, t1, t2, "up." + std::to_string(l) + ".block." + std::to_string(b), B, Dd, Hh, Ww, cin, cout, st));
            cin = cout;
        }
        if (l != 0) {
            RALD_TRY(upsample2_cast(x, n16, B, Dd, Hh, Ww, cin, st));
            Dd *= 2; Hh *= 2; Ww *= 2;
            RALD_TRY(run_conv(n16, "up." + std::to_string(l) + ".upsample.conv", nullptr, t1, B, Dd, Hh, Ww, cin, cin, 1, 1, st));
            std::swap(x, t1);
        }
    }
    RALD_TRY(gn(x, "norm_out", n16, B, Dd * Hh * Ww, cin, true, st));
    RALD_TRY(run_conv(n16, "conv_out", nullptr, out, B, Dd, Hh, Ww, cin, 4, 1, 1, st));       // [B][R][A][E][4]: channels 0..out_ch-1 are the reconstruction
    return 0;
}

// z [B][R/16][A/16][E/16][z_ch] fp32 (the layout RadarAutoencoder._encode returns) -> pred4 [B][R][A][E][4] fp32 (out_ch real channels + zero pad)
int RadarEncoder::decode(const float* z, int B, float* pred4, hipStream_t st) {
    RALD_CHECK(impl && impl->is_decoder && z && pred4 && B >= 1, "radar decoder: bad arguments");
    Impl& m = *impl;
    const int SUB = 4;
    const size_t zs = (size_t)(m.R / 16) * (m.A / 16) * (m.E / 16) * m.zc, os = (size_t)m.R * m.A * m.E * 4;
    for (int b0 = 0; b0 < B; b0 += SUB) {
        const int nb = B - b0 < SUB ? B - b0 : SUB;
        RALD_TRY(m.decode(z + (size_t)b0 * zs, nb, pred4 + (size_t)b0 * os, st));
    }
    return 0;
}

int RadarEncoder::encode(const float* cube, int cube_ch, int B, float** zptr, hipStream_t st) {
    RALD_CHECK(impl && cube && B >= 1, "radar encoder: bad arguments");
    Impl& m = *impl;
    const int ntok = (m.R / 16) * (m.A / 16) * (m.E / 16);
    if (B > m.tok_batch) {
        RALD_HIP(hipDeviceSynchronize());
        if (m.z) m.arena->release(m.z);
        if (m.tok) m.arena->release(m.tok);
        m.z = (float*)m.arena->alloc((size_t)B * ntok * m.zc * 4, true);
        m.tok = (float*)m.arena->alloc((size_t)B * ntok * m.token_ch * 4, true);
        RALD_CHECK(m.z && m.tok, "radar encoder: allocation failed");
        m.tok_batch = B;
    }
    const int SUB = 4;                                         // samples per pass: bounds the 67 MB/sample fp32 trunk buffers
    const size_t cube_stride = (size_t)m.R * m.A * m.E * cube_ch;
    for (int b0 = 0; b0 < B; b0 += SUB) {
        const int nb = B - b0 < SUB ? B - b0 : SUB;
        RALD_TRY(m.forward(cube + (size_t)b0 * cube_stride, cube_ch, nb, m.z + (size_t)b0 * ntok * m.zc, st));
    }
    *zptr = m.z;
    return 0;
}

int RadarEncoder::tokens(const float* cube, int B, float** tokens_out, hipStream_t st) {
    RALD_CHECK(impl, "radar encoder: not created");
    Impl& m = *impl;
    for (int i = 0; i < 5; ++i) RALD_CHECK(m.tok_loaded[i], "radar encoder: tokeniser weights missing");
    float* z = nullptr;
    RALD_TRY(encode(cube, 2, B, &z, st));                      // intensity channel of the [.,2] cube (:378)
    const int nr = m.R / 16, na = m.A / 16, ne = m.E / 16;
    RALD_TRY(radar_tokens(z, m.w_tok, m.b_tok, m.emb_r, m.emb_a, m.emb_e, m.tok, B, nr, na, ne, m.zc, m.token_ch, st));
    *tokens_out = m.tok;
    return 0;
}

RadarEncoder::~RadarEncoder() { delete impl; }

// ---- op-level launchers of the kernels above: the ONE launch site of each (the model above, the training path - radar_train.hip /
// train_encoder.py - and the tests all come through here) ------------------------------------------------------------------------
int groupnorm_fwd(const float* x, const float* gamma, const float* beta, bf16* y, double* stats, int B, int S, int C, int swish,
                  hipStream_t st) {
    RALD_CHECK(x && gamma && beta && y && stats, "groupnorm: null pointer");
    RALD_CHECK(B > 0 && S > 0 && C % 64 == 0 && 256 % (C / 4) == 0, "groupnorm: channel count must be 64, 128 or 256");
    double* part = stats + (size_t)B * 64;                 // caller contract: B*64*(1 + ceil(S/512)) doubles
    hipLaunchKernelGGL(gn_stats_kernel, dim3(gn_blocks(S), B), dim3(256), 0, st, x, part, S, C, GN_VPB);
    RALD_TRY(gn_finish(part, stats, B, gn_blocks(S), st));
    return groupnorm_apply(x, stats, gamma, beta, y, B, S, C, swish, st);
}

// the normalisation alone from statistics already in hand (the training backward re-creates the activations it did not keep)
int groupnorm_apply(const float* x, const double* stats, const float* gamma, const float* beta, bf16* y, int B, int S, int C, int swish, hipStream_t st) {
    RALD_CHECK(x && gamma && beta && y && stats, "groupnorm_apply: null pointer");
    RALD_CHECK(B > 0 && S > 0 && C % 64 == 0 && 256 % (C / 4) == 0, "groupnorm_apply: channel count must be 64, 128 or 256");
    const int64_t quads = (int64_t)S * C / 4;
    const int blocks = (int)((quads + 255) / 256 < 1024 ? (quads + 255) / 256 : 1024);
    hipLaunchKernelGGL(gn_apply_kernel, dim3(blocks, B), dim3(256), 0, st, x, stats, gamma, beta, y, S, C, 1e-6f, swish ? 1 : 0);
    RALD_HIP(hipGetLastError());
    return 0;
}

// gn_finish_kernel on caller partials: stats [B][32][2] = the sums over each sample's nblk slots part[b*nblk + k][32][2] (the route Impl::gn
// takes when the convolution epilogue left per-tile partials, nblk = S / 128)
int gn_finish(const double* part, double* stats, int B, int nblk, hipStream_t st) {
    RALD_CHECK(part && stats, "gn_finish: null pointer");
    RALD_CHECK(B > 0 && nblk > 0, "gn_finish: B and nblk must be positive");
    hipLaunchKernelGGL(gn_finish_kernel, dim3(B), dim3(1024), 0, st, part, stats, nblk);
    RALD_HIP(hipGetLastError());
    return 0;
}

int upsample2_cast(const float* x, bf16* y, int B, int D, int H, int W, int C, hipStream_t st) {
    RALD_CHECK(x && y, "upsample2_cast: null pointer");
    RALD_CHECK(B > 0 && D > 0 && H > 0 && W > 0 && C > 0, "upsample2_cast: bad shape");
    RALD_CHECK(C % 4 == 0, "upsample2_cast: C must be a multiple of 4 (float4 reads, 4 x bf16 stores)");
    RALD_CHECK((uintptr_t)x % 16 == 0 && (uintptr_t)y % 8 == 0, "upsample2_cast: x must be 16-byte and y 8-byte aligned");
    const int64_t quads = (int64_t)B * 8 * D * H * W * (C / 4);
    const unsigned blocks = (unsigned)((quads + 255) / 256 < 8192 ? (quads + 255) / 256 : 8192);
    hipLaunchKernelGGL(upsample2_cast_kernel, dim3(blocks), dim3(256), 0, st, x, y, B, D, H, W, C);
    RALD_HIP(hipGetLastError());
    return 0;
}

int pad_cast64(const float* z, bf16* y, int64_t rows, int zc, hipStream_t st) {
    RALD_CHECK(z && y, "pad_cast64: null pointer");
    RALD_CHECK(rows > 0 && rows <= ((int64_t)1 << 31), "pad_cast64: bad row count");
    RALD_CHECK(zc >= 1 && zc <= 64, "pad_cast64: zc must be in 1 .. 64 (rows of 64 channels)");
    hipLaunchKernelGGL(pad_cast64_kernel, dim3((unsigned)((rows * 64 + 255) / 256)), dim3(256), 0, st, z, y, rows, zc);
    RALD_HIP(hipGetLastError());
    return 0;
}

// the tokeniser half of RadarEncoder::tokens without the encoder: z [B][R*A*E][zc] (R, A, E = the token grid) -> tok [B][R*A*E][C]
int radar_tokens(const float* z, const float* Wp, const float* bp, const float* re, const float* ae, const float* ee, float* tok, int B, int R, int A,
                 int E, int zc, int C, hipStream_t st) {
    RALD_CHECK(z && Wp && bp && re && ae && ee && tok, "radar_tokens: null pointer");
    RALD_CHECK(B > 0 && B <= 65535 && R > 0 && A > 0 && E > 0 && C > 0, "radar_tokens: bad shape (B <= 65535)");
    RALD_CHECK(zc >= 1 && zc <= 64, "radar_tokens: zc must be in 1 .. 64");
    RALD_CHECK((int64_t)R * A * E <= 0x7fffffff, "radar_tokens: too many tokens per sample");
    hipLaunchKernelGGL(radar_token_kernel, dim3(R * A * E, B), dim3(256), 0, st, z, Wp, bp, re, ae, ee, tok, R, A, E, zc, C);
    RALD_HIP(hipGetLastError());
    return 0;
}

int conv_in_fwd(const float* cube, int cube_ch, int Cin, const float* W, const float* bias, float* out, int B, int D, int H, int Wd, int Cout,
                hipStream_t st) {
    RALD_CHECK(cube && W && bias && out && Cout % 8 == 0 && 256 % (Cout / 8) == 0 && cube_ch >= Cin, "conv_in: bad arguments");
    const int groups = Cout / 8, vpb = 256 / groups;
    const int64_t nvox = (int64_t)B * D * H * Wd;
    hipLaunchKernelGGL(conv_in_kernel, dim3((unsigned)((nvox + vpb - 1) / vpb)), dim3(256), Cin * 27 * Cout * 4, st, cube, cube_ch, Cin, W, bias, out,
                       B, D, H, Wd, Cout);
    RALD_HIP(hipGetLastError());
    return 0;
}

}  // namespace rald
