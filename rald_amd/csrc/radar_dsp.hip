// Radar front end on the device: raw ADC frames -> RAEIVV cubes (dataset_preprocessor/radar.py:64-76 load_radar_data and
// utils/radar_preprocessing.py:6-62 RAEIVVmap, a complex128 numpy chain in the reference).  Per frame:
//   dsp_channel_sums   (frame, channel)          exact int64 sums of I and Q: the complex mean of the frame, batch-independent
//   dsp_range_fft      (frame, channel, chirps)  mean removal + Blackman window on load, range FFT in LDS, stored [range][chirp]
//   dsp_doppler_fft    (frame, channel, ranges)  Doppler FFT in LDS over the chirps, fftshift + velocity compensation on store
//   dsp_angle          (frame, range bin, cells) virtual array + azimuth/elevation transform as a direct DFT over the populated
//                                                 grid (a zero-padded FFT is exactly that), |.|^2, argmax / top-2 / sum over Doppler
//   dsp_noise_db       (frame)                   exact 30 % quantile by radix select on the float bits, then the dB pass
// Everything is fp32 except the mean (exact integers, divided in double) and the quantile interpolation and dB conversion (double).
// No float atomics: every reduction has a fixed order, so a frame's cube is bit-identical whatever batch it runs in.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "radar_dsp.h"

namespace rald {

namespace {

constexpr int DSP_THREADS = 256;
constexpr int FFT_TILE = 2048;       // complex values per range / Doppler FFT tile in LDS (16 KiB + padding)
constexpr int TW_N = 256;            // twiddle table exp(-2 pi i k / TW_N), k < TW_N / 2, serves every FFT length up to 256
constexpr int MAX_GRID = 32;         // cells of the dense virtual grid the angle DFT reads
constexpr int ANGLE_CELLS = 64;      // output cells per dsp_angle workgroup: 4 Doppler groups of one wave each
constexpr double NOISE_Q = 0.30;     // radar_preprocessing.py:4 NOISE_THRESHOLD

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ int bitrev(int x, int log2n) { return (int)(__brev((unsigned)x) >> (32 - log2n)); }

// In-place radix-2 decimation-in-time FFT of `rows` rows of length 1 << log2n, row stride ld (complex), held in LDS in
// bit-reversed order.  The caller synchronises before; this synchronises after every stage.
__device__ void lds_fft_rows(float2* s, int rows, int log2n, int ld, const float2* __restrict__ tw) {
    const int half = 1 << (log2n - 1), total = rows * half;
    for (int lh = 0; lh < log2n; ++lh) {
        const int h = 1 << lh, tstep = (TW_N / 2) >> lh;
        for (int j = threadIdx.x; j < total; j += blockDim.x) {
            const int row = j >> (log2n - 1), k = j & (half - 1);
            const int pos = k & (h - 1), i0 = ((k >> lh) << (lh + 1)) + pos;
            float2* r = s + row * ld;
            const float2 a = r[i0], t = cmul(r[i0 + h], tw[pos * tstep]);
            r[i0] = make_float2(a.x + t.x, a.y + t.y);
            r[i0 + h] = make_float2(a.x - t.x, a.y - t.y);
        }
        __syncthreads();
    }
}

// grid (nch, B): sums[b][ch] = {sum I, sum Q} over the channel's n_per_ch samples
__global__ __launch_bounds__(DSP_THREADS) void dsp_channel_sums(const short2* __restrict__ frames, int n_per_ch, long long* __restrict__ sums) {
    __shared__ long long red[2][DSP_THREADS];
    const int ch = blockIdx.x, b = blockIdx.y, nch = gridDim.x, tid = threadIdx.x;
    const short2* p = frames + ((size_t)b * nch + ch) * n_per_ch;
    long long si = 0, sq = 0;
    for (int i = tid; i < n_per_ch; i += DSP_THREADS) {
        const short2 v = p[i];
        si += v.x;
        sq += v.y;
    }
    red[0][tid] = si;
    red[1][tid] = sq;
    __syncthreads();
    for (int off = DSP_THREADS / 2; off > 0; off >>= 1) {
        if (tid < off) {
            red[0][tid] += red[0][tid + off];
            red[1][tid] += red[1][tid + off];
        }
        __syncthreads();
    }
    if (tid == 0) {
        sums[((size_t)b * nch + ch) * 2] = red[0][0];
        sums[((size_t)b * nch + ch) * 2 + 1] = red[1][0];
    }
}

// grid (chirp tiles, nch, B): buf[b][ch][range bin][chirp] (row stride nd) = FFT_nr(window * (x - mean)) of chirps
// [tile*ct, tile*ct + ct) ∩ [0, nc_used); samples >= ns_used are cut (numpy's n < length), the rest zero-pads.
template <bool INT16>
__global__ __launch_bounds__(DSP_THREADS) void dsp_range_fft(const void* __restrict__ frames, const long long* __restrict__ sums,
                                                             const float* __restrict__ win, const float2* __restrict__ tw,
                                                             float2* __restrict__ buf, int nc, int ns, int nc_used, int ns_used, int log2r,
                                                             int log2d, int ct) {
    extern __shared__ __attribute__((aligned(16))) float2 lds[];
    const int c0 = blockIdx.x * ct, ch = blockIdx.y, b = blockIdx.z, nch = gridDim.y, tid = threadIdx.x;
    const int nr = 1 << log2r, ld = nr + 1, rows = min(ct, nc_used - c0);
    double mi = 0.0, mq = 0.0;
    if (INT16) {
        long long si = 0, sq = 0;
        for (int c = 0; c < nch; ++c) {
            si += sums[((size_t)b * nch + c) * 2];
            sq += sums[((size_t)b * nch + c) * 2 + 1];
        }
        const double n = (double)nch * nc * ns;
        mi = (double)si / n;
        mq = (double)sq / n;
    }
    const size_t in0 = ((size_t)(b * nch + ch) * nc + c0) * ns;
    for (int idx = tid; idx < rows * nr; idx += DSP_THREADS) {
        const int r = idx >> log2r, s = idx & (nr - 1);
        float2 v = make_float2(0.f, 0.f);
        if (s < ns_used) {
            const size_t e = in0 + (size_t)r * ns + s;
            if (INT16) {
                const short2 q = ((const short2*)frames)[e];
                v = make_float2((float)((double)q.x - mi), (float)((double)q.y - mq));
            } else {
                v = ((const float2*)frames)[e];
            }
            const float w = win[s];
            v.x *= w;
            v.y *= w;
        }
        lds[r * ld + bitrev(s, log2r)] = v;
    }
    __syncthreads();
    lds_fft_rows(lds, rows, log2r, ld, tw);
    float2* o = buf + ((size_t)(b * nch + ch) << (log2r + log2d)) + c0;
    for (int idx = tid; idx < rows * nr; idx += DSP_THREADS) {
        const int rb = idx / rows, r = idx - rb * rows;
        o[((size_t)rb << log2d) + r] = lds[r * ld + rb];
    }
}

// grid (range tiles, nch, B), in place on buf: row [b][ch][r][0, nc_used) -> fftshift(FFT_nd(row))[d] * vcomp[ch / nrx][d]
__global__ __launch_bounds__(DSP_THREADS) void dsp_doppler_fft(float2* __restrict__ buf, const float2* __restrict__ tw,
                                                               const float2* __restrict__ vcomp, int nrx, int nc_used, int log2r, int log2d,
                                                               int rt) {
    extern __shared__ __attribute__((aligned(16))) float2 lds[];
    const int r0 = blockIdx.x * rt, ch = blockIdx.y, b = blockIdx.z, nch = gridDim.y, tid = threadIdx.x;
    const int nd = 1 << log2d, ld = nd + 1, rows = min(rt, (1 << log2r) - r0);
    float2* rowp = buf + ((size_t)(b * nch + ch) << (log2r + log2d)) + ((size_t)r0 << log2d);
    for (int idx = tid; idx < rows * nd; idx += DSP_THREADS) {
        const int r = idx >> log2d, c = idx & (nd - 1);
        lds[r * ld + bitrev(c, log2d)] = c < nc_used ? rowp[idx] : make_float2(0.f, 0.f);
    }
    __syncthreads();
    lds_fft_rows(lds, rows, log2d, ld, tw);
    const float2* vc = vcomp + (size_t)(ch / nrx) * nd;
    for (int idx = tid; idx < rows * nd; idx += DSP_THREADS) {
        const int r = idx >> log2d, d = idx & (nd - 1);
        rowp[idx] = cmul(lds[r * ld + ((d + nd / 2) & (nd - 1))], vc[d]);
    }
}

struct AngleArgs {
    const float2* buf;
    const float2* waz;     // [A][naz]
    const float2* wel;     // [E][nel]
    const int2* pairs;     // {channel, grid cell}
    const float* vbins;
    float* out;            // [B][nr][A][E][3]
    int nch, npairs, nel, naz, A, E, log2r, log2d, crop_lo, crop_hi;
};

// grid (nr, cell chunks, B): each workgroup takes ANGLE_CELLS output cells of one range bin (more workgroups, fewer Doppler bins per
// thread; every chunk rebuilds the small virtual array).  LDS: va [nel*naz][nd] | waz [A*naz] | wel [E*nel] | 4 x DSP_THREADS merge slots
__global__ __launch_bounds__(DSP_THREADS) void dsp_angle(AngleArgs p) {
    extern __shared__ __attribute__((aligned(16))) float2 lds[];
    const int r = blockIdx.x, chunk = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
    const int nr = 1 << p.log2r, nd = 1 << p.log2d, cells = p.A * p.E, ng = p.nel * p.naz;
    float* o = p.out + ((size_t)b * nr + r) * cells * 3;
    if (r < p.crop_lo || r >= nr - p.crop_hi) {          // zeroed bins: P = 0 everywhere -> argmax 0, invalid, S = 0
        const float v0 = p.vbins[0];
        for (int c = chunk * ANGLE_CELLS + tid; c < min(cells, (chunk + 1) * ANGLE_CELLS); c += DSP_THREADS) {
            o[3 * c] = 0.f;
            o[3 * c + 1] = v0;
            o[3 * c + 2] = 0.f;
        }
        return;
    }
    float2* va = lds;
    float2* waz = va + ng * nd;
    float2* wel = waz + p.A * p.naz;
    float* m_best = (float*)(wel + p.E * p.nel);
    float* m_second = m_best + DSP_THREADS;
    float* m_sum = m_second + DSP_THREADS;
    int* m_idx = (int*)(m_sum + DSP_THREADS);
    for (int i = tid; i < p.A * p.naz; i += DSP_THREADS) waz[i] = p.waz[i];
    for (int i = tid; i < p.E * p.nel; i += DSP_THREADS) wel[i] = p.wel[i];
    const float2* rows = p.buf + ((size_t)b * p.nch << (p.log2r + p.log2d)) + ((size_t)r << p.log2d);   // + ch * nr * nd: channel row at r
    for (int d = tid; d < nd; d += DSP_THREADS) {
        for (int g = 0; g < ng; ++g) va[g * nd + d] = make_float2(0.f, 0.f);
        for (int q = 0; q < p.npairs; ++q) {                // the reference's loop order: va[tel+rel, taz+raz] += dfft[tidx, ridx]
            const int2 pr = p.pairs[q];
            const float2 x = rows[((size_t)pr.x << (p.log2r + p.log2d)) + d];
            float2& v = va[pr.y * nd + d];
            v.x += x.x;
            v.y += x.y;
        }
    }
    __syncthreads();
    const int cpp = min(cells, ANGLE_CELLS);                // cells per workgroup
    const int G = min(DSP_THREADS / cpp, nd);               // Doppler groups per cell (a function of the config only)
    {
        const int cell = chunk * cpp + tid % cpp, g = tid / cpp;
        const bool active = g < G && cell < cells;
        float best = -1.f, second = -1.f, sum = 0.f;
        int idx = 0;
        if (active) {
            const int a = cell / p.E, e = cell - a * p.E;
            const float2* wa = waz + a * p.naz;
            const float2* we = wel + e * p.nel;
            for (int d = g; d < nd; d += G) {
                float2 acc = make_float2(0.f, 0.f);
                for (int el = 0; el < p.nel; ++el) {
                    float2 inner = make_float2(0.f, 0.f);
                    const float2* row = va + (el * p.naz) * nd + d;
                    for (int az = 0; az < p.naz; ++az) {
                        const float2 t = cmul(row[az * nd], wa[az]);
                        inner.x += t.x;
                        inner.y += t.y;
                    }
                    const float2 t = cmul(inner, we[el]);
                    acc.x += t.x;
                    acc.y += t.y;
                }
                const float pw = acc.x * acc.x + acc.y * acc.y;
                if (pw > best) {           // numpy argmax keeps the first maximum; an equal later value becomes the second entry
                    second = best;
                    best = pw;
                    idx = d;
                } else {
                    second = fmaxf(second, pw);
                }
                sum += pw;
            }
        }
        m_best[tid] = best;
        m_second[tid] = second;
        m_sum[tid] = sum;
        m_idx[tid] = idx;
        __syncthreads();
        if (active && g == 0) {
            for (int j = 1; j < G; ++j) {       // fixed merge order: group j covers d = j (mod G)
                const int s = tid + j * cpp;
                const float b2 = m_best[s];
                second = fmaxf(fmaxf(second, m_second[s]), fminf(best, b2));
                if (b2 > best || (b2 == best && m_idx[s] < idx)) {
                    best = b2;
                    idx = m_idx[s];
                }
                sum += m_sum[s];
            }
            o[3 * cell] = sum;
            o[3 * cell + 1] = p.vbins[idx];
            o[3 * cell + 2] = (double)best * (1.0 - NOISE_Q) > (double)second ? 1.f : 0.f;
        }
        __syncthreads();
    }
}

// NOISE_UNROLL independent loads in flight per thread: the single workgroup of a frame is otherwise latency-bound
constexpr int NOISE_UNROLL = 8;
__device__ __forceinline__ void load_bits(const float* o, int n, int i0, unsigned (&u)[NOISE_UNROLL]) {
#pragma unroll
    for (int j = 0; j < NOISE_UNROLL; ++j) {
        const int i = i0 + j * 1024;
        u[j] = i < n ? __float_as_uint(o[3 * i]) : 0u;
    }
}

// grid (B): S = out[b][i][0] for i < n.  noise = np.quantile(S, 0.3) ('linear': order statistics k, k + 1 and the fraction),
// then out[b][i][0] = 10 log10(S / (noise + 1e-6) + 1).  Radix select over the bit patterns of S >= 0 (their integer order is
// the float order), 8 bits per pass; LDS integer atomics only.
__global__ __launch_bounds__(1024) void dsp_noise_db(float* __restrict__ out, int n, int k, double frac) {
    __shared__ unsigned hist[256], scan[256];
    __shared__ unsigned s_prefix, s_krem, s_cnt, s_min;
    const int tid = threadIdx.x;
    float* o = out + (size_t)blockIdx.x * n * 3;
    unsigned prefix = 0, mask = 0, krem = (unsigned)k;
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        for (int i0 = tid; i0 < n; i0 += NOISE_UNROLL * 1024) {
            unsigned u[NOISE_UNROLL];
            load_bits(o, n, i0, u);
#pragma unroll
            for (int j = 0; j < NOISE_UNROLL; ++j)
                if (i0 + j * 1024 < n && (u[j] & mask) == prefix) atomicAdd(&hist[(u[j] >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid < 256) scan[tid] = hist[tid];
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            unsigned v = 0;
            if (tid < 256 && tid >= off) v = scan[tid - off];
            __syncthreads();
            if (tid < 256) scan[tid] += v;
            __syncthreads();
        }
        if (tid < 256) {
            const unsigned incl = scan[tid], excl = incl - hist[tid];
            if (excl <= krem && krem < incl) {
                s_prefix = prefix | ((unsigned)tid << shift);
                s_krem = krem - excl;
                s_cnt = hist[tid];
            }
        }
        __syncthreads();
        prefix = s_prefix;
        krem = s_krem;
        mask |= 255u << shift;
        __syncthreads();
    }
    const double vk = (double)__uint_as_float(prefix);
    double vk1 = vk;
    if (k + 1 < n && krem + 1 >= s_cnt) {     // the (k+1)-th value is the smallest one above v_k
        if (tid == 0) s_min = 0xffffffffu;
        __syncthreads();
        unsigned m = 0xffffffffu;
        for (int i0 = tid; i0 < n; i0 += NOISE_UNROLL * 1024) {
            unsigned u[NOISE_UNROLL];
            load_bits(o, n, i0, u);
#pragma unroll
            for (int j = 0; j < NOISE_UNROLL; ++j)
                if (i0 + j * 1024 < n && u[j] > prefix) m = min(m, u[j]);
        }
        atomicMin(&s_min, m);
        __syncthreads();
        vk1 = (double)__uint_as_float(s_min);
    }
    const double diff = vk1 - vk;             // numpy's _lerp
    const double noise = frac >= 0.5 ? vk1 - diff * (1.0 - frac) : vk + diff * frac;
    const double inv = 1.0 / (noise + 1e-6);
    for (int i0 = tid; i0 < n; i0 += NOISE_UNROLL * 1024) {
        unsigned u[NOISE_UNROLL];
        load_bits(o, n, i0, u);
#pragma unroll
        for (int j = 0; j < NOISE_UNROLL; ++j)
            if (i0 + j * 1024 < n) o[3 * (i0 + j * 1024)] = (float)(10.0 * log10((double)__uint_as_float(u[j]) * inv + 1.0));
    }
}

bool pow2_in(int v, int lo, int hi) { return v >= lo && v <= hi && (v & (v - 1)) == 0; }
int ilog2(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }
size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

size_t angle_lds_bytes(const RadarDsp& h) {
    const rald_radar_dsp_config& c = h.cfg;
    return (size_t)(h.nel * h.naz * c.doppler_fft + c.angle_fft * h.naz + c.elevation_fft * h.nel) * 8 + DSP_THREADS * 16;
}

}  // namespace

int radar_dsp_check_sizes(const rald_radar_dsp_config& c) {
    RALD_CHECK(c.ntx >= 1 && c.ntx <= 16 && c.nrx >= 1 && c.nrx <= 16, "radar_dsp: ntx and nrx must be in [1, 16]");
    RALD_CHECK(c.n_chirps >= 1 && c.n_chirps <= 4096 && c.n_samples >= 1 && c.n_samples <= 4096,
               "radar_dsp: n_chirps and n_samples must be in [1, 4096]");
    RALD_CHECK(pow2_in(c.range_fft, 2, 256) && pow2_in(c.doppler_fft, 2, 256),
               "radar_dsp: range_fftsize and doppler_fftsize must be powers of two in [2, 256], got " + std::to_string(c.range_fft) + " and " +
                   std::to_string(c.doppler_fft));
    RALD_CHECK(c.angle_fft >= 1 && c.angle_fft <= 64 && c.elevation_fft >= 1 && c.elevation_fft <= 64,
               "radar_dsp: ANGLE_fftsize and ELEVATION_fftsize must be in [1, 64], got " + std::to_string(c.angle_fft) + " and " +
                   std::to_string(c.elevation_fft));
    const int nr = c.range_fft;
    RALD_CHECK(c.crop_low >= 0.0 && c.crop_high >= 0.0 && c.crop_low <= 1.0 && c.crop_high <= 1.0, "radar_dsp: crop_low / crop_high must be in [0, 1]");
    RALD_CHECK((int)(nr * c.crop_high) >= 1, "radar_dsp: int(range_fftsize * crop_high) = 0: the reference's efft[..., -0:] = 0 would zero every range bin; "
                               "use a crop_high of at least 1 / range_fftsize");
    return 0;
}

int radar_dsp_plan(const rald_radar_dsp_config& c, const int32_t* tx, const int32_t* rx, const double* vbins, int32_t n_vbins, RadarDsp& h,
                   std::vector<char>* tables) {
    RALD_TRY(radar_dsp_check_sizes(c));
    const int nr = c.range_fft;
    h.crop_lo = (int)(nr * c.crop_low);
    h.crop_hi = (int)(nr * c.crop_high);
    RALD_CHECK(vbins && n_vbins >= c.doppler_fft, "radar_dsp: need a velocity for each of the " + std::to_string(c.doppler_fft) +
                                                      " Doppler bins, got " + std::to_string(n_vbins));
    RALD_CHECK(tx && rx, "radar_dsp: null antenna layout");
    int max_tel = 0, max_taz = 0, max_rel = 0, max_raz = 0;
    for (int i = 0; i < c.ntx; ++i) {
        RALD_CHECK(tx[3 * i] >= 0 && tx[3 * i] < c.ntx && tx[3 * i + 1] >= 0 && tx[3 * i + 1] < 64 && tx[3 * i + 2] >= 0 && tx[3 * i + 2] < 64,
                   "radar_dsp: tx layout row " + std::to_string(i) + " out of range");
        max_taz = std::max(max_taz, tx[3 * i + 1]);
        max_tel = std::max(max_tel, tx[3 * i + 2]);
    }
    for (int i = 0; i < c.nrx; ++i) {
        RALD_CHECK(rx[3 * i] >= 0 && rx[3 * i] < c.nrx && rx[3 * i + 1] >= 0 && rx[3 * i + 1] < 64 && rx[3 * i + 2] >= 0 && rx[3 * i + 2] < 64,
                   "radar_dsp: rx layout row " + std::to_string(i) + " out of range");
        max_raz = std::max(max_raz, rx[3 * i + 1]);
        max_rel = std::max(max_rel, rx[3 * i + 2]);
    }
    // virtual_array (radardsp.py:54-111) spans [max tel + max rel + 1][max taz + max raz + 1]; the angle FFTs read at most
    // ANGLE_fftsize azimuth and ELEVATION_fftsize elevation positions of it
    h.nel = std::min(max_tel + max_rel + 1, c.elevation_fft);
    h.naz = std::min(max_taz + max_raz + 1, c.angle_fft);
    RALD_CHECK(h.nel * h.naz <= MAX_GRID, "radar_dsp: the virtual array grid the angle transform reads has " + std::to_string(h.nel * h.naz) +
                                              " cells; at most " + std::to_string(MAX_GRID) + " are supported");
    h.cfg = c;
    h.nch = c.ntx * c.nrx;
    h.nc_used = std::min(c.n_chirps, c.doppler_fft);
    h.ns_used = std::min(c.n_samples, c.range_fft);
    if (!tables) return 0;

    const int nd = c.doppler_fft, A = c.angle_fft, E = c.elevation_fft, ns = c.n_samples;
    std::vector<float> win(ns);
    for (int i = 0; i < ns; ++i) {                       // np.blackman
        if (ns == 1) { win[i] = 1.f; break; }
        const double m = (double)(1 - ns + 2 * i);
        win[i] = (float)(0.42 + 0.5 * std::cos(M_PI * m / (ns - 1)) + 0.08 * std::cos(2.0 * M_PI * m / (ns - 1)));
    }
    auto cexp = [](double ph) { return make_float2((float)std::cos(ph), (float)std::sin(ph)); };
    std::vector<float2> tw(TW_N / 2), vc((size_t)c.ntx * nd), waz((size_t)A * h.naz), wel((size_t)E * h.nel);
    for (int i = 0; i < TW_N / 2; ++i) tw[i] = cexp(-2.0 * M_PI * i / TW_N);
    for (int t = 0; t < c.ntx; ++t)                      // velocity_compensation (radardsp.py:526-545)
        for (int d = 0; d < nd; ++d) vc[(size_t)t * nd + d] = cexp(-2.0 * M_PI * (double)t * (d - nd / 2) / ((double)c.ntx * nd));
    for (int a = 0; a < A; ++a) {                        // output bin a of the shifted FFT is frequency (a - A/2) mod A
        const int ka = ((a - A / 2) % A + A) % A;
        for (int az = 0; az < h.naz; ++az) waz[(size_t)a * h.naz + az] = cexp(-2.0 * M_PI * (double)((ka * az) % A) / A);
    }
    for (int e = 0; e < E; ++e) {
        const int ke = ((e - E / 2) % E + E) % E;
        for (int el = 0; el < h.nel; ++el) wel[(size_t)e * h.nel + el] = cexp(-2.0 * M_PI * (double)((ke * el) % E) / E);
    }
    std::vector<float> vb(nd);
    for (int d = 0; d < nd; ++d) vb[d] = (float)vbins[d];
    std::vector<int2> pairs;
    for (int i = 0; i < c.ntx; ++i)
        for (int j = 0; j < c.nrx; ++j) {
            const int el = tx[3 * i + 2] + rx[3 * j + 2], az = tx[3 * i + 1] + rx[3 * j + 1];
            if (el < h.nel && az < h.naz) pairs.push_back(make_int2(tx[3 * i] * c.nrx + rx[3 * j], el * h.naz + az));
        }
    h.npairs = (int)pairs.size();
    // one blob: window | twiddles | vcomp | waz | wel | vbins | pairs, each 16-byte aligned
    size_t off = 0;
    auto place = [&](size_t bytes) { const size_t o = off; off = align16(off + bytes); return o; };
    const size_t o_win = place(win.size() * 4), o_tw = place(tw.size() * 8), o_vc = place(vc.size() * 8), o_waz = place(waz.size() * 8),
                 o_wel = place(wel.size() * 8), o_vb = place(vb.size() * 4), o_pr = place(std::max<size_t>(pairs.size(), 1) * 8);
    tables->assign(off, 0);
    char* t = tables->data();
    memcpy(t + o_win, win.data(), win.size() * 4);
    memcpy(t + o_tw, tw.data(), tw.size() * 8);
    memcpy(t + o_vc, vc.data(), vc.size() * 8);
    memcpy(t + o_waz, waz.data(), waz.size() * 8);
    memcpy(t + o_wel, wel.data(), wel.size() * 8);
    memcpy(t + o_vb, vb.data(), vb.size() * 4);
    if (!pairs.empty()) memcpy(t + o_pr, pairs.data(), pairs.size() * 8);
    // device pointers are offsets until radar_dsp_create rebases them
    h.win = (const float*)o_win;
    h.tw = (const float2*)o_tw;
    h.vcomp = (const float2*)o_vc;
    h.waz = (const float2*)o_waz;
    h.wel = (const float2*)o_wel;
    h.vbins = (const float*)o_vb;
    h.pairs = (const int2*)o_pr;
    return 0;
}

int64_t radar_dsp_workspace_bytes(const rald_radar_dsp_config& c, int32_t batch) {
    const int64_t nch = (int64_t)c.ntx * c.nrx;
    return round_up(batch * nch * 16, 256) + batch * nch * c.range_fft * c.doppler_fft * 8;
}

RadarDsp::~RadarDsp() {
    if (dev) (void)hipFree(dev);
}

int radar_dsp_create(const rald_radar_dsp_config& cfg, const int32_t* tx, const int32_t* rx, const double* vbins, int32_t n_vbins,
                     RadarDsp** out) {
    RadarDsp* h = new RadarDsp();
    std::vector<char> tables;
    int rc = radar_dsp_plan(cfg, tx, rx, vbins, n_vbins, *h, &tables);
    if (rc) { delete h; return rc; }
    const size_t lds = angle_lds_bytes(*h);
    hipError_t e = hipMalloc(&h->dev, tables.size());
    if (e == hipSuccess) e = hipMemcpy(h->dev, tables.data(), tables.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess && lds > 65536) e = hipFuncSetAttribute((const void*)dsp_angle, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) {
        set_error(std::string("radar_dsp_create: ") + hipGetErrorString(e));
        delete h;
        return 2;
    }
    char* base = (char*)h->dev;
    h->win = (const float*)(base + (size_t)h->win);
    h->tw = (const float2*)(base + (size_t)h->tw);
    h->vcomp = (const float2*)(base + (size_t)h->vcomp);
    h->waz = (const float2*)(base + (size_t)h->waz);
    h->wel = (const float2*)(base + (size_t)h->wel);
    h->vbins = (const float*)(base + (size_t)h->vbins);
    h->pairs = (const int2*)(base + (size_t)h->pairs);
    *out = h;
    return 0;
}

int radar_dsp_run(const RadarDsp& h, const void* frames, int input_kind, int32_t batch, float* out, void* workspace, int64_t workspace_bytes,
                  hipStream_t st) {
    const rald_radar_dsp_config& c = h.cfg;
    RALD_CHECK(frames && out && workspace && batch >= 1, "radar_dsp_run: bad argument");
    RALD_CHECK(input_kind == 0 || input_kind == 1, "radar_dsp_run: input_kind must be 0 (int16) or 1 (fp32)");
    RALD_CHECK(workspace_bytes >= radar_dsp_workspace_bytes(c, batch), "radar_dsp_run: workspace too small (rald_radar_dsp_workspace_bytes)");
    const int nr = c.range_fft, nd = c.doppler_fft, log2r = ilog2(nr), log2d = ilog2(nd);
    long long* sums = (long long*)workspace;
    float2* buf = (float2*)((char*)workspace + round_up((int64_t)batch * h.nch * 16, 256));
    const int ct = std::min(FFT_TILE / nr, h.nc_used), rt = std::min(FFT_TILE / nd, nr);
    const dim3 g_range(cdiv(h.nc_used, ct), h.nch, batch), g_dopp(cdiv(nr, rt), h.nch, batch);
    const size_t lds_range = (size_t)ct * (nr + 1) * 8, lds_dopp = (size_t)rt * (nd + 1) * 8;
    if (input_kind == 0) {
        hipLaunchKernelGGL(dsp_channel_sums, dim3(h.nch, batch), dim3(DSP_THREADS), 0, st, (const short2*)frames, c.n_chirps * c.n_samples, sums);
        hipLaunchKernelGGL(dsp_range_fft<true>, g_range, dim3(DSP_THREADS), lds_range, st, frames, (const long long*)sums, h.win, h.tw, buf,
                           c.n_chirps, c.n_samples, h.nc_used, h.ns_used, log2r, log2d, ct);
    } else {
        hipLaunchKernelGGL(dsp_range_fft<false>, g_range, dim3(DSP_THREADS), lds_range, st, frames, (const long long*)sums, h.win, h.tw, buf,
                           c.n_chirps, c.n_samples, h.nc_used, h.ns_used, log2r, log2d, ct);
    }
    hipLaunchKernelGGL(dsp_doppler_fft, g_dopp, dim3(DSP_THREADS), lds_dopp, st, buf, h.tw, h.vcomp, c.nrx, h.nc_used, log2r, log2d, rt);
    AngleArgs a{buf, h.waz, h.wel, h.pairs, h.vbins, out, h.nch, h.npairs, h.nel, h.naz, c.angle_fft, c.elevation_fft, log2r, log2d, h.crop_lo, h.crop_hi};
    hipLaunchKernelGGL(dsp_angle, dim3(nr, cdiv(c.angle_fft * c.elevation_fft, ANGLE_CELLS), batch), dim3(DSP_THREADS), angle_lds_bytes(h), st, a);
    const int n = nr * c.angle_fft * c.elevation_fft;
    const double vi = NOISE_Q * (n - 1);
    const int k = (int)std::floor(vi);
    hipLaunchKernelGGL(dsp_noise_db, dim3(batch), dim3(1024), 0, st, out, n, k, vi - k);
    RALD_HIP(hipGetLastError());
    return 0;
}

}  // namespace rald
