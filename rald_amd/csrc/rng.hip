// Counter-based normal generator (Philox4x32-10 + Box-Muller) and the sampler's churn step (edm_sampler :258-260).
//
// The noise is a pure function of (seed, purpose, step, element): no generator state, no atomics, nothing to advance, so a captured
// hipGraph draws fresh noise on every replay just because its `seeds` input changed.
//   key     = (seed mod 2^32, tag)         tag 0 = initial latents, 1 = churn noise
//   counter = (e4, step, 0, 0)             e4 = index of the 4-element group inside the sample's [n_latents*channels] elements
// One thread makes one Philox call = 4 uniform words = 4 normals = one 16-byte store:
//   u1 = ((x >> 8) + 1) * 2^-24  in (0, 1]   u2 = (y >> 8) * 2^-24  in [0, 1)      (both exact in fp32)
//   r = sqrtf(-2 logf(u1));  (x0, x1) -> elements 0, 1 = r cosf(2 pi u2), r sinf(2 pi u2);  (x2, x3) -> elements 2, 3 likewise
// with the accurate logf / sinf / cosf (the library is built without fast-math).
#include "common.h"
#include "kernels.h"
#include "philox.h"

namespace rald {

namespace {

__device__ __forceinline__ void box_muller(uint32_t x, uint32_t y, float& z0, float& z1) {
    const float u1 = (float)((x >> 8) + 1u) * 5.9604644775390625e-8f;      // 2^-24
    const float u2 = (float)(y >> 8) * 5.9604644775390625e-8f;
    const float r = sqrtf(-2.0f * logf(u1));
    const float a = 6.28318530717958647692f * u2;
    z0 = r * cosf(a);
    z1 = r * sinf(a);
}

__device__ __forceinline__ f32x4 philox_normal4(int64_t seed, uint32_t tag, uint32_t step, uint32_t e4) {
    uint32_t c[4] = {e4, step, 0u, 0u};
    philox4x32_10(c, (uint32_t)((uint64_t)seed & 0xffffffffu), tag);
    f32x4 z;
    float a, b;
    box_muller(c[0], c[1], a, b);
    z[0] = a; z[1] = b;
    box_muller(c[2], c[3], a, b);
    z[2] = a; z[3] = b;
    return z;
}

// grid (ceil(n4 / 256), B): thread = one 4-element group of one sample
__global__ __launch_bounds__(256) void philox_normal_kernel(const int64_t* __restrict__ seeds, uint32_t n4, uint32_t tag, uint32_t step,
                                                            f32x4* __restrict__ out) {
    const uint32_t e4 = blockIdx.x * 256u + threadIdx.x;
    if (e4 >= n4) return;
    const uint32_t b = blockIdx.y;
    out[(int64_t)b * n4 + e4] = philox_normal4(seeds[b], tag, step, e4);
}

// x_hat = x + scale * n in place, in the reference's operation order (the product is rounded before the sum, :260);
// n = noise[b][e4] (GEN = false) or Philox(seeds[b], tag 1, step, e4) (GEN = true)
template <bool GEN>
__global__ __launch_bounds__(256) void churn_kernel(f32x4* __restrict__ x, const f32x4* __restrict__ noise, const int64_t* __restrict__ seeds,
                                                    uint32_t n4, uint32_t step, float scale) {
#pragma clang fp contract(off)
    const uint32_t e4 = blockIdx.x * 256u + threadIdx.x;
    if (e4 >= n4) return;
    const uint32_t b = blockIdx.y;
    const int64_t i = (int64_t)b * n4 + e4;
    const f32x4 n = GEN ? philox_normal4(seeds[b], 1u, step, e4) : noise[i];
    const f32x4 v = x[i];
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float p = scale * n[j];
        o[j] = v[j] + p;
    }
    x[i] = o;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

int philox_normal(const int64_t* seeds, int B, int64_t n_per_sample, int tag, int step, float* out, hipStream_t st) {
    RALD_CHECK(seeds && out, "philox_normal: null pointer");
    RALD_CHECK(B >= 1 && B <= 65535, "philox_normal: batch must be in [1, 65535]");
    RALD_CHECK(n_per_sample >= 4 && n_per_sample % 4 == 0 && n_per_sample / 4 <= 0x7fffffffLL,
               "philox_normal: n_per_sample must be a positive multiple of 4 (one Philox call makes 4 normals) below 2^33");
    RALD_CHECK(tag >= 0 && step >= 0, "philox_normal: tag and step must be non-negative");
    RALD_CHECK(aligned16(out), "philox_normal: out must be 16-byte aligned");
    const uint32_t n4 = (uint32_t)(n_per_sample / 4);
    hipLaunchKernelGGL(philox_normal_kernel, dim3((n4 + 255u) / 256u, (unsigned)B), dim3(256), 0, st, seeds, n4, (uint32_t)tag, (uint32_t)step,
                       (f32x4*)out);
    RALD_HIP(hipGetLastError());
    return 0;
}

int churn_noise(float* x, const float* noise, const int64_t* seeds, int B, int64_t n_per_sample, int step, float scale, hipStream_t st) {
    RALD_CHECK(x && ((noise != nullptr) != (seeds != nullptr)), "churn_noise: exactly one of noise / seeds");
    RALD_CHECK(B >= 1 && B <= 65535 && n_per_sample >= 4 && n_per_sample % 4 == 0 && n_per_sample / 4 <= 0x7fffffffLL && step >= 0,
               "churn_noise: bad shape");
    RALD_CHECK(aligned16(x) && aligned16(noise), "churn_noise: x and noise must be 16-byte aligned");
    const uint32_t n4 = (uint32_t)(n_per_sample / 4);
    const dim3 grid((n4 + 255u) / 256u, (unsigned)B);
    if (seeds)
        hipLaunchKernelGGL(churn_kernel<true>, grid, dim3(256), 0, st, (f32x4*)x, (const f32x4*)nullptr, seeds, n4, (uint32_t)step, scale);
    else
        hipLaunchKernelGGL(churn_kernel<false>, grid, dim3(256), 0, st, (f32x4*)x, (const f32x4*)noise, seeds, n4, (uint32_t)step, scale);
    RALD_HIP(hipGetLastError());
    return 0;
}

// Karras schedule (edm_sampler :246-249) and the churned noise levels (:258-259) in the reference's operation order and roundings.
int edm_schedule(int num_steps, double smin, double smax, double rho, double S_churn, double S_min, double S_max, float* t, float* t_hat) {
#pragma clang fp contract(off)
    RALD_CHECK(t && t_hat, "edm_schedule: null pointer");
    RALD_CHECK(num_steps >= 2 && num_steps <= 2048, "dit: num_steps must be in [2,2048]");
    RALD_CHECK(S_churn >= 0.0 && rho > 0.0 && smin > 0.0 && smax >= smin, "edm_schedule: needs S_churn >= 0, rho > 0 and 0 < sigma_min <= sigma_max");
    // The reference evaluates sigma^(1/rho) and their difference as Python floats (doubles) and hands them to fp32 tensor arithmetic as
    // scalars (hence the double arguments); the tensor power agrees with the double-precision power rounded once (checked on the golden levels, bit for bit).  The
    // deterministic sampler's all-fp32 table (Dit::sample) is a few ulp away from this one and stays as it is: its results are pinned.
    const double ad = pow(smax, 1.0 / rho), bd = pow(smin, 1.0 / rho);
    const float a = (float)ad, d = (float)(bd - ad);
    for (int i = 0; i < num_steps; ++i) {
        const float s = (float)i / (float)(num_steps - 1) * d;
        const float base = a + s;
        t[i] = (float)pow((double)base, rho);
    }
    t[num_steps] = 0.f;
    const double g = S_churn / (double)num_steps;
    const double gmax = sqrt(2.0) - 1.0;
    const float gamma = (float)(g < gmax ? g : gmax);                                    // min(S_churn / num_steps, sqrt(2) - 1)
    const float lo = (float)S_min, hi = (float)S_max;                                    // compared as fp32 scalars, like the tensor comparison of :258
    for (int i = 0; i < num_steps; ++i) {
        const float gt = (lo <= t[i] && t[i] <= hi) ? gamma * t[i] : 0.f;
        t_hat[i] = t[i] + gt;
    }
    return 0;
}

}  // namespace rald
