// Shared device/host helpers for the gfx950 (MI355X, CDNA4) kernels.  wave = 64 lanes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>

namespace rald {

typedef __bf16 bf16;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;   // one MFMA A/B fragment (4 VGPRs)
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;     // 16x16 MFMA accumulator
typedef __attribute__((ext_vector_type(16))) float f32x16;   // 32x32 MFMA accumulator

typedef __attribute__((address_space(3))) void lds_void;          // the operand types of __builtin_amdgcn_global_load_lds (LDS-DMA)
typedef const __attribute__((address_space(1))) void glb_void;

constexpr int WAVE = 64;

// ---- error plumbing: C-ABI functions return int status + rald_last_error() ------------
void set_error(const std::string& msg);
#define RALD_CHECK(cond, msg)                                                       \
    do {                                                                            \
        if (!(cond)) {                                                              \
            ::rald::set_error(std::string(__FILE__) + ":" + std::to_string(__LINE__) + ": " + (msg)); \
            return 1;                                                               \
        }                                                                           \
    } while (0)
#define RALD_HIP(expr)                                                              \
    do {                                                                            \
        hipError_t _e = (expr);                                                     \
        if (_e != hipSuccess) {                                                     \
            ::rald::set_error(std::string(__FILE__) + ":" + std::to_string(__LINE__) + ": " #expr " -> " + hipGetErrorString(_e)); \
            return 2;                                                               \
        }                                                                           \
    } while (0)
#define RALD_TRY(expr)                                                              \
    do {                                                                            \
        int _rc = (expr);                                                           \
        if (_rc) return _rc;                                                        \
    } while (0)

#ifdef __HIPCC__
// Launch of a kernel that takes `smem` bytes of dynamic LDS: above the 64-KiB default the kernel's limit is raised first, once per kernel
// (`raised` is the caller's static flag for this kernel).
template <typename Args>
static int launch_dyn_lds(void (*kern)(Args), bool& raised, dim3 grid, int threads, int smem, hipStream_t st, const Args& a) {
    if (!raised && smem > 64 * 1024) {
        RALD_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, smem));
        raised = true;
    }
    hipLaunchKernelGGL(kern, grid, dim3(threads), smem, st, a);
    RALD_HIP(hipGetLastError());
    return 0;
}
#endif

// ---- device helpers --------------------------------------------------------------------
// Wave-wide reductions on DPP (data-parallel primitives: a VALU operand read through a fixed lane permutation) instead of __shfl_xor, which
// hipcc lowers to six dependent ds_bpermute_b32 - LDS-crossbar round trips of ~60-100 clocks each - per reduction: every LayerNorm-type kernel
// here is a chain of two or three such reductions per row.  Four row-local steps (quad swaps, half-mirror, mirror) leave each 16-lane row's result
// in all of its lanes, row_bcast15 / row_bcast31 carry it across the four rows into lane 63, and a readlane hands it to every lane.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_read(float keep, float v) {   // lanes of rows outside ROW_MASK (and lanes without a source) receive `keep`
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, keep), __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xf, false));
}
__device__ __forceinline__ float wave_sum(float v) {
    v += dpp_read<0xB1, 0xf>(0.f, v);       // quad_perm [1,0,3,2]
    v += dpp_read<0x4E, 0xf>(0.f, v);       // quad_perm [2,3,0,1]
    v += dpp_read<0x141, 0xf>(0.f, v);      // row_half_mirror
    v += dpp_read<0x140, 0xf>(0.f, v);      // row_mirror: every lane now holds its row's sum
    v += dpp_read<0x142, 0xa>(0.f, v);      // row_bcast15 into rows 1 and 3
    v += dpp_read<0x143, 0xc>(0.f, v);      // row_bcast31 into rows 2 and 3: lane 63 holds the wave's sum
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
__device__ __forceinline__ float wave_max(float v) {
    v = fmaxf(v, dpp_read<0xB1, 0xf>(v, v));
    v = fmaxf(v, dpp_read<0x4E, 0xf>(v, v));
    v = fmaxf(v, dpp_read<0x141, 0xf>(v, v));
    v = fmaxf(v, dpp_read<0x140, 0xf>(v, v));
    v = fmaxf(v, dpp_read<0x142, 0xa>(v, v));
    v = fmaxf(v, dpp_read<0x143, 0xc>(v, v));
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
// erf by Abramowitz-Stegun 7.1.26 (|abs error| <= 1.5e-7, branch-free: 1 rcp + 1 exp + 6 FMA) - libm's
// erff is a two-branch polynomial that diverges per lane and costs ~3x as many VALU slots in the
// GEGLU epilogue.  The result feeds a bf16 store (2^-9 relative), so 1.5e-7 is far below rounding.
__device__ __forceinline__ float erf_as(float x) {
    const float ax = fabsf(x);
    const float t = __frcp_rn(fmaf(0.3275911f, ax, 1.0f));
    float p = fmaf(1.061405429f, t, -1.453152027f);
    p = fmaf(p, t, 1.421413741f);
    p = fmaf(p, t, -0.284496736f);
    p = fmaf(p, t, 0.254829592f);
    const float r = 1.0f - p * t * __expf(-ax * ax);
    return copysignf(r, x);
}
__device__ __forceinline__ float gelu_erf(float x) {   // erf GELU (F.gelu default, approximate='none')
    return 0.5f * x * (1.0f + erf_as(x * 0.70710678118654752440f));
}
// GELU for the GEGLU epilogue, two values at a time on packed fp32 ops (v_pk_mul/fma_f32), no
// transcendental: erf(x/sqrt2) = xc * R(xc^2), xc = clamp(x, -3*sqrt2, 3*sqrt2), R = degree-8 minimax
// fit (tools: fitted in float64, verified in fp32 Horner).  |gelu error| <= 4.5e-5 absolute, <= 0.4
// bf16 ulp of the result wherever |gelu| > 0.01 - the epilogue rounds to bf16 right after.
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 gelu_poly2(f32x2 x) {
    constexpr float L = 4.242640687f;
    f32x2 xc;
    xc[0] = __builtin_amdgcn_fmed3f(x[0], -L, L);
    xc[1] = __builtin_amdgcn_fmed3f(x[1], -L, L);
    const f32x2 s = xc * xc;
    f32x2 r = f32x2{1.1252621139e-10f, 1.1252621139e-10f};
    r = r * s + f32x2{-1.0743099887e-08f, -1.0743099887e-08f};
    r = r * s + f32x2{4.5364107280e-07f, 4.5364107280e-07f};
    r = r * s + f32x2{-1.1292158697e-05f, -1.1292158697e-05f};
    r = r * s + f32x2{1.8717898050e-04f, 1.8717898050e-04f};
    r = r * s + f32x2{-2.2187900973e-03f, -2.2187900973e-03f};
    r = r * s + f32x2{1.9636213653e-02f, 1.9636213653e-02f};
    r = r * s + f32x2{-1.3269382422e-01f, -1.3269382422e-01f};
    r = r * s + f32x2{7.9780625133e-01f, 7.9780625133e-01f};
    const f32x2 e = xc * r;                  // erf(x/sqrt2)
    const f32x2 h = x * f32x2{0.5f, 0.5f};
    return h * e + h;
}
__device__ __forceinline__ float silu(float x) { return x / (1.0f + __expf(-x)); }

__device__ __forceinline__ bf16x4 pack4(float a, float b, float c, float d) {
    bf16x4 r;
    r[0] = (bf16)a; r[1] = (bf16)b; r[2] = (bf16)c; r[3] = (bf16)d;
    return r;
}

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }
static inline int64_t round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }

}  // namespace rald
