// Philox4x32-10 (Salmon et al., SC'11), the counter-based generator of rng.hip (the sampler's noise, key tags 0 and 1) and of
// cloud_plane.hip (the hypotheses' rows, key tag 2): ten rounds on a 4-word counter under a 2-word key, no state.
#pragma once
#include "common.h"

namespace rald {

__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[0] = n0; c[1] = (uint32_t)p1; c[2] = n2; c[3] = (uint32_t)p0;
}

__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(c, k0, k1);
        k0 += 0x9E3779B9u;                  // Weyl sequence of the key
        k1 += 0xBB67AE85u;
    }
}

}  // namespace rald
