// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC11), written out in integer code: the
// counter-based generator of the surface sampler (pedp_sample.hip).  A block is a pure function of its
// 128-bit counter and 64-bit key, so sample k of a seed is the same whoever draws it and in whatever order.
//   known answers: counter 0 0 0 0, key 0 0 -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8
//                  all ones                 -> 408f276d 41c83b0e a20bc7c6 6d5451fd
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace philox {

constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;  // the round's two multipliers
constexpr uint32_t W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;  // the key's Weyl increments

// out = philox4x32-10(counter c[4], key (k0, k1))
__host__ __device__ inline void block(const uint32_t c[4], uint32_t k0, uint32_t k1, uint32_t out[4]) {
    uint32_t x0 = c[0], x1 = c[1], x2 = c[2], x3 = c[3];
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)M0 * x0, p1 = (uint64_t)M1 * x2;
        const uint32_t y0 = (uint32_t)(p1 >> 32) ^ x1 ^ k0, y1 = (uint32_t)p1;
        const uint32_t y2 = (uint32_t)(p0 >> 32) ^ x3 ^ k1, y3 = (uint32_t)p0;
        x0 = y0; x1 = y1; x2 = y2; x3 = y3;
        k0 += W0; k1 += W1;
    }
    out[0] = x0; out[1] = x1; out[2] = x2; out[3] = x3;
}

// block `which` (0: x, 1: y, 2: the thinning key of a given cloud) of sample or point k under a 64-bit seed
__host__ __device__ inline void draw(uint64_t k, uint32_t which, uint64_t seed, uint32_t out[4]) {
    const uint32_t c[4] = {(uint32_t)k, (uint32_t)(k >> 32), which, 0u};
    block(c, (uint32_t)seed, (uint32_t)(seed >> 32), out);
}

}  // namespace philox
