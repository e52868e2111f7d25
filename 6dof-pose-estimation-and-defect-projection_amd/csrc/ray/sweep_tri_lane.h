// Ray stage, variant 2 (the auto choice below 16,384 rays), triangle per lane: few rays against a big mesh.  Lanes
// own consecutive triangles (coalesced 16-B loads of the AoS records), 4 wave-uniform rays per wave, and the packed
// key is min-reduced across the 64 lanes: the wavefront-wide min-t reduction.
#pragma once
#include "mt.h"

namespace {

// ------------------------------------------------------------------ sweep, triangle per lane
constexpr int TPL_BLOCK = 256;
constexpr int TPL_RAYS = 4;

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        unsigned lo = __shfl_xor((unsigned)(v & 0xFFFFFFFFull), off, 64);
        unsigned hi = __shfl_xor((unsigned)(v >> 32), off, 64);
        unsigned long long o = ((unsigned long long)hi << 32) | lo;
        v = o < v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(TPL_BLOCK) void ray_sweep_tpl_kernel(
    const float4 *__restrict__ tri, int64_t F_padded, int tris_per_chunk, int n_chunks,
    const float *__restrict__ rays6, int64_t N, unsigned long long *__restrict__ keys) {
    const int b = blockIdx.x;
    const int chunk = b % n_chunks;
    const int64_t rb = b / n_chunks;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t ray0 = (rb * (TPL_BLOCK / 64) + wave) * TPL_RAYS;
    if (ray0 >= N) return;  // wave-uniform
    Ray r[TPL_RAYS];
#pragma unroll
    for (int k = 0; k < TPL_RAYS; ++k) {
        int64_t rl = ray0 + k < N ? ray0 + k : N - 1;  // wave-uniform address: stays in SGPRs
        r[k].ox = rays6[6 * rl + 0]; r[k].oy = rays6[6 * rl + 1]; r[k].oz = rays6[6 * rl + 2];
        r[k].dx = rays6[6 * rl + 3]; r[k].dy = rays6[6 * rl + 4]; r[k].dz = rays6[6 * rl + 5];
    }
    unsigned long long best[TPL_RAYS];
#pragma unroll
    for (int k = 0; k < TPL_RAYS; ++k) best[k] = KEY_MISS;
    int64_t f0 = (int64_t)chunk * tris_per_chunk;
    int64_t f1 = f0 + tris_per_chunk;
    if (f1 > F_padded) f1 = F_padded;
    for (int64_t f = f0 + lane; f < f1; f += 64) {
        const float4 a = tri[3 * f + 0], bq = tri[3 * f + 1], c = tri[3 * f + 2];
        const float rec[12] = {a.x, a.y, a.z, a.w, bq.x, bq.y, bq.z, bq.w, c.x, c.y, c.z, c.w};
#pragma unroll
        for (int k = 0; k < TPL_RAYS; ++k) {
            MT m = mt_eval(r[k], rec);
            if (mt_accept(m)) {
                unsigned long long key = mt_key(m, (unsigned)f);
                best[k] = key < best[k] ? key : best[k];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < TPL_RAYS; ++k) {
        unsigned long long v = wave_min_u64(best[k]);  // the wavefront-wide min-t reduction
        if (lane == 0 && ray0 + k < N && v != KEY_MISS) atomicMin(&keys[ray0 + k], v);
    }
}

}  // namespace
