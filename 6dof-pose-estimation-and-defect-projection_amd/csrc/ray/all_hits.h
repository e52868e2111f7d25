// Ray stage, the all-hits queries (count_intersections, test_occlusions, list_intersections; DESIGN s4.24): what sits
// behind the pair test when "smallest key wins" is not the question.
//
// A ray intersects a triangle exactly when mt_accept(mt_eval(ray, record)) holds (ray/mt.h decides, nothing here does);
// its t is the quotient mt_key forms.  The SELECTORS are the casts': the grid of ray/grid.h (rast_tri_kernel /
// rast_item_kernel / rast_full_kernel, instantiated with one of the sinks below in the place of HitMin) and, for rays
// the grid cannot hold, the exhaustive ah_sweep_kernel.  A sink is what an accepted pair is handed to:
//
//   HitCount   atomicAdd(&counts[ray], 1)
//   HitInRange occluded[ray] = 1 when tnear <= t <= tfar (float32 compare, both ends inclusive, a NaN bound never holds)
//   HitFill    keys[splits[ray] + atomicAdd(&cursor[ray], 1)] = (bits(t) << 32) | triangle
//
// None of them is idempotent the way the casts' atomicMin is, so every accepted pair must reach the sink exactly once
// (DESIGN s4.24 "once only"), and a grid that gave up mid-way (hdr.ok == 0) leaves nothing behind: ah_close_kernel then
// clears every ray's word and ah_sweep_kernel, which runs only in that case (or without a grid at all), recounts.
// Only integer atomics; the list's keys are unique within a ray, so sorting a ray's segment by key makes the result
// independent of the order of arrival.
#pragma once
#include "mt.h"
#include "grid.h"

namespace {

struct HitCount {
    int *__restrict__ counts;
    typedef int Acc;
    __device__ __forceinline__ Acc start() const { return 0; }
    __device__ __forceinline__ void one(unsigned ray, const MT &, unsigned) const { atomicAdd(&counts[ray], 1); }
    __device__ __forceinline__ void gather(Acc &a, int64_t, const MT &, unsigned) const { a += 1; }
    __device__ __forceinline__ void finish(Acc a, int64_t ray) const { if (a) atomicAdd(&counts[ray], a); }
    __device__ __forceinline__ void clear(int64_t ray) const { counts[ray] = 0; }
};

struct HitInRange {
    uint8_t *__restrict__ occluded;
    float tnear, tfar;
    typedef int Acc;
    __device__ __forceinline__ bool in_range(const MT &m) const {
        const float t = __uint_as_float((unsigned)(mt_key(m, 0u) >> 32));
        return (tnear <= t) & (t <= tfar);
    }
    __device__ __forceinline__ Acc start() const { return 0; }
    __device__ __forceinline__ void one(unsigned ray, const MT &m, unsigned) const { if (in_range(m)) occluded[ray] = 1; }
    __device__ __forceinline__ void gather(Acc &a, int64_t, const MT &m, unsigned) const { a |= (int)in_range(m); }
    __device__ __forceinline__ void finish(Acc a, int64_t ray) const { if (a) occluded[ray] = 1; }
    __device__ __forceinline__ void clear(int64_t ray) const { occluded[ray] = 0; }
};

struct HitFill {
    const long long *__restrict__ splits;   // N + 1: where a ray's segment starts (the count pass's exclusive scan)
    int *__restrict__ cursor;               // N, zero before the pass
    unsigned long long *__restrict__ keys;  // splits[N] entries
    typedef int Acc;
    __device__ __forceinline__ Acc start() const { return 0; }
    __device__ __forceinline__ void one(unsigned ray, const MT &m, unsigned f) const {
        const long long at = splits[ray], room = splits[ray + 1] - at;
        const int k = atomicAdd(&cursor[ray], 1);
        // (the count pass met the same pairs, so k < room always: the test only keeps a write inside the buffer)
        if (k < room) keys[at + k] = mt_key(m, f);
    }
    __device__ __forceinline__ void gather(Acc &, int64_t ray, const MT &m, unsigned f) const { one((unsigned)ray, m, f); }
    __device__ __forceinline__ void finish(Acc, int64_t) const {}
    __device__ __forceinline__ void clear(int64_t ray) const { cursor[ray] = 0; }
};

// Behind the three grid kernels of a query: how the grid went, into the query's own status words; the OTHER header back
// to its start values with this one's frame and grid (what ray_finalize_kernel does for a cast; the frame goes along so
// that a list's fill pass can walk the grid its count pass built); and, where the grid gave up, every ray's word cleared
// for the sweep below.
template <class Sink>
__global__ __launch_bounds__(256) void ah_close_kernel(int64_t N, const RastHdr *__restrict__ rast, RastHdr *__restrict__ rast_next,
                                                      int *__restrict__ status, unsigned long long owner, Sink sink) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int ok = rast->ok;
    if (i == 0) {
        status[1] = (int)(N & 0x7FFFFFFF);
        status[2] = (int)(owner & 0xFFFFFFFFull);   // whose rays: a ray set's id, 0 for a call's own
        status[3] = (int)(owner >> 32);
        status[0] = ok ? 0 : rast->reason;
        __threadfence_system();
        RastHdr n = *rast;
        n.ok = 1; n.n_items = 0; n.reason = 0; n.n_full = 0;
        *rast_next = n;
    }
    if (i < N && ok == 0) sink.clear(i);
}

// Every ray against every record of one triangle chunk: blockIdx.x picks 256 rays, blockIdx.y the chunk, the records
// come through scalar loads (the index is uniform).  rast != nullptr: the completion of a grid pass, which leaves at
// once unless the grid gave up.
template <class Sink>
__global__ __launch_bounds__(256) void ah_sweep_kernel(const float *__restrict__ aos, int64_t F, int64_t tris_per_chunk,
                                                      const float *__restrict__ rays6, int64_t N, const RastHdr *__restrict__ rast,
                                                      Sink sink) {
    if (rast && rast->ok != 0) return;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int64_t f0 = (int64_t)blockIdx.y * tris_per_chunk;
    const int64_t f1 = f0 + tris_per_chunk < F ? f0 + tris_per_chunk : F;
    Ray r;
    r.ox = rays6[6 * i]; r.oy = rays6[6 * i + 1]; r.oz = rays6[6 * i + 2];
    r.dx = rays6[6 * i + 3]; r.dy = rays6[6 * i + 4]; r.dz = rays6[6 * i + 5];
    typename Sink::Acc acc = sink.start();
    for (int64_t f = f0; f < f1; ++f) {
        const MT m = mt_eval(r, aos + (size_t)f * PEDP_TRI_STRIDE);
        if (mt_accept(m)) sink.gather(acc, i, m, (unsigned)f);
    }
    sink.finish(acc, i);
}

// The list's outputs from the sorted keys: entry j belongs to the last ray whose segment starts at or before j
// (empty segments share their start with the next one); (u, v) are re-evaluated the way ray_finalize_kernel does.
__global__ __launch_bounds__(256) void ah_emit_kernel(const float *__restrict__ aos, int64_t F, const float *__restrict__ rays6, int64_t N,
                                                     const long long *__restrict__ splits, const unsigned long long *__restrict__ keys,
                                                     int64_t M, long long *__restrict__ ray_ids, float *__restrict__ t_hit,
                                                     uint32_t *__restrict__ prim_id, float *__restrict__ uv) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= M) return;
    int64_t lo = 0, hi = N;   // splits[lo] <= j < splits[hi]
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (splits[mid] <= j) lo = mid; else hi = mid;
    }
    const unsigned long long key = keys[j];
    const unsigned id = (unsigned)(key & 0xFFFFFFFFull);
    ray_ids[j] = lo;
    t_hit[j] = __uint_as_float((unsigned)(key >> 32));
    prim_id[j] = id;
    Ray r;
    r.ox = rays6[6 * lo + 0]; r.oy = rays6[6 * lo + 1]; r.oz = rays6[6 * lo + 2];
    r.dx = rays6[6 * lo + 3]; r.dy = rays6[6 * lo + 4]; r.dz = rays6[6 * lo + 5];
    // (id < F always, the fill pass wrote every key: the test only keeps the read inside the records)
    const MT m = mt_eval(r, aos + (size_t)(id < F ? id : 0u) * PEDP_TRI_STRIDE);
    const unsigned sg = __float_as_uint(m.det) & 0x80000000u;
    const float U = __uint_as_float(__float_as_uint(m.un) ^ sg);
    const float V = __uint_as_float(__float_as_uint(m.vn) ^ sg);
    const float ad = fabsf(m.det);
    uv[2 * j] = __fdiv_rn(U, ad);
    uv[2 * j + 1] = __fdiv_rn(V, ad);
}

}  // namespace
