// The topology of an indexed triangle mesh, shared by the defect map (pedp_defectmap.hip) and the solid
// (pedp_solid.hip): the weld of its vertices and its edge slots sorted by their welded end points.  The refinement
// (pedp_refine.hip) takes the weld and the slots' numbering from here and keys only the slots of its long edges.
//   weld        w[v] = the lowest index of a vertex at v's position; positions compare with ==, so -0 equals +0, and a
//               vertex with a NaN is welded to nothing (w[v] = v)
//   edge slots  slot e = 3 f + k joins corners k and (k + 1) % 3 of face f; its key is (min w, max w), or all ones where
//               the two corners weld to one vertex (no edge).  The slots are sorted by key with the context's pooled
//               sort, which is stable: the slots of one edge form a run in slot order, the slots that are no edge come last
// Everything here has internal linkage: each including file gets its own copy of the kernels.
#pragma once
#include "../pedp_internal.h"

namespace {
namespace topology {

constexpr int TT = 256;  // threads per block
constexpr uint32_t NO_VERTEX = 0xFFFFFFFFu;
constexpr unsigned long long NO_EDGE = ~0ull;

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + TT - 1) / TT); }
__host__ __device__ inline uint64_t bits_of(double x) { uint64_t b; memcpy(&b, &x, 8); return b; }

// The weld: a hash table of vertex indices, open addressing.  A slot holds the lowest index seen so far of one
// position; positions compare with ==, so -0 equals +0 (and hashes like it); a vertex with a NaN stays out.
__device__ __forceinline__ bool vertex_has_nan(const double *v, size_t i) { return !(v[3 * i] == v[3 * i] && v[3 * i + 1] == v[3 * i + 1] && v[3 * i + 2] == v[3 * i + 2]); }
__device__ __forceinline__ bool vertex_equal(const double *v, size_t i, size_t j) {
    return v[3 * i] == v[3 * j] && v[3 * i + 1] == v[3 * j + 1] && v[3 * i + 2] == v[3 * j + 2];
}
__device__ __forceinline__ uint64_t vertex_hash(const double *v, size_t i) {
    uint64_t h = 0x9E3779B97F4A7C15ull;
    for (int d = 0; d < 3; ++d) {
        const double x = v[3 * i + d];
        uint64_t b = x == 0.0 ? 0ull : bits_of(x);
        b *= 0xFF51AFD7ED558CCDull; b ^= b >> 33;
        h = (h ^ b) * 0xC4CEB9FE1A85EC53ull; h ^= h >> 29;
    }
    return h;
}
__global__ __launch_bounds__(TT) void weld_insert_kernel(const double *__restrict__ v, int64_t V, uint32_t *__restrict__ slot, uint64_t mask) {
    const int64_t i = (int64_t)blockIdx.x * TT + threadIdx.x;
    if (i >= V || vertex_has_nan(v, (size_t)i)) return;
    uint64_t h = vertex_hash(v, (size_t)i) & mask;
    while (true) {  // the table has at least 2 V slots: an empty one is always met
        const uint32_t u = atomicCAS(&slot[h], NO_VERTEX, (uint32_t)i);
        if (u == NO_VERTEX) return;
        if (vertex_equal(v, u, (size_t)i)) { atomicMin(&slot[h], (uint32_t)i); return; }  // whoever holds the slot has this position
        h = (h + 1) & mask;
    }
}
__global__ __launch_bounds__(TT) void weld_lookup_kernel(const double *__restrict__ v, int64_t V, const uint32_t *__restrict__ slot, uint64_t mask,
                                                        uint32_t *__restrict__ w) {
    const int64_t i = (int64_t)blockIdx.x * TT + threadIdx.x;
    if (i >= V) return;
    uint32_t r = (uint32_t)i;
    if (!vertex_has_nan(v, (size_t)i)) {
        uint64_t h = vertex_hash(v, (size_t)i) & mask;
        while (true) {
            const uint32_t u = slot[h];
            if (u == NO_VERTEX) break;  // cannot happen: the vertex was inserted
            if (vertex_equal(v, u, (size_t)i)) { r = u; break; }
            h = (h + 1) & mask;
        }
    }
    w[i] = r;
}

// edge slot e = 3 f + k joins corners k and (k + 1) % 3 of face f: key (min w, max w), or all ones where the two weld
// to one vertex (such a slot names no edge; the sort puts these last)
__global__ __launch_bounds__(TT) void edge_key_kernel(const uint32_t *__restrict__ tri, const uint32_t *__restrict__ w, int64_t E,
                                                     unsigned long long *__restrict__ key, unsigned long long *__restrict__ key_copy) {
    const int64_t e = (int64_t)blockIdx.x * TT + threadIdx.x;
    if (e >= E) return;
    const int64_t f = e / 3;
    const int k = (int)(e - 3 * f);
    const uint32_t a = w[tri[3 * f + k]], b = w[tri[3 * f + (k + 1) % 3]];
    const unsigned long long q = a == b ? NO_EDGE : ((unsigned long long)(a < b ? a : b) << 32) | (a < b ? b : a);
    key[e] = q;
    key_copy[e] = q;
}

// the table of the weld: a power of two of at least 2 V slots (and 64)
inline uint64_t weld_slots(int64_t V) {
    uint64_t slots = 64;
    while (slots < 2 * (uint64_t)V) slots <<= 1;
    return slots;
}

// d_w[v] for the V vertices d_v; d_slot: weld_slots(V) x uint32 of scratch.  Enqueued on the context's stream.
inline int weld(pedp_ctx_t c, const double *d_v, int64_t V, uint32_t *d_slot, uint32_t *d_w) {
    const uint64_t slots = weld_slots(V);
    PEDP_HIP_CHECK(hipMemsetAsync(d_slot, 0xFF, 4 * slots, c->stream));
    if (V == 0) return PEDP_OK;
    hipLaunchKernelGGL(weld_insert_kernel, dim3(blocks_for(V)), dim3(TT), 0, c->stream, d_v, V, d_slot, slots - 1);
    hipLaunchKernelGGL(weld_lookup_kernel, dim3(blocks_for(V)), dim3(TT), 0, c->stream, d_v, V, d_slot, slots - 1, d_w);
    PEDP_HIP_CHECK(hipGetLastError());
    return PEDP_OK;
}

// The E = 3 F edge slots sorted by key: perm[p] is the slot at sorted position p, key_copy[e] the key of slot e (the
// sort consumes its own copy).  Enqueued on the context's stream, in its pooled sort buffers.
inline int sort_edges(pedp_ctx_t c, const uint32_t *d_tri, const uint32_t *d_w, int64_t E, unsigned long long *key_copy, int32_t *perm) {
    unsigned long long *keys = nullptr;
    int rc = pedp_sort_keys64_exact_begin(c, E, 64, &keys);
    if (rc) return rc;
    hipLaunchKernelGGL(edge_key_kernel, dim3(blocks_for(E)), dim3(TT), 0, c->stream, d_tri, d_w, E, keys, key_copy);
    return pedp_sort_keys64_exact_run(c, E, 64, perm);
}

}  // namespace topology
}  // namespace
