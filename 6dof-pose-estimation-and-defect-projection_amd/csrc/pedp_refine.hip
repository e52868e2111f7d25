// Mesh refinement: every edge of an indexed triangle mesh longer than max_edge is bisected, round after
// round, until none is left; every refined face carries the face of the input it came from.  This gives a coarse CAD
// model (a flat side is two triangles) the resolution that the per-face maps need to say anything local.
//   * conforming: an edge is long or not by a test that is bit-symmetric in its end points, one midpoint per welded edge
//     (mesh/topology.h's weld and its sorted edge slots), so both faces at an edge always agree and name the same vertex
//   * deterministic: new vertices are numbered in ascending key order of the stable pooled sort, children are laid out by
//     an exclusive scan over the faces; the only atomics are the weld's and the validation's integer minima, whose
//     results do not depend on the order of arrival
// float64, no contraction, every expression in the order of the contract (include/pedp.h).
#include "mesh/topology.h"
#include <cmath>
#include <rocprim/device/device_scan.hpp>

#pragma clang fp contract(off)

struct pedp_refined_s {
    pedp_ctx_t ctx = nullptr;
    int device = 0;
    int64_t V0 = 0, F0 = 0;   // the input's sizes
    int64_t V = 0, F = 0;     // the result's
    int32_t rounds = 0;
    double *v = nullptr;      // V x 3
    uint32_t *t = nullptr;    // F x 3
    int32_t *pf = nullptr;    // F: parent_face
    int32_t *start = nullptr; // F0 + 1: the first child of every input face; start[F0] = F
    pedp_scratch io;          // staging of host-memory reads and reductions
};

namespace {

using topology::NO_EDGE;
using topology::TT;
using topology::blocks_for;

constexpr int64_t MAX_FACES = 1 << 28;            // 3 F edge slots are sorted with int32 positions
constexpr int64_t MAX_VERTS = 0xFFFFFFFEll;       // 2^32 - 2
constexpr int MAX_ROUNDS = 64;
constexpr uint32_t NONE = 0xFFFFFFFFu;

inline size_t a256(size_t b) { return (b + 255) & ~(size_t)255; }

#define PEDP_ROCPRIM(expr)                                                                     \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) {                                                                \
            pedp_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(e_)); \
            return PEDP_ERR_HIP;                                                               \
        }                                                                                      \
    } while (0)

// ------------------------------------------------------------------ validation
// first[0]: the lowest corner slot 3 f + k that names a vertex >= V; first[1]: the lowest vertex with a non-finite
// coordinate.  Integer minima: the same answer whatever the order of arrival.
__global__ __launch_bounds__(TT) void check_tris_kernel(const uint32_t *__restrict__ tri, int64_t E, int64_t V, uint32_t *__restrict__ first) {
    const int64_t e = (int64_t)blockIdx.x * TT + threadIdx.x;
    if (e < E && (int64_t)tri[e] >= V) atomicMin(&first[0], (uint32_t)e);
}
__global__ __launch_bounds__(TT) void check_verts_kernel(const double *__restrict__ v, int64_t V, uint32_t *__restrict__ first) {
    const int64_t i = (int64_t)blockIdx.x * TT + threadIdx.x;
    if (i < V && !pedp_row_finite(v, i)) atomicMin(&first[1], (uint32_t)i);
}
__global__ __launch_bounds__(TT) void iota_parent_kernel(int64_t F, int32_t *__restrict__ pf) {
    const int64_t f = (int64_t)blockIdx.x * TT + threadIdx.x;
    if (f < F) pf[f] = (int32_t)f;
}

// ------------------------------------------------------------------ one round
// the squared length of (a, b), d = b - a: bit-symmetric in a and b (b - a = -(a - b) exactly, and x * x = (-x) * (-x))
__device__ __forceinline__ double edge_len2(const double *a, const double *b) {
    const double dx = b[0] - a[0], dy = b[1] - a[1], dz = b[2] - a[2];
    return (dx * dx + dy * dy) + dz * dz;
}
__device__ __forceinline__ void load_vertex(const double *__restrict__ v, uint32_t i, double *p) {
    p[0] = v[3 * (size_t)i]; p[1] = v[3 * (size_t)i + 1]; p[2] = v[3 * (size_t)i + 2];
}

// Step 1, a lane per face: which of its edges k = (c_k, c_(k+1)%3) are long, its number of children, and its three edge
// slots' keys (min w, max w) -- NO_EDGE for an edge that is not long.  Vertices made by earlier rounds (index >= V0)
// are unique and weld to themselves.
__global__ __launch_bounds__(TT) void flag_kernel(const double *__restrict__ v, const uint32_t *__restrict__ tri, const uint32_t *__restrict__ w,
                                                 int64_t V0, int64_t F, double limit2, unsigned long long *__restrict__ key,
                                                 unsigned long long *__restrict__ key_copy, uint32_t *__restrict__ count /* F + 1 */) {
    const int64_t f = (int64_t)blockIdx.x * TT + threadIdx.x;
    if (f > F) return;
    if (f == F) { count[F] = 0; return; }
    uint32_t c[3], cw[3];
    double p[3][3];
    for (int k = 0; k < 3; ++k) {
        c[k] = tri[3 * f + k];
        cw[k] = (int64_t)c[k] < V0 ? w[c[k]] : c[k];
        load_vertex(v, c[k], p[k]);
    }
    uint32_t n = 1;
    for (int k = 0; k < 3; ++k) {
        const int k1 = (k + 1) % 3;
        const bool is_long = edge_len2(p[k], p[k1]) > limit2;
        const uint32_t a = cw[k], b = cw[k1];
        const unsigned long long q = is_long ? ((unsigned long long)(a < b ? a : b) << 32) | (a < b ? b : a) : NO_EDGE;
        key[3 * f + k] = q;
        key_copy[3 * f + k] = q;
        n += is_long;
    }
    count[f] = n;
}

// Step 3a, a lane per sorted position: 1 where it opens a run of equal keys that names an edge
__global__ __launch_bounds__(TT) void run_head_kernel(const unsigned long long *__restrict__ key, const int32_t *__restrict__ perm, int64_t E,
                                                     uint32_t *__restrict__ head /* E + 1 */) {
    const int64_t p = (int64_t)blockIdx.x * TT + threadIdx.x;
    if (p > E) return;
    if (p == E) { head[E] = 0; return; }
    const unsigned long long q = key[perm[p]];
    head[p] = q != NO_EDGE && (p == 0 || q != key[perm[p - 1]]);
}
// Step 3b, after the scan: run r (in ascending key order) is vertex V + r.  Every slot of the run learns the id; the
// run's first slot writes the midpoint 0.5 * (a + b) per component from its own face's corners (bit-symmetric, and the
// other slots' corners hold the same positions: they weld to the same two vertices).
__global__ __launch_bounds__(TT) void midpoint_kernel(const unsigned long long *__restrict__ key, const int32_t *__restrict__ perm,
                                                     const uint32_t *__restrict__ head, const uint32_t *__restrict__ rank, int64_t E, int64_t V,
                                                     const uint32_t *__restrict__ tri, double *__restrict__ v, uint32_t *__restrict__ slot_mid) {
    const int64_t p = (int64_t)blockIdx.x * TT + threadIdx.x;
    if (p >= E) return;
    const int32_t e = perm[p];
    if (key[e] == NO_EDGE) { slot_mid[e] = NONE; return; }
    const uint32_t h = head[p];
    const uint32_t id = (uint32_t)(V + (int64_t)rank[p] + (int64_t)h - 1);  // rank is exclusive: behind the head it counts the head
    slot_mid[e] = id;
    if (!h) return;
    const int64_t f = e / 3;
    const int k = (int)(e - 3 * f);
    double a[3], b[3];
    load_vertex(v, tri[3 * f + k], a);
    load_vertex(v, tri[3 * f + (k + 1) % 3], b);
    for (int d = 0; d < 3; ++d) v[3 * (size_t)id + d] = 0.5 * (a[d] + b[d]);
}

// Step 4, a lane per face: its children, in place in the face order (off: the exclusive scan of the child counts), with
// the parent's winding and the parent's parent_face.
__device__ __forceinline__ void put(uint32_t *__restrict__ out, int32_t *__restrict__ pf_out, size_t o, uint32_t a, uint32_t b, uint32_t c, int32_t pf) {
    out[3 * o] = a; out[3 * o + 1] = b; out[3 * o + 2] = c;
    pf_out[o] = pf;
}
__global__ __launch_bounds__(TT) void emit_kernel(const double *__restrict__ v, const uint32_t *__restrict__ tri, const int32_t *__restrict__ pf,
                                                 const uint32_t *__restrict__ slot_mid, const uint32_t *__restrict__ off, int64_t F,
                                                 uint32_t *__restrict__ out, int32_t *__restrict__ pf_out) {
    const int64_t f = (int64_t)blockIdx.x * TT + threadIdx.x;
    if (f >= F) return;
    uint32_t c[3], m[3];
    int n_long = 0, first_long = -1, short_edge = -1;
    for (int k = 0; k < 3; ++k) {
        c[k] = tri[3 * f + k];
        m[k] = slot_mid[3 * f + k];
        if (m[k] != NONE) { ++n_long; if (first_long < 0) first_long = k; }
        else short_edge = k;
    }
    const size_t o = off[f];
    const int32_t parent = pf[f];
    if (n_long == 0) {
        put(out, pf_out, o, c[0], c[1], c[2], parent);
    } else if (n_long == 1) {  // rotated so that the long edge is edge 0
        const int r = first_long;
        const uint32_t c0 = c[r], c1 = c[(r + 1) % 3], c2 = c[(r + 2) % 3], mid = m[r];
        put(out, pf_out, o, c0, mid, c2, parent);
        put(out, pf_out, o + 1, mid, c1, c2, parent);
    } else if (n_long == 2) {  // rotated so that the short edge is edge 2
        const int r = (short_edge + 1) % 3;
        const uint32_t c0 = c[r], c1 = c[(r + 1) % 3], c2 = c[(r + 2) % 3], m0 = m[r], m1 = m[(r + 1) % 3];
        double pm0[3], pm1[3], p0[3], p2[3];
        load_vertex(v, m0, pm0); load_vertex(v, m1, pm1); load_vertex(v, c0, p0); load_vertex(v, c2, p2);
        put(out, pf_out, o, m0, c1, m1, parent);
        if (edge_len2(pm0, p2) <= edge_len2(pm1, p0)) {  // the shorter diagonal of the quadrilateral (c0, m0, m1, c2); a tie: m0 - c2
            put(out, pf_out, o + 1, c0, m0, c2, parent);
            put(out, pf_out, o + 2, m0, m1, c2, parent);
        } else {
            put(out, pf_out, o + 1, c0, m0, m1, parent);
            put(out, pf_out, o + 2, c0, m1, c2, parent);
        }
    } else {
        put(out, pf_out, o, c[0], m[0], m[2], parent);
        put(out, pf_out, o + 1, m[0], c[1], m[1], parent);
        put(out, pf_out, o + 2, m[2], m[1], c[2], parent);
        put(out, pf_out, o + 3, m[0], m[1], m[2], parent);
    }
}

// ------------------------------------------------------------------ per input face
// parent_face is non-decreasing and every input face has a child: the first child of every input face
__global__ __launch_bounds__(TT) void run_start_kernel(const int32_t *__restrict__ pf, int64_t F, int64_t F0, int32_t *__restrict__ start /* F0 + 1 */) {
    const int64_t i = (int64_t)blockIdx.x * TT + threadIdx.x;
    if (i > F) return;
    if (i == F) { start[F0] = (int32_t)F; return; }
    if (i == 0 || pf[i] != pf[i - 1]) start[pf[i]] = (int32_t)i;
}
// a lane per input face folds its children's values in ascending child index, starting from the first child's value
__global__ __launch_bounds__(TT) void reduce_kernel(const int32_t *__restrict__ start, int64_t F0, int op, const double *__restrict__ x,
                                                   double *__restrict__ out) {
    const int64_t f = (int64_t)blockIdx.x * TT + threadIdx.x;
    if (f >= F0) return;
    const int32_t i0 = start[f], i1 = start[f + 1];
    double acc = x[i0];
    for (int32_t i = i0 + 1; i < i1; ++i) {
        const double y = x[i];
        if (op == PEDP_REDUCE_SUM) acc = acc + y;
        else if (op == PEDP_REDUCE_MAX) { if (y > acc || y != y) acc = y; }
        else { if (y < acc || y != y) acc = y; }
    }
    out[f] = acc;
}

// ------------------------------------------------------------------ host side
int dev_alloc(void **p, size_t bytes, const char *who) {
    const hipError_t e = hipMalloc(p, bytes ? bytes : 256);
    if (e != hipSuccess) {
        *p = nullptr;
        pedp_set_error("%s: hipMalloc(%zu) -> %s", who, bytes, hipGetErrorString(e));
        return PEDP_ERR_HIP;
    }
    return PEDP_OK;
}
int copy_in(pedp_ctx_t c, void *dst, const void *src, size_t bytes, int mem) {
    if (bytes == 0) return PEDP_OK;
    if (mem == PEDP_HOST) return pedp_upload(c, dst, src, bytes);
    PEDP_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream));
    return PEDP_OK;
}
int copy_out(pedp_ctx_t c, void *dst, const void *src, size_t bytes, int mem) {
    if (bytes == 0 || !dst) return PEDP_OK;
    if (mem == PEDP_HOST) return pedp_download(c, dst, src, bytes);
    PEDP_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream));
    return PEDP_OK;
}

// what the rounds need besides the handle's arrays; freed when the call returns
struct Work {
    uint32_t *w = nullptr;        // V0: the weld
    uint32_t *t_next = nullptr;   // the round's output, until it is swapped in
    int32_t *pf_next = nullptr;
    double *v_next = nullptr;
    pedp_scratch ws;
    ~Work() {
        if (w) (void)hipFree(w);
        if (t_next) (void)hipFree(t_next);
        if (pf_next) (void)hipFree(pf_next);
        if (v_next) (void)hipFree(v_next);
        ws.release();
    }
};

int refine_rounds(pedp_refined_s *r, Work &k, double max_edge, int64_t face_cap, int64_t *faces_reached, const char *who) {
    pedp_ctx_t c = r->ctx;
    hipStream_t s = c->stream;
    const double limit2 = max_edge * max_edge;
    while (true) {
        const int64_t F = r->F, E = 3 * F, V = r->V;
        size_t tmp_bytes = 0, tmp_faces = 0;  // the two scans share one scratch
        PEDP_ROCPRIM(rocprim::exclusive_scan(nullptr, tmp_bytes, (uint32_t *)nullptr, (uint32_t *)nullptr, 0u, (size_t)E + 1,
                                             rocprim::plus<uint32_t>(), s));
        PEDP_ROCPRIM(rocprim::exclusive_scan(nullptr, tmp_faces, (uint32_t *)nullptr, (uint32_t *)nullptr, 0u, (size_t)F + 1,
                                             rocprim::plus<uint32_t>(), s));
        tmp_bytes = tmp_bytes > tmp_faces ? tmp_bytes : tmp_faces;
        PEDP_TRY(k.ws.reserve(a256(8 * (size_t)E) + 4 * a256(4 * ((size_t)E + 1)) + 2 * a256(4 * ((size_t)F + 1)) + a256(tmp_bytes) + 1024));
        char *base = (char *)k.ws.ptr;
        size_t o = 0;
        auto take = [&](size_t bytes) { char *p = base + o; o += a256(bytes); return p; };
        unsigned long long *key_copy = (unsigned long long *)take(8 * (size_t)E);
        int32_t *perm = (int32_t *)take(4 * ((size_t)E + 1));
        uint32_t *head = (uint32_t *)take(4 * ((size_t)E + 1)), *rank = (uint32_t *)take(4 * ((size_t)E + 1));
        uint32_t *slot_mid = (uint32_t *)take(4 * ((size_t)E + 1));
        uint32_t *count = (uint32_t *)take(4 * ((size_t)F + 1)), *off = (uint32_t *)take(4 * ((size_t)F + 1));
        void *tmp = take(tmp_bytes);
        // 1  flags, child counts, slot keys;  2  the pooled stable sort;  3a  run heads and their scan;  the children's scan
        unsigned long long *keys = nullptr;
        PEDP_TRY(pedp_sort_keys64_exact_begin(c, E, 64, &keys));
        hipLaunchKernelGGL(flag_kernel, dim3(blocks_for(F + 1)), dim3(TT), 0, s, r->v, r->t, k.w, r->V0, F, limit2, keys, key_copy, count);
        PEDP_TRY(pedp_sort_keys64_exact_run(c, E, 64, perm));
        hipLaunchKernelGGL(run_head_kernel, dim3(blocks_for(E + 1)), dim3(TT), 0, s, key_copy, perm, E, head);
        PEDP_ROCPRIM(rocprim::exclusive_scan(tmp, tmp_bytes, head, rank, 0u, (size_t)E + 1, rocprim::plus<uint32_t>(), s));
        PEDP_ROCPRIM(rocprim::exclusive_scan(tmp, tmp_bytes, count, off, 0u, (size_t)F + 1, rocprim::plus<uint32_t>(), s));
        PEDP_HIP_CHECK(hipGetLastError());
        // the round's two counts size its outputs: the one wait of the round
        uint32_t n_new = 0, f_new = 0;
        PEDP_HIP_CHECK(hipMemcpyAsync(&n_new, rank + E, 4, hipMemcpyDeviceToHost, s));
        PEDP_HIP_CHECK(hipMemcpyAsync(&f_new, off + F, 4, hipMemcpyDeviceToHost, s));
        PEDP_HIP_CHECK(hipStreamSynchronize(s));
        c->stage_busy = false;
        if (n_new == 0) return PEDP_OK;
        if (faces_reached) *faces_reached = (int64_t)f_new;
        PEDP_REQUIRE(r->rounds < MAX_ROUNDS, "%s: long edges are left after %d rounds", who, MAX_ROUNDS);
        PEDP_REQUIRE((int64_t)f_new <= face_cap, "%s: round %d reaches %lld faces, max_faces allows %lld", who, r->rounds + 1, (long long)f_new,
                     (long long)face_cap);
        PEDP_REQUIRE(V + (int64_t)n_new <= MAX_VERTS, "%s: round %d reaches %lld vertices (at most 2^32 - 2)", who, r->rounds + 1,
                     (long long)(V + (int64_t)n_new));
        const int64_t Vn = V + (int64_t)n_new, Fn = (int64_t)f_new;
        PEDP_TRY(dev_alloc((void **)&k.v_next, 24 * (size_t)Vn, who));
        PEDP_TRY(dev_alloc((void **)&k.t_next, 12 * (size_t)Fn, who));
        PEDP_TRY(dev_alloc((void **)&k.pf_next, 4 * (size_t)Fn, who));
        PEDP_HIP_CHECK(hipMemcpyAsync(k.v_next, r->v, 24 * (size_t)V, hipMemcpyDeviceToDevice, s));
        // 3b  the midpoints and every slot's vertex;  4  the children
        hipLaunchKernelGGL(midpoint_kernel, dim3(blocks_for(E)), dim3(TT), 0, s, key_copy, perm, head, rank, E, V, r->t, k.v_next, slot_mid);
        hipLaunchKernelGGL(emit_kernel, dim3(blocks_for(F)), dim3(TT), 0, s, k.v_next, r->t, r->pf, slot_mid, off, F, k.t_next, k.pf_next);
        PEDP_HIP_CHECK(hipGetLastError());
        PEDP_HIP_CHECK(hipStreamSynchronize(s));  // the old arrays are freed next
        std::swap(r->v, k.v_next); std::swap(r->t, k.t_next); std::swap(r->pf, k.pf_next);
        (void)hipFree(k.v_next); (void)hipFree(k.t_next); (void)hipFree(k.pf_next);
        k.v_next = nullptr; k.t_next = nullptr; k.pf_next = nullptr;
        r->V = Vn;
        r->F = Fn;
        r->rounds += 1;
    }
}

int refine_build(pedp_refined_s *r, const double *verts, const uint32_t *tris, int mem, double max_edge, int64_t face_cap,
                 int64_t *faces_reached, const char *who) {
    pedp_ctx_t c = r->ctx;
    hipStream_t s = c->stream;
    const int64_t V = r->V0, F = r->F0, E = 3 * F;
    Work k;
    PEDP_TRY(dev_alloc((void **)&r->v, 24 * (size_t)V, who));
    PEDP_TRY(dev_alloc((void **)&r->t, 4 * (size_t)E, who));
    PEDP_TRY(dev_alloc((void **)&r->pf, 4 * (size_t)F, who));
    PEDP_TRY(dev_alloc((void **)&r->start, 4 * ((size_t)F + 1), who));
    PEDP_TRY(dev_alloc((void **)&k.w, 4 * (size_t)V, who));
    PEDP_TRY(copy_in(c, r->v, verts, 24 * (size_t)V, mem));
    PEDP_TRY(copy_in(c, r->t, tris, 4 * (size_t)E, mem));
    // the arguments' check, before any kernel follows an index
    const uint64_t slots = topology::weld_slots(V);
    PEDP_TRY(k.ws.reserve(a256(4 * slots) + 256));
    uint32_t *first = (uint32_t *)((char *)k.ws.ptr + a256(4 * slots));
    PEDP_HIP_CHECK(hipMemsetAsync(first, 0xFF, 8, s));
    if (E) hipLaunchKernelGGL(check_tris_kernel, dim3(blocks_for(E)), dim3(TT), 0, s, r->t, E, V, first);
    if (V) hipLaunchKernelGGL(check_verts_kernel, dim3(blocks_for(V)), dim3(TT), 0, s, r->v, V, first);
    PEDP_HIP_CHECK(hipGetLastError());
    uint32_t bad[2] = {NONE, NONE};
    PEDP_TRY(pedp_download(c, bad, first, sizeof(bad)));
    PEDP_REQUIRE(bad[0] == NONE, "%s: triangle %u names a vertex outside the %lld given", who, bad[0] / 3, (long long)V);
    PEDP_REQUIRE(bad[1] == NONE, "%s: vertex %u has a non-finite coordinate", who, bad[1]);
    if (F) hipLaunchKernelGGL(iota_parent_kernel, dim3(blocks_for(F)), dim3(TT), 0, s, F, r->pf);
    if (F) {
        PEDP_TRY(topology::weld(c, r->v, V, (uint32_t *)k.ws.ptr, k.w));
        PEDP_TRY(refine_rounds(r, k, max_edge, face_cap, faces_reached, who));
    }
    hipLaunchKernelGGL(run_start_kernel, dim3(blocks_for(r->F + 1)), dim3(TT), 0, s, r->pf, r->F, r->F0, r->start);
    PEDP_HIP_CHECK(hipGetLastError());
    PEDP_HIP_CHECK(hipStreamSynchronize(s));
    if (faces_reached) *faces_reached = r->F;
    return PEDP_OK;
}

}  // namespace

extern "C" {

int pedp_mesh_refine(pedp_ctx_t c, const double *verts, int64_t V, const uint32_t *tris, int64_t F, int mem, double max_edge,
                     int64_t max_faces, pedp_refined_t *out, int64_t *faces_reached) {
    const char *who = "pedp_mesh_refine";
    PEDP_REQUIRE(out, "%s: null out", who);
    *out = nullptr;
    if (faces_reached) *faces_reached = 0;
    PEDP_REQUIRE(c, "%s: null context", who);
    PEDP_REQUIRE(mem == PEDP_HOST || mem == PEDP_DEVICE, "%s: bad mem flag %d", who, mem);
    PEDP_REQUIRE(V >= 0 && V <= MAX_VERTS && F >= 0 && F <= MAX_FACES, "%s: V = %lld, F = %lld (at most 2^28 faces)", who, (long long)V,
                 (long long)F);
    PEDP_REQUIRE((verts || V == 0) && (tris || F == 0), "%s: null array", who);
    PEDP_REQUIRE(max_edge > 0.0 && std::isfinite(max_edge), "%s: max_edge = %g must be a positive finite number", who, max_edge);
    PEDP_REQUIRE(max_faces >= 0, "%s: max_faces = %lld", who, (long long)max_faces);
    PEDP_REQUIRE(!c->icp_pending, "%s: a registration is pending on this context (the call waits for the stream)", who);
    if (faces_reached) *faces_reached = F;
    PEDP_REQUIRE(F <= max_faces, "%s: the input has %lld faces, max_faces allows %lld", who, (long long)F, (long long)max_faces);
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    pedp_refined_s *r = new pedp_refined_s;
    r->ctx = c;
    r->device = c->device;
    r->V0 = r->V = V;
    r->F0 = r->F = F;
    const int rc = refine_build(r, verts, tris, mem, max_edge, max_faces < MAX_FACES ? max_faces : MAX_FACES, faces_reached, who);
    if (rc) {
        (void)hipStreamSynchronize(c->stream);
        pedp_refined_destroy(r);
        return rc;
    }
    *out = r;
    return PEDP_OK;
}

int pedp_refined_destroy(pedp_refined_t r) {
    if (!r) return PEDP_OK;
    if (hipSetDevice(r->device) == hipSuccess) {
        if (r->v) (void)hipFree(r->v);  // waits for the device: nothing enqueued still uses it
        if (r->t) (void)hipFree(r->t);
        if (r->pf) (void)hipFree(r->pf);
        if (r->start) (void)hipFree(r->start);
        r->io.release();
    }
    delete r;
    return PEDP_OK;
}

int pedp_refined_size(pedp_refined_t r, int64_t *V_out, int64_t *F_out, int32_t *rounds) {
    PEDP_REQUIRE(r, "pedp_refined_size: null handle");
    if (V_out) *V_out = r->V;
    if (F_out) *F_out = r->F;
    if (rounds) *rounds = r->rounds;
    return PEDP_OK;
}

int pedp_refined_read(pedp_refined_t r, int mem, double *verts, uint32_t *tris, int32_t *parent_face) {
    const char *who = "pedp_refined_read";
    PEDP_REQUIRE(r, "%s: null handle", who);
    pedp_ctx_t c = r->ctx;
    PEDP_REQUIRE(mem == PEDP_HOST || mem == PEDP_DEVICE, "%s: bad mem flag %d", who, mem);
    PEDP_REQUIRE(mem == PEDP_DEVICE || !c->icp_pending, "%s: a registration is pending on this context (host-memory call)", who);
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    PEDP_TRY(copy_out(c, verts, r->v, 24 * (size_t)r->V, mem));
    PEDP_TRY(copy_out(c, tris, r->t, 12 * (size_t)r->F, mem));
    PEDP_TRY(copy_out(c, parent_face, r->pf, 4 * (size_t)r->F, mem));
    return PEDP_OK;
}

int pedp_refined_reduce(pedp_refined_t r, int op, int mem, const double *child_values, double *parent_values) {
    const char *who = "pedp_refined_reduce";
    PEDP_REQUIRE(r, "%s: null handle", who);
    pedp_ctx_t c = r->ctx;
    PEDP_REQUIRE(mem == PEDP_HOST || mem == PEDP_DEVICE, "%s: bad mem flag %d", who, mem);
    PEDP_REQUIRE(op == PEDP_REDUCE_MAX || op == PEDP_REDUCE_MIN || op == PEDP_REDUCE_SUM, "%s: op = %d", who, op);
    PEDP_REQUIRE(mem == PEDP_DEVICE || !c->icp_pending, "%s: a registration is pending on this context (host-memory call)", who);
    if (r->F0 == 0) return PEDP_OK;
    PEDP_REQUIRE(child_values && parent_values, "%s: null array", who);
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    const double *d_x = child_values;
    double *d_out = parent_values;
    if (mem == PEDP_HOST) {
        PEDP_TRY(r->io.reserve(a256(8 * (size_t)r->F) + a256(8 * (size_t)r->F0)));
        double *x = (double *)r->io.ptr;
        PEDP_TRY(pedp_upload(c, x, child_values, 8 * (size_t)r->F));
        d_x = x;
        d_out = (double *)((char *)r->io.ptr + a256(8 * (size_t)r->F));
    }
    hipLaunchKernelGGL(reduce_kernel, dim3(blocks_for(r->F0)), dim3(TT), 0, c->stream, r->start, r->F0, op, d_x, d_out);
    PEDP_HIP_CHECK(hipGetLastError());
    if (mem == PEDP_HOST) return pedp_download(c, parent_values, d_out, 8 * (size_t)r->F0);
    return PEDP_OK;
}

}  // extern "C"
