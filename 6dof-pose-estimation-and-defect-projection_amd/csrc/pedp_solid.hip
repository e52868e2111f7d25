// The solid: the topology of a closed triangle mesh, and with it the exact SIGNED distance and the
// occupancy of points (RaycastingScene.compute_signed_distance / compute_occupancy stand-ins).
//   * creation, once per model and independent of the pose: the weld and the sorted edge slots of mesh/topology.h
//     give every edge slot its twin and every welded vertex the list of its corners; the counts of boundary,
//     non-manifold and flipped edges say whether the mesh bounds a solid at all, the sign of its volume which way its
//     normals point.
//   * the query: pedp_closest_points' own search (pedp_closest_launch) with one more output, the rule of Ericson's
//     table that decided the closest point; a pass over the welded vertices forms their angle-weighted pseudonormals
//     from the mesh's records as posed; a pass over the points takes the pseudonormal N of the closest FEATURE (face,
//     edge or vertex: Baerentzen & Aanaes 2005) and signs the distance with (p - c) . N.
// float64 with no contraction, every expression in the order written, no floating-point atomics: the vertex sums
// run over the corner lists in their stored order, the volume is a block-tree sum.  tests/_signed_ref.py restates it.
#include "solid/shared.h"
#include "mesh/topology.h"
#include <cmath>

namespace {

using namespace solid;

constexpr int64_t MAX_FACES = 1 << 28;   // 3 F slots are sorted with int32 positions
constexpr int VOL_BLOCK = 4096;          // faces of one block's partial volume (16 per thread)
enum { C_WELDED = 0, C_EDGES, C_BOUNDARY, C_NONMANIFOLD, C_FLIPPED, C_DEGENERATE, C_VOLUME, C_COUNT };

// one atomic per wave: the number of lanes whose `flag` is set
__device__ __forceinline__ void count_lanes(bool flag, unsigned long long *counter) {
    const unsigned long long m = __ballot(flag);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(counter, (unsigned long long)__popcll(m));
}

// ------------------------------------------------------------------ creation
__global__ __launch_bounds__(ST) void corner_weld_kernel(const uint32_t *__restrict__ tri, const uint32_t *__restrict__ w, int64_t E,
                                                        uint32_t *__restrict__ wid) {
    const int64_t e = (int64_t)blockIdx.x * ST + threadIdx.x;
    if (e < E) wid[e] = w[tri[e]];
}

// vertices that stand for themselves; faces of which two corners weld to one vertex
__global__ __launch_bounds__(ST) void count_kernel(const uint32_t *__restrict__ w, int64_t V, const uint32_t *__restrict__ wid, int64_t F,
                                                  unsigned long long *__restrict__ counters) {
    const int64_t i = (int64_t)blockIdx.x * ST + threadIdx.x;
    count_lanes(i < V && w[i] == (uint32_t)i, &counters[C_WELDED]);
    bool degenerate = false;
    if (i < F) {
        const uint32_t a = wid[3 * i], b = wid[3 * i + 1], c = wid[3 * i + 2];
        degenerate = a == b || b == c || c == a;
    }
    count_lanes(degenerate, &counters[C_DEGENERATE]);
}

// Sorted position p opens the run of its edge: one slot is a boundary edge, three or more a non-manifold one, two are
// each other's twins unless both faces run through the edge in the same direction (flipped).  Only twins are stored.
__global__ __launch_bounds__(ST) void twin_kernel(const unsigned long long *__restrict__ key, const int32_t *__restrict__ perm,
                                                 const uint32_t *__restrict__ wid, int64_t E, uint32_t *__restrict__ twin,
                                                 unsigned long long *__restrict__ counters) {
    const int64_t p = (int64_t)blockIdx.x * ST + threadIdx.x;
    int len = 0;
    bool flipped = false;
    if (p < E) {
        const int32_t e = perm[p];
        const unsigned long long k = key[e];
        if (k != topology::NO_EDGE && (p == 0 || key[perm[p - 1]] != k)) {
            len = 1;
            while (len < 3 && p + len < E && key[perm[p + len]] == k) ++len;
            if (len == 2) {
                const int32_t e2 = perm[p + 1];
                // slot e runs from corner e to the next corner of its face
                const bool up = wid[e] < wid[e - e % 3 + (e % 3 + 1) % 3], up2 = wid[e2] < wid[e2 - e2 % 3 + (e2 % 3 + 1) % 3];
                flipped = up == up2;
                if (!flipped) { twin[e] = (uint32_t)e2; twin[e2] = (uint32_t)e; }
            }
        }
    }
    count_lanes(len > 0, &counters[C_EDGES]);
    count_lanes(len == 1, &counters[C_BOUNDARY]);
    count_lanes(len >= 3, &counters[C_NONMANIFOLD]);
    count_lanes(flipped, &counters[C_FLIPPED]);
}

__global__ __launch_bounds__(ST) void corner_key_kernel(const uint32_t *__restrict__ wid, int64_t E, unsigned long long *__restrict__ key) {
    const int64_t e = (int64_t)blockIdx.x * ST + threadIdx.x;
    if (e < E) key[e] = wid[e];
}
// the corners sorted by (welded id, face, corner): position p opens its vertex's list
__global__ __launch_bounds__(ST) void corner_list_kernel(const uint32_t *__restrict__ wid, const int32_t *__restrict__ corner, int64_t E,
                                                        uint32_t *__restrict__ vstart, uint32_t *__restrict__ vcount) {
    const int64_t p = (int64_t)blockIdx.x * ST + threadIdx.x;
    if (p >= E) return;
    const uint32_t w = wid[corner[p]];
    if (p > 0 && wid[corner[p - 1]] == w) return;
    int64_t q = p + 1;
    while (q < E && wid[corner[q]] == w) ++q;
    vstart[w] = (uint32_t)p;
    vcount[w] = (uint32_t)(q - p);
}

// a . (b x c) / 6 of the faces [VOL_BLOCK b, VOL_BLOCK (b + 1)): thread t adds its faces t, t + 256, ... one after the
// other, then the threads' sums are added pairwise, t with t + 128, t + 64, ... t + 1
__device__ __forceinline__ double block_tree_sum(double x, double *sh) {
    sh[threadIdx.x] = x;
    __syncthreads();
    for (int s = ST / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] = sh[threadIdx.x] + sh[threadIdx.x + s];
        __syncthreads();
    }
    return sh[0];
}
__global__ __launch_bounds__(ST) void volume_block_kernel(const double *__restrict__ v, const uint32_t *__restrict__ tri, int64_t F,
                                                         double *__restrict__ partial) {
    __shared__ double sh[ST];
    const int64_t f0 = (int64_t)blockIdx.x * VOL_BLOCK;
    double sum = 0.0;
    for (int j = 0; j < VOL_BLOCK / ST; ++j) {
        const int64_t f = f0 + (int64_t)j * ST + threadIdx.x;
        if (f >= F) break;
        const double *a = v + 3 * (size_t)tri[3 * f], *b = v + 3 * (size_t)tri[3 * f + 1], *c = v + 3 * (size_t)tri[3 * f + 2];
        double bc[3];
        cross3(b, c, bc);
        sum = sum + dot3(a, bc) / 6.0;
    }
    const double total = block_tree_sum(sum, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = total;
}
// one block: thread t adds the partial sums t, t + 256, ... one after the other, then the same tree
__global__ __launch_bounds__(ST) void volume_final_kernel(const double *__restrict__ partial, int64_t n, double *__restrict__ out) {
    __shared__ double sh[ST];
    double sum = 0.0;
    for (int64_t b = threadIdx.x; b < n; b += ST) sum = sum + partial[b];
    const double total = block_tree_sum(sum, sh);
    if (threadIdx.x == 0) *out = total;
}

// ------------------------------------------------------------------ the query
// the vertex pseudonormals and the sign of a point: solid/shared.h
struct FinishArgs {
    SignArgs sign;
    const double *pts, *closest, *dist;
    const uint32_t *prim;
    const uint8_t *region;
    int64_t n;
    double *sdist, *normal;
    int8_t *occupancy;
    uint8_t *feature;
};
// one lane per point: the pseudonormal of the feature the search's rule names, the sign of (p - c) . N
__global__ __launch_bounds__(ST) void finish_kernel(FinishArgs a) {
    const int64_t i = (int64_t)blockIdx.x * ST + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t f = a.prim[i];
    double sd = a.dist[i];  // no triangle: NaN for a non-finite point, +inf otherwise
    double nrm[3] = {quiet_nan(), quiet_nan(), quiet_nan()};
    double N[3];
    const double p[3] = {a.pts[3 * i], a.pts[3 * i + 1], a.pts[3 * i + 2]};
    const double c[3] = {a.closest[3 * i], a.closest[3 * i + 1], a.closest[3 * i + 2]};
    const int feature = sign_of_point(a.sign, f, f != NONE ? a.region[i] : 0, p, c, sd, N);
    if (feature != FEATURE_NONE) {
        const double len = sqrt(dot3(N, N));
        for (int d = 0; d < 3; ++d) nrm[d] = (N[d] / len) * a.sign.orientation;
    }
    if (a.sdist) a.sdist[i] = sd;
    if (a.occupancy) a.occupancy[i] = (int8_t)(sd < 0.0);
    if (a.feature) a.feature[i] = (uint8_t)feature;
    if (a.normal) { a.normal[3 * i] = nrm[0]; a.normal[3 * i + 1] = nrm[1]; a.normal[3 * i + 2] = nrm[2]; }
}

}  // namespace

namespace {

int build(pedp_solid_s *s, const double *verts, const uint32_t *tris) {
    pedp_ctx_t c = s->ctx;
    const int64_t V = s->info.V, F = s->info.F, E = 3 * F;
    const size_t v = (size_t)V, e = (size_t)E;
    const uint64_t slots = topology::weld_slots(V);
    const int64_t n_partial = (F + VOL_BLOCK - 1) / VOL_BLOCK;
    const size_t o_v = 0, o_slot = o_v + a256(24 * v), o_w = o_slot + a256(4 * slots), o_key = o_w + a256(4 * v), o_perm = o_key + a256(8 * e),
                 o_part = o_perm + a256(4 * e), o_cnt = o_part + a256(8 * (size_t)n_partial), bytes = o_cnt + a256(8 * C_COUNT);
    int rc = s->ws.reserve(bytes);
    if (rc) return rc;
    char *ws = (char *)s->ws.ptr;
    double *d_v = (double *)(ws + o_v), *d_part = (double *)(ws + o_part);
    uint32_t *d_slot = (uint32_t *)(ws + o_slot), *d_w = (uint32_t *)(ws + o_w);
    unsigned long long *d_key = (unsigned long long *)(ws + o_key), *d_cnt = (unsigned long long *)(ws + o_cnt);
    int32_t *d_perm = (int32_t *)(ws + o_perm);
    rc = pedp_upload(c, d_v, verts, 24 * v);
    if (!rc) rc = pedp_upload(c, s->tri, tris, 4 * e);
    if (rc) return rc;
    PEDP_HIP_CHECK(hipMemsetAsync(d_cnt, 0, 8 * C_COUNT, c->stream));
    PEDP_HIP_CHECK(hipMemsetAsync(s->twin, 0xFF, 4 * e, c->stream));
    PEDP_HIP_CHECK(hipMemsetAsync(s->vstart, 0xFF, 4 * v, c->stream));
    PEDP_HIP_CHECK(hipMemsetAsync(s->vcount, 0, 4 * v, c->stream));
    rc = topology::weld(c, d_v, V, d_slot, d_w);
    if (rc) return rc;
    const dim3 gE(blocks_for(E)), bt(ST);
    hipLaunchKernelGGL(corner_weld_kernel, gE, bt, 0, c->stream, s->tri, d_w, E, s->wid);
    hipLaunchKernelGGL(count_kernel, dim3(blocks_for(V > F ? V : F)), bt, 0, c->stream, d_w, V, s->wid, F, d_cnt);
    rc = topology::sort_edges(c, s->tri, d_w, E, d_key, d_perm);
    if (rc) return rc;
    hipLaunchKernelGGL(twin_kernel, gE, bt, 0, c->stream, d_key, d_perm, s->wid, E, s->twin, d_cnt);
    unsigned long long *keys = nullptr;
    rc = pedp_sort_keys64_exact_begin(c, E, 32, &keys);
    if (rc) return rc;
    hipLaunchKernelGGL(corner_key_kernel, gE, bt, 0, c->stream, s->wid, E, keys);
    rc = pedp_sort_keys64_exact_run(c, E, 32, s->corner);
    if (rc) return rc;
    hipLaunchKernelGGL(corner_list_kernel, gE, bt, 0, c->stream, s->wid, s->corner, E, s->vstart, s->vcount);
    hipLaunchKernelGGL(volume_block_kernel, dim3((unsigned)n_partial), bt, 0, c->stream, d_v, s->tri, F, d_part);
    hipLaunchKernelGGL(volume_final_kernel, dim3(1), bt, 0, c->stream, d_part, n_partial, (double *)(d_cnt + C_VOLUME));
    PEDP_HIP_CHECK(hipGetLastError());
    unsigned long long cnt[C_COUNT];
    rc = pedp_download(c, cnt, d_cnt, sizeof(cnt));
    if (rc) return rc;
    pedp_solid_info &o = s->info;
    o.welded_vertices = (int64_t)cnt[C_WELDED];
    o.edges = (int64_t)cnt[C_EDGES];
    o.boundary_edges = (int64_t)cnt[C_BOUNDARY];
    o.nonmanifold_edges = (int64_t)cnt[C_NONMANIFOLD];
    o.flipped_edges = (int64_t)cnt[C_FLIPPED];
    o.degenerate_faces = (int64_t)cnt[C_DEGENERATE];
    memcpy(&o.volume, &cnt[C_VOLUME], 8);
    o.closed = o.boundary_edges == 0 && o.nonmanifold_edges == 0 && o.flipped_edges == 0;
    o.orientation = o.volume > 0.0 ? 1 : (o.volume < 0.0 ? -1 : 0);
    return PEDP_OK;
}

}  // namespace

extern "C" {

int pedp_solid_create(pedp_ctx_t c, const double *verts, int64_t V, const uint32_t *tris, int64_t F, pedp_solid_t *out) {
    const char *who = "pedp_solid_create";
    PEDP_REQUIRE(c && out, "%s: null context/out", who);
    *out = nullptr;
    PEDP_REQUIRE(V >= 0 && V < ((int64_t)1 << 32) - 1 && F >= 0 && F <= MAX_FACES, "%s: V = %lld, F = %lld (at most 2^28 faces)", who,
                 (long long)V, (long long)F);
    PEDP_REQUIRE((verts || V == 0) && (tris || F == 0), "%s: null array", who);
    PEDP_REQUIRE(!c->icp_pending, "%s: a registration is pending on this context (the call waits for the stream)", who);
    for (int64_t i = 0; i < 3 * F; ++i)
        PEDP_REQUIRE((int64_t)tris[i] < V, "%s: triangle %lld names vertex %u of %lld", who, (long long)(i / 3), tris[i], (long long)V);
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    pedp_solid_s *s = new pedp_solid_s;
    s->ctx = c;
    s->device = c->device;
    s->info.V = V;
    s->info.F = F;
    *out = s;
    if (F == 0) return PEDP_OK;  // no faces: every count 0, not closed
    const size_t e = 3 * (size_t)F, v = (size_t)V;
    const size_t o_tri = 0, o_wid = o_tri + a256(4 * e), o_twin = o_wid + a256(4 * e), o_corner = o_twin + a256(4 * e),
                 o_vs = o_corner + a256(4 * e), o_vc = o_vs + a256(4 * v), bytes = o_vc + a256(4 * v);
    int rc = PEDP_OK;
    const hipError_t err = hipMalloc((void **)&s->store, bytes);
    if (err != hipSuccess) {
        pedp_set_error("%s: hipMalloc(%zu) -> %s", who, bytes, hipGetErrorString(err));
        rc = PEDP_ERR_HIP;
    }
    if (!rc) {
        s->tri = (uint32_t *)(s->store + o_tri); s->wid = (uint32_t *)(s->store + o_wid); s->twin = (uint32_t *)(s->store + o_twin);
        s->corner = (int32_t *)(s->store + o_corner); s->vstart = (uint32_t *)(s->store + o_vs); s->vcount = (uint32_t *)(s->store + o_vc);
        rc = build(s, verts, tris);
    }
    if (rc) {
        pedp_solid_destroy(s);
        *out = nullptr;
    }
    return rc;
}

int pedp_solid_destroy(pedp_solid_t s) {
    if (!s) return PEDP_OK;
    if (hipSetDevice(s->device) == hipSuccess) {
        if (s->store) (void)hipFree(s->store);  // waits for the device: nothing enqueued still uses it
        s->ws.release();
        s->io.release();
    }
    delete s;
    return PEDP_OK;
}

int pedp_solid_get_info(pedp_solid_t s, pedp_solid_info *out) {
    PEDP_REQUIRE(s && out, "pedp_solid_get_info: null argument");
    *out = s->info;
    return PEDP_OK;
}

int pedp_signed_distance(pedp_ctx_t c, pedp_mesh_t mesh, pedp_solid_t solid, const double *pts, int64_t N, int mem, double *sdist,
                         int8_t *occupancy, uint8_t *feature, double *normal) {
    const char *who = "pedp_signed_distance";
    int rc = check_query(who, c, mesh, solid, N, mem);
    if (rc) return rc;
    const pedp_solid_info &info = solid->info;
    if (N == 0) return PEDP_OK;
    PEDP_REQUIRE(pts, "%s: null points", who);
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    const int64_t V = info.V, F = info.F;
    const size_t n = (size_t)N;
    // the vertex table, the search's outputs, the flag of the index comparison
    const size_t o_table = 0, o_cl = o_table + a256(24 * (size_t)V), o_d = o_cl + a256(24 * n), o_id = o_d + a256(8 * n),
                 o_reg = o_id + a256(4 * n), o_flag = o_reg + a256(n), ws_bytes = o_flag + 256;
    rc = solid->ws.reserve(ws_bytes);
    if (rc) return rc;
    char *ws = (char *)solid->ws.ptr;
    rc = verify_indices(who, c, mesh, solid, (uint32_t *)(ws + o_flag));
    if (rc) return rc;
    const double *d_pts = pts;
    double *d_sd = sdist, *d_nrm = normal;
    int8_t *d_occ = occupancy;
    uint8_t *d_feat = feature;
    const size_t o_pts = 0, o_sd = o_pts + a256(24 * n), o_occ = o_sd + a256(8 * n), o_feat = o_occ + a256(n), o_nrm = o_feat + a256(n),
                 io_bytes = o_nrm + a256(24 * n);
    if (mem == PEDP_HOST) {
        rc = solid->io.reserve(io_bytes);
        if (rc) return rc;
        char *io = (char *)solid->io.ptr;
        rc = pedp_upload(c, io + o_pts, pts, 24 * n);
        if (rc) return rc;
        d_pts = (const double *)(io + o_pts);
        d_sd = sdist ? (double *)(io + o_sd) : nullptr;
        d_occ = occupancy ? (int8_t *)(io + o_occ) : nullptr;
        d_feat = feature ? (uint8_t *)(io + o_feat) : nullptr;
        d_nrm = normal ? (double *)(io + o_nrm) : nullptr;
    }
    FinishArgs a;
    a.sign.rec = mesh->tri;
    a.pts = d_pts;
    a.closest = (double *)(ws + o_cl); a.dist = (double *)(ws + o_d); a.prim = (uint32_t *)(ws + o_id); a.region = (uint8_t *)(ws + o_reg);
    a.sign.table = (double *)(ws + o_table);
    a.sign.wid = solid->wid; a.sign.twin = solid->twin;
    a.n = N;
    a.sign.orientation = info.orientation < 0 ? -1.0 : 1.0;
    a.sdist = d_sd; a.normal = d_nrm; a.occupancy = d_occ; a.feature = d_feat;
    rc = pedp_closest_launch(c, mesh, d_pts, N, (double *)a.closest, (double *)a.dist, (uint32_t *)a.prim, nullptr, nullptr,
                             (uint8_t *)a.region);
    if (rc) return rc;
    if (F > 0)
        hipLaunchKernelGGL(vertex_normal_kernel, dim3(blocks_for(V)), dim3(ST), 0, c->stream, mesh->tri, solid->vstart, solid->vcount,
                           solid->corner, V, (double *)a.sign.table);
    hipLaunchKernelGGL(finish_kernel, dim3(blocks_for(N)), dim3(ST), 0, c->stream, a);
    PEDP_HIP_CHECK(hipGetLastError());
    if (mem == PEDP_HOST) {
        if (sdist) rc = pedp_download(c, sdist, d_sd, 8 * n);
        if (!rc && occupancy) rc = pedp_download(c, occupancy, d_occ, n);
        if (!rc && feature) rc = pedp_download(c, feature, d_feat, n);
        if (!rc && normal) rc = pedp_download(c, normal, d_nrm, 24 * n);
    }
    return rc;
}

}  // extern "C"
