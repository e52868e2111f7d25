// What the signed query (pedp_solid.hip) shares with the deviation map fed straight from a frame's
// points (pedp_deviationmap.hip): the solid's handle, the vertex pseudonormals, the sign of a point
// against its closest feature, and the checks of a query.  Internal linkage: each including file gets its own copy.
#pragma once
#include "../pedp_internal.h"
#include "../mesh/record.h"
#include <cmath>

struct pedp_solid_s {
    pedp_ctx_t ctx = nullptr;
    int device = 0;
    pedp_solid_info info = {};
    char *store = nullptr;  // one allocation: everything below
    uint32_t *tri = nullptr;     // 3 F: the index buffer (what a posable mesh's own is compared with)
    uint32_t *wid = nullptr;     // 3 F: the welded id of every corner
    uint32_t *twin = nullptr;    // 3 F: the twin of every edge slot, or NONE
    int32_t *corner = nullptr;   // 3 F: the corners sorted by (welded id, face, corner)
    uint32_t *vstart = nullptr, *vcount = nullptr;  // V: a welded vertex's run in `corner` (NONE, 0: it has none)
    uint64_t verified_gen = 0;   // the posable mesh whose index buffer was found equal
    pedp_scratch ws;  // a query: the vertex table and the search's outputs; the build's scratch
    pedp_scratch io;  // staging of host-memory calls
};

namespace {
namespace solid {

using namespace record;

constexpr int ST = 256;                  // threads per block
constexpr int64_t MAX_POINTS = (int64_t)1 << 24;
constexpr uint32_t NONE = 0xFFFFFFFFu;
enum { FEATURE_FACE = 0, FEATURE_EDGE = 1, FEATURE_VERTEX = 2, FEATURE_NONE = 255 };

inline size_t a256(size_t b) { return (b + 255) & ~(size_t)255; }
inline unsigned blocks_for(int64_t n) { return (unsigned)((n + ST - 1) / ST); }

__global__ __launch_bounds__(ST) void index_compare_kernel(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, int64_t E,
                                                          uint32_t *__restrict__ differs) {
    const int64_t e = (int64_t)blockIdx.x * ST + threadIdx.x;
    if (e < E && a[e] != b[e]) atomicOr(differs, 1u);
}

// The angle-weighted pseudonormal of every welded vertex from the records as posed: over the vertex's corners in list
// order, N = N + n angle with n the face's unit normal and angle = atan2(|q x s|, q . s) between the record's two edges
// q, s that leave the corner.  Records that load_tri refuses, and faces whose normal has no length, add nothing.
__global__ __launch_bounds__(ST) void vertex_normal_kernel(const float *__restrict__ rec, const uint32_t *__restrict__ vstart,
                                                          const uint32_t *__restrict__ vcount, const int32_t *__restrict__ corner, int64_t V,
                                                          double *__restrict__ table) {
    const int64_t v = (int64_t)blockIdx.x * ST + threadIdx.x;
    if (v >= V) return;
    const uint32_t p0 = vstart[v];
    if (p0 == NONE) return;  // welded to a lower vertex, or in no face: never looked up
    double N[3] = {0.0, 0.0, 0.0};
    const uint32_t n = vcount[v];
    for (uint32_t j = 0; j < n; ++j) {
        const int32_t e = corner[p0 + j];
        const int32_t f = e / 3, k = e - 3 * f;
        Tri t;
        if (!load_tri(rec + (size_t)f * PEDP_TRI_STRIDE, t)) continue;
        double nh[3], q[3], s[3], qs[3];
        unit_normal(t, nh);
        if (!(nh[0] == nh[0])) continue;
        for (int d = 0; d < 3; ++d) {
            q[d] = k == 0 ? t.ab[d] : (k == 1 ? t.ac[d] - t.ab[d] : -t.ac[d]);
            s[d] = k == 0 ? t.ac[d] : (k == 1 ? -t.ab[d] : t.ab[d] - t.ac[d]);
        }
        cross3(q, s, qs);
        const double angle = atan2(sqrt(dot3(qs, qs)), dot3(q, s));
        for (int d = 0; d < 3; ++d) N[d] = N[d] + nh[d] * angle;
    }
    table[3 * v] = N[0]; table[3 * v + 1] = N[1]; table[3 * v + 2] = N[2];
}

// what the sign of a point needs besides the search's outputs
struct SignArgs {
    const float *rec;       // the mesh's records as posed
    const double *table;    // vertex_normal_kernel's
    const uint32_t *wid, *twin;
    double orientation;     // +1 / -1
};
// The pseudonormal N of the feature that the search's rule names for point p with closest point c on triangle f, and the
// sign of (p - c) . N on `sd` (the search's distance on entry).  Returns the feature; FEATURE_NONE (no triangle, or a
// record the search skips) leaves sd and N as they are.
__device__ __forceinline__ int sign_of_point(const SignArgs &a, uint32_t f, int rule, const double p[3], const double c[3], double &sd,
                                             double N[3]) {
    int feature = FEATURE_NONE;
    Tri t;
    if (f != NONE && load_tri(a.rec + (size_t)f * PEDP_TRI_STRIDE, t)) {
        if (rule == 1 || rule == 2 || rule == 4) {  // corners 0, 1, 2
            feature = FEATURE_VERTEX;
            const size_t v = a.wid[3 * (size_t)f + (rule >> 1)];
            N[0] = a.table[3 * v]; N[1] = a.table[3 * v + 1]; N[2] = a.table[3 * v + 2];
        } else {
            unit_normal(t, N);
            if (rule != 7) {  // rules 3, 6, 5: the edge slots 0 (ab), 1 (bc), 2 (ca)
                feature = FEATURE_EDGE;
                const uint32_t tw = a.twin[3 * (size_t)f + (rule == 3 ? 0 : (rule == 6 ? 1 : 2))];
                Tri u;
                double m[3];
                if (tw != NONE && load_tri(a.rec + (size_t)(tw / 3) * PEDP_TRI_STRIDE, u)) {
                    unit_normal(u, m);
                    if (m[0] == m[0])
                        for (int d = 0; d < 3; ++d) N[d] = N[d] + m[d];
                }
            } else {
                feature = FEATURE_FACE;
            }
        }
        double r[3];
        for (int d = 0; d < 3; ++d) r[d] = p[d] - c[d];
        const double s = dot3(r, N) * a.orientation;
        if (s < 0.0) sd = -sd;  // s == 0 counts as outside
    }
    return feature;
}

// The argument checks of a signed query (`who` names it) on context c.
inline int check_query(const char *who, pedp_ctx_t c, pedp_mesh_t mesh, pedp_solid_s *solid, int64_t N, int mem) {
    PEDP_REQUIRE(c && mesh && solid, "%s: null context/mesh/solid", who);
    PEDP_REQUIRE(mesh->ctx == c && solid->ctx == c, "%s: the %s belongs to another context", who, mesh->ctx == c ? "solid" : "mesh");
    PEDP_REQUIRE(mem == PEDP_HOST || mem == PEDP_DEVICE, "%s: bad mem flag %d", who, mem);
    PEDP_REQUIRE(N >= 0 && N <= MAX_POINTS, "%s: N = %lld, at most %lld points", who, (long long)N, (long long)MAX_POINTS);
    const pedp_solid_info &info = solid->info;
    PEDP_REQUIRE(info.F == mesh->F, "%s: the solid has %lld faces, the mesh %lld", who, (long long)info.F, (long long)mesh->F);
    PEDP_REQUIRE(info.F == 0 || (info.closed && info.orientation != 0),
                 "%s: the mesh bounds no solid (%lld boundary, %lld non-manifold, %lld flipped edges, volume %g)", who,
                 (long long)info.boundary_edges, (long long)info.nonmanifold_edges, (long long)info.flipped_edges, info.volume);
    // the workspace is sized by N and V: growing it waits for the device, as the staging of a host-memory call does
    PEDP_REQUIRE(!c->icp_pending, "%s: a registration is pending on this context (the call may wait for the stream)", who);
    return PEDP_OK;
}

// A posable mesh keeps its index buffer: compared with the solid's once per mesh, on the device (d_flag: 4 bytes there).
inline int verify_indices(const char *who, pedp_ctx_t c, pedp_mesh_t mesh, pedp_solid_s *solid, uint32_t *d_flag) {
    const int64_t E = 3 * solid->info.F;
    if (!(E > 0 && mesh->idx && solid->verified_gen != mesh->gen)) return PEDP_OK;
    uint32_t differs = 0;
    PEDP_HIP_CHECK(hipMemsetAsync(d_flag, 0, 4, c->stream));
    hipLaunchKernelGGL(index_compare_kernel, dim3(blocks_for(E)), dim3(ST), 0, c->stream, mesh->idx, solid->tri, E, d_flag);
    PEDP_HIP_CHECK(hipGetLastError());
    const int rc = pedp_download(c, &differs, d_flag, 4);
    if (rc) return rc;
    PEDP_REQUIRE(!differs, "%s: the mesh's triangles are not the ones the solid was built from", who);
    solid->verified_gen = mesh->gen;
    return PEDP_OK;
}

}  // namespace solid
}  // namespace
