// Closest point of a triangle mesh to every point of a batch (RaycastingScene.compute_closest_points stand-in).
//
//   closest_exhaustive_kernel   one point per lane, every triangle record in index order (the address is the same in
//                               every lane), a running (d^2, id) minimum: the yardstick, and what
//                               pedp_closest_configure(ctx, 1) selects
//   closest_culled_kernel       one wave per 64 consecutive points, branch and bound on the spheres the mesh carries for the
//                               ray caster: the wave walks super-clusters, then clusters, in index order; a lane tests a
//                               cluster's triangles unless a proven lower bound of its distance to the sphere exceeds the
//                               lane's running best; a sphere no lane wants is passed by the whole wave.  The running best
//                               starts from the cluster nearest to each lane (tested first).
//   closest_wave_kernel         the same branch and bound with one wave per point, for batches too small to fill the
//                               device with a point per lane (and for scattered points, whose lanes share no candidates):
//                               the lanes take the 64 clusters of a super-cluster for the sphere tests and 4 x 16 triangles
//                               for the triangle tests, and fold their minima with a butterfly of lexicographic minima
//
// Arithmetic: float64 with no contraction (-ffp-contract=off), every expression in the order written,
// no floating-point atomics.  All three kernels call the same point_triangle() and keep the lexicographic minimum of
// (d^2, triangle index), which does not depend on the order of the tests: the culled path returns the bits of the
// exhaustive one as long as it never drops a triangle that could win, which the margin of sphere_culls() is there for.
// tests/_closest_ref.py restates the contract in numpy.
//
// pedp_fit_to_surface (pedp_surface_fit.hip) runs the same three kernels instantiated with FIT = true,
// which read two more arguments: T, a pose the finite rows go through as they are loaded, and done, a device flag that
// makes a launch return at once.  pedp_closest_points runs them with FIT = false and reads neither.
#include "pedp_internal.h"
#include "mesh/cluster.h"              // CL_TRIS: triangles per cluster sphere
#include "mesh/record.h"
#include "closest/move_point.h"
#include <cmath>
#include <type_traits>

namespace {

constexpr int SUPER_CL = 64;           // clusters per super-cluster sphere
constexpr int CT = 256;                // threads per workgroup
constexpr unsigned NONE = 0xFFFFFFFFu;
constexpr int64_t MAX_POINTS = (int64_t)1 << 24;
constexpr int64_t WAVE_POINTS_MAX = 16384;  // up to here a wave per point: as many waves as the device holds at once (256 CUs x 32) twice over
enum { MODE_AUTO = 0, MODE_EXHAUSTIVE = 1, MODE_LANE = 2, MODE_WAVE = 3 };

using namespace record;

// Ericson's closest point of a triangle: the barycentrics (v, w) of the first matching region, then the squared
// distance of p from c = (a + ab v) + ac w; rule: the number 1 ... 7 of the region that matched (pedp.h's table)
__device__ __forceinline__ double point_triangle(const double p[3], const Tri &t, double &v, double &w, double c[3], double r[3], int &rule) {
    double ap[3], bp[3], cp[3];
    for (int k = 0; k < 3; ++k) {
        ap[k] = p[k] - t.a[k];
        bp[k] = ap[k] - t.ab[k];
        cp[k] = ap[k] - t.ac[k];
    }
    const double d1 = dot3(t.ab, ap), d2 = dot3(t.ac, ap), d3 = dot3(t.ab, bp), d4 = dot3(t.ac, bp), d5 = dot3(t.ab, cp),
                 d6 = dot3(t.ac, cp);
    const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    if (d1 <= 0.0 && d2 <= 0.0) {
        v = 0.0; w = 0.0; rule = 1;
    } else if (d3 >= 0.0 && d4 <= d3) {
        v = 1.0; w = 0.0; rule = 2;
    } else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
        v = d1 / (d1 - d3); w = 0.0; rule = 3;
    } else if (d6 >= 0.0 && d5 <= d6) {
        v = 0.0; w = 1.0; rule = 4;
    } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
        v = 0.0; w = d2 / (d2 - d6); rule = 5;
    } else if (va <= 0.0 && d4 - d3 >= 0.0 && d5 - d6 >= 0.0) {
        const double e = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        v = 1.0 - e; w = e; rule = 6;
    } else {
        const double den = 1.0 / ((va + vb) + vc);
        v = vb * den; w = vc * den; rule = 7;
    }
    for (int k = 0; k < 3; ++k) {
        c[k] = (t.a[k] + t.ab[k] * v) + t.ac[k] * w;
        r[k] = p[k] - c[k];
    }
    return (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
}
__device__ __forceinline__ double point_triangle(const double p[3], const Tri &t, double &v, double &w, double c[3], double r[3]) {
    int rule;
    return point_triangle(p, t, v, w, c, r, rule);
}

// the running minimum of (d^2, id): a NaN never enters, ties go to the lower index
__device__ __forceinline__ void take(double d2, unsigned id, double &best, unsigned &bid) {
    if (d2 < best || (d2 == best && id < bid)) { best = d2; bid = id; }
}

struct Args {
    const float *tri;          // F_padded records
    const float4 *sph, *ssph;  // cluster and super-cluster spheres
    int64_t F, n_clusters, n_super;
    const double *pts;
    int64_t n;
    double *closest, *dist, *uv;
    uint32_t *prim;
    int8_t *side;
    uint8_t *region;  // the rule (1 ... 7) that point_triangle took for the chosen triangle, 0 where there is none
    unsigned long long *pairs;
};

// what the kernels get as pedp_fit_to_surface runs them (FIT); pedp_closest_points' kernels keep Args as it was
struct FitArgs : Args {
    const double *T;   // a row-major 4 x 4 the finite rows are moved by as they are loaded
    const int *done;   // a device flag: non-zero turns the launch into an early exit
};
template <bool FIT> using ArgsOf = std::conditional_t<FIT, FitArgs, Args>;

// the outputs of point i from its chosen triangle: the same point_triangle() as the search
__device__ __forceinline__ void store_result(const Args &a, int64_t i, bool finite, const double p[3], double best, unsigned bid) {
    double c[3] = {quiet_nan(), quiet_nan(), quiet_nan()}, v = quiet_nan(), w = quiet_nan();
    double d = finite ? pos_inf() : quiet_nan();
    unsigned id = NONE;
    int s = 0, rule = 0;
    if (finite && bid != NONE && best < pos_inf()) {
        Tri t;
        (void)load_tri(a.tri + (size_t)bid * PEDP_TRI_STRIDE, t);
        double r[3];
        const double d2 = point_triangle(p, t, v, w, c, r, rule);
        d = sqrt(d2);
        id = bid;
        const double nrm[3] = {t.ab[1] * t.ac[2] - t.ab[2] * t.ac[1], t.ab[2] * t.ac[0] - t.ab[0] * t.ac[2],
                               t.ab[0] * t.ac[1] - t.ab[1] * t.ac[0]};
        const double sd = dot3(r, nrm);
        s = sd > 0.0 ? 1 : (sd < 0.0 ? -1 : 0);
    }
    if (a.closest) { a.closest[3 * i] = c[0]; a.closest[3 * i + 1] = c[1]; a.closest[3 * i + 2] = c[2]; }
    if (a.dist) a.dist[i] = d;
    if (a.prim) a.prim[i] = id;
    if (a.uv) { a.uv[2 * i] = v; a.uv[2 * i + 1] = w; }
    if (a.side) a.side[i] = (int8_t)s;
    if (a.region) a.region[i] = (uint8_t)rule;
}

template <bool FIT> __device__ __forceinline__ bool load_point(const ArgsOf<FIT> &a, int64_t i, double p[3]) {
    p[0] = p[1] = p[2] = 0.0;
    if (i >= a.n) return false;
    if (!pedp_row_finite(a.pts, i)) return false;
    p[0] = a.pts[3 * i]; p[1] = a.pts[3 * i + 1]; p[2] = a.pts[3 * i + 2];
    if constexpr (FIT) surface_fit::move_point(a.T, p);
    return true;
}

template <bool FIT> __device__ __forceinline__ bool finished(const ArgsOf<FIT> &a) {
    if constexpr (FIT) return *a.done != 0;
    return false;
}

__device__ __forceinline__ void add_pairs(const Args &a, unsigned long long n) {
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(a.pairs, n);
}

template <bool FIT> __global__ __launch_bounds__(CT) void closest_exhaustive_kernel(ArgsOf<FIT> a) {
    if (finished<FIT>(a)) return;
    const int64_t i = (int64_t)blockIdx.x * CT + threadIdx.x;
    double p[3];
    const bool live = load_point<FIT>(a, i, p);
    double best = pos_inf();
    unsigned bid = NONE;
    unsigned long long tested = 0;  // the same in every lane
    for (int64_t f = 0; f < a.F; ++f) {
        Tri t;
        if (!load_tri(a.tri + (size_t)f * PEDP_TRI_STRIDE, t)) continue;
        ++tested;
        double v, w, c[3], r[3];
        const double d2 = point_triangle(p, t, v, w, c, r);
        take(d2, (unsigned)f, best, bid);
    }
    add_pairs(a, tested * (unsigned long long)__popcll(__ballot(live)));
    if (i < a.n) store_result(a, i, live, p, best, bid);
}

// May the sphere q be passed by for a point whose running best squared distance is `best`?  Only if a lower bound of the
// distance of p to anything inside the sphere, |p - centre| - radius, exceeds it strictly after a margin for the rounding
// of that expression (DESIGN.md s4.16 "margin"); an empty sphere (radius < 0) always.
__device__ __forceinline__ bool sphere_culls(const double p[3], const float4 q, double best) {
    if (q.w < 0.0f) return true;
    const double dx = p[0] - (double)q.x, dy = p[1] - (double)q.y, dz = p[2] - (double)q.z;
    const double lb = sqrt((dx * dx + dy * dy) + dz * dz) - (double)q.w;
    return lb > 0.0 && (lb * lb) * (1.0 - 0x1p-40) > best;
}

// float32 |p - centre| - radius: orders the spheres for the seed only, decides nothing
__device__ __forceinline__ float seed_key(const float p[3], const float4 q) {
    const float dx = p[0] - q.x, dy = p[1] - q.y, dz = p[2] - q.z;
    return sqrtf(dx * dx + dy * dy + dz * dz) - q.w;
}

// the triangles of cluster c against the lanes that want it; returns the number of records tested (the same in every lane)
__device__ __forceinline__ int visit_cluster(const Args &a, int64_t c, bool want, const double p[3], double &best, unsigned &bid) {
    int tested = 0;
    for (int k = 0; k < CL_TRIS; ++k) {
        const int64_t f = c * CL_TRIS + k;
        if (f >= a.F) break;
        Tri t;
        if (!load_tri(a.tri + (size_t)f * PEDP_TRI_STRIDE, t)) continue;
        ++tested;
        if (want) {
            double v, w, cc[3], r[3];
            const double d2 = point_triangle(p, t, v, w, cc, r);
            take(d2, (unsigned)f, best, bid);
        }
    }
    return tested;
}

template <bool FIT> __global__ __launch_bounds__(CT) void closest_culled_kernel(ArgsOf<FIT> a) {
    if (finished<FIT>(a)) return;
    const int64_t i = (int64_t)blockIdx.x * CT + threadIdx.x;
    double p[3];
    const bool live = load_point<FIT>(a, i, p);
    double best = pos_inf();
    unsigned bid = NONE;
    unsigned long long pairs = 0;  // the same in every lane

    // the seed: the cluster that looks nearest to this lane, through the nearest-looking super-cluster
    const float pf[3] = {(float)p[0], (float)p[1], (float)p[2]};
    int64_t seed = -1;
    {
        float key = 3e38f;
        int64_t s0 = -1;
        for (int64_t s = 0; s < a.n_super; ++s) {
            const float4 q = a.ssph[s];
            const float k = seed_key(pf, q);
            if (q.w >= 0.0f && k < key) { key = k; s0 = s; }
        }
        if (s0 >= 0) {
            key = 3e38f;
            const int64_t c1 = (s0 + 1) * SUPER_CL < a.n_clusters ? (s0 + 1) * SUPER_CL : a.n_clusters;
            for (int64_t c = s0 * SUPER_CL; c < c1; ++c) {
                const float4 q = a.sph[c];
                const float k = seed_key(pf, q);
                if (q.w >= 0.0f && k < key) { key = k; seed = c; }
            }
        }
        if (!live) seed = -1;
    }
    // every distinct seed of the wave, offered to all of its lanes (the first one is taken by all: best is +inf)
    for (unsigned long long todo = __ballot(seed >= 0); todo;) {
        const int src = __ffsll((long long)todo) - 1;
        const int64_t c = __shfl(seed, src, 64);
        todo &= ~__ballot(seed == c);
        const bool want = live && !sphere_culls(p, a.sph[c], best);
        const unsigned long long m = __ballot(want);
        if (m) pairs += (unsigned long long)__popcll(m) * (unsigned long long)visit_cluster(a, c, want, p, best, bid);
    }
    // the walk: super-clusters, then their clusters, in index order
    for (int64_t s = 0; s < a.n_super; ++s) {
        const bool want_s = live && !sphere_culls(p, a.ssph[s], best);
        if (!__ballot(want_s)) continue;
        const int64_t c1 = (s + 1) * SUPER_CL < a.n_clusters ? (s + 1) * SUPER_CL : a.n_clusters;
        for (int64_t c = s * SUPER_CL; c < c1; ++c) {
            if (__ballot(seed == c)) continue;  // tested above
            const bool want = want_s && !sphere_culls(p, a.sph[c], best);
            const unsigned long long m = __ballot(want);
            if (m) pairs += (unsigned long long)__popcll(m) * (unsigned long long)visit_cluster(a, c, want, p, best, bid);
        }
    }
    add_pairs(a, pairs);
    if (i < a.n) store_result(a, i, live, p, best, bid);
}

// every lane ends with the minimum of (d^2, id) over the wave
__device__ __forceinline__ void wave_min(double &best, unsigned &bid) {
    for (int off = 32; off > 0; off >>= 1) {
        const double ob = __shfl_xor(best, off, 64);
        const unsigned oi = __shfl_xor(bid, off, 64);
        take(ob, oi, best, bid);
    }
}

// every lane ends with the smallest key of the wave and its index (ties: the larger index, so that the lanes agree)
__device__ __forceinline__ void wave_argmin(float &key, int64_t &idx) {
    for (int off = 32; off > 0; off >>= 1) {
        const float ok = __shfl_xor(key, off, 64);
        const int64_t oi = __shfl_xor(idx, off, 64);
        if (ok < key || (ok == key && oi > idx)) { key = ok; idx = oi; }
    }
}

// lane l tests triangle (l & 15) of the cluster `c` its group of 16 lanes was given (c < 0: none); returns the records tested
__device__ __forceinline__ int test_quad(const Args &a, int64_t c, const double p[3], double &best, unsigned &bid) {
    const int64_t f = c * CL_TRIS + (threadIdx.x & 15);
    Tri t;
    const bool on = c >= 0 && f < a.F && load_tri(a.tri + (size_t)f * PEDP_TRI_STRIDE, t);
    if (on) {
        double v, w, cc[3], r[3];
        const double d2 = point_triangle(p, t, v, w, cc, r);
        take(d2, (unsigned)f, best, bid);
    }
    wave_min(best, bid);
    return __popcll(__ballot(on));
}

template <bool FIT> __global__ __launch_bounds__(CT) void closest_wave_kernel(ArgsOf<FIT> a) {
    if (finished<FIT>(a)) return;
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * (CT / 64) + (threadIdx.x >> 6);
    if (i >= a.n) return;  // the whole wave
    double p[3];
    const bool live = load_point<FIT>(a, i, p);
    double best = pos_inf();  // the same in every lane from here on
    unsigned bid = NONE;
    unsigned long long pairs = 0;
    int64_t seed = -1;
    if (live) {
        const float pf[3] = {(float)p[0], (float)p[1], (float)p[2]};
        float key = 3e38f;
        int64_t s0 = -1;
        for (int64_t s = lane; s < a.n_super; s += 64) {
            const float4 q = a.ssph[s];
            const float k = seed_key(pf, q);
            if (q.w >= 0.0f && k < key) { key = k; s0 = s; }
        }
        wave_argmin(key, s0);
        if (s0 >= 0) {
            const int64_t c = s0 * SUPER_CL + lane;
            key = 3e38f;
            if (c < a.n_clusters) {
                const float4 q = a.sph[c];
                const float k = seed_key(pf, q);
                if (q.w >= 0.0f && k < 3e38f) { key = k; seed = c; }
            }
            wave_argmin(key, seed);
        }
        if (seed >= 0) pairs += test_quad(a, lane < CL_TRIS ? seed : -1, p, best, bid);
        for (int64_t s = 0; s < a.n_super; ++s) {
            if (sphere_culls(p, a.ssph[s], best)) continue;  // the same in every lane
            const int64_t c = s * SUPER_CL + lane;
            const bool mine = c < a.n_clusters && c != seed;
            const float4 q = mine ? a.sph[c] : make_float4(0.f, 0.f, 0.f, -1.f);
            unsigned long long m = __ballot(mine && !sphere_culls(p, q, best));
            while (m) {
                int sel = -1;
                for (int j = 0; j < 4 && m; ++j) {  // the next four clusters, one per group of 16 lanes
                    const int b = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    if (j == (lane >> 4)) sel = b;
                }
                pairs += test_quad(a, sel >= 0 ? s * SUPER_CL + sel : -1, p, best, bid);
                m &= __ballot(mine && !sphere_culls(p, q, best));  // the rest against the new best
            }
        }
    }
    add_pairs(a, pairs);
    if (lane == 0) store_result(a, i, live, p, best, bid);
}

// the unit normal ab x ac of the listed triangles (NaN for an id that names none)
__global__ __launch_bounds__(CT) void face_normal_kernel(const float *__restrict__ tri, int64_t F, const uint32_t *__restrict__ prim,
                                                         int64_t n, double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * CT + threadIdx.x;
    if (i >= n) return;
    double nrm[3] = {quiet_nan(), quiet_nan(), quiet_nan()};
    const uint32_t f = prim[i];
    Tri t;
    if ((int64_t)f < F && load_tri(tri + (size_t)f * PEDP_TRI_STRIDE, t)) unit_normal(t, nrm);
    out[3 * i] = nrm[0]; out[3 * i + 1] = nrm[1]; out[3 * i + 2] = nrm[2];
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

namespace {

// one search on device memory, enqueued on the context's stream; `pairs` is the caller's counter, already zero
template <bool FIT> int launch_search(pedp_ctx_t c, pedp_mesh_t mesh, ArgsOf<FIT> &a, int64_t N) {
    a.tri = mesh->tri;
    a.sph = (const float4 *)mesh->spheres;
    a.ssph = (const float4 *)mesh->super_spheres;
    a.F = mesh->F;
    a.n_clusters = mesh->n_clusters;
    a.n_super = mesh->n_super;
    a.n = N;
    const dim3 grid((unsigned)((N + CT - 1) / CT));
    const int mode = c->closest_mode != MODE_AUTO ? c->closest_mode : (N <= WAVE_POINTS_MAX ? MODE_WAVE : MODE_LANE);
    if (mode == MODE_EXHAUSTIVE) hipLaunchKernelGGL(closest_exhaustive_kernel<FIT>, grid, dim3(CT), 0, c->stream, a);
    else if (mode == MODE_LANE) hipLaunchKernelGGL(closest_culled_kernel<FIT>, grid, dim3(CT), 0, c->stream, a);
    else hipLaunchKernelGGL(closest_wave_kernel<FIT>, dim3((unsigned)((N + CT / 64 - 1) / (CT / 64))), dim3(CT), 0, c->stream, a);
    PEDP_HIP_CHECK(hipGetLastError());
    return PEDP_OK;
}

}  // namespace

// The search of pedp_closest_points on device memory, enqueued on the context's stream: what the public call and
// pedp_signed_distance (pedp_solid.hip) both run.  region (nullable): the rule of pedp.h's table, 1 ... 7, that
// point_triangle took for the chosen triangle (0: no triangle); with it null every other output keeps its bits.
int pedp_closest_launch(pedp_ctx_t c, pedp_mesh_t mesh, const double *pts, int64_t N, double *closest, double *dist, uint32_t *prim_id,
                        double *uv, int8_t *side, uint8_t *region) {
    int rc = c->closest_ws.reserve(256);
    if (rc) return rc;
    Args a;
    a.pts = pts;
    a.closest = closest; a.dist = dist; a.prim = prim_id; a.uv = uv; a.side = side; a.region = region;
    a.pairs = (unsigned long long *)c->closest_ws.ptr;
    PEDP_HIP_CHECK(hipMemsetAsync(a.pairs, 0, sizeof(unsigned long long), c->stream));
    return launch_search<false>(c, mesh, a, N);
}

// The same search for pedp_fit_to_surface (pedp_surface_fit.hip): every finite row of pts goes through T (device, 4 x 4)
// as it is loaded, the whole launch exits at once when *done is set, and the pair counter is the caller's (the fit zeroes
// it once per call, so pedp_closest_last_stats keeps answering for the last pedp_closest_points).
int pedp_closest_launch_posed(pedp_ctx_t c, pedp_mesh_t mesh, const double *pts, int64_t N, const double *T, const int *done,
                              unsigned long long *pairs, double *closest, double *dist, uint32_t *prim_id) {
    FitArgs a;
    a.pts = pts;
    a.T = T; a.done = done;
    a.closest = closest; a.dist = dist; a.prim = prim_id; a.uv = nullptr; a.side = nullptr; a.region = nullptr;
    a.pairs = pairs;
    return launch_search<true>(c, mesh, a, N);
}

extern "C" {

int pedp_closest_configure(pedp_ctx_t c, int exhaustive) {
    PEDP_REQUIRE(c, "pedp_closest_configure: null context");
    PEDP_REQUIRE(exhaustive >= MODE_AUTO && exhaustive <= MODE_WAVE, "pedp_closest_configure: exhaustive %d", exhaustive);
    c->closest_mode = exhaustive;
    return PEDP_OK;
}

int pedp_closest_last_stats(pedp_ctx_t c, int64_t *pairs_tested) {
    const char *who = "pedp_closest_last_stats";
    PEDP_REQUIRE(c && pairs_tested, "%s: null argument", who);
    PEDP_REQUIRE(!c->icp_pending, "%s: a registration is pending on this context (the call waits for the stream)", who);
    *pairs_tested = 0;
    if (!c->closest_ws.ptr) return PEDP_OK;  // no call yet
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    unsigned long long v = 0;
    const int rc = pedp_download(c, &v, c->closest_ws.ptr, sizeof(v));
    if (rc) return rc;
    *pairs_tested = (int64_t)v;
    return PEDP_OK;
}

int pedp_mesh_face_normals(pedp_ctx_t c, pedp_mesh_t mesh, const uint32_t *prim_id, int64_t N, int mem, double *normals) {
    const char *who = "pedp_mesh_face_normals";
    PEDP_REQUIRE(c && mesh, "%s: null context/mesh", who);
    PEDP_REQUIRE(mesh->ctx == c, "%s: the mesh belongs to another context", who);
    PEDP_REQUIRE(mem == PEDP_HOST || mem == PEDP_DEVICE, "%s: bad mem flag %d", who, mem);
    PEDP_REQUIRE(N >= 0 && N <= MAX_POINTS, "%s: N = %lld, at most %lld ids", who, (long long)N, (long long)MAX_POINTS);
    if (N == 0) return PEDP_OK;
    PEDP_REQUIRE(prim_id && normals, "%s: null array", who);
    PEDP_REQUIRE(mem == PEDP_DEVICE || !c->icp_pending, "%s: a registration is pending on this context (host-memory call)", who);
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    const size_t n = (size_t)N;
    const uint32_t *d_id = prim_id;
    double *d_out = normals;
    if (mem == PEDP_HOST) {
        int rc = c->closest_io.reserve(align256(4 * n) + align256(24 * n));
        if (rc) return rc;
        char *io = (char *)c->closest_io.ptr;
        rc = pedp_upload(c, io, prim_id, 4 * n);
        if (rc) return rc;
        d_id = (const uint32_t *)io;
        d_out = (double *)(io + align256(4 * n));
    }
    hipLaunchKernelGGL(face_normal_kernel, dim3((unsigned)((N + CT - 1) / CT)), dim3(CT), 0, c->stream, mesh->tri, mesh->F, d_id, N,
                       d_out);
    PEDP_HIP_CHECK(hipGetLastError());
    if (mem == PEDP_HOST) return pedp_download(c, normals, d_out, 24 * n);
    return PEDP_OK;
}

int pedp_closest_points(pedp_ctx_t c, pedp_mesh_t mesh, const double *pts, int64_t N, int mem, double *closest, double *dist,
                        uint32_t *prim_id, double *uv, int8_t *side) {
    const char *who = "pedp_closest_points";
    PEDP_REQUIRE(c && mesh, "%s: null context/mesh", who);
    PEDP_REQUIRE(mesh->ctx == c, "%s: the mesh belongs to another context", who);
    PEDP_REQUIRE(mem == PEDP_HOST || mem == PEDP_DEVICE, "%s: bad mem flag %d", who, mem);
    PEDP_REQUIRE(N >= 0 && N <= MAX_POINTS, "%s: N = %lld, at most %lld points", who, (long long)N, (long long)MAX_POINTS);
    if (N == 0) return PEDP_OK;
    PEDP_REQUIRE(pts, "%s: null points", who);
    // the counter and the staging of a host-memory call are this call's own; a host-memory call also waits on the
    // context's stream, which a pending registration (pedp_icp_begin) owns until pedp_icp_end
    PEDP_REQUIRE(mem == PEDP_DEVICE || !c->icp_pending, "%s: a registration is pending on this context (host-memory call)", who);
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    int rc = PEDP_OK;
    const double *d_pts = pts;
    double *d_closest = closest, *d_dist = dist, *d_uv = uv;
    uint32_t *d_prim = prim_id;
    int8_t *d_side = side;
    const size_t n = (size_t)N;
    const size_t o_pts = 0, o_cl = o_pts + align256(24 * n), o_uv = o_cl + align256(24 * n), o_d = o_uv + align256(16 * n),
                 o_id = o_d + align256(8 * n), o_side = o_id + align256(4 * n), io_bytes = o_side + align256(n);
    if (mem == PEDP_HOST) {
        rc = c->closest_io.reserve(io_bytes);
        if (rc) return rc;
        char *io = (char *)c->closest_io.ptr;
        rc = pedp_upload(c, io + o_pts, pts, 24 * n);
        if (rc) return rc;
        d_pts = (const double *)(io + o_pts);
        d_closest = closest ? (double *)(io + o_cl) : nullptr;
        d_uv = uv ? (double *)(io + o_uv) : nullptr;
        d_dist = dist ? (double *)(io + o_d) : nullptr;
        d_prim = prim_id ? (uint32_t *)(io + o_id) : nullptr;
        d_side = side ? (int8_t *)(io + o_side) : nullptr;
    }
    rc = pedp_closest_launch(c, mesh, d_pts, N, d_closest, d_dist, d_prim, d_uv, d_side, nullptr);
    if (rc) return rc;
    if (mem == PEDP_HOST) {
        if (closest) rc = pedp_download(c, closest, d_closest, 24 * n);
        if (!rc && uv) rc = pedp_download(c, uv, d_uv, 16 * n);
        if (!rc && dist) rc = pedp_download(c, dist, d_dist, 8 * n);
        if (!rc && prim_id) rc = pedp_download(c, prim_id, d_prim, 4 * n);
        if (!rc && side) rc = pedp_download(c, side, d_side, n);
    }
    return rc;
}

}  // extern "C"
