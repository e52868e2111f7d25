// Ray stage, what a mesh handle holds: everything derived from the posed float32 vertices.
//   tri_setup_kernel             the AoS triangle records (v0, e1, e2, m = e2 x e1; PEDP_TRI_STRIDE floats), pad
//                                records all zero (det == 0: never hit)
//   pair_general_kernel          the same records pair-interleaved for the packed fp32 sweep (ray/sweep_packed.h):
//                                one aligned SGPR pair = (A.x, B.x) = one packed operand
//   cluster_sphere_kernel,       bounding spheres of CL_TRIS consecutive records and of every 64 such clusters
//   supercluster_sphere_kernel   (variant 3's cones, pedp_closest.hip's search)
//   pose_verts*_kernel           the posed vertices of a posable mesh
#pragma once
#include "mt.h"
#include "../mesh/cluster.h"

namespace {

// ------------------------------------------------------------------ mesh setup
__global__ void tri_setup_kernel(const float *__restrict__ verts, const uint32_t *__restrict__ tris,
                                 int64_t F, int64_t F_padded, float *__restrict__ rec) {
    int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F_padded) return;
    float *r = rec + f * PEDP_TRI_STRIDE;
    if (f >= F) {
#pragma unroll
        for (int k = 0; k < PEDP_TRI_STRIDE; ++k) r[k] = 0.0f;  // det == 0: can never be hit
        return;
    }
    const float *a = verts + 3 * (int64_t)tris[3 * f + 0];
    const float *b = verts + 3 * (int64_t)tris[3 * f + 1];
    const float *c = verts + 3 * (int64_t)tris[3 * f + 2];
    float e1[3], e2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        e1[k] = subr(b[k], a[k]);
        e2[k] = subr(c[k], a[k]);
        r[k] = a[k];
        r[3 + k] = e1[k];
        r[6 + k] = e2[k];
    }
    r[9] = fmar(e2[1], e1[2], -mulr(e2[2], e1[1]));  // m = e2 x e1
    r[10] = fmar(e2[2], e1[0], -mulr(e2[0], e1[2]));
    r[11] = fmar(e2[0], e1[1], -mulr(e2[1], e1[0]));
}

// ------------------------------------------------------------------ pair-interleaved records
constexpr int PAIR_GEN = 24;  // floats per pair record, general origin: v0 e1 e2 m
constexpr int PAIR_SH = 20;   // floats per pair record, shared origin:  a' b' c' kappa (pair_shared_kernel)

__global__ void pair_general_kernel(const float *__restrict__ aos, int64_t F_padded, float *__restrict__ out) {
    int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F_padded) return;
    const float *r = aos + f * PEDP_TRI_STRIDE;
    float *o = out + (f >> 1) * PAIR_GEN + (f & 1);
#pragma unroll
    for (int k = 0; k < 12; ++k) o[2 * k] = r[k];
}

// bounding sphere (center, radius) of each cluster's real triangles; radius < 0: empty
__global__ void cluster_sphere_kernel(const float *__restrict__ aos, int64_t F, int64_t n_clusters,
                                      float4 *__restrict__ sph) {
    int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_clusters) return;
    float lo[3] = {3e38f, 3e38f, 3e38f}, hi[3] = {-3e38f, -3e38f, -3e38f};
    int n = 0;
    for (int k = 0; k < CL_TRIS; ++k) {
        int64_t f = c * CL_TRIS + k;
        if (f >= F) break;
        const float *r = aos + f * PEDP_TRI_STRIDE;
        for (int a = 0; a < 3; ++a) {
            float p0 = r[a], p1 = r[a] + r[3 + a], p2 = r[a] + r[6 + a];
            lo[a] = fminf(lo[a], fminf(p0, fminf(p1, p2)));
            hi[a] = fmaxf(hi[a], fmaxf(p0, fmaxf(p1, p2)));
        }
        ++n;
    }
    if (n == 0) { sph[c] = make_float4(0.f, 0.f, 0.f, -1.f); return; }
    float cx = 0.5f * (lo[0] + hi[0]), cy = 0.5f * (lo[1] + hi[1]), cz = 0.5f * (lo[2] + hi[2]);
    float r2 = 0.f;
    for (int k = 0; k < n; ++k) {
        const float *r = aos + (c * CL_TRIS + k) * PEDP_TRI_STRIDE;
        for (int v = 0; v < 3; ++v) {
            float px = r[0] + (v ? r[3 * v] : 0.f) - cx, py = r[1] + (v ? r[3 * v + 1] : 0.f) - cy,
                  pz = r[2] + (v ? r[3 * v + 2] : 0.f) - cz;
            r2 = fmaxf(r2, px * px + py * py + pz * pz);
        }
    }
    // inflate: vertices re-derived from (v0, e1, e2) and fp32 accept decisions near the rim
    float rad = sqrtf(r2) * 1.001f + 1e-5f * (fabsf(cx) + fabsf(cy) + fabsf(cz)) + 1e-30f;
    sph[c] = make_float4(cx, cy, cz, rad);
}

// bounding sphere of 64 consecutive cluster spheres (one mask word of clusters): lets the cull
// kernel dismiss 1024 triangles with one test
// one wave per super-cluster, lane = cluster: min / max are order-free, so the result does not
// depend on the reduction shape
__global__ __launch_bounds__(256) void supercluster_sphere_kernel(const float4 *__restrict__ sph, int64_t n_clusters,
                                                                  int64_t n_super, float4 *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= n_super) return;  // wave-uniform
    const int64_t c = s * 64 + lane;
    const float4 q = c < n_clusters ? sph[c] : make_float4(0.f, 0.f, 0.f, -1.f);
    const bool live = q.w >= 0.f;
    float lo[3] = {live ? q.x - q.w : 3e38f, live ? q.y - q.w : 3e38f, live ? q.z - q.w : 3e38f};
    float hi[3] = {live ? q.x + q.w : -3e38f, live ? q.y + q.w : -3e38f, live ? q.z + q.w : -3e38f};
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            lo[k] = fminf(lo[k], __shfl_xor(lo[k], off, 64));
            hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], off, 64));
        }
    if (__builtin_amdgcn_ballot_w64(live) == 0ull) {
        if (lane == 0) out[s] = make_float4(0.f, 0.f, 0.f, -1.f);
        return;
    }
    const float cx = 0.5f * (lo[0] + hi[0]), cy = 0.5f * (lo[1] + hi[1]), cz = 0.5f * (lo[2] + hi[2]);
    const float dx = q.x - cx, dy = q.y - cy, dz = q.z - cz;
    float rad = live ? sqrtf(dx * dx + dy * dy + dz * dz) + q.w : 0.f;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) rad = fmaxf(rad, __shfl_xor(rad, off, 64));
    if (lane == 0)
        out[s] = make_float4(cx, cy, cz, rad * 1.0001f + 1e-6f * (fabsf(cx) + fabsf(cy) + fabsf(cz)) + 1e-30f);
}

// TriangleMesh.transform (pose_estimation.py:406-409, defect_projection.py:549-550) followed by
// from_legacy's float32 cast (defect_projection.py:245): Open3D forms T * (x, y, z, 1) in
// float64, divides by the fourth component and the tensor mesh stores float32.  One thread per
// vertex, fixed operation order ((T0 x + T1 y) + T2 z) + T3, no contraction.
struct Pose16 { double m[16]; };

__global__ void pose_verts_kernel(const double *__restrict__ v64, int64_t V, Pose16 T, int identity,
                                  float *__restrict__ v32) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= V) return;
    const double x = v64[3 * i], y = v64[3 * i + 1], z = v64[3 * i + 2];
    if (identity) {
        v32[3 * i] = (float)x;
        v32[3 * i + 1] = (float)y;
        v32[3 * i + 2] = (float)z;
        return;
    }
    double h[4];
    for (int r = 0; r < 4; ++r)
        h[r] = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(T.m[4 * r], x), __dmul_rn(T.m[4 * r + 1], y)),
                                   __dmul_rn(T.m[4 * r + 2], z)), T.m[4 * r + 3]);
    v32[3 * i] = (float)(h[0] / h[3]);
    v32[3 * i + 1] = (float)(h[1] / h[3]);
    v32[3 * i + 2] = (float)(h[2] / h[3]);
}

// the same T * (x, y, z, 1) / w in float64, kept as float64: what TriangleMesh.transform leaves in `vertices`
__global__ void pose_verts64_kernel(const double *__restrict__ v64, int64_t V, Pose16 T, double *__restrict__ out) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= V) return;
    const double x = v64[3 * i], y = v64[3 * i + 1], z = v64[3 * i + 2];
    double h[4];
    for (int r = 0; r < 4; ++r)
        h[r] = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(T.m[4 * r], x), __dmul_rn(T.m[4 * r + 1], y)),
                                   __dmul_rn(T.m[4 * r + 2], z)), T.m[4 * r + 3]);
    out[3 * i] = h[0] / h[3];
    out[3 * i + 1] = h[1] / h[3];
    out[3 * i + 2] = h[2] / h[3];
}

}  // namespace
