// ICP, per-cloud preparation: the spatial (Hilbert) order of a cloud with its chunk spheres, and the
// sorted target operand with its tile spheres.  Built once per cloud handle.
#pragma once
#include "common.h"

namespace {

// ------------------------------------------------------------------ spatial order of a cloud
// Stable sort by the Hilbert-curve index of the point's cell in a 65536^3 grid over the cloud's OWN
// bounding box: consecutive entries of `perm` are neighbours in space, so 128-point scene chunks and
// 16-point target tiles are compact and their bounding spheres are small.  Inside a cell the points
// keep ascending index (stable radix sort).  The order -- and with it the order of every float64 sum
// of a registration -- is a function of the cloud's data alone: not of the registration that first
// touched the handle, not of its start pose (round 2 laid 256^3 cells over the region the target
// could reach from the first start pose, so two handles of the same data could sum in different
// orders).  48 bits keep the cells far below the point spacing even when one stray point stretches
// the box a hundredfold.
// 3-D Hilbert index of cell (x, y, z), SORT_BITS bits per axis (Skilling, "Programming the
// Hilbert curve", 2004: axes -> transpose, then bit interleave).  Unlike Morton order, points
// that are consecutive along the curve are always neighbours in space, so no 128-point scene
// block or 16-point target tile straddles a long jump (such blocks would defeat the culling).
__device__ __forceinline__ unsigned long long hilbert3(unsigned x, unsigned y, unsigned z) {
    unsigned X[3] = {x, y, z};
    const unsigned M = 1u << (SORT_BITS - 1);
    for (unsigned Q = M; Q > 1; Q >>= 1) {
        const unsigned Pm = Q - 1;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            if (X[i] & Q) X[0] ^= Pm;
            else { const unsigned t = (X[0] ^ X[i]) & Pm; X[0] ^= t; X[i] ^= t; }
        }
    }
    X[1] ^= X[0];
    X[2] ^= X[1];
    unsigned t = 0;
    for (unsigned Q = M; Q > 1; Q >>= 1)
        if (X[2] & Q) t ^= Q - 1;
    X[0] ^= t; X[1] ^= t; X[2] ^= t;
    unsigned long long h = 0;
#pragma unroll
    for (int b = SORT_BITS - 1; b >= 0; --b)
        h = (h << 3) | (unsigned long long)((((X[0] >> b) & 1u) << 2) | (((X[1] >> b) & 1u) << 1) | ((X[2] >> b) & 1u));
    return h;
}
// Cell of point i; a point without a cell (a non-finite coordinate) goes to the extra bucket behind
// the curve.
__device__ __forceinline__ unsigned long long point_cell(const double *__restrict__ pts, int64_t i, double lox, double loy,
                                                         double loz, double sx, double sy, double sz) {
    const double fx = (pts[3 * i] - lox) * sx, fy = (pts[3 * i + 1] - loy) * sy, fz = (pts[3 * i + 2] - loz) * sz;
    const double top = (double)(1 << SORT_BITS);
    if (!pedp_row_finite(pts, i)) return 1ull << (3 * SORT_BITS);  // (bit test: this file is built with -fno-honor-nans)
    if (!(fx >= 0.0 && fx < top && fy >= 0.0 && fy < top && fz >= 0.0 && fz < top)) return 1ull << (3 * SORT_BITS);
    return hilbert3((unsigned)(int)fx, (unsigned)(int)fy, (unsigned)(int)fz);
}
// the box is read where it was made: on the device (lo xyz, hi xyz)
__global__ void cell_key_kernel(const double *__restrict__ pts, int64_t N, const double *__restrict__ box,
                                unsigned long long *__restrict__ key) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    double sc[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double ext = box[3 + k] - box[k];
        sc[k] = ext > 0.0 && isfinite(ext) ? (double)(1 << SORT_BITS) / ext * (1.0 - 1e-9) : 0.0;
    }
    key[i] = point_cell(pts, i, box[0], box[1], box[2], sc[0], sc[1], sc[2]);
}
// Bounding spheres (centre xyz, radius; float64, the cloud's own frame) of the eight runs of 16 consecutive
// points of every 128-point chunk of the spatial order: a rebuild pass of a registration asks the spheres,
// moved by the pose so far, which chunks can be near the target at all, and touches only those chunks'
// points.  (One sphere per chunk let through twice as many chunks as are live; with eight the workgroups of a
// rebuild pass mostly get one chunk each.)  One wave per chunk: lane = point of a half, 16 lanes = a run.
__global__ __launch_bounds__(64) void chunk_sphere_kernel(const double *__restrict__ pts, const int32_t *__restrict__ perm,
                                                          int64_t N, double *__restrict__ sph /* [chunk][8][4] */) {
    const int64_t chunk = blockIdx.x;
    const int lane = threadIdx.x;
    const double big = 1.7976931348623157e308;
    for (int h = 0; h < 2; ++h) {
        double lo[3] = {big, big, big}, hi[3] = {-big, -big, -big};
        const int64_t k = chunk * 128 + h * 64 + lane;
        if (k < N) {
            const int64_t i = perm[k];
            for (int c = 0; c < 3; ++c) lo[c] = hi[c] = pts[3 * i + c];
        }
        for (int c = 0; c < 3; ++c)
            for (int off = 8; off >= 1; off >>= 1) {
                const double l2 = __shfl_xor(lo[c], off, 64), h2 = __shfl_xor(hi[c], off, 64);
                lo[c] = l2 < lo[c] ? l2 : lo[c];
                hi[c] = h2 > hi[c] ? h2 : hi[c];
            }
        if ((lane & 15) == 0) {
            double *o = sph + ((chunk * 8) + h * 4 + (lane >> 4)) * 4;
            if (!(hi[0] >= lo[0])) {  // a run behind the cloud's last point: matches nothing
                o[0] = o[1] = o[2] = 0.0;
                o[3] = -1.0;
            } else {
                double m[3], r2 = 0.0;
                for (int c = 0; c < 3; ++c) {
                    m[c] = 0.5 * (lo[c] + hi[c]);
                    const double e = hi[c] - m[c];
                    r2 += e * e;
                }
                // non-finite coordinates give a non-finite sphere: such a chunk is never skipped
                o[0] = m[0]; o[1] = m[1]; o[2] = m[2];
                o[3] = sqrt(r2) * (1.0 + 1e-12) + 1e-300;
            }
        }
    }
}

// ------------------------------------------------------------------ target preparation
// Rows of a target that take part in the search: the finite ones (host statistics count them; they come first in
// the spatial order, the non-finite ones last).  A non-finite row is never a neighbour.
inline int64_t target_rows(pedp_cloud_t t) { return t->n_finite >= 0 ? t->n_finite : t->N; }

// Sorted target operand: row k holds point perm[k] as float4 (x', y', z', |t'|^2), centred on
// c; pad rows can never win.  One bounding sphere per 64-row unit (centred coordinates);
// radius < 0 marks a unit without real points.
__global__ void pack_target_kernel(const double *__restrict__ pts, const int32_t *__restrict__ perm, int64_t N,
                                   int64_t N_pad, double cx, double cy, double cz, float4 *__restrict__ out) {
    int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= N_pad) return;
    if (k >= N) { out[k] = make_float4(0.f, 0.f, 0.f, 1e30f); return; }
    const int64_t i = perm[k];
    float x = (float)(pts[3 * i] - cx), y = (float)(pts[3 * i + 1] - cy), z = (float)(pts[3 * i + 2] - cz);
    double w = (double)x * x + (double)y * y + (double)z * z;
    out[k] = make_float4(x, y, z, (float)w);
}
// sorted float64 rows of the target (row k = point perm[k]): x y z nx ny nz, so that the exact
// re-scoring reads a candidate row -- and with it what the winner contributes to the sums -- with
// one contiguous 48-byte load instead of perm -> point -> normal
__global__ void sort_rows_kernel(const double *__restrict__ pts, const double *__restrict__ nrm, const int32_t *__restrict__ perm,
                                 int64_t N, int64_t N_pad, double *__restrict__ out) {
    int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= N_pad) return;
    const bool real = k < N;
    const int64_t i = real ? perm[k] : 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        out[6 * k + c] = real ? pts[3 * i + c] : 0.0;
        out[6 * k + 3 + c] = real && nrm ? nrm[3 * i + c] : 0.0;
    }
}
__global__ void tile_sphere_kernel(const float4 *__restrict__ t4, int64_t N, int64_t n_units_all, int UNIT_ROWS,
                                   float4 *__restrict__ sph) {
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_units_all) return;
    float lo[3] = {3e38f, 3e38f, 3e38f}, hi[3] = {-3e38f, -3e38f, -3e38f};
    int n = 0;
    for (int r = 0; r < UNIT_ROWS; ++r) {
        int64_t k = t * UNIT_ROWS + r;
        if (k >= N) break;
        const float4 p = t4[k];
        lo[0] = fminf(lo[0], p.x); hi[0] = fmaxf(hi[0], p.x);
        lo[1] = fminf(lo[1], p.y); hi[1] = fmaxf(hi[1], p.y);
        lo[2] = fminf(lo[2], p.z); hi[2] = fmaxf(hi[2], p.z);
        ++n;
    }
    if (n == 0) { sph[t] = make_float4(0.f, 0.f, 0.f, -1.f); return; }
    const float cx = 0.5f * (lo[0] + hi[0]), cy = 0.5f * (lo[1] + hi[1]), cz = 0.5f * (lo[2] + hi[2]);
    float r2 = 0.f;
    for (int r = 0; r < n; ++r) {
        const float4 p = t4[t * UNIT_ROWS + r];
        const float dx = p.x - cx, dy = p.y - cy, dz = p.z - cz;
        r2 = fmaxf(r2, dx * dx + dy * dy + dz * dz);
    }
    sph[t] = make_float4(cx, cy, cz, sqrtf(r2) * 1.0001f + 1e-6f * (fabsf(cx) + fabsf(cy) + fabsf(cz)) + 1e-30f);
}

}  // namespace
