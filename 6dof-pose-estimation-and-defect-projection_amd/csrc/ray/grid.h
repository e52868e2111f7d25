// Ray stage, variant 4: the triangle-driven sweep over a grid of ray directions (the auto choice from 16,384 rays,
// and what a resident ray set keeps built).
#pragma once
#include "mt.h"

namespace {

// ------------------------------------------------------------------ sweep, triangle-driven (variant 4)
// All rays leave one origin O, so a triangle is seen under one fixed solid angle.  Take a frame
// (A, E1, E2) with A = the mean direction of eight rays spread over the array, map every ray to p = (d.E1, d.E2) / d.A (the
// plane at unit distance along A: straight lines stay straight, so a triangle in front of O maps
// to the triangle of its mapped corners) and lay a grid of about N cells over the rays' bounding
// rectangle.  Rays are threaded into per-cell chains (head[cell] -> node -> node ...; a node is the
// ray's direction + the next index, the node index IS the ray index, nothing is sorted or moved).
// Then the TRIANGLES drive the sweep: a thread per triangle maps the three corners, takes their
// bounding rectangle widened by a margin (an eighth of a cell + sixteen times the dilation the fp32
// test's own rounding can give the triangle) and applies the oracle's exact test to the rays in those cells --
// the same mt_eval / mt_accept / mt_key on the same (ray, triangle) operands as the exhaustive
// sweep, met in the same 64-bit atomicMin, so t, primitive ids and (u, v) are the same bits.
// Every ray x triangle pair is still accounted for: a ray can only hit a triangle whose mapped
// rectangle holds the ray's point.  Work per cast is O(N + F + covered cells) instead of O(N x F).
//
//   rast_bounds_kernel   origins equal? rays inside the frame's half space (d.A > 0.17 |d|)?
//                        bounds of p; clears keys and chain heads
//   rast_insert_kernel   grid from the bounds; node[i] = (d_i, atomicExch(head[cell_i], i))
//   rast_tri_kernel      triangle per thread: up to RAST_INLINE cells walked by the thread itself,
//                        larger rectangles cut into tiles of RAST_TILE x RAST_TILE cells
//   rast_item_kernel     a wave per item, a cell per lane
// Whatever the grid cannot answer -- origins differ, a ray outside the half space, more than
// RAST_CHAIN_MAX rays in one cell, a full item table -- clears hdr.ok on the device, and the last
// kernel of the cast (ray_finalize_kernel) then runs the general exhaustive loop for every ray before
// it writes the results; the status reaches the host through a pinned word and the next cast of the
// same ray count takes the cone culling of variant 3 instead.  A triangle that comes within eps of
// the plane through O perpendicular to A has no bounded image: it is tested against every cell.
constexpr unsigned RAST_NONE = 0xFFFFFFFFu;
constexpr int RAST_INLINE = 16;
constexpr int RAST_TILE = 16;          // larger rectangles are cut into tiles of 16 x 16 cells, one wave each
constexpr int RAST_ITEM_CAP = 1 << 18;
constexpr int RAST_CHAIN_MAX = 64;
constexpr float RAST_COS_MIN = 0.17f;
constexpr int RAST_ITEM_WAVES = 2048;
constexpr int RAST_FULL_CAP = 8192;     // triangles without a bounded image that one cast can list

struct RastHdr {  // two per context (used in turn), device memory; ray_finalize_kernel puts the other one back to its start values
    int ok;       // 1: the grid answers this cast; 0: the exhaustive loop in ray_finalize_kernel does
    int n_items;
    int reason;   // why ok was cleared: 1 origins differ, 2 ray outside the half space, 4 chain too long, 8 item table full
    int n_full;   // triangles without a bounded image (listed; rast_full_kernel tests them against every ray)
    float O[3], A[3], E1[3], E2[3];
    float u0, v0, su, sv;
    int GX, GY;
};
struct RastItem { int tri, x0, y0, w, h, pad0, pad1, pad2; };

struct RastFrame { float A[3], E1[3], E2[3]; bool valid; };

__device__ __forceinline__ RastFrame rast_frame(const float *__restrict__ rays6, int64_t N) {
    // A = the mean of eight rays spread over the array (k (N - 1) / 7: first, last and six between them;
    // for a row-major pixel grid they fall on different columns, so A points near the middle of the view)
    float sx = 0.f, sy = 0.f, sz = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int64_t i = (N - 1) * k / 7;
        const float dx = rays6[6 * i + 3], dy = rays6[6 * i + 4], dz = rays6[6 * i + 5];
        const float l2 = dx * dx + dy * dy + dz * dz;
        if (l2 > 1e-30f && l2 < 1e30f) {
            const float inv = 1.0f / sqrtf(l2);
            sx += dx * inv; sy += dy * inv; sz += dz * inv;
        }
    }
    const float l2 = sx * sx + sy * sy + sz * sz;
    RastFrame f;
    f.valid = l2 > 1e-6f;
    const float inv = 1.0f / sqrtf(f.valid ? l2 : 1.0f);
    f.A[0] = sx * inv; f.A[1] = sy * inv; f.A[2] = sz * inv;
    const float ax = fabsf(f.A[0]), ay = fabsf(f.A[1]), az = fabsf(f.A[2]);
    float ex = 0.f, ey = 0.f, ez = 0.f;
    if (ax <= ay && ax <= az) ex = 1.f; else if (ay <= az) ey = 1.f; else ez = 1.f;
    float cx = ey * f.A[2] - ez * f.A[1], cy = ez * f.A[0] - ex * f.A[2], cz = ex * f.A[1] - ey * f.A[0];
    const float ci = 1.0f / sqrtf(fmaxf(cx * cx + cy * cy + cz * cz, 1e-30f));
    f.E1[0] = cx * ci; f.E1[1] = cy * ci; f.E1[2] = cz * ci;
    f.E2[0] = f.A[1] * f.E1[2] - f.A[2] * f.E1[1];
    f.E2[1] = f.A[2] * f.E1[0] - f.A[0] * f.E1[2];
    f.E2[2] = f.A[0] * f.E1[1] - f.A[1] * f.E1[0];
    return f;
}

// 0: no direction (zero or NaN: such a ray hits nothing in the exhaustive sweep either), 1: mapped, 2: outside the half space
__device__ __forceinline__ int rast_map(float dx, float dy, float dz, const float *A, const float *E1, const float *E2,
                                        float &u, float &v) {
    const float l2 = dx * dx + dy * dy + dz * dz;
    if (!(l2 > 0.f)) return 0;            // zero, or NaN
    if (!(l2 < 3e38f)) return 2;          // infinite components: leave them to the exhaustive sweep
    const float w = dx * A[0] + dy * A[1] + dz * A[2];
    if (!(w * fabsf(w) > RAST_COS_MIN * RAST_COS_MIN * l2)) return 2;
    const float iw = 1.0f / w;
    u = (dx * E1[0] + dy * E1[1] + dz * E1[2]) * iw;
    v = (dx * E2[0] + dy * E2[1] + dz * E2[2]) * iw;
    return 1;
}

constexpr int RAST_BBLOCKS = 256;   // workgroups of rast_bounds_kernel = partial bounds the insert kernel folds
constexpr int RAST_BUNROLL = 4;

__global__ __launch_bounds__(256) void rast_bounds_kernel(const float *__restrict__ rays6, int64_t N, RastHdr *__restrict__ h,
                                                         unsigned long long *__restrict__ keys, unsigned *__restrict__ head,
                                                         uint4 *__restrict__ part) {
    const RastFrame f = rast_frame(rays6, N);
    const unsigned ox = __float_as_uint(rays6[0]), oy = __float_as_uint(rays6[1]), oz = __float_as_uint(rays6[2]);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { h->O[k] = rays6[k]; h->A[k] = f.A[k]; h->E1[k] = f.E1[k]; h->E2[k] = f.E2[k]; }
        if (!f.valid) { atomicAnd(&h->ok, 0); atomicOr(&h->reason, 2); }
    }
    unsigned lo_u = 0xFFFFFFFFu, hi_u = 0u, lo_v = 0xFFFFFFFFu, hi_v = 0u;
    int bad = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i0 < N; i0 += RAST_BUNROLL * stride) {
        float r[RAST_BUNROLL][6];
#pragma unroll
        for (int k = 0; k < RAST_BUNROLL; ++k) {  // all loads of the trip first
            const int64_t i = i0 + k * stride < N ? i0 + k * stride : i0;
#pragma unroll
            for (int c = 0; c < 6; ++c) r[k][c] = rays6[6 * i + c];
        }
#pragma unroll
        for (int k = 0; k < RAST_BUNROLL; ++k) {
            const int64_t i = i0 + k * stride;
            if (i >= N) break;
            keys[i] = KEY_MISS;
            head[i] = RAST_NONE;
            if (__float_as_uint(r[k][0]) != ox || __float_as_uint(r[k][1]) != oy || __float_as_uint(r[k][2]) != oz) bad |= 1;
            float u, v;
            const int kind = rast_map(r[k][3], r[k][4], r[k][5], f.A, f.E1, f.E2, u, v);
            if (kind == 2) bad |= 2;
            if (kind == 1) {
                const unsigned eu = enc_f(u), ev = enc_f(v);
                lo_u = eu < lo_u ? eu : lo_u; hi_u = eu > hi_u ? eu : hi_u;
                lo_v = ev < lo_v ? ev : lo_v; hi_v = ev > hi_v ? ev : hi_v;
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        unsigned t;
        t = __shfl_xor(lo_u, off, 64); lo_u = t < lo_u ? t : lo_u;
        t = __shfl_xor(hi_u, off, 64); hi_u = t > hi_u ? t : hi_u;
        t = __shfl_xor(lo_v, off, 64); lo_v = t < lo_v ? t : lo_v;
        t = __shfl_xor(hi_v, off, 64); hi_v = t > hi_v ? t : hi_v;
        bad |= __shfl_xor(bad, off, 64);
    }
    __shared__ unsigned red[4][4];
    __shared__ int badw[4];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[wave][0] = lo_u; red[wave][1] = hi_u; red[wave][2] = lo_v; red[wave][3] = hi_v; badw[wave] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            lo_u = red[w][0] < lo_u ? red[w][0] : lo_u; hi_u = red[w][1] > hi_u ? red[w][1] : hi_u;
            lo_v = red[w][2] < lo_v ? red[w][2] : lo_v; hi_v = red[w][3] > hi_v ? red[w][3] : hi_v;
            bad |= badw[w];
        }
        part[blockIdx.x] = make_uint4(lo_u, hi_u, lo_v, hi_v);
        if (bad) { atomicAnd(&h->ok, 0); atomicOr(&h->reason, bad); }
    }
}

// fold of the RAST_BBLOCKS partial bounds; every workgroup that needs the grid does it for itself
__device__ __forceinline__ void rast_fold_bounds(const uint4 *__restrict__ part, unsigned *bnd /* LDS, 4 words */) {
    __shared__ unsigned fred[4][4];
    unsigned lo_u = 0xFFFFFFFFu, hi_u = 0u, lo_v = 0xFFFFFFFFu, hi_v = 0u;
    for (int k = threadIdx.x; k < RAST_BBLOCKS; k += blockDim.x) {
        const uint4 q = part[k];
        lo_u = q.x < lo_u ? q.x : lo_u; hi_u = q.y > hi_u ? q.y : hi_u;
        lo_v = q.z < lo_v ? q.z : lo_v; hi_v = q.w > hi_v ? q.w : hi_v;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        unsigned t;
        t = __shfl_xor(lo_u, off, 64); lo_u = t < lo_u ? t : lo_u;
        t = __shfl_xor(hi_u, off, 64); hi_u = t > hi_u ? t : hi_u;
        t = __shfl_xor(lo_v, off, 64); lo_v = t < lo_v ? t : lo_v;
        t = __shfl_xor(hi_v, off, 64); hi_v = t > hi_v ? t : hi_v;
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { fred[wave][0] = lo_u; fred[wave][1] = hi_u; fred[wave][2] = lo_v; fred[wave][3] = hi_v; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) {
            lo_u = fred[w][0] < lo_u ? fred[w][0] : lo_u; hi_u = fred[w][1] > hi_u ? fred[w][1] : hi_u;
            lo_v = fred[w][2] < lo_v ? fred[w][2] : lo_v; hi_v = fred[w][3] > hi_v ? fred[w][3] : hi_v;
        }
        bnd[0] = lo_u; bnd[1] = hi_u; bnd[2] = lo_v; bnd[3] = hi_v;
    }
    __syncthreads();
}

struct RastGrid { float u0, v0, su, sv; int GX, GY; };

// the grid over [u0, u1] x [v0, v1]: about one cell per ray, never finer than 1e-4 (the mapped
// coordinates carry ~1e-7 of rounding)
__device__ __forceinline__ RastGrid rast_grid(const unsigned *bnd, int64_t N) {
    RastGrid g;
    const bool any = bnd[0] <= bnd[1] && bnd[2] <= bnd[3];
    const float u0 = any ? dec_f(bnd[0]) : 0.f, u1 = any ? dec_f(bnd[1]) : 0.f;
    const float v0 = any ? dec_f(bnd[2]) : 0.f, v1 = any ? dec_f(bnd[3]) : 0.f;
    const float du = fmaxf(u1 - u0, 1e-6f), dv = fmaxf(v1 - v0, 1e-6f);
    const float aspect = fminf(fmaxf(du / dv, 1.0f / 64.0f), 64.0f);
    const float n = (float)(N < (int64_t)1 << 30 ? N : (int64_t)1 << 30);
    float gx = floorf(sqrtf(n * aspect));
    gx = fminf(fmaxf(gx, 1.0f), fminf(n, du * 1e4f + 1.0f));
    float gy = floorf(n / gx);
    gy = fminf(fmaxf(gy, 1.0f), dv * 1e4f + 1.0f);
    g.GX = (int)gx; g.GY = (int)gy;
    g.u0 = u0; g.v0 = v0;
    g.su = gx / du; g.sv = gy / dv;
    return g;
}

__device__ __forceinline__ int rast_clampi(float x, int hi) {  // floor(x) clamped to [0, hi]
    const float c = fminf(fmaxf(floorf(x), 0.0f), (float)hi);
    return (int)c;
}

__global__ __launch_bounds__(256) void rast_insert_kernel(const float *__restrict__ rays6, int64_t N, RastHdr *__restrict__ h,
                                                         unsigned *__restrict__ head, float4 *__restrict__ nodes,
                                                         const uint4 *__restrict__ part) {
    if (h->ok == 0) return;
    __shared__ unsigned bnd[4];
    rast_fold_bounds(part, bnd);
    const RastGrid g = rast_grid(bnd, N);
    if (blockIdx.x == 0 && threadIdx.x == 0) { h->u0 = g.u0; h->v0 = g.v0; h->su = g.su; h->sv = g.sv; h->GX = g.GX; h->GY = g.GY; }
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float dx = rays6[6 * i + 3], dy = rays6[6 * i + 4], dz = rays6[6 * i + 5];
    float A[3], E1[3], E2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { A[k] = h->A[k]; E1[k] = h->E1[k]; E2[k] = h->E2[k]; }
    float u, v;
    if (rast_map(dx, dy, dz, A, E1, E2, u, v) != 1) return;
    const int cx = rast_clampi((u - g.u0) * g.su, g.GX - 1), cy = rast_clampi((v - g.v0) * g.sv, g.GY - 1);
    const unsigned nxt = atomicExch(&head[(size_t)cy * g.GX + cx], (unsigned)i);
    nodes[i] = make_float4(dx, dy, dz, __uint_as_float(nxt));
}

// the rays of one chain against one triangle
__device__ __forceinline__ void rast_fail(RastHdr *h, int why) {
    atomicAnd(&h->ok, 0);
    atomicOr(&h->reason, why);
}

template <class Sink>
__device__ __forceinline__ void rast_test(const float4 nd, unsigned ray, const float *O, const TriRec &q, unsigned f,
                                          const Sink &sink) {
    Ray r;
    r.ox = O[0]; r.oy = O[1]; r.oz = O[2];
    r.dx = nd.x; r.dy = nd.y; r.dz = nd.z;
    const MT m = mt_eval(r, q);
    if (mt_accept(m)) sink.one(ray, m, f);
}

// The cells of the rays that can meet triangle q (origin O, frame A/E1/E2, grid u0/v0/su/sv, GX x GY): the
// bounding rectangle of its mapped corners, widened by a margin that is PROVEN to hold every ray the oracle's
// fp32 test accepts (DESIGN s4.1 "Margin": derivation; tests/test_ray_gpu.py::test_grid_margin_* measure it).
//   An accepted ray has, in exact arithmetic on the stored operands, barycentric coordinates no farther outside
//   the triangle than the roundings of un, vn, det allow: with u = 2^-24, s = O - v0, L the longest edge, m = e2 x e1
//   its exact hit point lies within  6.5 u (3 |s| + L) L^2 / (|m| cos theta_d) + 2.1 u L  of the triangle; mapped
//   to the plane at unit distance along A (a point at depth w, off axis by |p|, moves by (1 + |p|) / w per unit)
//   and with cos theta_d |P - O| = |s . m| / |m| that is at most
//       u c_a [6.5 (3 |s| + L) L^2 + 2.1 L |m|] / |s . m|,     c_a = (1 + |p|) sqrt(1 + |p|^2),
//   |p| taken at its largest over the rectangle.  TWICE that is used, plus 64 u (1 + |p|^2) for the roundings of
//   the two mappings (ray and corners) and an eighth of a cell for the cell arithmetic.  The margin is never cut
//   off (round 2 capped it at 64 cells).  A triangle seen so nearly edge-on that s . m is rounding (the origin
//   within ~1e-6 rad of its plane) has no bounded image, like one that reaches the plane through O: such triangles
//   are LISTED and tested against every ray by rast_full_kernel.  m == 0 exactly: det is 0 for every ray, nothing
//   can be accepted.
struct RastRect { float fx0, fx1, fy0, fy1, mx, my; int full; };  // unwidened rectangle in cell units, the margins, "every cell"
__device__ __forceinline__ bool rast_rect(const TriRec &q, const float *O, const float *A, const float *E1, const float *E2,
                                          float u0, float v0, float su, float sv, int GX, int GY, int &x0, int &x1, int &y0,
                                          int &y1, RastRect &rr) {
    // corners relative to O (v1, v2 re-derived from the record's edges: one more rounding, far below the margins)
    float X[3][3];
    X[0][0] = q.v0x - O[0]; X[0][1] = q.v0y - O[1]; X[0][2] = q.v0z - O[2];
    X[1][0] = X[0][0] + q.e1x; X[1][1] = X[0][1] + q.e1y; X[1][2] = X[0][2] + q.e1z;
    X[2][0] = X[0][0] + q.e2x; X[2][1] = X[0][1] + q.e2y; X[2][2] = X[0][2] + q.e2z;
    float wmin = 3e38f, wmax = -3e38f, scale = fabsf(O[0]) + fabsf(O[1]) + fabsf(O[2]);
    float pu[3], pv[3], pw[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        pw[k] = X[k][0] * A[0] + X[k][1] * A[1] + X[k][2] * A[2];
        pu[k] = X[k][0] * E1[0] + X[k][1] * E1[1] + X[k][2] * E1[2];
        pv[k] = X[k][0] * E2[0] + X[k][1] * E2[1] + X[k][2] * E2[2];
        wmin = fminf(wmin, pw[k]); wmax = fmaxf(wmax, pw[k]);
        scale = fmaxf(scale, fabsf(X[k][0]) + fabsf(X[k][1]) + fabsf(X[k][2]));
    }
    const float eps = 1e-5f * scale;
    bool live = !(wmax < -eps);  // wholly behind the plane through O: t . (d.A) = w > 0 is impossible
    if (q.mx == 0.0f && q.my == 0.0f && q.mz == 0.0f) live = false;  // det = d . m == 0 for every ray
    x0 = 0; x1 = GX - 1; y0 = 0; y1 = GY - 1;
    rr.fx0 = 0.f; rr.fx1 = (float)GX; rr.fy0 = 0.f; rr.fy1 = (float)GY; rr.mx = rr.my = 0.f; rr.full = 1;
    if ((wmin > eps) && (scale < 3e38f)) {  // otherwise it reaches the plane (or has a NaN / infinite corner): no bounded image
        float umin = 3e38f, umax = -3e38f, vmin = 3e38f, vmax = -3e38f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float iw = 1.0f / pw[k];
            const float a = pu[k] * iw, b = pv[k] * iw;
            umin = fminf(umin, a); umax = fmaxf(umax, a);
            vmin = fminf(vmin, b); vmax = fmaxf(vmax, b);
        }
        const float l1 = sqrtf(q.e1x * q.e1x + q.e1y * q.e1y + q.e1z * q.e1z), l2 = sqrtf(q.e2x * q.e2x + q.e2y * q.e2y + q.e2z * q.e2z);
        const float gx = q.e2x - q.e1x, gy = q.e2y - q.e1y, gz = q.e2z - q.e1z;
        const float L = fmaxf(fmaxf(l1, l2), sqrtf(gx * gx + gy * gy + gz * gz));
        const float ls = sqrtf(X[0][0] * X[0][0] + X[0][1] * X[0][1] + X[0][2] * X[0][2]);
        const float lm = sqrtf(q.mx * q.mx + q.my * q.my + q.mz * q.mz);
        const float sm = fabsf(X[0][0] * q.mx + X[0][1] * q.my + X[0][2] * q.mz);
        const float pa = fmaxf(fabsf(umin), fabsf(umax)), pb = fmaxf(fabsf(vmin), fabsf(vmax));
        const float pm2 = (pa * pa + pb * pb) * 1.01f + 1e-6f, pm = sqrtf(pm2);
        const float ca = (1.0f + pm) * sqrtf(1.0f + pm2);
        const float U = 5.9604645e-8f;
        const float dil = 2.0f * U * ca * (6.5f * (3.0f * ls + L) * L * L + 2.1f * L * lm) / fmaxf(sm, 1e-37f) + 64.0f * U * (1.0f + pm2);
        // (s . m itself carries up to 4 u |s| |m| of rounding: below sixteen times u |s| |m| it says nothing -- the
        // triangle has no bounded image; above, it is within a third of the exact value, which the factor two absorbs)
        if (sm > 16.0f * U * ls * lm && dil * su < 1e9f && dil * sv < 1e9f) {  // (false for NaN / inf too)
            const float mx_ = 0.125f + dil * su, my_ = 0.125f + dil * sv;
            rr.fx0 = (umin - u0) * su; rr.fx1 = (umax - u0) * su; rr.fy0 = (vmin - v0) * sv; rr.fy1 = (vmax - v0) * sv;
            rr.mx = mx_; rr.my = my_; rr.full = 0;
            const float fx0 = rr.fx0 - mx_, fx1 = rr.fx1 + mx_, fy0 = rr.fy0 - my_, fy1 = rr.fy1 + my_;
            if (!(fx1 >= 0.0f) || !(fy1 >= 0.0f) || !(fx0 < (float)GX) || !(fy0 < (float)GY)) live = false;  // beside the rays' rectangle
            x0 = rast_clampi(fx0, GX - 1); x1 = rast_clampi(fx1, GX - 1);
            y0 = rast_clampi(fy0, GY - 1); y1 = rast_clampi(fy1, GY - 1);
        }
    }
    return live;
}

// diagnostics (pedp_debug_rast_rects): the rectangle of every triangle and the continuous cell coordinates of every ray
__global__ void rast_debug_tri_kernel(const float *__restrict__ aos, int64_t F, const RastHdr *__restrict__ h, float *__restrict__ out) {
    const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const float *rec = aos + f * PEDP_TRI_STRIDE;
    const TriRec q = {rec[0], rec[1], rec[2], rec[3], rec[4], rec[5], rec[6], rec[7], rec[8], rec[9], rec[10], rec[11]};
    float O[3], A[3], E1[3], E2[3];
    for (int k = 0; k < 3; ++k) { O[k] = h->O[k]; A[k] = h->A[k]; E1[k] = h->E1[k]; E2[k] = h->E2[k]; }
    int x0, x1, y0, y1;
    RastRect rr;
    const bool live = rast_rect(q, O, A, E1, E2, h->u0, h->v0, h->su, h->sv, h->GX, h->GY, x0, x1, y0, y1, rr);
    float *o = out + 12 * f;
    o[0] = live ? 1.f : 0.f; o[1] = (float)rr.full; o[2] = rr.fx0; o[3] = rr.fx1; o[4] = rr.fy0; o[5] = rr.fy1; o[6] = rr.mx; o[7] = rr.my;
    o[8] = (float)x0; o[9] = (float)x1; o[10] = (float)y0; o[11] = (float)y1;
}
__global__ void rast_debug_ray_kernel(const float *__restrict__ rays6, int64_t N, const RastHdr *__restrict__ h, float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    float A[3], E1[3], E2[3], u = 0.f, v = 0.f;
    for (int k = 0; k < 3; ++k) { A[k] = h->A[k]; E1[k] = h->E1[k]; E2[k] = h->E2[k]; }
    const int kind = rast_map(rays6[6 * i + 3], rays6[6 * i + 4], rays6[6 * i + 5], A, E1, E2, u, v);
    out[3 * i] = (float)kind; out[3 * i + 1] = (u - h->u0) * h->su; out[3 * i + 2] = (v - h->v0) * h->sv;
}

// (Sink, here and in the two kernels below: what an accepted pair is handed to -- HitMin for a cast, ray/all_hits.h's
// for the all-hits queries, which need every pair met ONCE: DESIGN s4.24 names the lines that see to it)
template <class Sink>
__global__ __launch_bounds__(256) void rast_tri_kernel(const float *__restrict__ aos, int64_t F, RastHdr *__restrict__ h,
                                                      const unsigned *__restrict__ head, const float4 *__restrict__ nodes,
                                                      RastItem *__restrict__ items, Sink sink,
                                                      unsigned *__restrict__ full_list) {
    if (h->ok == 0) return;
    const int lane = threadIdx.x & 63;
    const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t fl = f < F ? f : F - 1;  // tail lanes re-run the last triangle and drop it below
    const float *rec = aos + fl * PEDP_TRI_STRIDE;
    const TriRec q = {rec[0], rec[1], rec[2], rec[3], rec[4], rec[5], rec[6], rec[7], rec[8], rec[9], rec[10], rec[11]};
    float O[3], A[3], E1[3], E2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { O[k] = h->O[k]; A[k] = h->A[k]; E1[k] = h->E1[k]; E2[k] = h->E2[k]; }
    const int GX = h->GX, GY = h->GY;
    const float u0 = h->u0, v0 = h->v0, su = h->su, sv = h->sv;
    int x0, x1, y0, y1;
    RastRect rr;
    bool live = rast_rect(q, O, A, E1, E2, u0, v0, su, sv, GX, GY, x0, x1, y0, y1, rr) && f < F;
    if (live && rr.full) {  // no bounded image: every ray, by the kernel made for that (a handful of silhouette triangles)
        const int at = atomicAdd(&h->n_full, 1);
        if (at < RAST_FULL_CAP) full_list[at] = (unsigned)f;
        else rast_fail(h, 8);
        live = false;
    }
    const int w = x1 - x0 + 1, hh = y1 - y0 + 1;
    const long long ncell = live ? (long long)w * hh : 0;
    // larger rectangles: cut into tiles of RAST_TILE x RAST_TILE cells.  One reservation in the item
    // table per wave (exclusive scan of the lanes' tile counts), the tiles written by the whole wave.
    const bool big = ncell > RAST_INLINE;
    unsigned long long bigm = __builtin_amdgcn_ballot_w64(big);
    if (bigm != 0ull) {  // wave-uniform
        const int ntx_l = (w + RAST_TILE - 1) / RAST_TILE, nty_l = (hh + RAST_TILE - 1) / RAST_TILE;
        const int n_l = big ? ntx_l * nty_l : 0;  // <= (N / 256 + ...) tiles: fits an int
        int incl = n_l;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_up(incl, off, 64);
            if (lane >= off) incl += o;
        }
        const int total = __shfl(incl, 63, 64);
        int base = 0;
        if (lane == 0) base = atomicAdd(&h->n_items, total);
        base = __shfl(base, 0, 64);
        if ((long long)base + total > RAST_ITEM_CAP) {
            if (lane == 0) rast_fail(h, 8);
            bigm = 0ull;
        }
        const int mine = base + incl - n_l;
        while (bigm != 0ull) {
            const int src = __builtin_ctzll(bigm);
            bigm &= bigm - 1ull;
            const int tf = __shfl((int)fl, src, 64), tx0 = __shfl(x0, src, 64), ty0 = __shfl(y0, src, 64);
            const int tw = __shfl(w, src, 64), th = __shfl(hh, src, 64), at = __shfl(mine, src, 64);
            const int ntx = __shfl(ntx_l, src, 64), n = __shfl(n_l, src, 64);
            for (int j = lane; j < n; j += 64) {
                const int ty = j / ntx, tx = j - ty * ntx;
                RastItem it;
                it.tri = tf;
                it.x0 = tx0 + tx * RAST_TILE; it.y0 = ty0 + ty * RAST_TILE;
                it.w = (tx0 + tw - it.x0) < RAST_TILE ? (tx0 + tw - it.x0) : RAST_TILE;
                it.h = (ty0 + th - it.y0) < RAST_TILE ? (ty0 + th - it.y0) : RAST_TILE;
                it.pad0 = it.pad1 = it.pad2 = 0;
                items[at + j] = it;
            }
        }
    }
    if (ncell == 0 || ncell > RAST_INLINE) return;
    const int nc = (int)ncell;
    constexpr int U = 8;  // cells in flight: all their heads are requested first, then the nodes side by side
    for (int c0 = 0; c0 < nc; c0 += U) {
        unsigned idx[U];
#pragma unroll
        for (int j = 0; j < U; ++j) {
            const int c = c0 + j;
            const int yy = c / w, xx = c - yy * w;
            idx[j] = c < nc ? head[(size_t)(y0 + yy) * GX + (x0 + xx)] : RAST_NONE;
        }
        int steps = 0;
        for (;;) {
            unsigned all = idx[0];
#pragma unroll
            for (int j = 1; j < U; ++j) all &= idx[j];
            if (all == RAST_NONE) break;
            float4 nd[U];
#pragma unroll
            for (int j = 0; j < U; ++j) nd[j] = nodes[idx[j] != RAST_NONE ? idx[j] : 0u];
#pragma unroll
            for (int j = 0; j < U; ++j)
                if (idx[j] != RAST_NONE) {
                    rast_test(nd[j], idx[j], O, q, (unsigned)f, sink);
                    idx[j] = __float_as_uint(nd[j].w);
                }
            if (++steps > RAST_CHAIN_MAX) { rast_fail(h, 4); break; }
        }
    }
}

// The listed triangles (no bounded image) against EVERY ray: a thread per ray, the records through scalar loads.
template <class Sink>
__global__ __launch_bounds__(256) void rast_full_kernel(const float *__restrict__ aos, const float *__restrict__ rays6, int64_t N,
                                                       const RastHdr *__restrict__ h, const unsigned *__restrict__ full_list,
                                                       Sink sink) {
    if (h->ok == 0) return;
    const int n = h->n_full < RAST_FULL_CAP ? h->n_full : RAST_FULL_CAP;
    if (n == 0) return;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    Ray r;
    r.ox = rays6[6 * i]; r.oy = rays6[6 * i + 1]; r.oz = rays6[6 * i + 2];
    r.dx = rays6[6 * i + 3]; r.dy = rays6[6 * i + 4]; r.dz = rays6[6 * i + 5];
    typename Sink::Acc acc = sink.start();
    for (int k = 0; k < n; ++k) {
        const unsigned f = full_list[k];  // wave-uniform
        const MT m = mt_eval(r, aos + (size_t)f * PEDP_TRI_STRIDE);
        if (mt_accept(m)) sink.gather(acc, i, m, f);
    }
    sink.finish(acc, i);
}

template <class Sink>
__global__ __launch_bounds__(256) void rast_item_kernel(const float *__restrict__ aos, RastHdr *__restrict__ h,
                                                       const unsigned *__restrict__ head, const float4 *__restrict__ nodes,
                                                       const RastItem *__restrict__ items, Sink sink) {
    if (h->ok == 0) return;
    const int n_items = h->n_items < RAST_ITEM_CAP ? h->n_items : RAST_ITEM_CAP;
    const int lane = threadIdx.x & 63;
    const int wave0 = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), n_waves = gridDim.x * (blockDim.x >> 6);
    float O[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) O[k] = h->O[k];
    const int GX = h->GX;
    static_assert(RAST_TILE * RAST_TILE == 4 * 64, "a tile is four cells per lane");
    for (int it = wave0; it < n_items; it += n_waves) {  // wave-uniform
        const RastItem I = items[it];
        const float *rec = aos + (size_t)I.tri * PEDP_TRI_STRIDE;
        const TriRec q = {rec[0], rec[1], rec[2], rec[3], rec[4], rec[5], rec[6], rec[7], rec[8], rec[9], rec[10], rec[11]};
        const int nc = I.w * I.h;
        unsigned idx[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {  // the lane's four cells: all heads first, then the chains side by side
            const int c = lane + 64 * j;
            const int yy = c / I.w, xx = c - yy * I.w;
            idx[j] = c < nc ? head[(size_t)(I.y0 + yy) * GX + (I.x0 + xx)] : RAST_NONE;
        }
        int steps = 0;
        while ((idx[0] & idx[1] & idx[2] & idx[3]) != RAST_NONE) {
            float4 nd[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) nd[j] = nodes[idx[j] != RAST_NONE ? idx[j] : 0u];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (idx[j] != RAST_NONE) {
                    rast_test(nd[j], idx[j], O, q, (unsigned)I.tri, sink);
                    idx[j] = __float_as_uint(nd[j].w);
                }
            if (++steps > RAST_CHAIN_MAX) { rast_fail(h, 4); break; }
        }
    }
}

}  // namespace
