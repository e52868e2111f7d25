// Ray stage, variant 5 and the general-origin sweep behind variants 1, 3 and 5: ray per lane, every triangle, packed
// fp32 on the vector pipe.
// One ray per lane, origin/direction in VGPRs for the whole sweep.  The triangle index is wave-uniform, so records
// are fetched with SCALAR loads and feed the VALU as SGPR operands (the scalar cache is the broadcast: no LDS
// traffic, no VGPRs for triangle data).  Two triangles ride in the two halves of every packed fp32 instruction
// (v_pk_mul_f32 / v_pk_fma_f32 deliver 1.54x the flops per issue slot of the scalar forms on this chip,
// tools/microbench_valu.hip): records are stored pair-interleaved so one aligned SGPR pair = (A.x, B.x) = one
// packed operand.
//   * general origins: 12 x 2 floats per pair (v0, e1, e2, m), 24 arithmetic ops per test;
//   * all rays share one origin (always true for the reference, defect_projection.py:545): the origin-dependent
//     terms e2 x s, s x e1, s . m are evaluated once per triangle by pair_shared_kernel with the very same
//     operations, leaving 3 dot products per test (10 x 2 floats per pair).
// origin_check_kernel sets a device-side flag; the shared-origin sweep of the configured variant and the
// general-origin instantiation are launched back to back and the flag lets exactly one work: no host round trip.
// The hot loop only decides "inside the triangle?" with a branch-free score
//     min3(un*det, vn*det, |det| - |un+vn|) >= 0
// which is a superset of the oracle's accept set (products keep the sign, underflow gives +-0 which passes); the
// division, tn, and the 64-bit min sit on a rarely taken wave-level branch that applies the oracle's exact predicate.
// Grid = (ray blocks) x (triangle chunks); chunk c is always served by workgroups with blockIdx % 8 == c % 8, i.e.
// one XCD, so each XCD's L2 only holds its part of the records.
#pragma once
#include "mt.h"
#include "mesh_records.h"

namespace {

// Shared-origin pair records.  With one origin O for every ray, s = O - v0 and with it a = e2 x s, b = s x e1 and
// tn = -(s . m) are constants of the triangle (computed here in the oracle's own operations), and so is the SIDE of the
// triangle the rays come from: the oracle accepts only if T = tn ^ sign(det) >= 0, i.e. sign(det) = sign(tn) =: sigma.
// Under that orientation the accept test reads  d . (sigma a) >= 0,  d . (sigma b) >= 0,  U + V <= |det|;  the first two
// dot products are the oracle's un, vn up to the sign (negating a vector negates its rounded dot product exactly), the
// third is replaced by a bound that is never tighter:  d . c + kappa |d|_1 >= 0  with c = sigma (m - a - b) and
// kappa = 20 u (|m|_1 + |a|_1 + |b|_1): every rounding that separates fl(d . c) from fl(d . m) - fl(fl(d . a) + fl(d . b))
// (three dot products of three roundings each, one addition, two subtractions per component of c) is below half of
// that.  The hot loop thus needs THREE packed dot products, one packed fma and one min3 per triangle -- a superset of
// the oracle's accept set; the exact predicate runs on the rarely taken branch, from the AoS record.
//   record (20 floats per pair, the two triangles interleaved): a'[3] b'[3] c'[3] kappa
//   tn == 0 (the origin in the triangle's plane: either side) -> a record that always passes to the exact test;
//   m == 0 exactly (pad records, zero-area triangles: det = 0 for every ray) -> a record that never does.
__global__ void pair_shared_kernel(const float *__restrict__ aos, int64_t F_padded, const float *__restrict__ rays6,
                                   const int *__restrict__ shared_flag, float *__restrict__ out) {
    if (*shared_flag == 0) return;
    int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F_padded) return;
    const float *r = aos + f * PEDP_TRI_STRIDE;
    const float e1x = r[3], e1y = r[4], e1z = r[5], e2x = r[6], e2y = r[7], e2z = r[8];
    const float mx = r[9], my = r[10], mz = r[11];
    const float sx = subr(rays6[0], r[0]), sy = subr(rays6[1], r[1]), sz = subr(rays6[2], r[2]);
    const float ax = fmar(e2y, sz, -mulr(e2z, sy));
    const float ay = fmar(e2z, sx, -mulr(e2x, sz));
    const float az = fmar(e2x, sy, -mulr(e2y, sx));
    const float bx = fmar(sy, e1z, -mulr(sz, e1y));
    const float by = fmar(sz, e1x, -mulr(sx, e1z));
    const float bz = fmar(sx, e1y, -mulr(sy, e1x));
    const float tn = -dot3(sx, sy, sz, mx, my, mz);
    float v[10];
    if (mx == 0.0f && my == 0.0f && mz == 0.0f) {          // never accepted
        for (int k = 0; k < 9; ++k) v[k] = 0.0f;
        v[9] = -1.0f;
    } else if (!(tn > 0.0f) && !(tn < 0.0f)) {             // tn == 0 (or NaN): always to the exact test
        for (int k = 0; k < 9; ++k) v[k] = 0.0f;
        v[9] = 1e30f;
    } else {
        const float sg = tn < 0.0f ? -1.0f : 1.0f;
        v[0] = sg * ax; v[1] = sg * ay; v[2] = sg * az;
        v[3] = sg * bx; v[4] = sg * by; v[5] = sg * bz;
        v[6] = sg * subr(subr(mx, ax), bx); v[7] = sg * subr(subr(my, ay), by); v[8] = sg * subr(subr(mz, az), bz);
        v[9] = 1.2e-6f * ((fabsf(mx) + fabsf(my) + fabsf(mz)) + (fabsf(ax) + fabsf(ay) + fabsf(az)) + (fabsf(bx) + fabsf(by) + fabsf(bz))) + 1e-37f;
    }
    float *o = out + (f >> 1) * PAIR_SH + (f & 1);
#pragma unroll
    for (int k = 0; k < 10; ++k) o[2 * k] = v[k];
}

// all ray origins bit-identical to ray 0's?  flag preset to non-zero, cleared on a mismatch
__global__ void origin_check_kernel(const float *__restrict__ rays6, int64_t N, int *__restrict__ flag) {
    const unsigned ox = __float_as_uint(rays6[0]), oy = __float_as_uint(rays6[1]), oz = __float_as_uint(rays6[2]);
    bool same = true;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x)
        same = same && (__float_as_uint(rays6[6 * i]) == ox) && (__float_as_uint(rays6[6 * i + 1]) == oy) &&
               (__float_as_uint(rays6[6 * i + 2]) == oz);
    if (__builtin_amdgcn_ballot_w64(!same) != 0 && (threadIdx.x & 63) == 0) atomicAnd(flag, 0);
}

// ------------------------------------------------------------------ sweep, ray per lane (packed)
__device__ __forceinline__ f2 splat(float a) { return (f2){a, a}; }
__device__ __forceinline__ f2 fma2(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f2 dot3p(f2 ax, f2 ay, f2 az, f2 bx, f2 by, f2 bz) {
    return fma2(az, bz, fma2(ay, by, ax * bx));
}

struct MT2 {  // det, un, vn of the two triangles of a pair
    f2 det, un, vn;
};

__device__ __forceinline__ MT2 eval_pair_general(const Ray &r, const f2 *t) {
    const f2 v0x = t[0], v0y = t[1], v0z = t[2], e1x = t[3], e1y = t[4], e1z = t[5];
    const f2 e2x = t[6], e2y = t[7], e2z = t[8], mx = t[9], my = t[10], mz = t[11];
    const f2 dx = splat(r.dx), dy = splat(r.dy), dz = splat(r.dz);
    MT2 m;
    m.det = dot3p(dx, dy, dz, mx, my, mz);
    const f2 sx = splat(r.ox) - v0x, sy = splat(r.oy) - v0y, sz = splat(r.oz) - v0z;
    const f2 ax = fma2(e2y, sz, -(e2z * sy));
    const f2 ay = fma2(e2z, sx, -(e2x * sz));
    const f2 az = fma2(e2x, sy, -(e2y * sx));
    m.un = dot3p(dx, dy, dz, ax, ay, az);
    const f2 bx = fma2(sy, e1z, -(sz * e1y));
    const f2 by = fma2(sz, e1x, -(sx * e1z));
    const f2 bz = fma2(sx, e1y, -(sy * e1x));
    m.vn = dot3p(dx, dy, dz, bx, by, bz);
    return m;
}

// shared origin: score of both halves from the oriented record, >= 0 is a superset of the oracle's accept set
// (pair_shared_kernel); dn = |d|_1 of the ray.  Ten packed and two scalar instructions per pair.
__device__ __forceinline__ f2 score_pair_shared(const Ray &r, float dn, const f2 *t) {
    const f2 dx = splat(r.dx), dy = splat(r.dy), dz = splat(r.dz);
    const f2 ua = dot3p(dx, dy, dz, t[0], t[1], t[2]);
    const f2 ub = dot3p(dx, dy, dz, t[3], t[4], t[5]);
    const f2 uc = fma2(t[9], splat(dn), dot3p(dx, dy, dz, t[6], t[7], t[8]));
    f2 s;
    s.x = fminf(fminf(ua.x, ub.x), uc.x);
    s.y = fminf(fminf(ua.y, ub.y), uc.y);
    return s;
}

// "inside the triangle" score of both halves; >= 0 is a superset of the oracle's accept set
__device__ __forceinline__ f2 inside_score(const MT2 &m) {
    const f2 a = m.un * m.det, b = m.vn * m.det, w = m.un + m.vn;
    f2 s;
    s.x = fminf(fminf(a.x, b.x), subr(fabsf(m.det.x), fabsf(w.x)));
    s.y = fminf(fminf(a.y, b.y), subr(fabsf(m.det.y), fabsf(w.y)));
    return s;
}

constexpr int RPL_BLOCK = 256;
constexpr int RPL_PAIRS = 2;  // pair records per loop iteration (4 triangles)

// the sweep loop: ray r against the 4-triangle groups [g0, g1)
template <bool SHARED>
__device__ __forceinline__ unsigned long long sweep_groups(const Ray &r, const f2 *__restrict__ rec, const float *__restrict__ aos,
                                                           int g0, int g1, unsigned long long best) {
    constexpr int PF = (SHARED ? PAIR_SH : PAIR_GEN) / 2;  // f2 per pair record
    const float dn = fabsf(r.dx) + fabsf(r.dy) + fabsf(r.dz);
    for (int g = g0; g < g1; ++g) {
        const f2 *t = rec + (size_t)g * (RPL_PAIRS * PF);
        f2 sc[RPL_PAIRS];
#pragma unroll
        for (int p = 0; p < RPL_PAIRS; ++p)
            sc[p] = SHARED ? score_pair_shared(r, dn, t + p * PF) : inside_score(eval_pair_general(r, t + p * PF));
        static_assert(RPL_PAIRS == 2, "score reduction below is written for 2 pairs");
        const float top = fmaxf(fmaxf(sc[0].x, sc[0].y), fmaxf(sc[1].x, sc[1].y));
        if (__builtin_amdgcn_ballot_w64(top >= 0.0f) != 0) {  // wave-uniform, rarely taken
            const int f0 = g * (2 * RPL_PAIRS);
#pragma unroll
            for (int k = 0; k < 2 * RPL_PAIRS; ++k) {
                const float s = (k & 1) ? sc[k >> 1].y : sc[k >> 1].x;
                if (s >= 0.0f) {
                    MT m = mt_eval(r, aos + (size_t)(f0 + k) * PEDP_TRI_STRIDE);  // exact, from the AoS record
                    if (mt_accept(m)) {
                        unsigned long long key = mt_key(m, (unsigned)(f0 + k));
                        best = key < best ? key : best;
                    }
                }
            }
        }
    }
    return best;
}

// The two instantiations are launched back to back; the device flag lets exactly one work.
template <bool SHARED>
__global__ __launch_bounds__(RPL_BLOCK) void ray_sweep_rpl_kernel(
    const f2 *__restrict__ rec, const float *__restrict__ aos, int groups_total, int groups_per_chunk, int n_chunks,
    const float *__restrict__ rays6, int64_t N, unsigned long long *__restrict__ keys,
    const int *__restrict__ shared_flag) {
    if ((*shared_flag != 0) != SHARED) return;
    const int b = blockIdx.x;
    const int chunk = b % n_chunks;  // n_chunks % 8 == 0: chunk % 8 == b % 8, one XCD per chunk
    const int64_t rb = b / n_chunks;
    const int64_t ray = rb * RPL_BLOCK + threadIdx.x;
    const int64_t rl = ray < N ? ray : N - 1;  // tail lanes re-run the last ray, never store
    Ray r;
    r.ox = rays6[6 * rl + 0]; r.oy = rays6[6 * rl + 1]; r.oz = rays6[6 * rl + 2];
    r.dx = rays6[6 * rl + 3]; r.dy = rays6[6 * rl + 4]; r.dz = rays6[6 * rl + 5];
    int g0 = chunk * groups_per_chunk;
    int g1 = g0 + groups_per_chunk;
    if (g1 > groups_total) g1 = groups_total;
    const unsigned long long best = sweep_groups<SHARED>(r, rec, aos, g0, g1, KEY_MISS);
    if (ray < N && best != KEY_MISS) atomicMin(&keys[ray], best);
}

}  // namespace
