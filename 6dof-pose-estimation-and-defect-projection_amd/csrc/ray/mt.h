// Ray stage, shared by every variant: the oracle's ray / triangle test (oracle/ray.c) and the packed result key.
//
//   per triangle:  e1 = v1 - v0, e2 = v2 - v0, m = e2 x e1
//   per test:      det = d . m ; s = o - v0 ; un = d . (e2 x s) ; vn = d . (s x e1) ; tn = -(s . m)
//
// Moeller-Trumbore in scalar-triple-product form, division deferred to accepted hits, every operation one fp32
// rounding in a fixed order (the *r helpers below).  mt_eval / mt_accept / mt_key are the ONLY code that decides a
// hit: whatever a sweep does in front of them (packed scores, the bf16 filter, cones, the grid) merely selects the
// pairs they see, conservatively.
// key = (bits(t) << 32) | triangle id orders by t (t >= 0: IEEE bits are monotone), then by triangle index -- the
// oracle's tie rule, independent of execution order; partial results meet in one 64-bit atomicMin per ray.
#pragma once
#include "../pedp_internal.h"

namespace {

constexpr unsigned long long KEY_MISS = 0xFFFFFFFFFFFFFFFFull;
typedef float f2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float mulr(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float fmar(float a, float b, float c) { return __fmaf_rn(a, b, c); }
__device__ __forceinline__ float subr(float a, float b) { return __fsub_rn(a, b); }
__device__ __forceinline__ float addr(float a, float b) { return __fadd_rn(a, b); }

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
    return fmar(az, bz, fmar(ay, by, mulr(ax, bx)));
}

struct Ray {
    float ox, oy, oz, dx, dy, dz;
};

struct MT {
    float det, un, vn, tn;
};

// The oracle's operation order (oracle/ray.c header comment), verbatim.  rec = 12 floats.
struct TriRec {
    float v0x, v0y, v0z, e1x, e1y, e1z, e2x, e2y, e2z, mx, my, mz;
};
__device__ __forceinline__ MT mt_eval(const Ray &r, const TriRec &q) {
    const float v0x = q.v0x, v0y = q.v0y, v0z = q.v0z, e1x = q.e1x, e1y = q.e1y, e1z = q.e1z;
    const float e2x = q.e2x, e2y = q.e2y, e2z = q.e2z, mx = q.mx, my = q.my, mz = q.mz;
    MT m;
    m.det = dot3(r.dx, r.dy, r.dz, mx, my, mz);
    const float sx = subr(r.ox, v0x), sy = subr(r.oy, v0y), sz = subr(r.oz, v0z);
    const float ax = fmar(e2y, sz, -mulr(e2z, sy));  // a = e2 x s
    const float ay = fmar(e2z, sx, -mulr(e2x, sz));
    const float az = fmar(e2x, sy, -mulr(e2y, sx));
    m.un = dot3(r.dx, r.dy, r.dz, ax, ay, az);
    const float bx = fmar(sy, e1z, -mulr(sz, e1y));  // b = s x e1
    const float by = fmar(sz, e1x, -mulr(sx, e1z));
    const float bz = fmar(sx, e1y, -mulr(sy, e1x));
    m.vn = dot3(r.dx, r.dy, r.dz, bx, by, bz);
    m.tn = -dot3(sx, sy, sz, mx, my, mz);
    return m;
}
__device__ __forceinline__ MT mt_eval(const Ray &r, const float *rec) {
    const TriRec q = {rec[0], rec[1], rec[2], rec[3], rec[4], rec[5], rec[6], rec[7], rec[8], rec[9], rec[10], rec[11]};
    return mt_eval(r, q);
}

// Exact acceptance predicate of the oracle.
__device__ __forceinline__ bool mt_accept(const MT &m) {
    unsigned sg = __float_as_uint(m.det) & 0x80000000u;
    float U = __uint_as_float(__float_as_uint(m.un) ^ sg);
    float V = __uint_as_float(__float_as_uint(m.vn) ^ sg);
    float T = __uint_as_float(__float_as_uint(m.tn) ^ sg);
    float W = addr(U, V);
    return (m.det != 0.0f) & (U >= 0.0f) & (V >= 0.0f) & (T >= 0.0f) & (W <= fabsf(m.det));
}

__device__ __forceinline__ unsigned long long mt_key(const MT &m, unsigned id) {
    unsigned sg = __float_as_uint(m.det) & 0x80000000u;
    float T = __uint_as_float(__float_as_uint(m.tn) ^ sg);
    float t = __fdiv_rn(T, fabsf(m.det));
    unsigned tb = __float_as_uint(t) & 0x7FFFFFFFu;
    return ((unsigned long long)tb << 32) | (unsigned long long)id;
}

// What a selector hands an accepted pair to.  The casts' sink: the closest hit, the packed atomicMin.  `one` takes a
// pair as it is met; gather / finish let a thread that owns a ray fold its pairs before it touches memory.  (The
// all-hits queries' sinks, ray/all_hits.h, have the same members.)
struct HitMin {
    unsigned long long *__restrict__ keys;
    typedef unsigned long long Acc;
    __device__ __forceinline__ Acc start() const { return KEY_MISS; }
    __device__ __forceinline__ void one(unsigned ray, const MT &m, unsigned f) const { atomicMin(&keys[ray], mt_key(m, f)); }
    __device__ __forceinline__ void gather(Acc &best, int64_t, const MT &m, unsigned f) const {
        const unsigned long long key = mt_key(m, f);
        best = key < best ? key : best;
    }
    __device__ __forceinline__ void finish(Acc best, int64_t ray) const { if (best != KEY_MISS) atomicMin(&keys[ray], best); }
};

// (for the atomic min / max of direction bounds in variants 3 and 4)
__device__ __forceinline__ unsigned enc_f(float f) {  // order-preserving float -> uint
    unsigned b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float dec_f(unsigned e) {
    return __uint_as_float((e & 0x80000000u) ? (e & 0x7FFFFFFFu) : ~e);
}

}  // namespace
