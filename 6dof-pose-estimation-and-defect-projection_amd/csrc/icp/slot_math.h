// ICP: the arithmetic that several kernels must do alike -- candidate tests, search radii and the certificate's steps.
// Exactness and the certificates' soundness rest on every kernel forming these numbers by the same sequence of operations
// (built with -ffp-contract=off: the order written here is the order executed).
#pragma once
#include "common.h"

namespace {

// "No neighbour" in Tprev is a NaN's bits, stored as two integer words made where they are stored: as a double constant
// the pair was kept in registers through the chunk loop, and spilled.  (pedp_icp.hip is built with -fno-honor-nans.)
__device__ __forceinline__ void store_nan(PEDP_GLOBAL double *p) {
    int z = 0;
    asm volatile("" : "+v"(z));
    typedef int v2i_ __attribute__((ext_vector_type(2)));
    const v2i_ w = {z, 0x7FF80000 | z};
    *(PEDP_GLOBAL v2i_ *)p = w;
}
__device__ __forceinline__ void lds_nan(double *p) {
    int z = 0;
    asm volatile("" : "+v"(z));
    ((int *)p)[0] = z;
    ((int *)p)[1] = 0x7FF80000 | z;
}

// Squared distance of (x, y, z) from the box (lo, hi): 0 inside.  (Written out in icp_pass_kernel's rebuild test of the chunk
// spheres, where the call moved instructions, and in pack_one, whose box arrives as scalars.)
__device__ __forceinline__ double box_dist2(double x, double y, double z, const double (&lo)[3], const double (&hi)[3]) {
    const double ex = fmax(fmax(lo[0] - x, x - hi[0]), 0.0), ey = fmax(fmax(lo[1] - y, y - hi[1]), 0.0), ez = fmax(fmax(lo[2] - z, z - hi[2]), 0.0);
    return ex * ex + ey * ey + ez * ez;
}

// What the rounding of a centred point to fp32 can move it by, from the 1-norm s1 of its fp32 coordinates.
__device__ __forceinline__ float point_slack(float s1) { return 1e-5f * s1 + 1e-6f; }
__device__ __forceinline__ float point_slack(float sx, float sy, float sz) { return point_slack(fabsf(sx) + fabsf(sy) + fabsf(sz)); }

// The sphere test of every culling level: is the offset between two centres longer than lim -- a search radius, both
// spheres' radii, a slack?  Rounded towards no; callers ask !offset_beyond(...), which is true for NaN.
__device__ __forceinline__ bool offset_beyond(float dx, float dy, float dz, float lim) {
    return (dx * dx + dy * dy + dz * dz) > lim * lim * 1.00001f + 1e-6f;
}
// Can the target sphere ts (w < 0: no rows) hold a point within rho of the slot's centred point s?
__device__ __forceinline__ bool sphere_near_slot(const float4 &ts, float sx, float sy, float sz, float rho, float slack) {
    const float dx = ts.x - sx, dy = ts.y - sy, dz = ts.z - sz;
    const float lim = rho + ts.w + slack;
    return !offset_beyond(dx, dy, dz, lim) && ts.w >= 0.f;
}

// Search radius of a slot, before the cap at r: the distance to last pass's neighbour, rounded up.  With certificates KAPPA
// times that: any radius not below the true nearest distance gives the same result; the wider one leaves a margin between
// the neighbour and the bound the certificate is made from.
__device__ __forceinline__ float slot_radius(double dprev, float s1) { return (float)dprev * 1.00001f + 1e-5f * s1 + 1e-6f; }
__device__ __forceinline__ float slot_radius_kappa(double dprev, float s1) { return PEDP_ICP_KAPPA * ((float)dprev * 1.00001f) + 1e-5f * s1 + 1e-6f; }

// A certificate carried over a pass.  Every target point but last pass's neighbour was at least c_in from the point; the
// point has moved by m, so they are at least cert_moved(c_in, m) from it now (rounded down: the factors cover the float64
// roundings of dist2 and sqrt a thousand times over, the last one the rounding to float32).  The old neighbour strictly
// inside that bound (cert_inside; dprev is its distance now) is the unique nearest neighbour, and dist2 to it is the very
// number the selection would produce.  Non-finite values, told by their exponent bits, never certify.  Certified:
//     cert_finite(d2prev, m, c_new) && jprev >= 0 && c_new > 0.f && cert_inside(dprev, c_new)      (else c_new becomes 0)
__device__ __forceinline__ float cert_moved(float c_in, double m) { return (float)(((double)c_in - m * (1.0 + 1e-12)) * (1.0 - 2e-7)); }
__device__ __forceinline__ bool cert_finite(double d2prev, double m, float c_new) {
    return (__double2hiint(d2prev) & 0x7FF00000) != 0x7FF00000 && (__double2hiint(m) & 0x7FF00000) != 0x7FF00000 &&
           (__float_as_int(c_new) & 0x7F800000) != 0x7F800000;
}
__device__ __forceinline__ bool cert_inside(double dprev, float c_new) { return dprev * (1.0 + 1e-12) < (double)c_new; }

// The certificate a searching slot leaves.  Target points it did not list are farther than the radius rho_f it searched
// within, less the rounding allowance that radius was given (the point's slack, or the 1-norm s1 the slack is made from);
// L2 is the squared lower bound on every target point but the winner, and the certificate its root, rounded down.
__device__ __forceinline__ double cert_rho(float rho_f, float slack) { return (double)rho_f * (1.0 - 2e-5) - (double)slack * 1.000001; }
__device__ __forceinline__ double cert_rho_s1(float rho_f, float s1) { return (double)rho_f * (1.0 - 2e-5) - (double)point_slack(s1) * 1.000001; }
__device__ __forceinline__ float cert_bound(double L2) { return (float)(sqrt(L2) * (1.0 - 2e-7)); }

}  // namespace
