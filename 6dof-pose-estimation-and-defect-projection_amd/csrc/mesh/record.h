// The triangle record of a mesh handle as the float64 queries read it (pedp_closest.hip, pedp_solid.hip): a = v0,
// ab = e1, ac = e2, float32 values promoted to float64.  Internal linkage: each including file gets its own copy.
#pragma once
#include "../pedp_internal.h"
#include <cmath>

namespace {
namespace record {

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7FF8000000000000ll); }
__device__ __forceinline__ double pos_inf() { return __longlong_as_double(0x7FF0000000000000ll); }

__device__ __forceinline__ double dot3(const double x[3], const double y[3]) { return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]; }
__device__ __forceinline__ void cross3(const double x[3], const double y[3], double out[3]) {
    out[0] = x[1] * y[2] - x[2] * y[1];
    out[1] = x[2] * y[0] - x[0] * y[2];
    out[2] = x[0] * y[1] - x[1] * y[0];
}

struct Tri {
    double a[3], ab[3], ac[3];
};

// the record as stored, promoted; false: a record no ray can hit either (m all zero: a pad or a degenerate triangle)
__device__ __forceinline__ bool load_tri(const float *__restrict__ rec, Tri &t) {
    if (rec[9] == 0.0f && rec[10] == 0.0f && rec[11] == 0.0f) return false;
    for (int k = 0; k < 3; ++k) {
        t.a[k] = (double)rec[k];
        t.ab[k] = (double)rec[3 + k];
        t.ac[k] = (double)rec[6 + k];
    }
    return true;
}

// the unit normal (ab x ac) / |ab x ac|: the length as sqrt((x^2 + y^2) + z^2), one division per component
__device__ __forceinline__ void unit_normal(const Tri &t, double n[3]) {
    double c[3];
    cross3(t.ab, t.ac, c);
    const double len = sqrt(dot3(c, c));
    for (int k = 0; k < 3; ++k) n[k] = c[k] / len;
}

}  // namespace record
}  // namespace
