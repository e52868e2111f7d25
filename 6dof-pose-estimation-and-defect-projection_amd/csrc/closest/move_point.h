// q = R p + t of a row-major 4 x 4 float64 T, as the surface fit's search and its rows kernel both form it
// (DESIGN.md s4.21): ((T[4k] p0 + T[4k+1] p1) + T[4k+2] p2) + T[4k+3], no contraction.  The two kernels must agree in
// every bit of q, so there is one copy of the expression.
#pragma once

namespace {
namespace surface_fit {

__host__ __device__ __forceinline__ void move_point(const double *__restrict__ T, double p[3]) {
    const double x = p[0], y = p[1], z = p[2];
    for (int k = 0; k < 3; ++k) p[k] = ((T[4 * k] * x + T[4 * k + 1] * y) + T[4 * k + 2] * z) + T[4 * k + 3];
}

}  // namespace surface_fit
}  // namespace
