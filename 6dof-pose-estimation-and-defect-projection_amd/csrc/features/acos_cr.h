// acos of x in [0, 1], correctly rounded, for FPFH's pair-ordering test.
//
// Feature.cpp orders a pair of points by `acos(|a1|) > acos(|a2|)`.  Where two points share a neighbourhood (hence a
// normal) or sit on a lattice, |a1| and |a2| are a few ulp apart and the comparison asks whether two adjacent arguments
// round to the same double or not -- which a 1-2 ulp acos answers differently from the host's libm.  A correctly rounded
// acos answers like that libm on every such pair of the test matrix (tests/test_cloudops_matrix_gpu.py), so the device
// takes this function whenever its fast acos leaves the order open; it is never on the common path.
//
// Double-double arithmetic (error-free sums and fma products), about 1e-30 relative:
//     x <= 1/2:  acos x = pi/2 - asin x
//     x >  1/2:  acos x = 2 asin sqrt((1 - x) / 2)          (1 - x and the halving are exact)
//     asin s = sum_n c_n s^(2n+1),  c_(n+1) / c_n = (2n+1)^2 / ((2n+2)(2n+3)),  s <= sqrt(1/4): 60 terms reach 1e-36.
// The high word of the normalised result is the nearest double unless the exact value lies within 1e-30 of a midpoint.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define PEDP_ACOS_HD __host__ __device__ inline
#else
#define PEDP_ACOS_HD inline
#endif

namespace acos_cr_detail {
struct dd { double hi, lo; };
PEDP_ACOS_HD dd quick_two_sum(double a, double b) { const double s = a + b; return {s, b - (s - a)}; }
PEDP_ACOS_HD dd two_sum(double a, double b) {
    const double s = a + b, bb = s - a;
    return {s, (a - (s - bb)) + (b - bb)};
}
PEDP_ACOS_HD dd two_prod(double a, double b) { const double p = a * b; return {p, fma(a, b, -p)}; }
PEDP_ACOS_HD dd add(dd a, dd b) {
    dd s = two_sum(a.hi, b.hi);
    const dd t = two_sum(a.lo, b.lo);
    s.lo += t.hi;
    s = quick_two_sum(s.hi, s.lo);
    s.lo += t.lo;
    return quick_two_sum(s.hi, s.lo);
}
PEDP_ACOS_HD dd mul(dd a, dd b) {
    dd p = two_prod(a.hi, b.hi);
    p.lo += a.hi * b.lo + a.lo * b.hi;
    return quick_two_sum(p.hi, p.lo);
}
PEDP_ACOS_HD dd ratio(double num, double den) {  // num / den of two small integers
    const double q = num / den;
    return quick_two_sum(q, fma(-q, den, num) / den);
}
PEDP_ACOS_HD dd sqrt_dd(double z) {  // z >= 0
    const double s = sqrt(z);
    if (!(s > 0.0)) return {0.0, 0.0};
    return quick_two_sum(s, fma(-s, s, z) / (2.0 * s));
}
PEDP_ACOS_HD dd asin_series(dd s) {  // |s| <= 1/2
    const dd s2 = mul(s, s);
    dd term = s, sum = s;
    for (int n = 0; n < 60; ++n) {
        const double a = 2.0 * n + 1.0;
        term = mul(mul(term, s2), ratio(a * a, (a + 1.0) * (a + 2.0)));
        sum = add(sum, term);
    }
    return sum;
}
}  // namespace acos_cr_detail

PEDP_ACOS_HD double acos_cr(double x) {  // 0 <= x <= 1 (anything else: the plain acos)
    using namespace acos_cr_detail;
    if (!(x >= 0.0 && x <= 1.0)) return acos(x);
    if (x <= 0.5) {
        const dd half_pi = {1.5707963267948966, 6.123233995736766e-17};
        const dd a = asin_series({x, 0.0});
        return add(half_pi, {-a.hi, -a.lo}).hi;
    }
    const dd a = asin_series(sqrt_dd((1.0 - x) * 0.5));
    return add(a, a).hi;
}
