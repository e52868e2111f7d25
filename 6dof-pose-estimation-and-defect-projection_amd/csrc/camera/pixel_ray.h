// The ray of a pinhole camera's pixel as compute_rays forms it (src/defect_projection.py:196-223): float64, one
// rounding per operation.  What pedp_project.hip casts and what pedp_coverage.hip judges a cast by.  Internal linkage:
// each including file gets its own copy.
#pragma once
#include "../pedp_internal.h"

namespace {
namespace camera {

struct Cam {
    double fx, fy, cx, cy;
    int width;
};

// d = (xn, yn, 1) / sqrt((xn xn + yn yn) + 1), xn = (x - cx) / fx, yn = (y - cy) / fy, of pixel pix = y width + x
__device__ __forceinline__ void pixel_direction(const Cam &cam, int64_t pix, double d[3]) {
    const int64_t y = pix / cam.width, x = pix - y * cam.width;
    const double xn = __ddiv_rn(__dsub_rn((double)x, cam.cx), cam.fx);
    const double yn = __ddiv_rn(__dsub_rn((double)y, cam.cy), cam.fy);
    const double len = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(xn, xn), __dmul_rn(yn, yn)), 1.0));
    d[0] = __ddiv_rn(xn, len);
    d[1] = __ddiv_rn(yn, len);
    d[2] = __ddiv_rn(1.0, len);
}

}  // namespace camera
}  // namespace
