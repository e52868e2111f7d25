// Bounding box of device-resident points: per-workgroup partial minima / maxima (the host loop's
// comparisons), folded on the host from the pinned block.  One small read-back instead of a host pass over
// the caller's array (0.5 ms for 365 k points).  The comparisons pass over a NaN, so the same sweep keeps a
// flag: a workgroup that met a NaN or infinite coordinate writes NaN as its first partial (poisoned), and the
// fold hands the caller a NaN box -- every consumer refuses that (make_grid, voxel_core).
#pragma once
#include "common.h"

namespace {

constexpr int BND_BLOCKS = 256;
__global__ __launch_bounds__(256) void bounds_kernel(const double *__restrict__ pts, int64_t N, double *__restrict__ part) {
    const double inf = __longlong_as_double(0x7FF0000000000000ll);
    double lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    int bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double v = pts[3 * i + k];
            if (v < lo[k]) lo[k] = v;
            if (v > hi[k]) hi[k] = v;
            bad |= !(fabs(v) < inf);  // NaN or +-inf
        }
    bad = __syncthreads_or(bad);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double a = __shfl_xor(lo[k], off, 64), b = __shfl_xor(hi[k], off, 64);
            if (a < lo[k]) lo[k] = a;
            if (b > hi[k]) hi[k] = b;
        }
    __shared__ double red[4][6];
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 3; ++k) { red[threadIdx.x >> 6][k] = lo[k]; red[threadIdx.x >> 6][3 + k] = hi[k]; }
    __syncthreads();
    if (threadIdx.x < 6) {
        double v = red[0][threadIdx.x];
        for (int w = 1; w < 4; ++w) {
            const double o = red[w][threadIdx.x];
            if (threadIdx.x < 3 ? o < v : o > v) v = o;
        }
        part[6 * blockIdx.x + threadIdx.x] = (bad && threadIdx.x == 0) ? __longlong_as_double(0x7FF8000000000000ll) : v;
    }
}

}  // namespace
