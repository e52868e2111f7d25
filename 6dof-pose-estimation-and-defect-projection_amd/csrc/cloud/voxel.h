// ------------------------------------------------------------------ voxel grid
// key = (cx, cy, cz) packed most significant first into just the bits the box needs (sy, sz: the widths of cy and cz):
// the radix sort's passes follow the key's width
#pragma once
#include "common.h"

namespace {

__global__ void voxel_key_kernel(const double *__restrict__ pts, int64_t N, double lox, double loy, double loz, double voxel, int sy,
                                 int sz, unsigned long long *__restrict__ key, int *__restrict__ val) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const unsigned long long cx = (unsigned long long)(long long)floor((pts[3 * i] - lox) / voxel);
    const unsigned long long cy = (unsigned long long)(long long)floor((pts[3 * i + 1] - loy) / voxel);
    const unsigned long long cz = (unsigned long long)(long long)floor((pts[3 * i + 2] - loz) / voxel);
    key[i] = ((cx & 0x1FFFFFull) << (sy + sz)) | ((cy & ((1ull << sy) - 1ull)) << sz) | (cz & ((1ull << sz) - 1ull));
    val[i] = (int)i;
}

__global__ void voxel_average_kernel(const double *__restrict__ pts, const double *__restrict__ nrm,
                                     const int *__restrict__ sorted_idx, const unsigned *__restrict__ counts,
                                     const unsigned *__restrict__ offsets, const unsigned *__restrict__ n_runs,
                                     double *__restrict__ out_pts, double *__restrict__ out_nrm) {
    const unsigned v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= *n_runs) return;
    const unsigned a = offsets[v], n = counts[v];
    double s0 = 0, s1 = 0, s2 = 0, n0 = 0, n1 = 0, n2 = 0;
    for (unsigned j = 0; j < n; ++j) {  // members in point order (stable sort)
        const int64_t i = sorted_idx[a + j];
        s0 += pts[3 * i]; s1 += pts[3 * i + 1]; s2 += pts[3 * i + 2];
        if (nrm) { n0 += nrm[3 * i]; n1 += nrm[3 * i + 1]; n2 += nrm[3 * i + 2]; }
    }
    const double c = (double)n;
    out_pts[3 * (size_t)v] = s0 / c; out_pts[3 * (size_t)v + 1] = s1 / c; out_pts[3 * (size_t)v + 2] = s2 / c;
    if (nrm) { out_nrm[3 * (size_t)v] = n0 / c; out_nrm[3 * (size_t)v + 1] = n1 / c; out_nrm[3 * (size_t)v + 2] = n2 / c; }
}

}  // namespace
