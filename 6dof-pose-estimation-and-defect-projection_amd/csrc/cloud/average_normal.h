// ------------------------------------------------------------------ compute_average_normal on the device
// src/pose_estimation.py:314-321: the normals' averages over a 10-unit voxel grid (voxel_down_sample: members summed in
// point order, divided by the count; voxels in ascending (ix, iy, iz)), then numpy's mean over the voxels (row by row).
// The sort-based grid above costs two dozen launches and two trips to the host for the 38 k points of a frame; here the
// voxels are cells of a dense grid (ids ascending in (ix, iy, iz)), members are counted and placed, and a thread per
// cell adds its members in ascending point index by repeated selection (a few dozen members).  No trip to the host:
// the grid's origin (the cloud's own minimum, less half a voxel: voxel_down_sample's) is folded on the device, its
// dimensions come from a box the caller knows to contain the cloud.  Same sums in the same order as the grid above.
#pragma once
#include "common.h"

namespace {

struct AvgGrid { int dim[3]; double voxel; };
__global__ __launch_bounds__(256) void avgn_origin_kernel(const double *__restrict__ part /* n_part x 6 */, int n_part, double voxel,
                                                          double *__restrict__ org) {
    __shared__ double red[4][3];
    double lo[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        lo[k] = (int)threadIdx.x < n_part ? part[6 * threadIdx.x + k] : __longlong_as_double(0x7FF0000000000000ll);
        for (int b = threadIdx.x + 256; b < n_part; b += 256) lo[k] = part[6 * b + k] < lo[k] ? part[6 * b + k] : lo[k];
        for (int off = 32; off >= 1; off >>= 1) {
            const double o = __shfl_xor(lo[k], off, 64);
            lo[k] = o < lo[k] ? o : lo[k];
        }
    }
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 3; ++k) red[threadIdx.x >> 6][k] = lo[k];
    __syncthreads();
    if (threadIdx.x < 3) {
        double v = red[0][threadIdx.x];
        for (int w = 1; w < 4; ++w) v = red[w][threadIdx.x] < v ? red[w][threadIdx.x] : v;
        org[threadIdx.x] = v - voxel * 0.5;
    }
}
__device__ __forceinline__ unsigned avgn_cell(const double *p, const double *org, const AvgGrid &g) {
    int c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const long long v = (long long)floor((p[k] - org[k]) / g.voxel);
        c[k] = v < 0 ? 0 : (v >= g.dim[k] ? g.dim[k] - 1 : (int)v);  // (never clamps: the box contains the cloud)
    }
    return (unsigned)((c[0] * g.dim[1] + c[1]) * g.dim[2] + c[2]);
}
__global__ void avgn_count_kernel(const double *__restrict__ pts, int64_t N, const double *__restrict__ org, AvgGrid g,
                                  unsigned *__restrict__ cell, int *__restrict__ slot, unsigned *__restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const unsigned c = avgn_cell(pts + 3 * i, org, g);
    cell[i] = c;
    slot[i] = (int)atomicAdd(&count[c], 1u);
}
__global__ void avgn_place_kernel(int64_t N, const unsigned *__restrict__ cell, const int *__restrict__ slot, const unsigned *__restrict__ begin,
                                  int *__restrict__ member) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) member[begin[cell[i]] + (unsigned)slot[i]] = (int)i;
}
struct NonEmpty { __host__ __device__ unsigned operator()(unsigned n) const { return n != 0u ? 1u : 0u; } };
constexpr int AVGN_MAX_MEMBERS = 512, AVGN_WPB = 4;
// A wave per 64 consecutive cells; every non-empty cell of them is served by the whole wave: the members' indices go to
// LDS, every member's rank among them is the number of smaller indices, its normal goes to the LDS row of that rank, and
// three lanes -- one per component -- add the rows in order (eight reads in flight, then their additions).
__global__ __launch_bounds__(AVGN_WPB * 64) void avgn_mean_kernel(int64_t n_cells, const unsigned *__restrict__ begin,
                                                                   const unsigned *__restrict__ rank, const int *__restrict__ member,
                                                                   const double *__restrict__ nrm, double *__restrict__ means,
                                                                   int *__restrict__ overflow) {
    __shared__ int idx_s[AVGN_WPB][AVGN_MAX_MEMBERS];
    __shared__ double row_s[AVGN_WPB][3 * AVGN_MAX_MEMBERS];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t c0 = ((int64_t)blockIdx.x * AVGN_WPB + wv) * 64, cl = c0 + lane;
    const unsigned b = cl < n_cells ? begin[cl] : 0u, e = cl < n_cells ? begin[cl + 1] : 0u;
    unsigned long long todo = __builtin_amdgcn_ballot_w64(e > b);
    int *ids = idx_s[wv];
    double *rows = row_s[wv];
    while (todo) {  // wave-uniform
        const int j = __builtin_ctzll(todo);
        todo &= todo - 1;
        const unsigned cb = __builtin_amdgcn_readlane(b, j), k = __builtin_amdgcn_readlane(e, j) - cb;
        if (k > (unsigned)AVGN_MAX_MEMBERS) { if (lane == 0) *overflow = 1; continue; }
        for (unsigned t = lane; t < k; t += 64) ids[t] = member[cb + t];
        __builtin_amdgcn_s_waitcnt(0xc07f);  // (this wave's LDS writes are complete: lgkmcnt(0))
        __builtin_amdgcn_wave_barrier();
        for (unsigned t = lane; t < k; t += 64) {
            const int mine = ids[t];
            unsigned r = 0;
            for (unsigned u = 0; u < k; ++u) r += ids[u] < mine ? 1u : 0u;
            rows[3 * r] = nrm[3 * (size_t)mine];
            rows[3 * r + 1] = nrm[3 * (size_t)mine + 1];
            rows[3 * r + 2] = nrm[3 * (size_t)mine + 2];
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
        if (lane < 3) {
            double s = 0.0;
            for (unsigned t = 0; t < k; t += 8) {
                double v[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) v[q] = t + q < k ? rows[3 * (t + q) + lane] : 0.0;
#pragma unroll
                for (int q = 0; q < 8; ++q)
                    if (t + q < k) s += v[q];
            }
            means[3 * (size_t)rank[c0 + j] + lane] = s / (double)k;
        }
        __builtin_amdgcn_wave_barrier();
    }
}
// numpy's mean over axis 0 adds the rows one after the other: a serial chain of a few thousand additions, which one GPU
// thread takes 170 us over.  The means are therefore written straight into pinned host memory by the kernel above, and the
// host adds them after the stream's next wait (microseconds); this kernel only reports how many there are.
__global__ void avgn_rows_kernel(int64_t n_cells, const unsigned *__restrict__ rank, const unsigned *__restrict__ count,
                                 const int *__restrict__ overflow, double *__restrict__ res) {
    res[3] = (double)((int64_t)rank[n_cells - 1] + (count[n_cells - 1] != 0u ? 1 : 0));
    res[4] = (double)*overflow;
}

}  // namespace
