// ------------------------------------------------------------------ uniform grid
#pragma once
#include "common.h"

namespace {

struct Grid {
    double lo[3], cell;
    int dim[3];
};

__device__ __forceinline__ int grid_axis(double p, double lo, double cell, int dim) {
    int c = (int)floor((p - lo) / cell);
    return c < 0 ? 0 : (c >= dim ? dim - 1 : c);
}

__global__ void grid_cell_kernel(const double *__restrict__ pts, int64_t N, Grid g, unsigned *__restrict__ cell,
                                 int *__restrict__ val) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int cx = grid_axis(pts[3 * i], g.lo[0], g.cell, g.dim[0]), cy = grid_axis(pts[3 * i + 1], g.lo[1], g.cell, g.dim[1]),
              cz = grid_axis(pts[3 * i + 2], g.lo[2], g.cell, g.dim[2]);
    cell[i] = (unsigned)(cx + g.dim[0] * (cy + g.dim[1] * cz));
    val[i] = (int)i;
}

// sorted by cell: where each cell's run starts and ends (empty cells keep the 0 / 0 they were cleared to), and the
// points gathered in that order
__global__ void grid_ranges_kernel(const unsigned *__restrict__ cell_sorted, const int *__restrict__ idx_sorted,
                                   const double *__restrict__ pts, int64_t N, int *__restrict__ cell_start,
                                   int *__restrict__ cell_end, double *__restrict__ sp) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    const unsigned c = cell_sorted[j];
    if (j == 0 || cell_sorted[j - 1] != c) cell_start[c] = (int)j;
    if (j == N - 1 || cell_sorted[j + 1] != c) cell_end[c] = (int)j + 1;
    const int64_t i = idx_sorted[j];
    sp[3 * j] = pts[3 * i]; sp[3 * j + 1] = pts[3 * i + 1]; sp[3 * j + 2] = pts[3 * i + 2];
}

// The index by counting: a point's cell and its slot among the cell's points (an atomic count: the slots' order is
// whatever the hardware made it -- every reader of the index is indifferent to the order inside a cell: counts,
// minima, sets, and lists with explicit (distance, index) order), an exclusive scan of the counts, the points placed.
// Six launches; a sort of nine thousand pairs is a dozen.  begin[] has n_cells + 1 entries and is monotone, so cell
// c's run is begin[c] .. begin[c + 1] and the cells c .. c' of one x row are the one run begin[c] .. begin[c' + 1].
__global__ void grid_count_kernel(const double *__restrict__ pts, int64_t N, Grid g, unsigned *__restrict__ cell, int *__restrict__ slot,
                                  unsigned *__restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int cx = grid_axis(pts[3 * i], g.lo[0], g.cell, g.dim[0]), cy = grid_axis(pts[3 * i + 1], g.lo[1], g.cell, g.dim[1]),
              cz = grid_axis(pts[3 * i + 2], g.lo[2], g.cell, g.dim[2]);
    const unsigned c = (unsigned)(cx + g.dim[0] * (cy + g.dim[1] * cz));
    cell[i] = c;
    slot[i] = (int)atomicAdd(&count[c], 1u);
}
__global__ void grid_place_kernel(const double *__restrict__ pts, int64_t N, const unsigned *__restrict__ cell,
                                  const int *__restrict__ slot, const int *__restrict__ begin, double *__restrict__ sp,
                                  int *__restrict__ idx_sorted, unsigned *__restrict__ cell_s) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const unsigned c = cell[i];
    const int64_t j = (int64_t)begin[c] + slot[i];
    sp[3 * j] = pts[3 * i]; sp[3 * j + 1] = pts[3 * i + 1]; sp[3 * j + 2] = pts[3 * i + 2];
    idx_sorted[j] = (int)i;
    cell_s[j] = c;
}

// The cells x0 .. x1 of one x row have consecutive ids, so their points are ONE run of the cell-sorted order
// (rs = re: the row is empty).
__device__ __forceinline__ void row_run(const int *__restrict__ cell_start, const int *__restrict__ cell_end, int base, int x0, int x1,
                                        int &rs, int &re) {
    rs = cell_start[base + x0];
    re = cell_end[base + x1];
}

// calls f(q) for every sorted position q whose point lies in one of the 27 cells around p
template <class F>
__device__ __forceinline__ void for_neighbours(const Grid &g, const double *p, const int *__restrict__ cell_start,
                                               const int *__restrict__ cell_end, F f) {
    const int cx = grid_axis(p[0], g.lo[0], g.cell, g.dim[0]), cy = grid_axis(p[1], g.lo[1], g.cell, g.dim[1]),
              cz = grid_axis(p[2], g.lo[2], g.cell, g.dim[2]);
    for (int z = max(cz - 1, 0); z <= min(cz + 1, g.dim[2] - 1); ++z)
        for (int y = max(cy - 1, 0); y <= min(cy + 1, g.dim[1] - 1); ++y)
            for (int x = max(cx - 1, 0); x <= min(cx + 1, g.dim[0] - 1); ++x) {
                const int c = x + g.dim[0] * (y + g.dim[1] * z);
                for (int q = cell_start[c]; q < cell_end[c]; ++q) f(q);
            }
}

constexpr int NRM_THREADS = 64;
// KDTreeSearchParamHybrid(radius, max_nn): the max_nn nearest of the points closer than the radius
// (strictly, like nanoflann's radius search), sorted by (d^2, original index), kept per thread in LDS
// columns top_d / top_j [rank][64].  Returns how many there are.
__device__ __forceinline__ int hybrid_collect(const Grid &g, const double *p, const double *__restrict__ sp,
                                              const int *__restrict__ cell_start, const int *__restrict__ cell_end,
                                              const int *__restrict__ idx_sorted, double r2, int max_nn, double *top_d, int *top_j,
                                              int t) {
    int have = 0;
    for_neighbours(g, p, cell_start, cell_end, [&](int q) {
        const double d = dist2(p, sp + 3 * (size_t)q);
        if (!(d < r2)) return;
        const int jq = idx_sorted[q];
        int r = have < max_nn ? have : max_nn - 1;
        if (have == max_nn) {  // full: only a candidate ahead of the current last one enters
            const double dl = top_d[r * NRM_THREADS + t];
            if (!(d < dl || (d == dl && jq < top_j[r * NRM_THREADS + t]))) return;
        }
        while (r > 0) {
            const double dp = top_d[(r - 1) * NRM_THREADS + t];
            const int jp = top_j[(r - 1) * NRM_THREADS + t];
            if (!(dp > d || (dp == d && jp > jq))) break;
            top_d[r * NRM_THREADS + t] = dp;
            top_j[r * NRM_THREADS + t] = jp;
            --r;
        }
        top_d[r * NRM_THREADS + t] = d;
        top_j[r * NRM_THREADS + t] = jq;
        if (have < max_nn) ++have;
    });
    return have;
}

}  // namespace
