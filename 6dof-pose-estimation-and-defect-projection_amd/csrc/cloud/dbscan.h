// ------------------------------------------------------------------ DBSCAN
// The grid cell is eps / sqrt(3) less a hair: two points of one cell are closer than eps, so the core points of a
// cell form a clique -- they are one component without looking -- and a cell pair needs ONE edge between two of
// their core points to be united.  Points within eps lie at most DB_R = 2 cells apart per axis: the neighbourhood
// is 25 x rows of 5 cells, each row one run of the cell-sorted points (row_run), so lanes 0..24 of a
// wave fetch the 25 runs at once and the wave takes the non-empty ones 64 points at a time.  (With cells of eps
// every core point united itself with every core neighbour: 350 k finds and compare-and-swaps for 9 k points,
// 340 us; cells as cliques leave about a tenth of that.)
// A cloud whose extent over eps is beyond the grid's cell budget gets cells of eps or more (make_grid doubles them until
// they fit): no cliques there, 9 rows of 3 cells, and every core point unites itself with every core neighbour
// (CLIQUE = false below).
#pragma once
#include "common.h"
#include "grid.h"

namespace {

struct DbCell { int x, y, z; };
__device__ __forceinline__ DbCell db_cell(const Grid &g, const double *p) {
    return {grid_axis(p[0], g.lo[0], g.cell, g.dim[0]), grid_axis(p[1], g.lo[1], g.cell, g.dim[1]),
            grid_axis(p[2], g.lo[2], g.cell, g.dim[2])};
}
// the run of row `r` (0 .. (2R+1)^2 - 1) around cell c: sorted positions rs .. re
template <int DB_R>
__device__ __forceinline__ void db_row(const Grid &g, const DbCell &c, int r, const int *__restrict__ cell_start,
                                       const int *__restrict__ cell_end, int &rs, int &re) {
    constexpr int DB_SIDE = 2 * DB_R + 1;
    const int y = c.y + r % DB_SIDE - DB_R, z = c.z + r / DB_SIDE - DB_R;
    rs = re = 0;
    if (r < DB_SIDE * DB_SIDE && y >= 0 && y < g.dim[1] && z >= 0 && z < g.dim[2]) {
        row_run(cell_start, cell_end, g.dim[0] * (y + g.dim[1] * z), max(c.x - DB_R, 0), min(c.x + DB_R, g.dim[0] - 1), rs, re);
    }
}
template <int DB_R, class F>
__device__ __forceinline__ void for_rows_wave(const Grid &g, const double *p, const int *__restrict__ cell_start,
                                              const int *__restrict__ cell_end, int lane, F f) {
    int rs, re;
    db_row<DB_R>(g, db_cell(g, p), lane, cell_start, cell_end, rs, re);
    unsigned long long busy = __builtin_amdgcn_ballot_w64(re > rs);
    while (busy) {  // wave-uniform
        const int b = __builtin_ctzll(busy);
        busy &= busy - 1;
        const int e = __builtin_amdgcn_readlane(re, b);
        for (int q0 = __builtin_amdgcn_readlane(rs, b); q0 < e; q0 += 64) f(q0 + lane, q0 + lane < e);  // wave-uniform trip count
    }
}

constexpr int DB_WPB = 4;  // point waves per workgroup
template <bool CLIQUE>
__global__ __launch_bounds__(DB_WPB * 64) void dbscan_core_kernel(Grid g, const double *__restrict__ sp, int64_t N,
                                                                 const int *__restrict__ cell_start,
                                                                 const int *__restrict__ cell_end, double e2, int min_points,
                                                                 const int *__restrict__ idx_sorted,
                                                                 int *__restrict__ core /* by original index */,
                                                                 int *__restrict__ parent) {
    const int lane = threadIdx.x & 63;
    const int64_t j = (int64_t)blockIdx.x * DB_WPB + (threadIdx.x >> 6);
    if (j >= N) return;  // wave-uniform
    const double p[3] = {sp[3 * j], sp[3 * j + 1], sp[3 * j + 2]};
    int cnt = 0;
    for_rows_wave<CLIQUE ? 2 : 1>(g, p, cell_start, cell_end, lane, [&](int q, bool valid) {
        const bool in = valid && dist2(p, sp + 3 * (size_t)q) < e2;
        cnt += __builtin_popcountll(__builtin_amdgcn_ballot_w64(in));
    });
    if (lane == 0) {
        const int i = idx_sorted[j];
        core[i] = cnt >= min_points;
        parent[i] = i;
    }
}

// a thread per cell: rep[c] = the smallest index among the cell's core points (none: INT_MAX), and every core point
// of the cell hangs under it -- the clique, united without an atomic
__global__ void dbscan_cell_kernel(int64_t n_cells, const int *__restrict__ cell_start, const int *__restrict__ cell_end,
                                   const int *__restrict__ idx_sorted,
                                   const int *__restrict__ core, int *__restrict__ rep, int *__restrict__ parent) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_cells) return;
    const int a = cell_start[c], e = cell_end[c];
    int r = 0x7FFFFFFF;
    for (int q = a; q < e; ++q) {
        const int i = idx_sorted[q];
        if (core[i]) r = min(r, i);
    }
    rep[c] = r;
    if (r == 0x7FFFFFFF) return;
    for (int q = a; q < e; ++q) {
        const int i = idx_sorted[q];
        if (core[i]) parent[i] = r;
    }
}

// Find with path halving.  parent[x] <= x always points at a member of x's component, and only roots are
// ever hooked (atomicCAS on parent[root] == root in the union loop), so overwriting a NON-root's parent with
// its grandparent -- a plain store, whoever wins a race stores an ancestor -- keeps every invariant and the
// component's smallest index as its root; without it the index-ordered hooking grows chains hundreds of
// links long.
__device__ __forceinline__ int uf_find(int *parent, int a) {
    int r = a;
    while (true) {
        const int p = ((volatile int *)parent)[r];
        if (p == r) return r;
        const int gp = ((volatile int *)parent)[p];
        if (gp != p) ((volatile int *)parent)[r] = gp;
        r = p;
    }
}

// Uniting the cells.  With cliques a wave per CELL (the wave of the cell's first point; the others leave): the cell's
// core points wait in LDS, the wave walks the neighbourhood once, and a core neighbour q in a cell ABOVE this one
// (the pair is seen from the lower cell) within eps of any of them lists q's cell -- the first of every run of equal
// cells in a pass of 64.  The union-find is touched once per cell at the end (its loads and compare-and-swaps are
// device-coherent, a microsecond each): the listed cells' components are resolved to their roots, and every
// distinct root above the smallest of them (and of the cell's own) is hooked under that one, so the lanes'
// compare-and-swaps go to different words.  Without cliques a wave per core point i lists its core neighbours of
// smaller index (the pair is seen from the larger) and unites itself with them the same way.
constexpr int DB_LIST = 128;  // listed cells per wave before the union-find is visited
template <bool CLIQUE>
__global__ __launch_bounds__(DB_WPB * 64) void dbscan_union_kernel(Grid g, const double *__restrict__ sp, int64_t N,
                                                                  const int *__restrict__ cell_start,
                                                                  const int *__restrict__ cell_end, const unsigned *__restrict__ cell_s,
                                                                  double e2, const int *__restrict__ idx_sorted,
                                                                  const int *__restrict__ core, const int *__restrict__ rep,
                                                                  int *__restrict__ parent) {
    __shared__ int list_all[DB_WPB][DB_LIST];
    __shared__ double mine_all[DB_WPB][64][3];
    const int lane = threadIdx.x & 63;
    int *list = list_all[threadIdx.x >> 6];
    double (*mine)[3] = mine_all[threadIdx.x >> 6];
    const int64_t j = (int64_t)blockIdx.x * DB_WPB + (threadIdx.x >> 6);
    if (j >= N) return;  // wave-uniform
    const unsigned ci = cell_s[j];
    int i = idx_sorted[j];
    if (CLIQUE) {
        if (cell_start[ci] != (int)j) return;  // wave-uniform: not the cell's first point
        i = rep[ci];
        if (i == 0x7FFFFFFF) return;  // no core point in the cell
    } else if (!core[i]) return;  // wave-uniform
    const double p[3] = {sp[3 * j], sp[3 * j + 1], sp[3 * j + 2]};
    const unsigned long long below = (1ull << lane) - 1ull;
    int listed = 0;
    auto unite = [&]() {
        __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): the list has landed
        for (int l0 = 0; l0 < listed; l0 += 64) {
            const bool act = l0 + lane < listed;
            const int r = act ? uf_find(parent, CLIQUE ? rep[list[l0 + lane]] : list[l0 + lane]) : 0x7FFFFFFF, ri = uf_find(parent, i);
            int low = min(r, ri);
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) low = min(low, __shfl_xor(low, off, 64));
#pragma unroll
            for (int round = 0; round < 2; ++round) {  // the listed roots, then i's own (lane 0)
                int a = round == 0 ? (act ? r : low) : (lane == 0 ? ri : low), b = low;
                while (a != b) {  // union: the larger root is hooked under the smaller one
                    if (a < b) { const int t = a; a = b; b = t; }
                    if (atomicCAS(&parent[a], a, b) == a) break;
                    a = uf_find(parent, a);
                    b = uf_find(parent, b);
                }
            }
        }
        listed = 0;
    };
    const int own_end = CLIQUE ? cell_end[ci] : (int)j + 1;
    for (int a0 = (int)j; a0 < own_end; a0 += 64) {  // the cell's points, 64 at a time (CLIQUE; else the one point)
        int n_mine = 1;
        if (CLIQUE) {
            const bool is_core = a0 + lane < own_end && core[idx_sorted[a0 + lane]];
            const unsigned long long cm = __builtin_amdgcn_ballot_w64(is_core);
            n_mine = __builtin_popcountll(cm);
            if (!n_mine) continue;  // wave-uniform
            if (is_core) {
                const int slot = __builtin_popcountll(cm & below);
                mine[slot][0] = sp[3 * (size_t)(a0 + lane)]; mine[slot][1] = sp[3 * (size_t)(a0 + lane) + 1];
                mine[slot][2] = sp[3 * (size_t)(a0 + lane) + 2];
            }
            __builtin_amdgcn_s_waitcnt(0xC07F);
        }
        for_rows_wave<CLIQUE ? 2 : 1>(g, p, cell_start, cell_end, lane, [&](int q, bool valid) {
            unsigned cq = 0;
            int other = 0;
            bool act = false;
            if (valid) {
                cq = cell_s[q];
                other = idx_sorted[q];
                act = (CLIQUE ? cq > ci : other < i) && core[other];
            }
            if (CLIQUE) {
                if (act) {
                    const double pq[3] = {sp[3 * (size_t)q], sp[3 * (size_t)q + 1], sp[3 * (size_t)q + 2]};
                    bool near = false;
                    for (int a = 0; a < n_mine; ++a) near |= dist2(mine[a], pq) < e2;
                    act = near;
                }
                const unsigned key = act ? cq : 0xFFFFFFFFu, before = __shfl_up(key, 1, 64);
                act = act && (lane == 0 || before != key);  // one lane per run of equal cells (position order = cell order)
            } else act = act && dist2(p, sp + 3 * (size_t)q) < e2;
            const unsigned long long mask = __builtin_amdgcn_ballot_w64(act);
            if (!mask) return;  // wave-uniform
            if (listed + 64 > DB_LIST) unite();
            if (act) list[listed + __builtin_popcountll(mask & below)] = CLIQUE ? (int)cq : other;
            listed += __builtin_popcountll(mask);
        });
    }
    unite();
}

// roots of core components in index order -> flags for the rank scan
__global__ void dbscan_root_kernel(int64_t N, const int *__restrict__ core, int *__restrict__ parent, int *__restrict__ root,
                                   unsigned *__restrict__ is_rep) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    int r = -1;
    if (core[i]) r = uf_find(parent, (int)i);
    root[i] = r;
    is_rep[i] = (r == (int)i) ? 1u : 0u;
}

// labels: a component's rank among the roots in index order; a point that is not core takes the smallest rank among
// the core points within eps (none: -1, noise).  A wave per point; the core points' waves leave at once.
template <bool CLIQUE>
__global__ __launch_bounds__(DB_WPB * 64) void dbscan_label_kernel(Grid g, const double *__restrict__ sp, int64_t N,
                                                                  const int *__restrict__ cell_start,
                                                                  const int *__restrict__ cell_end, double e2,
                                                                  const int *__restrict__ idx_sorted, const int *__restrict__ root,
                                                                  const unsigned *__restrict__ rank /* exclusive scan of is_rep */,
                                                                  int32_t *__restrict__ labels) {
    const int lane = threadIdx.x & 63;
    const int64_t j = (int64_t)blockIdx.x * DB_WPB + (threadIdx.x >> 6);
    if (j >= N) return;  // wave-uniform
    const int i = idx_sorted[j];
    if (root[i] >= 0) {  // wave-uniform
        if (lane == 0) labels[i] = (int32_t)rank[root[i]];
        return;
    }
    const double p[3] = {sp[3 * j], sp[3 * j + 1], sp[3 * j + 2]};
    int best = 0x7FFFFFFF;
    for_rows_wave<CLIQUE ? 2 : 1>(g, p, cell_start, cell_end, lane, [&](int q, bool valid) {
        if (!valid) return;
        const int rq = root[idx_sorted[q]];
        if (rq >= 0 && dist2(p, sp + 3 * (size_t)q) < e2) best = min(best, (int)rank[rq]);
    });
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) best = min(best, __shfl_xor(best, off, 64));
    if (lane == 0) labels[i] = best == 0x7FFFFFFF ? -1 : best;
}

}  // namespace
