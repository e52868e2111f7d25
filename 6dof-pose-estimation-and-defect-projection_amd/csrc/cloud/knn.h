// ------------------------------------------------------------------ k nearest neighbours (mean distance)
// One thread per query walks the grid shell by shell around its own cell: after the shell at
// Chebyshev distance rho every unvisited point is farther than rho * cell, so the search ends as
// soon as the k-th best squared distance is within (rho * cell)^2.  Near cells come first, so the
// k smallest squared distances -- kept sorted ascending in LDS, k x 64 doubles per workgroup --
// settle after little more than k insertions.  Candidates are fetched four at a time.
#pragma once
#include "common.h"
#include "grid.h"

namespace {

constexpr int KNN_THREADS = 64;
__global__ __launch_bounds__(KNN_THREADS) void knn_mean_kernel(Grid g, const double *__restrict__ sp, int64_t N,
                                                               const int *__restrict__ cell_start,
                                                               const int *__restrict__ cell_end,
                                                               const int *__restrict__ idx_sorted, int k,
                                                               double *__restrict__ avg /* by original index */,
                                                               const int *__restrict__ gate /* run only if *gate != 0 */) {
    extern __shared__ double top[];  // element r of thread t at top[r * KNN_THREADS + t]
    const int t = threadIdx.x;
    const int64_t j = (int64_t)blockIdx.x * KNN_THREADS + t;
    if (j >= N || *gate == 0) return;
    const double p[3] = {sp[3 * j], sp[3 * j + 1], sp[3 * j + 2]};
    const int m = (int)(N < k ? N : k);
    const double inf = __longlong_as_double(0x7FF0000000000000ll);
    int have = 0;
    double worst = inf;  // the m-th best once m candidates are in
    auto offer = [&](double d) {
        if (!(d < worst)) return;
        int r = have < m ? have : m - 1;  // slot that opens up
        while (r > 0 && top[(r - 1) * KNN_THREADS + t] > d) {
            top[r * KNN_THREADS + t] = top[(r - 1) * KNN_THREADS + t];
            --r;
        }
        top[r * KNN_THREADS + t] = d;
        if (have < m) ++have;
        if (have == m) worst = top[(m - 1) * KNN_THREADS + t];
    };
    const int cx = grid_axis(p[0], g.lo[0], g.cell, g.dim[0]), cy = grid_axis(p[1], g.lo[1], g.cell, g.dim[1]),
              cz = grid_axis(p[2], g.lo[2], g.cell, g.dim[2]);
    const int far = max(max(max(cx, g.dim[0] - 1 - cx), max(cy, g.dim[1] - 1 - cy)), max(cz, g.dim[2] - 1 - cz));
    for (int rho = 0; rho <= far; ++rho) {
        for (int z = max(cz - rho, 0); z <= min(cz + rho, g.dim[2] - 1); ++z)
            for (int y = max(cy - rho, 0); y <= min(cy + rho, g.dim[1] - 1); ++y) {
                const bool face = (abs(z - cz) == rho) || (abs(y - cy) == rho);
                for (int x = max(cx - rho, 0); x <= min(cx + rho, g.dim[0] - 1); ++x) {
                    if (!face && abs(x - cx) != rho) continue;  // interior of the cube: visited by an earlier shell
                    const int c = x + g.dim[0] * (y + g.dim[1] * z);
                    const int e = cell_end[c];
                    for (int q = cell_start[c]; q < e; q += 4) {
                        double d[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u) d[u] = (q + u < e) ? dist2(p, sp + 3 * (size_t)(q + u)) : inf;
#pragma unroll
                        for (int u = 0; u < 4; ++u) offer(d[u]);
                    }
                }
            }
        const double reach = (double)rho * g.cell * (1.0 - 1e-9);
        if (have == m && worst <= reach * reach) break;
    }
    double s = 0.0;
    for (int r = 0; r < m; ++r) s += sqrt(top[r * KNN_THREADS + t]);
    avg[idx_sorted[j]] = m > 0 ? s / (double)m : -1.0;
}

// The k smallest of the n_c squared distances in cand[] (a wave's LDS share), summed as square roots in
// ascending order -- the order the oracle's sorted top-k list is summed in.  `hi` is a value with
// chi = #{cand <= hi} >= m.  Three steps, none of them a serial extraction (75 wave-wide argmins cost
// more than everything else the query does):
//   1. halve [lo, hi] on the value until about m + 24 candidates lie below hi (counts by ballot),
//   2. compact those survivors to the front of cand[] (in place: writes trail the reads),
//   3. rank each survivor by counting the survivors below it ((d, position) order, so ties get distinct
//      ranks), write sqrt(d) of ranks < m to srt[rank], and sum srt[0..m) in order.
// Same multiset, same summation order, same bits as the extraction it replaces.
constexpr int KNN_KMAX = 304;  // k <= 300 (pedp_knn_mean_distance)
__device__ __forceinline__ double knn_select_sum(double *cand, int n_c, int m, double hi, int chi, double *srt, int lane) {
    const unsigned long long below = (1ull << lane) - 1ull;
    double lo = -1.0;  // #{cand <= lo} < m
    for (int it = 0; it < 64 && chi > m + 24; ++it) {
        const double mid = 0.5 * ((lo > 0.0 ? lo : 0.0) + hi);
        if (!(mid > lo && mid < hi)) break;
        int cnt = 0;
        for (int q0 = 0; q0 < n_c; q0 += 64) {
            const int q = q0 + lane;
            cnt += __builtin_popcountll(__builtin_amdgcn_ballot_w64(q < n_c && cand[q] <= mid));
        }
        if (cnt >= m) { hi = mid; chi = cnt; } else lo = mid;
    }
    int S = 0;
    for (int q0 = 0; q0 < n_c; q0 += 64) {
        const int q = q0 + lane;
        const double d = q < n_c ? cand[q] : 0.0;
        const bool keep = q < n_c && d <= hi;
        const unsigned long long mask = __builtin_amdgcn_ballot_w64(keep);
        if (keep) cand[S + __builtin_popcountll(mask & below)] = d;  // S + ... <= q: behind every unread element
        S += __builtin_popcountll(mask);
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
    for (int i = lane; i < S; i += 64) {
        const double d = cand[i];
        int r0 = 0, r1 = 0;
        int j = 0;
        for (; j + 1 < S; j += 2) {
            const double o0 = cand[j], o1 = cand[j + 1];
            r0 += (o0 < d || (o0 == d && j < i)) ? 1 : 0;
            r1 += (o1 < d || (o1 == d && j + 1 < i)) ? 1 : 0;
        }
        if (j < S) { const double o0 = cand[j]; r0 += (o0 < d || (o0 == d && j < i)) ? 1 : 0; }
        const int rank = r0 + r1;
        if (rank < m) srt[rank] = sqrt(d);
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);
    double s = 0.0;
    for (int r = 0; r < m; ++r) s += srt[r];  // every lane forms the same sum
    return s;
}

// One WAVE per query on the grid (clouds above KNN_SMALL_MAX points).  The candidates are the points of the cube of
// cells within rho of the query's cell: (2 rho + 1)^2 x rows, each one run of the cell-sorted points
// (row_run), so the lanes fetch the runs' bounds at once, and the candidates are then numbered through
// the runs and fetched 256 at a time -- four independent loads in flight per lane.  (Visiting the cells one after the
// other cost a memory latency per cell, most of them empty in a scanned sheet.)  The squared distances are parked
// in LDS; the cube is large enough when at least k of them lie within its reach rho * cell (every point outside
// the cube is farther: the k-th best is then settled -- the rule of the thread-per-query kernel's shells), else
// the next larger cube is gathered.  knn_select_sum does the rest.  A query whose cube holds more candidates than
// the LDS share raises `overflow`; the host then runs the thread-per-query kernel for the cloud.
constexpr int KNN_WCAP = 2048;  // candidates per query wave (16 KB)
constexpr int KNN_WPB = 4;      // query waves per workgroup
__global__ __launch_bounds__(KNN_WPB * 64) void knn_mean_wave_kernel(Grid g, const double *__restrict__ sp, int64_t N,
                                                                    const int *__restrict__ cell_start,
                                                                    const int *__restrict__ cell_end,
                                                                    const int *__restrict__ idx_sorted, int k,
                                                                    double *__restrict__ avg, int *__restrict__ overflow) {
    __shared__ double cand_all[KNN_WPB][KNN_WCAP];
    __shared__ double srt_all[KNN_WPB][KNN_KMAX];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t j = (int64_t)blockIdx.x * KNN_WPB + wave;
    if (j >= N) return;  // wave-uniform
    double *cand = cand_all[wave];
    const double p[3] = {sp[3 * j], sp[3 * j + 1], sp[3 * j + 2]};
    const int m = (int)(N < k ? N : k);
    const int cx = grid_axis(p[0], g.lo[0], g.cell, g.dim[0]), cy = grid_axis(p[1], g.lo[1], g.cell, g.dim[1]),
              cz = grid_axis(p[2], g.lo[2], g.cell, g.dim[2]);
    const int far = max(max(max(cx, g.dim[0] - 1 - cx), max(cy, g.dim[1] - 1 - cy)), max(cz, g.dim[2] - 1 - cz));
    int n_c = 0, within = 0;
    double reach2 = 0.0;
    for (int rho = 1;; ++rho) {
        n_c = 0;
        const int side = 2 * rho + 1, rows = side * side;
        const int x0 = max(cx - rho, 0), x1 = min(cx + rho, g.dim[0] - 1);
        for (int r0 = 0; r0 < rows; r0 += 64) {
            const int r = r0 + lane, y = cy + r % side - rho, z = cz + r / side - rho;
            int rs = 0, re = 0;
            if (r < rows && y >= 0 && y < g.dim[1] && z >= 0 && z < g.dim[2])
                row_run(cell_start, cell_end, g.dim[0] * (y + g.dim[1] * z), x0, x1, rs, re);
            const int cnt = re - rs;
            int incl = cnt;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int up = __shfl_up(incl, off, 64);
                if (lane >= off) incl += up;
            }
            const int first = incl - cnt, tot = __builtin_amdgcn_readlane(incl, 63);
            const unsigned long long busy = __builtin_amdgcn_ballot_w64(cnt > 0);
            if (n_c + tot <= KNN_WCAP) {  // wave-uniform; beyond it the query overflows below
                for (int c0 = 0; c0 < tot; c0 += 256) {
                    int src[4] = {0, 0, 0, 0};
                    for (unsigned long long bb = busy; bb; bb &= bb - 1) {  // the run each of the four candidates lies in
                        const int b = __builtin_ctzll(bb);
                        const int pb = __builtin_amdgcn_readlane(first, b), sb = __builtin_amdgcn_readlane(rs, b);
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const int idx = c0 + 64 * u + lane;
                            if (idx >= pb) src[u] = sb + (idx - pb);
                        }
                    }
                    double d[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) d[u] = dist2(p, sp + 3 * (size_t)(c0 + 64 * u + lane < tot ? src[u] : 0));
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (c0 + 64 * u + lane < tot) cand[n_c + c0 + 64 * u + lane] = d[u];
                }
            }
            n_c += tot;
        }
        if (n_c > KNN_WCAP) {  // wave-uniform
            if (lane == 0) atomicOr(overflow, 1);
            return;
        }
        __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): the wave's LDS writes have landed
        const double reach = (double)rho * g.cell * (1.0 - 1e-9);
        reach2 = reach * reach;
        within = 0;
        for (int q0 = 0; q0 < n_c; q0 += 64) {
            const int q = q0 + lane;
            within += __builtin_popcountll(__builtin_amdgcn_ballot_w64(q < n_c && cand[q] <= reach2));
        }
        if (within >= m || rho >= far) break;  // rho >= far: the cube is the whole grid
    }
    double s;
    if (within >= m) s = knn_select_sum(cand, n_c, m, reach2, within, srt_all[wave], lane);
    else {  // the whole cloud without k points in reach: all n_c = N >= m candidates compete
        double mx = 0.0;
        for (int q = lane; q < n_c; q += 64) mx = fmax(mx, cand[q]);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off, 64));
        s = knn_select_sum(cand, n_c, m, mx, n_c, srt_all[wave], lane);
    }
    if (lane == 0) avg[idx_sorted[j]] = m > 0 ? s / (double)m : -1.0;
}

// Small clouds (the largest cluster that reaches the outlier filter is a few thousand points): one
// WAVE per query.  The wave writes the squared distances to all N points into LDS and hands them to
// knn_select_sum with the largest of them as the first bound.  Same multiset and same summation
// order as the grid kernel and the oracle.
constexpr int KNN_SMALL_MAX = 4096;  // 32 KB of distances per query wave; beyond ~4k points the grid walk is faster
__global__ __launch_bounds__(64) void knn_mean_small_kernel(const double *__restrict__ pts, int N, int k,
                                                            double *__restrict__ avg) {
    extern __shared__ double dist[];  // N squared distances of this query
    __shared__ double srt[KNN_KMAX];
    const int lane = threadIdx.x, i = blockIdx.x;
    const double p[3] = {pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]};
    double mx = 0.0;
    for (int q = lane; q < N; q += 64) {
        const double d = dist2(p, pts + 3 * (size_t)q);
        dist[q] = d;
        mx = fmax(mx, d);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off, 64));
    const int m = N < k ? N : k;
    __builtin_amdgcn_s_waitcnt(0xC07F);
    const double s = knn_select_sum(dist, N, m, mx, N, srt, lane);
    if (lane == 0) avg[i] = m > 0 ? s / (double)m : -1.0;
}

}  // namespace
