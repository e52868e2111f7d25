// ------------------------------------------------------------------ FPFH (compute_fpfh_feature)
// Open3D 0.18 Feature.cpp: per point the SPFH histogram (3 x 11 bins of the Darboux-frame angles to
// the hybrid-search neighbours, the point itself skipped), then FPFH = own SPFH + the neighbours'
// SPFH weighted by 1 / squared distance, each third rescaled to 100.  Neighbour lists are written
// once ([rank][N], nearest first, ties by index) and read by both passes.
#pragma once
#include "common.h"
#include "grid.h"
#include "../features/acos_cr.h"

namespace {

__global__ __launch_bounds__(NRM_THREADS) void hybrid_list_kernel(Grid g, const double *__restrict__ sp, int64_t N,
                                                                  const int *__restrict__ cell_start,
                                                                  const int *__restrict__ cell_end,
                                                                  const int *__restrict__ idx_sorted, double r2, int max_nn,
                                                                  int *__restrict__ nbr_j, double *__restrict__ nbr_d,
                                                                  int *__restrict__ nbr_n) {
    extern __shared__ double lds[];
    double *top_d = lds;
    int *top_j = (int *)(lds + (size_t)max_nn * NRM_THREADS);
    const int t = threadIdx.x;
    const int64_t j = (int64_t)blockIdx.x * NRM_THREADS + t;
    if (j >= N) return;
    const double p[3] = {sp[3 * j], sp[3 * j + 1], sp[3 * j + 2]};
    const int have = hybrid_collect(g, p, sp, cell_start, cell_end, idx_sorted, r2, max_nn, top_d, top_j, t);
    const int64_t i = idx_sorted[j];
    nbr_n[i] = have;
    for (int k = 0; k < have; ++k) {
        nbr_j[(size_t)k * N + i] = top_j[k * NRM_THREADS + t];
        nbr_d[(size_t)k * N + i] = top_d[k * NRM_THREADS + t];
    }
}

// The same lists, one WAVE per query: the 64 lanes fetch a cell's points together, the candidates
// closer than the radius are packed into LDS (ballot + prefix count), and the max_nn nearest are
// extracted one by one with a wave-wide lexicographic argmin over (d^2, original index) -- the order
// of hybrid_collect -- every lane keeping the minimum of its strided share.  A query with more
// candidates than the LDS share raises `overflow`; the host then tries the larger share and, past that,
// the thread-per-query kernel.
// WCAP candidates per query wave (12 B each), WPB query waves per workgroup: <1024, 4> = 48 KB (three
// workgroups per CU) first, <4096, 2> = 96 KB for clouds with denser neighbourhoods
template <int HYB_WCAP, int HYB_WPB>
__global__ __launch_bounds__(HYB_WPB * 64) void hybrid_list_wave_kernel(Grid g, const double *__restrict__ sp, int64_t N,
                                                                       const int *__restrict__ cell_start,
                                                                       const int *__restrict__ cell_end,
                                                                       const int *__restrict__ idx_sorted, double r2, int max_nn,
                                                                       int *__restrict__ nbr_j, double *__restrict__ nbr_d,
                                                                       int *__restrict__ nbr_n, int *__restrict__ overflow) {
    __shared__ double cd_all[HYB_WPB][HYB_WCAP];
    __shared__ int cj_all[HYB_WPB][HYB_WCAP];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t j = (int64_t)blockIdx.x * HYB_WPB + wave;
    if (j >= N) return;  // wave-uniform
    double *cd = cd_all[wave];
    int *cj = cj_all[wave];
    const double p[3] = {sp[3 * j], sp[3 * j + 1], sp[3 * j + 2]};
    const int cx = grid_axis(p[0], g.lo[0], g.cell, g.dim[0]), cy = grid_axis(p[1], g.lo[1], g.cell, g.dim[1]),
              cz = grid_axis(p[2], g.lo[2], g.cell, g.dim[2]);
    int n_c = 0;
    bool over = false;
    for (int z = max(cz - 1, 0); z <= min(cz + 1, g.dim[2] - 1); ++z)
        for (int y = max(cy - 1, 0); y <= min(cy + 1, g.dim[1] - 1); ++y)
            for (int x = max(cx - 1, 0); x <= min(cx + 1, g.dim[0] - 1); ++x) {
                const int c = x + g.dim[0] * (y + g.dim[1] * z);
                const int e = cell_end[c];
                for (int q0 = cell_start[c]; q0 < e; q0 += 64) {  // wave-uniform bounds
                    const int q = q0 + lane;
                    double d = 0.0;
                    bool in = false;
                    if (q < e) { d = dist2(p, sp + 3 * (size_t)q); in = d < r2; }
                    const unsigned long long m = __builtin_amdgcn_ballot_w64(in);
                    const int at = n_c + __builtin_popcountll(m & ((1ull << lane) - 1ull));
                    if (in && at < HYB_WCAP) { cd[at] = d; cj[at] = idx_sorted[q]; }
                    n_c += __builtin_popcountll(m);
                    over |= n_c > HYB_WCAP;
                }
            }
    if (over) {  // wave-uniform
        if (lane == 0) atomicOr(overflow, 1);
        return;
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): the wave's LDS writes have landed
    const double inf = __longlong_as_double(0x7FF0000000000000ll);
    double lmin = inf;
    int lj = 0x7FFFFFFF, lidx = -1;
    for (int q = lane; q < n_c; q += 64) {
        const double d = cd[q];
        const int jq = cj[q];
        if (d < lmin || (d == lmin && jq < lj)) { lmin = d; lj = jq; lidx = q; }
    }
    const int have = n_c < max_nn ? n_c : max_nn;
    const int64_t i = idx_sorted[j];
    for (int r = 0; r < have; ++r) {
        double v = lmin;
        int vj = lj, owner = lane;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double ov = __shfl_xor(v, off, 64);
            const int oj = __shfl_xor(vj, off, 64), oo = __shfl_xor(owner, off, 64);
            if (ov < v || (ov == v && oj < vj)) { v = ov; vj = oj; owner = oo; }
        }
        if (lane == owner) {  // hand the entry over and find the share's next minimum
            nbr_j[(size_t)r * N + i] = vj;
            nbr_d[(size_t)r * N + i] = v;
            cd[lidx] = inf;
            cj[lidx] = 0x7FFFFFFF;
            lmin = inf; lj = 0x7FFFFFFF; lidx = -1;
            for (int q = lane; q < n_c; q += 64) {
                const double d = cd[q];
                const int jq = cj[q];
                if (d < lmin || (d == lmin && jq < lj)) { lmin = d; lj = jq; lidx = q; }
            }
        }
    }
    if (lane == 0) nbr_n[i] = have;
}

// Feature.cpp's ordering test acos(x1) > acos(x2).  Two arguments a few ulp apart (two points with one neighbourhood,
// hence one normal; a lattice) ask whether adjacent doubles round to the same angle: the fast acos (1-2 ulp) cannot say,
// so within 16 ulp of a tie the correctly rounded one decides (features/acos_cr.h), as the host's libm does.  Equal
// arguments never swap, an argument above 1 (NaN angle) never does.
__device__ __forceinline__ bool pair_order_swaps(double x1, double x2) {
    const double c1 = acos(x1), c2 = acos(x2);
    if (x1 != x2 && fabs(c1 - c2) <= 16.0 * 2.220446049250313e-16 * fmax(c1, c2)) return acos_cr(x1) > acos_cr(x2);
    return c1 > c2;
}

// Feature.cpp ComputePairFeatures, operation for operation (oracle/features.c pair_features)
__device__ __forceinline__ void pair_features_dev(const double *p1, const double *n1, const double *p2, const double *n2,
                                                  double r[4]) {
    double dp[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
    r[0] = r[1] = r[2] = 0.0;
    r[3] = sqrt(dot3(dp, dp));
    if (r[3] == 0.0) return;
    double a[3] = {n1[0], n1[1], n1[2]}, b[3] = {n2[0], n2[1], n2[2]};
    const double angle1 = dot3(a, dp) / r[3], angle2 = dot3(b, dp) / r[3];
    if (pair_order_swaps(fabs(angle1), fabs(angle2))) {
        for (int k = 0; k < 3; ++k) { a[k] = n2[k]; b[k] = n1[k]; dp[k] = -dp[k]; }
        r[2] = -angle2;
    } else {
        r[2] = angle1;
    }
    double v[3], w[3];
    cross3(dp, a, v);
    const double vn = sqrt(dot3(v, v));
    if (vn == 0.0) { r[0] = r[1] = r[2] = r[3] = 0.0; return; }
    for (int k = 0; k < 3; ++k) v[k] /= vn;
    cross3(a, v, w);
    r[1] = dot3(v, b);
    r[0] = atan2(dot3(w, b), dot3(a, b));
}

__device__ __forceinline__ int bin11(double x) {
    int h = (int)floor(x);
    return h < 0 ? 0 : (h >= 11 ? 10 : h);
}

__global__ __launch_bounds__(NRM_THREADS) void spfh_kernel(const double *__restrict__ pts, const double *__restrict__ nrm,
                                                           int64_t N, const int *__restrict__ nbr_j,
                                                           const int *__restrict__ nbr_n, double *__restrict__ spfh) {
    __shared__ double hist[33][NRM_THREADS];
    const int t = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * NRM_THREADS + t;
    if (i >= N) return;
#pragma unroll
    for (int k = 0; k < 33; ++k) hist[k][t] = 0.0;
    const int n = nbr_n[i];
    if (n > 1) {
        const double incr = 100.0 / (double)(n - 1);
        const double p1[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]}, n1[3] = {nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]};
        for (int k = 1; k < n; ++k) {
            const size_t q = (size_t)nbr_j[(size_t)k * N + i];
            double pf[4];
            pair_features_dev(p1, n1, pts + 3 * q, nrm + 3 * q, pf);
            hist[bin11(11.0 * (pf[0] + 3.14159265358979323846) / (2.0 * 3.14159265358979323846))][t] += incr;
            hist[11 + bin11(11.0 * (pf[1] + 1.0) * 0.5)][t] += incr;
            hist[22 + bin11(11.0 * (pf[2] + 1.0) * 0.5)][t] += incr;
        }
    }
#pragma unroll
    for (int k = 0; k < 33; ++k) spfh[33 * i + k] = hist[k][t];
}

__global__ __launch_bounds__(NRM_THREADS) void fpfh_kernel(int64_t N, const int *__restrict__ nbr_j, const double *__restrict__ nbr_d,
                                                           const int *__restrict__ nbr_n, const double *__restrict__ spfh,
                                                           double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * NRM_THREADS + threadIdx.x;
    if (i >= N) return;
    double f[33];
#pragma unroll
    for (int k = 0; k < 33; ++k) f[k] = 0.0;
    const int n = nbr_n[i];
    if (n > 1) {
        double sum[3] = {0.0, 0.0, 0.0};
        for (int k = 1; k < n; ++k) {
            const double dist = nbr_d[(size_t)k * N + i];
            if (dist == 0.0) continue;
            const double *h = spfh + 33 * (size_t)nbr_j[(size_t)k * N + i];
#pragma unroll
            for (int j = 0; j < 33; ++j) {
                const double val = h[j] / dist;
                sum[j / 11] += val;
                f[j] += val;
            }
        }
#pragma unroll
        for (int j = 0; j < 3; ++j)
            if (sum[j] != 0.0) sum[j] = 100.0 / sum[j];
#pragma unroll
        for (int j = 0; j < 33; ++j) {
            f[j] *= sum[j / 11];
            f[j] += spfh[33 * i + j];
        }
    }
#pragma unroll
    for (int j = 0; j < 33; ++j) out[33 * i + j] = f[j];
}

// nearest target feature of every source feature: squared L2 over the 33 components summed in order
// (float64, as KDTreeFlann::SearchKNN on the Feature matrix), ties to the lower index.  Grid = source
// blocks x target chunks: a workgroup holds 64 source features in registers (one per thread), streams
// its chunk of FM_CHUNK target features through LDS and leaves (d^2, index) per source and chunk; a
// second kernel takes the minimum over the chunks in chunk order (strict <, so the lowest index wins a tie).
constexpr int FM_TILE = 64;
constexpr int FM_CHUNK = 1024;
__global__ __launch_bounds__(64) void feature_match_kernel(const double *__restrict__ fs, int64_t Ns, const double *__restrict__ ft,
                                                           int64_t Nt, double *__restrict__ part_d, int32_t *__restrict__ part_j) {
    __shared__ double tile[FM_TILE][33];
    const int t = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * 64 + t;
    const int64_t c0 = (int64_t)blockIdx.y * FM_CHUNK, c1 = c0 + FM_CHUNK < Nt ? c0 + FM_CHUNK : Nt;
    double a[33];
#pragma unroll
    for (int k = 0; k < 33; ++k) a[k] = i < Ns ? fs[33 * i + k] : 0.0;
    double best = __longlong_as_double(0x7FF0000000000000ll);
    int bj = -1;
    for (int64_t j0 = c0; j0 < c1; j0 += FM_TILE) {
        const int m = (int)(c1 - j0 < FM_TILE ? c1 - j0 : FM_TILE);
        __syncthreads();
        for (int e = t; e < m * 33; e += 64) tile[e / 33][e % 33] = ft[33 * j0 + e];
        __syncthreads();
        for (int jj = 0; jj < m; ++jj) {
            double d = 0.0;
#pragma unroll
            for (int k = 0; k < 33; ++k) {
                const double e = a[k] - tile[jj][k];
                d += e * e;
            }
            if (d < best) { best = d; bj = (int)(j0 + jj); }
        }
    }
    if (i < Ns) {
        part_d[(size_t)blockIdx.y * Ns + i] = best;
        part_j[(size_t)blockIdx.y * Ns + i] = bj;
    }
}

__global__ void feature_match_fold_kernel(int64_t Ns, int n_chunks, const double *__restrict__ part_d,
                                          const int32_t *__restrict__ part_j, int32_t *__restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Ns) return;
    double best = __longlong_as_double(0x7FF0000000000000ll);
    int bj = -1;
    for (int c = 0; c < n_chunks; ++c) {
        const double d = part_d[(size_t)c * Ns + i];
        if (d < best) { best = d; bj = part_j[(size_t)c * Ns + i]; }
    }
    idx[i] = bj;
}

}  // namespace
