// ------------------------------------------------------------------ plane RANSAC
#pragma once
#include "common.h"

namespace {

__host__ __device__ inline unsigned long long splitmix64(unsigned long long x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
__host__ __device__ inline void sample3(unsigned long long seed, long long t, long long N, long long out[3]) {
    unsigned long long s = splitmix64(seed ^ splitmix64((unsigned long long)t));
    int n = 0;
    while (n < 3) {
        s = splitmix64(s);
        const long long c = (long long)(s % (unsigned long long)N);
        bool dup = false;
        for (int q = 0; q < n; ++q) dup |= (out[q] == c);
        if (!dup) out[n++] = c;
    }
}
__host__ __device__ inline bool triangle_plane(const double *p0, const double *p1, const double *p2, double pl[4]) {
    const double a[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]}, b[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
    const double x = a[1] * b[2] - a[2] * b[1], y = a[2] * b[0] - a[0] * b[2], z = a[0] * b[1] - a[1] * b[0];
    const double n = sqrt((x * x + y * y) + z * z);
    if (!(n > 0.0)) return false;
    pl[0] = x / n; pl[1] = y / n; pl[2] = z / n;
    pl[3] = -((pl[0] * p0[0] + pl[1] * p0[1]) + pl[2] * p0[2]);
    return true;
}
__host__ __device__ inline double plane_dist(const double pl[4], const double *p) {
    return fabs(((pl[0] * p[0] + pl[1] * p[1]) + pl[2] * p[2]) + pl[3]);
}

// Two kernels.  The first forms every iteration's plane (a thread per iteration; a plane that does not exist --
// collinear sample -- gets a NaN offset, which no distance test passes, and the count -1).  The second counts
// inliers tile by tile: a workgroup holds 256 points in registers and runs RS_PLANES planes from LDS over them,
// so the cloud is read once per RS_PLANES iterations (a workgroup per iteration streaming the whole cloud
// moved 228 MB through L2 for 9.5 k points x 1000 iterations: 166 us).  Integer adds: any order, same counts.
constexpr int RS_PLANES = 64;
// ransac_count_kernel takes a slab of RS_PLANES iterations per blockIdx.y, and a launch holds 65535 blocks in y
// (hipDeviceProp_t::maxGridSize[1] is 65536 on gfx950): the most iterations one call accepts
constexpr int RS_MAX_ITERATIONS = RS_PLANES * 65535;  // 4,194,240
__global__ void ransac_plane_kernel(const double *__restrict__ pts, long long N, unsigned long long seed, int n_iter,
                                    double *__restrict__ planes, int *__restrict__ counts) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_iter) return;
    long long s[3];
    double pl[4];
    sample3(seed, t, N, s);
    const bool ok = triangle_plane(pts + 3 * s[0], pts + 3 * s[1], pts + 3 * s[2], pl);
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    for (int k = 0; k < 4; ++k) planes[4 * (size_t)t + k] = ok ? pl[k] : (k == 3 ? nan : 0.0);
    counts[t] = ok ? 0 : -1;
}
__global__ __launch_bounds__(256) void ransac_count_kernel(const double *__restrict__ pts, long long N, double threshold, int n_iter,
                                                           const double *__restrict__ planes, int *__restrict__ counts) {
    __shared__ double pl_s[RS_PLANES][4];
    __shared__ int cnt_s[RS_PLANES];
    const int t0 = blockIdx.y * RS_PLANES, nt = min(RS_PLANES, n_iter - t0);
    if (threadIdx.x < RS_PLANES) {
        cnt_s[threadIdx.x] = 0;
        if ((int)threadIdx.x < nt)
            for (int k = 0; k < 4; ++k) pl_s[threadIdx.x][k] = planes[4 * (size_t)(t0 + threadIdx.x) + k];
    }
    __syncthreads();
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool have = i < N;
    double p[3] = {0.0, 0.0, 0.0};
    if (have) { p[0] = pts[3 * i]; p[1] = pts[3 * i + 1]; p[2] = pts[3 * i + 2]; }
    for (int t = 0; t < nt; ++t) {
        const double pl[4] = {pl_s[t][0], pl_s[t][1], pl_s[t][2], pl_s[t][3]};
        const int c = __builtin_popcountll(__builtin_amdgcn_ballot_w64(have && plane_dist(pl, p) < threshold));
        if ((threadIdx.x & 63) == 0 && c) atomicAdd(&cnt_s[t], c);
    }
    __syncthreads();
    if ((int)threadIdx.x < nt && cnt_s[threadIdx.x]) atomicAdd(&counts[t0 + threadIdx.x], cnt_s[threadIdx.x]);
}

// the best iteration -- most inliers, the earliest on ties -- with its three sampled points and its plane (the one the
// counts were taken with), in one small block: out[0] = iteration (-1: no plane at all), out[1..9] = the points,
// out[10..13] = the plane.  The host-array entry reads the points back and forms the plane itself; the device-resident
// chain hands the block to plane_keep_kernel and never asks.
__global__ __launch_bounds__(256) void ransac_best_kernel(const int *__restrict__ counts, int n_iter, const double *__restrict__ pts,
                                                          long long N, unsigned long long seed, const double *__restrict__ planes,
                                                          double *__restrict__ out) {
    __shared__ int cnt_s[256], it_s[256];
    int bc = -1, bt = -1;
    for (int t = threadIdx.x; t < n_iter; t += 256)
        if (counts[t] > bc) { bc = counts[t]; bt = t; }  // ascending t: the earliest of the thread's share
    cnt_s[threadIdx.x] = bc;
    it_s[threadIdx.x] = bt;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) {
            const int oc = cnt_s[threadIdx.x + w], ot = it_s[threadIdx.x + w];
            if (oc > cnt_s[threadIdx.x] || (oc == cnt_s[threadIdx.x] && ot >= 0 && (it_s[threadIdx.x] < 0 || ot < it_s[threadIdx.x]))) {
                cnt_s[threadIdx.x] = oc;
                it_s[threadIdx.x] = ot;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int best = it_s[0];
        out[0] = (double)best;
        if (best >= 0) {
            long long s[3];
            sample3(seed, best, N, s);
            for (int q = 0; q < 3; ++q)
                for (int k = 0; k < 3; ++k) out[1 + 3 * q + k] = pts[3 * s[q] + k];
            for (int k = 0; k < 4; ++k) out[10 + k] = planes[4 * (size_t)best + k];
        }
    }
}

// GetPlaneFromPoints, oracle/cloudops.c pedp_oracle_plane_from_points: centroid of the inliers, their six second moments
// about it, the largest-determinant closed form.  Every sum is taken in BLOCKS of the cloud -- the 256 points [256 j, 256 j +
// 256) contribute their value if they are inliers and zero otherwise, a block is added in a fixed binary tree, t[i] += t[i + w]
// for w = 128 ... 1, the block sums are added in order of j -- the order the device takes (refit_* kernels below:
// pedp_preprocess_source refits without a trip to the host and without compacting the inliers); this host statement serves
// pedp_segment_plane.  Differs from Open3D's running sums by rounding only.  idx ascends.
inline double block_tree_sum(double *t) {
    for (int w = 128; w >= 1; w >>= 1)
        for (int i = 0; i < w; ++i) t[i] += t[i + w];
    return t[0];
}
__host__ __device__ inline void plane_closed_form(const double c[3], const double m[6], double pl[4]) {
    pl[0] = pl[1] = pl[2] = pl[3] = 0.0;
    const double xx = m[0], xy = m[1], xz = m[2], yy = m[3], yz = m[4], zz = m[5];
    const double det_x = yy * zz - yz * yz, det_y = xx * zz - xz * xz, det_z = xx * yy - xy * xy;
    double a, b, cc;
    if (det_x >= det_y && det_x >= det_z) { a = det_x; b = xz * yz - xy * zz; cc = xy * yz - xz * yy; }
    else if (det_y >= det_z) { a = xz * yz - xy * zz; b = det_y; cc = xy * xz - yz * xx; }
    else { a = xy * yz - xz * yy; b = xy * xz - yz * xx; cc = det_z; }
    const double nrm = sqrt((a * a + b * b) + cc * cc);
    if (!(nrm > 0.0)) return;
    pl[0] = a / nrm; pl[1] = b / nrm; pl[2] = cc / nrm;
    pl[3] = -((pl[0] * c[0] + pl[1] * c[1]) + pl[2] * c[2]);
}
void blocked_sums(const double *pts, const int32_t *idx, int64_t n, const double *r0, int nq, double *out) {
    const int A[6] = {0, 0, 0, 1, 1, 2}, B[6] = {0, 1, 2, 1, 2, 2};
    double t[6][256];
    for (int q = 0; q < nq; ++q) out[q] = 0.0;
    int64_t i = 0;
    while (i < n) {
        const int64_t blk = idx[i] / 256;
        for (int q = 0; q < nq; ++q)
            for (int k = 0; k < 256; ++k) t[q][k] = 0.0;
        for (; i < n && idx[i] / 256 == blk; ++i) {
            const double *p = pts + 3 * (int64_t)idx[i];
            const int k = (int)(idx[i] % 256);
            if (!r0) { t[0][k] = p[0]; t[1][k] = p[1]; t[2][k] = p[2]; continue; }
            const double r[3] = {p[0] - r0[0], p[1] - r0[1], p[2] - r0[2]};
            for (int q = 0; q < nq; ++q) t[q][k] = r[A[q]] * r[B[q]];
        }
        for (int q = 0; q < nq; ++q) out[q] += block_tree_sum(t[q]);
    }
}
void plane_from_points(const double *pts, const int32_t *idx, int64_t n, double pl[4]) {
    pl[0] = pl[1] = pl[2] = pl[3] = 0.0;
    if (n < 3) return;
    double c[3], m[6];
    blocked_sums(pts, idx, n, nullptr, 3, c);
    for (int k = 0; k < 3; ++k) c[k] /= (double)n;
    blocked_sums(pts, idx, n, c, 6, m);
    plane_closed_form(c, m, pl);
}

// ---- the same on the device: per block of 256 points the tree sums of NV values per inlier (and, NV = 3, the block's
// inlier count), then the blocks added in order.
// NV = 3: the coordinates; NV = 6: the products of the residuals about the centroid in res[0..2].  part: NV (+ 1) per block.
template <int NV>
__global__ __launch_bounds__(256) void refit_block_kernel(const double *__restrict__ pts, int64_t N, const double *__restrict__ best, double thr,
                                                          const double *__restrict__ res, double *__restrict__ part) {
    constexpr int NP = NV == 3 ? 4 : 6;
    __shared__ double t[NP][256];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double v[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) v[k] = 0.0;
    if (i < N && best[0] >= 0.0) {
        const double pl[4] = {best[10], best[11], best[12], best[13]};
        const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
        const double p[3] = {x, y, z};
        if (plane_dist(pl, p) < thr) {
            if constexpr (NV == 3) { v[0] = x; v[1] = y; v[2] = z; v[3] = 1.0; }
            else {
                const double rx = x - res[0], ry = y - res[1], rz = z - res[2];
                v[0] = rx * rx; v[1] = rx * ry; v[2] = rx * rz; v[3] = ry * ry; v[4] = ry * rz; v[5] = rz * rz;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NP; ++k) t[k][threadIdx.x] = v[k];
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {  // t[i] += t[i + w], i < w: the oracle's tree
        if ((int)threadIdx.x < w)
#pragma unroll
            for (int k = 0; k < NP; ++k) t[k][threadIdx.x] += t[k][threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x < NP) part[NP * (size_t)blockIdx.x + threadIdx.x] = t[threadIdx.x][0];
}
// NV = 3: res[0..2] = centroid, res[7] = number of inliers.  NV = 6: res[3..6] = the plane (res[0..2], res[7] are read).
template <int NV>
__global__ __launch_bounds__(256) void refit_fold_kernel(const double *__restrict__ part, int64_t n_blocks, double *__restrict__ res) {
    constexpr int NP = NV == 3 ? 4 : 6;
    __shared__ double stage[NP * 1024];
    __shared__ double m[6];
    double s = 0.0;
    for (int64_t base = 0; base < n_blocks; base += 1024) {  // the block sums through LDS, then added in order: a lane per value
        const int nb = (int)(n_blocks - base < 1024 ? n_blocks - base : 1024);
        for (int j = threadIdx.x; j < NP * nb; j += 256) stage[j] = part[NP * (size_t)base + j];
        __syncthreads();
        if ((int)threadIdx.x < NP)
            for (int b = 0; b < nb; b += 8) {
                double v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = b + j < nb ? stage[NP * (b + j) + threadIdx.x] : 0.0;
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (b + j < nb) s += v[j];
            }
        __syncthreads();
    }
    if (NV == 3) {  // (the count is a sum of ones: exact in any order)
        if (threadIdx.x == 3) m[0] = s;
        __syncthreads();
        if (threadIdx.x < 3) res[threadIdx.x] = s / m[0];
        if (threadIdx.x == 3) res[7] = s;
        return;
    }
    if (threadIdx.x < 6) m[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double pl[4] = {0, 0, 0, 0};
        if (res[7] >= 3.0) {
            const double c[3] = {res[0], res[1], res[2]};
            plane_closed_form(c, m, pl);
        }
        for (int k = 0; k < 4; ++k) res[3 + k] = pl[k];
    }
}

// ---- the plane's keep flags (selected in index order: select.h)
__global__ void plane_keep_kernel(const double *__restrict__ pts, int64_t N, double a, double b, double cc, double d, double thr,
                                  int inliers, unsigned *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const double pl[4] = {a, b, cc, d};
    const bool in = plane_dist(pl, pts + 3 * i) < thr;
    flag[i] = (in == (inliers != 0)) ? 1u : 0u;
}

// the same from the device block of ransac_best_kernel (no plane found: everything is kept)
__global__ void plane_keep_best_kernel(const double *__restrict__ pts, int64_t N, const double *__restrict__ best, double thr,
                                       unsigned *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const double pl[4] = {best[10], best[11], best[12], best[13]};
    flag[i] = (best[0] < 0.0 || !(plane_dist(pl, pts + 3 * i) < thr)) ? 1u : 0u;
}

}  // namespace
