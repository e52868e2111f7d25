// ---- selection in index order: flags -> exclusive scan -> scatter
#pragma once
#include "common.h"

namespace {

// the largest cluster (np.unique + argmax: the lowest label among the largest) without a trip to the host: members per
// label, the label with most members, the flags of its points (no cluster at all: *label = -1, nothing is kept)
__global__ void label_count_kernel(const int32_t *__restrict__ labels, int64_t N, int *__restrict__ members) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int l = i < N ? labels[i] : -1;
    // one add per distinct label of the wave (most points carry the same label: a point's own add each queues
    // thousands of atomics on one word)
    unsigned long long left = __builtin_amdgcn_ballot_w64(l >= 0);
    while (left) {  // wave-uniform
        const int l0 = __builtin_amdgcn_readlane(l, __builtin_ctzll(left));
        const unsigned long long same = __builtin_amdgcn_ballot_w64(l == l0);
        if ((int)(threadIdx.x & 63) == __builtin_ctzll(left)) atomicAdd(&members[l0], __builtin_popcountll(same));
        left &= ~same;
    }
}
__global__ __launch_bounds__(256) void label_largest_kernel(const int *__restrict__ members, int64_t N, int *__restrict__ label) {
    __shared__ int cnt_s[256], lab_s[256];
    int bc = 0, bl = -1;
    for (int64_t l = threadIdx.x; l < N; l += 256)
        if (members[l] > bc) { bc = members[l]; bl = (int)l; }  // ascending l: the lowest of the thread's share
    cnt_s[threadIdx.x] = bc;
    lab_s[threadIdx.x] = bl;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) {
            const int oc = cnt_s[threadIdx.x + w], ol = lab_s[threadIdx.x + w];
            if (oc > cnt_s[threadIdx.x] || (oc == cnt_s[threadIdx.x] && ol >= 0 && ol < lab_s[threadIdx.x])) {
                cnt_s[threadIdx.x] = oc;
                lab_s[threadIdx.x] = ol;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) *label = lab_s[0];
}

// remove_points_below_plane (src/pose_estimation.py:366-378): keep `(a x + b y + c z + d) / sqrt(a^2 + b^2 + c^2) <= 0`.
// The divisor is positive, so the sign is the numerator's: numpy's left-to-right sum of three products and d, one
// rounding each (no contraction in this build).  A flipped plane negates every term exactly: `>= 0` on the same sum.
__global__ void halfspace_keep_kernel(const double *__restrict__ pts, int64_t N, double a, double b, double cc, double d, int flipped,
                                      unsigned *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const double s = ((a * pts[3 * i] + b * pts[3 * i + 1]) + cc * pts[3 * i + 2]) + d;
    flag[i] = (flipped ? s >= 0.0 : s <= 0.0) ? 1u : 0u;
}
__global__ void label_keep_kernel(const int32_t *__restrict__ labels, int64_t N, const int *__restrict__ label, unsigned *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) flag[i] = (*label >= 0 && labels[i] == *label) ? 1u : 0u;
}
__global__ void range_keep_kernel(const double *__restrict__ avg, int64_t N, double limit, unsigned *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) flag[i] = (avg[i] > 0.0 && avg[i] < limit) ? 1u : 0u;   // Open3D: 0 < mean distance < mean + ratio * std
}
__global__ void scatter_kept_kernel(const double *__restrict__ pts, const double *__restrict__ nrm, int64_t N,
                                    const unsigned *__restrict__ flag, const unsigned *__restrict__ pos, double *__restrict__ out_pts,
                                    double *__restrict__ out_nrm, unsigned *__restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    if (flag[i]) {
        const size_t o = pos[i];
        out_pts[3 * o] = pts[3 * i]; out_pts[3 * o + 1] = pts[3 * i + 1]; out_pts[3 * o + 2] = pts[3 * i + 2];
        if (nrm) { out_nrm[3 * o] = nrm[3 * i]; out_nrm[3 * o + 1] = nrm[3 * i + 1]; out_nrm[3 * o + 2] = nrm[3 * i + 2]; }
    }
    if (i == N - 1) *count = pos[i] + flag[i];
}

}  // namespace
