// ------------------------------------------------------------------ normal estimation
// PointCloud::EstimateNormals with a hybrid search (radius, max_nn): the max_nn nearest points with
// d^2 < radius^2 in ascending (d^2, index) -- kept sorted in LDS per thread -- give the nine
// cumulants and the covariance; the normal is the eigenvector of the smallest eigenvalue by the
// non-iterative solver Open3D uses (FastEigen3x3, after Eberly's robust 3x3 symmetric solver).
// oracle/cloudops.c states the same arithmetic; acos/cos come from different libms.
#pragma once
#include "common.h"
#include "grid.h"

namespace {

__device__ void eigenvector0(const double A[9], double e, double *out) {
    const double r0[3] = {A[0] - e, A[1], A[2]}, r1[3] = {A[1], A[4] - e, A[5]}, r2[3] = {A[2], A[5], A[8] - e};
    double c01[3], c02[3], c12[3];
    cross3(r0, r1, c01); cross3(r0, r2, c02); cross3(r1, r2, c12);
    const double d0 = dot3(c01, c01), d1 = dot3(c02, c02), d2_ = dot3(c12, c12);
    double b[3] = {c01[0], c01[1], c01[2]};
    double dm = d0;
    if (d1 > dm) { dm = d1; b[0] = c02[0]; b[1] = c02[1]; b[2] = c02[2]; }
    if (d2_ > dm) { dm = d2_; b[0] = c12[0]; b[1] = c12[1]; b[2] = c12[2]; }
    const double s = sqrt(dm);
    for (int k = 0; k < 3; ++k) out[k] = b[k] / s;
}
__device__ void eigenvector1(const double A[9], const double *ev0, double e, double *out) {
    double U[3], V[3];
    if (fabs(ev0[0]) > fabs(ev0[1])) {
        const double inv = 1.0 / sqrt(ev0[0] * ev0[0] + ev0[2] * ev0[2]);
        U[0] = -ev0[2] * inv; U[1] = 0.0; U[2] = ev0[0] * inv;
    } else {
        const double inv = 1.0 / sqrt(ev0[1] * ev0[1] + ev0[2] * ev0[2]);
        U[0] = 0.0; U[1] = ev0[2] * inv; U[2] = -ev0[1] * inv;
    }
    cross3(ev0, U, V);
    const double AU[3] = {(A[0] * U[0] + A[1] * U[1]) + A[2] * U[2], (A[1] * U[0] + A[4] * U[1]) + A[5] * U[2],
                          (A[2] * U[0] + A[5] * U[1]) + A[8] * U[2]};
    const double AV[3] = {(A[0] * V[0] + A[1] * V[1]) + A[2] * V[2], (A[1] * V[0] + A[4] * V[1]) + A[5] * V[2],
                          (A[2] * V[0] + A[5] * V[1]) + A[8] * V[2]};
    double m00 = dot3(U, AU) - e, m01 = dot3(U, AV), m11 = dot3(V, AV) - e;
    const double a00 = fabs(m00), a01 = fabs(m01), a11 = fabs(m11);
    if (a00 >= a11) {
        if (fmax(a00, a01) > 0.0) {
            if (a00 >= a01) { m01 /= m00; m00 = 1.0 / sqrt(1.0 + m01 * m01); m01 *= m00; }
            else { m00 /= m01; m01 = 1.0 / sqrt(1.0 + m00 * m00); m00 *= m01; }
            for (int k = 0; k < 3; ++k) out[k] = m01 * U[k] - m00 * V[k];
        } else {
            for (int k = 0; k < 3; ++k) out[k] = U[k];
        }
    } else {
        if (fmax(a11, a01) > 0.0) {
            if (a11 >= a01) { m01 /= m11; m11 = 1.0 / sqrt(1.0 + m01 * m01); m01 *= m11; }
            else { m11 /= m01; m01 = 1.0 / sqrt(1.0 + m11 * m11); m11 *= m01; }
            for (int k = 0; k < 3; ++k) out[k] = m11 * U[k] - m01 * V[k];
        } else {
            for (int k = 0; k < 3; ++k) out[k] = U[k];
        }
    }
}
__device__ void smallest_eigenvector(const double cov[9], double out[3]) {
    double A[9];
    double mx = cov[0];
    for (int k = 1; k < 9; ++k) if (cov[k] > mx) mx = cov[k];
    out[0] = out[1] = out[2] = 0.0;
    if (mx == 0.0) return;
    for (int k = 0; k < 9; ++k) A[k] = cov[k] / mx;
    const double norm = (A[1] * A[1] + A[2] * A[2]) + A[5] * A[5];
    if (norm > 0.0) {
        const double q = ((A[0] + A[4]) + A[8]) / 3.0;
        const double b00 = A[0] - q, b11 = A[4] - q, b22 = A[8] - q;
        const double p = sqrt((((b00 * b00 + b11 * b11) + b22 * b22) + norm * 2.0) / 6.0);
        const double c00 = b11 * b22 - A[5] * A[5], c01 = A[1] * b22 - A[5] * A[2], c02 = A[1] * A[5] - b11 * A[2];
        const double det = ((b00 * c00 - A[1] * c01) + A[2] * c02) / ((p * p) * p);
        double half = det * 0.5;
        half = half < -1.0 ? -1.0 : (half > 1.0 ? 1.0 : half);
        const double angle = acos(half) / 3.0;
        const double beta2 = cos(angle) * 2.0, beta0 = cos(angle + 2.09439510239319549) * 2.0, beta1 = -(beta0 + beta2);
        const double e0 = q + p * beta0, e1 = q + p * beta1, e2 = q + p * beta2;
        double v0[3], v1[3], v2[3];
        if (half >= 0.0) {
            eigenvector0(A, e2, v2);
            if (e2 < e0 && e2 < e1) { out[0] = v2[0]; out[1] = v2[1]; out[2] = v2[2]; return; }
            eigenvector1(A, v2, e1, v1);
            if (e1 < e0 && e1 < e2) { out[0] = v1[0]; out[1] = v1[1]; out[2] = v1[2]; return; }
            cross3(v1, v2, out);
        } else {
            eigenvector0(A, e0, v0);
            if (e0 < e1 && e0 < e2) { out[0] = v0[0]; out[1] = v0[1]; out[2] = v0[2]; return; }
            eigenvector1(A, v0, e1, v1);
            if (e1 < e0 && e1 < e2) { out[0] = v1[0]; out[1] = v1[1]; out[2] = v1[2]; return; }
            cross3(v0, v1, out);
        }
    } else {  // diagonal
        if (A[0] < A[4] && A[0] < A[8]) out[0] = 1.0;
        else if (A[4] < A[0] && A[4] < A[8]) out[1] = 1.0;
        else out[2] = 1.0;
    }
}

__global__ __launch_bounds__(NRM_THREADS) void normals_kernel(Grid g, const double *__restrict__ sp, int64_t N,
                                                              const int *__restrict__ cell_start,
                                                              const int *__restrict__ cell_end,
                                                              const int *__restrict__ idx_sorted, double r2, int max_nn,
                                                              const double *__restrict__ pts /* original order */,
                                                              const double *__restrict__ prior, double *__restrict__ out) {
    extern __shared__ double lds[];  // [max_nn][64] squared distances, then [max_nn][64] indices
    double *top_d = lds;
    int *top_j = (int *)(lds + (size_t)max_nn * NRM_THREADS);
    const int t = threadIdx.x;
    const int64_t j = (int64_t)blockIdx.x * NRM_THREADS + t;
    if (j >= N) return;
    const double p[3] = {sp[3 * j], sp[3 * j + 1], sp[3 * j + 2]};
    const int have = hybrid_collect(g, p, sp, cell_start, cell_end, idx_sorted, r2, max_nn, top_d, top_j, t);
    double cov[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (have >= 3) {
        double cu[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int q = 0; q < have; ++q) {
            const double *x = pts + 3 * (size_t)top_j[q * NRM_THREADS + t];
            cu[0] += x[0]; cu[1] += x[1]; cu[2] += x[2];
            cu[3] += x[0] * x[0]; cu[4] += x[0] * x[1]; cu[5] += x[0] * x[2];
            cu[6] += x[1] * x[1]; cu[7] += x[1] * x[2]; cu[8] += x[2] * x[2];
        }
        for (int k = 0; k < 9; ++k) cu[k] /= (double)have;
        cov[0] = cu[3] - cu[0] * cu[0]; cov[4] = cu[6] - cu[1] * cu[1]; cov[8] = cu[8] - cu[2] * cu[2];
        cov[1] = cov[3] = cu[4] - cu[0] * cu[1];
        cov[2] = cov[6] = cu[5] - cu[0] * cu[2];
        cov[5] = cov[7] = cu[7] - cu[1] * cu[2];
    }
    double n[3];
    smallest_eigenvector(cov, n);
    const int64_t i = idx_sorted[j];
    if (sqrt(dot3(n, n)) == 0.0) {
        if (prior) { n[0] = prior[3 * i]; n[1] = prior[3 * i + 1]; n[2] = prior[3 * i + 2]; }
        else { n[0] = 0.0; n[1] = 0.0; n[2] = 1.0; }
    }
    if (prior && dot3(n, prior + 3 * i) < 0.0) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
    out[3 * i] = n[0]; out[3 * i + 1] = n[1]; out[3 * i + 2] = n[2];
}

}  // namespace
