// ICP, the one-thread close of a pass on the segmented path: 6x6 pivoted LDLT, 3x3 Jacobi SVD, Umeyama,
// pose update and convergence test (icp_solve_kernel).
#pragma once
#include "common.h"

namespace {

// ------------------------------------------------------------------ solve (one thread)
__device__ void mat4_mul_dev(const double *A, const double *B, double *C) {
    double R[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double s = 0.0;
            for (int k = 0; k < 4; ++k) s += A[4 * i + k] * B[4 * k + j];
            R[4 * i + j] = s;
        }
    for (int k = 0; k < 16; ++k) C[k] = R[k];
}

__device__ void ident4(double *T) {
    for (int k = 0; k < 16; ++k) T[k] = 0.0;
    T[0] = T[5] = T[10] = T[15] = 1.0;
}

// Eigen-style LDLT (left-looking; pivot = largest remaining original diagonal entry), as
// in oracle/icp.c pedp_oracle_solve6_ldlt.
__device__ bool solve6_ldlt(const double *Ain, const double *b, double *x) {
    const int n = 6;
    // run by one thread; the pivoting indexes these arrays at run time, so they live in LDS
    // (private arrays with dynamic indices would go to scratch memory: ~10x the latency)
    __shared__ double A[6][6], tmp[6], y[6];
    __shared__ int tr[6];
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) A[i][j] = Ain[n * i + j];
    for (int k = 0; k < n; ++k) {
        int p = k;
        double big = fabs(A[k][k]);
        for (int i = k + 1; i < n; ++i)
            if (fabs(A[i][i]) > big) { big = fabs(A[i][i]); p = i; }
        tr[k] = p;
        if (p != k) {
            for (int j = 0; j < n; ++j) { double t = A[k][j]; A[k][j] = A[p][j]; A[p][j] = t; }
            for (int i = 0; i < n; ++i) { double t = A[i][k]; A[i][k] = A[i][p]; A[i][p] = t; }
        }
        if (k > 0) {
            for (int j = 0; j < k; ++j) tmp[j] = A[j][j] * A[k][j];
            double s = 0.0;
            for (int j = 0; j < k; ++j) s += A[k][j] * tmp[j];
            A[k][k] -= s;
            for (int i = k + 1; i < n; ++i) {
                double u = 0.0;
                for (int j = 0; j < k; ++j) u += A[i][j] * tmp[j];
                A[i][k] -= u;
            }
        }
        double akk = A[k][k];
        if (fabs(akk) > 0.0)
            for (int i = k + 1; i < n; ++i) A[i][k] /= akk;
    }
    for (int i = 0; i < n; ++i) y[i] = b[i];
    for (int k = 0; k < n; ++k)
        if (tr[k] != k) { double t = y[k]; y[k] = y[tr[k]]; y[tr[k]] = t; }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < i; ++j) y[i] -= A[i][j] * y[j];
    for (int i = 0; i < n; ++i) {
        if (fabs(A[i][i]) > 2.2250738585072014e-308) y[i] /= A[i][i];
        else y[i] = 0.0;
    }
    for (int i = n - 1; i >= 0; --i)
        for (int j = i + 1; j < n; ++j) y[i] -= A[j][i] * y[j];
    for (int k = n - 1; k >= 0; --k)
        if (tr[k] != k) { double t = y[k]; y[k] = y[tr[k]]; y[tr[k]] = t; }
    bool ok = true;
    for (int i = 0; i < n; ++i) {
        x[i] = y[i];
        if (!(y[i] == y[i]) || isinf(y[i])) ok = false;
    }
    return ok;
}

// the update from the angles' sines and cosines (the wide close computes the three sincos on three lanes at once
// and calls this with the values it has gathered: the same expressions either way)
__device__ __forceinline__ void sincos_to_T(double sa, double ca, double sb, double cb, double sc, double cc, const double *x, double *T) {
    ident4(T);
    T[0] = cc * cb;  T[1] = cc * sb * sa - sc * ca;  T[2] = cc * sb * ca + sc * sa;
    T[4] = sc * cb;  T[5] = sc * sb * sa + cc * ca;  T[6] = sc * sb * ca - cc * sa;
    T[8] = -sb;      T[9] = cb * sa;                 T[10] = cb * ca;
    T[3] = x[3]; T[7] = x[4]; T[11] = x[5];
}
__device__ void vec6_to_T(const double *x, double *T) {
    double ca, sa, cb, sb, cc, sc;  // one argument reduction per angle
    sincos(x[0], &sa, &ca);
    sincos(x[1], &sb, &cb);
    sincos(x[2], &sc, &cc);
    sincos_to_T(sa, ca, sb, cb, sc, cc, x, T);
}

__device__ double det3_dev(const double *M) {
    return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) +
           M[2] * (M[3] * M[7] - M[4] * M[6]);
}

// 3x3 SVD by one-sided Jacobi (same routine as oracle/icp.c svd3)
__device__ void svd3_dev(const double *Ain, double *U, double *w, double *V) {
    double A[3][3], Vv[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) A[i][j] = Ain[3 * i + j];
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                double alpha = 0, beta = 0, gamma = 0;
                for (int i = 0; i < 3; ++i) {
                    alpha += A[i][p] * A[i][p];
                    beta += A[i][q] * A[i][q];
                    gamma += A[i][p] * A[i][q];
                }
                if (gamma == 0.0) continue;
                off = fmax(off, fabs(gamma) / sqrt(fmax(alpha * beta, 2.2250738585072014e-308)));
                double zeta = (beta - alpha) / (2.0 * gamma);
                double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
                for (int i = 0; i < 3; ++i) {
                    double ap = A[i][p], aq = A[i][q];
                    A[i][p] = c * ap - s * aq;
                    A[i][q] = s * ap + c * aq;
                    double vp = Vv[i][p], vq = Vv[i][q];
                    Vv[i][p] = c * vp - s * vq;
                    Vv[i][q] = s * vp + c * vq;
                }
            }
        if (off < 1e-16) break;
    }
    double nrm[3];
    int ord[3] = {0, 1, 2};
    for (int j = 0; j < 3; ++j) nrm[j] = sqrt(A[0][j] * A[0][j] + A[1][j] * A[1][j] + A[2][j] * A[2][j]);
    for (int a = 0; a < 2; ++a)
        for (int b2 = a + 1; b2 < 3; ++b2)
            if (nrm[ord[b2]] > nrm[ord[a]]) { int t = ord[a]; ord[a] = ord[b2]; ord[b2] = t; }
    double Um[3][3];
    double tiny = nrm[ord[0]] * 1e-300 + 2.2250738585072014e-308;
    for (int k = 0; k < 3; ++k) {
        int j = ord[k];
        w[k] = nrm[j];
        for (int i = 0; i < 3; ++i) {
            V[3 * i + k] = Vv[i][j];
            Um[i][k] = (nrm[j] > tiny) ? A[i][j] / nrm[j] : 0.0;
        }
    }
    double rel = 1e-13 * w[0];
    if (w[0] <= tiny) {
        for (int i = 0; i < 3; ++i) for (int k = 0; k < 3; ++k) Um[i][k] = (i == k);
    } else {
        if (w[1] <= rel) {
            double a[3] = {Um[0][0], Um[1][0], Um[2][0]};
            int m = (fabs(a[0]) <= fabs(a[1]) && fabs(a[0]) <= fabs(a[2])) ? 0 : (fabs(a[1]) <= fabs(a[2]) ? 1 : 2);
            double e[3] = {0, 0, 0};
            e[m] = 1.0;
            double dt = a[m];
            double b2[3] = {e[0] - dt * a[0], e[1] - dt * a[1], e[2] - dt * a[2]};
            double nb = sqrt(b2[0] * b2[0] + b2[1] * b2[1] + b2[2] * b2[2]);
            for (int i = 0; i < 3; ++i) Um[i][1] = b2[i] / nb;
        }
        if (w[2] <= rel) {
            Um[0][2] = Um[1][0] * Um[2][1] - Um[2][0] * Um[1][1];
            Um[1][2] = Um[2][0] * Um[0][1] - Um[0][0] * Um[2][1];
            Um[2][2] = Um[0][0] * Um[1][1] - Um[1][0] * Um[0][1];
        }
    }
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) U[3 * i + k] = Um[i][k];
}

// pass p (0 = initial correspondence pass).  Records fitness/rmse of the pass, decides
// whether the loop ends, otherwise derives the next update from the packet.
__global__ __launch_bounds__(256) void icp_solve_kernel(IcpState *__restrict__ st, double *__restrict__ packet,
                                                        const double *__restrict__ partials, int pass, int max_iter,
                                                        int estimator, double n_source, double rel_fitness,
                                                        double rel_rmse, double *__restrict__ trace) {
    if (st->done) return;
    // single-GPU runs fold icp_reduce into this launch (partials != null); with an all-reduce
    // hook the packet was reduced (and summed over ranks) before.  Fixed order: 8 slices of 32
    // partials each, then the slices in order -- run-to-run bit-stable.
    __shared__ double pk[32];
    if (partials) {
        __shared__ double slice[8][32];
        const int k = threadIdx.x & 31, part = threadIdx.x >> 5;
        double v = 0.0;
        if (k < PACKET)
            for (int b = part * (ACC_BLOCKS / 8); b < (part + 1) * (ACC_BLOCKS / 8); ++b) v += partials[(size_t)b * PACKET + k];
        slice[part][k] = v;
        __syncthreads();
        if (threadIdx.x < PACKET) {
            double t = 0.0;
            for (int q = 0; q < 8; ++q) t += slice[q][threadIdx.x];
            packet[threadIdx.x] = t;
            pk[threadIdx.x] = t;
        }
    } else if (threadIdx.x < PACKET) {
        pk[threadIdx.x] = packet[threadIdx.x];
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    packet = pk;  // the serial part below reads the packet from LDS
    st->sum_cand += (long long)st->n_blocks * (NN_SB * 16);
    st->sum_fb += st->fb_count;
    st->fb_count = 0;
    st->n_cand = 0;
    st->n_blocks = 0;

    const double K = packet[28];
    double fit = 0.0, rmse = 0.0;
    if (K > 0.0) { fit = K / n_source; rmse = sqrt(packet[27] / K); }
    st->prev_fitness = st->fitness;
    st->prev_rmse = st->rmse;
    st->fitness = fit;
    st->rmse = rmse;
    if (trace) {
        double *tr = trace + 18 * pass;
        tr[0] = fit; tr[1] = rmse;
        for (int k = 0; k < 16; ++k) tr[2 + k] = st->T[k];
    }
    st->iters = pass;
    if (pass >= max_iter) { st->done = 1; return; }
    if (pass > 0 && fabs(st->prev_fitness - fit) < rel_fitness && fabs(st->prev_rmse - rmse) < rel_rmse) {
        st->done = 1;
        return;
    }
    double upd[16];
    ident4(upd);
    if (K > 0.0) {
        if (estimator == PEDP_POINT_TO_PLANE) {
            double A[36], nb[6], x[6];
            int k = 0;
            for (int a = 0; a < 6; ++a)
                for (int c = a; c < 6; ++c) { A[6 * a + c] = packet[k]; A[6 * c + a] = packet[k]; ++k; }
            for (int a = 0; a < 6; ++a) nb[a] = -packet[21 + a];
            if (solve6_ldlt(A, nb, x)) vec6_to_T(x, upd);
        } else {
            const double *c = st->centroid;
            double ms[3], mt[3], sig[9];
            for (int a = 0; a < 3; ++a) { ms[a] = packet[a] / K; mt[a] = packet[3 + a] / K; }
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) sig[3 * a + b] = packet[6 + 3 * a + b] / K - mt[a] * ms[b];
            double U[9], w[3], V[9];
            svd3_dev(sig, U, w, V);
            double sgn = (det3_dev(U) * det3_dev(V) < 0.0) ? -1.0 : 1.0;
            double R[9];
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b)
                    R[3 * a + b] = U[3 * a] * V[3 * b] + U[3 * a + 1] * V[3 * b + 1] + sgn * U[3 * a + 2] * V[3 * b + 2];
            for (int a = 0; a < 3; ++a) {
                for (int b = 0; b < 3; ++b) upd[4 * a + b] = R[3 * a + b];
                double msa[3] = {ms[0] + c[0], ms[1] + c[1], ms[2] + c[2]};
                upd[4 * a + 3] = (mt[a] + c[a]) - (R[3 * a] * msa[0] + R[3 * a + 1] * msa[1] + R[3 * a + 2] * msa[2]);
            }
        }
    }
    for (int k = 0; k < 16; ++k) st->upd[k] = upd[k];
    mat4_mul_dev(upd, st->T, st->T);
}

}  // namespace
