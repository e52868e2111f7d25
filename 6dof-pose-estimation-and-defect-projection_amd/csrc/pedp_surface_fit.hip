// Robust best fit of a point cloud to the mesh's surface (pedp_fit_to_surface): iteratively
// re-weighted Gauss-Newton over the exact closest-point search of pedp_closest.hip.  Every pass is three launches on the
// context's stream, and all passes are enqueued before anything is read back:
//
//   search             pedp_closest_launch_posed: the kernels of pedp_closest_points with q = R p + t formed as a point is
//                      loaded (the fused half: the points array is never rewritten); writes c, d and the face of every row
//   fit_rows_kernel    one workgroup per 256 consecutive points: normal, inlier test, weight and the 31 terms of a row, then
//                      a fixed tree over the block (a butterfly inside each wave, then ((w0 + w1) + (w2 + w3)))
//   fit_close_kernel   one workgroup: the blocks' partial sums in index order, fitness / rmse / trace, the convergence test,
//                      the 6 x 6 pivoted LDLT of icp/solve.h and T <- upd T
//
// A device flag (FitState::done) turns the launches behind the last pass into early exits.  The rows are a kernel of their
// own, for every search mode, because the order of the sums may depend on the point index alone: the wave-per-point search
// holds 4 points in a workgroup and the lane-per-point one 256, so a tree fused into the search's result step would differ
// between them.  Arithmetic as pedp_closest.hip: float64, no contraction, every expression in the order written, no
// floating-point atomics.  tests/_surface_fit_ref.py restates the contract in numpy.
#include "pedp_internal.h"
#include "mesh/record.h"
#include "closest/move_point.h"
// (the diagnostic build's stamp buffers and their readers, icp/common.h, are pedp_icp.hip's alone: defined here as well,
// the library of tools/icp_stamps.py does not link)
#undef PEDP_ICP_STAMPS
#define PEDP_ICP_STAMPS 0
#include "icp/solve.h"
#include <cmath>

namespace {

using namespace record;

constexpr int FT = 256;                 // points per block of the sums, threads per workgroup of the rows kernel
constexpr int TERMS = 31;               // 21 of sum w J J^T, 6 of sum w J d, sum d^2, K, sum w, finite rows
constexpr int TERMS_PAD = 32;           // doubles per block's partial sums
constexpr unsigned NO_FACE = 0xFFFFFFFFu;
constexpr int64_t MAX_FIT_POINTS = (int64_t)1 << 24;
constexpr int MAX_FIT_ITERATION = 1000;

struct FitState {
    double T[16];
    double T_closed[16];                // T of the last pass that was closed (what fitness and rmse belong to)
    double fitness, rmse, prev_fitness, prev_rmse;
    double packet[TERMS_PAD];           // the sums of the last pass that was closed
    unsigned long long pairs;           // the search's counter of tested pairs (this call's own)
    int done, iters, singular, pad;
};

struct Mat4 {
    double m[16];
};

__global__ void fit_init_kernel(FitState *__restrict__ st, Mat4 init) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    for (int k = 0; k < 16; ++k) st->T[k] = st->T_closed[k] = init.m[k];
    st->fitness = st->rmse = st->prev_fitness = st->prev_rmse = 0.0;
    for (int k = 0; k < TERMS_PAD; ++k) st->packet[k] = 0.0;
    st->pairs = 0;
    st->done = 0; st->iters = 0; st->singular = 0; st->pad = 0;
}

// the weight of an inlier at distance d (include/pedp.h)
__device__ __forceinline__ double loss_weight(int loss, double scale, double d) {
    if (loss == PEDP_FIT_HUBER) return d <= scale ? 1.0 : scale / d;
    if (loss == PEDP_FIT_TUKEY) {
        if (!(d < scale)) return 0.0;
        const double u = d / scale;
        const double t = 1.0 - u * u;
        return t * t;
    }
    return 1.0;
}

__global__ __launch_bounds__(FT) void fit_rows_kernel(const FitState *__restrict__ st, const float *__restrict__ tri,
                                                      const double *__restrict__ pts, int64_t n, const double *__restrict__ closest,
                                                      const double *__restrict__ dist, const uint32_t *__restrict__ prim, int loss,
                                                      double scale, double gate, double *__restrict__ partials) {
    if (st->done) return;
    const int64_t i = (int64_t)blockIdx.x * FT + threadIdx.x;
    double term[TERMS];
    for (int k = 0; k < TERMS; ++k) term[k] = 0.0;
    if (i < n && pedp_row_finite(pts, i)) {
        term[30] = 1.0;
        const uint32_t f = prim[i];
        const double d = dist[i];
        if (f != NO_FACE && d <= gate) {    // (a row without a triangle has d = +inf; the face test keeps gate = +inf out)
            double q[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
            surface_fit::move_point(st->T, q);
            double nrm[3];
            if (d > 0.0) {
                for (int k = 0; k < 3; ++k) nrm[k] = (q[k] - closest[3 * i + k]) / d;
            } else {
                Tri t;
                (void)load_tri(tri + (size_t)f * PEDP_TRI_STRIDE, t);
                unit_normal(t, nrm);
            }
            const double w = loss_weight(loss, scale, d);
            double J[6], wJ[6];
            cross3(q, nrm, J);
            for (int k = 0; k < 3; ++k) J[3 + k] = nrm[k];
            for (int k = 0; k < 6; ++k) wJ[k] = w * J[k];
            int k = 0;
            for (int a = 0; a < 6; ++a)
                for (int b = a; b < 6; ++b) term[k++] = wJ[a] * J[b];
            for (int a = 0; a < 6; ++a) term[21 + a] = wJ[a] * d;
            term[27] = d * d;
            term[28] = 1.0;
            term[29] = w;
        }
    }
    // the block's tree: inside a wave the butterfly (lanes l and l ^ 32, then ^ 16 ... ^ 1; x + y == y + x in every bit, so
    // all lanes hold the same sum), then the four waves as (w0 + w1) + (w2 + w3)
    __shared__ double wave_sum[FT / 64][TERMS_PAD];
    for (int k = 0; k < TERMS; ++k) {
        double v = term[k];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        term[k] = v;
    }
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < TERMS; ++k) wave_sum[threadIdx.x >> 6][k] = term[k];
    __syncthreads();
    if (threadIdx.x < TERMS_PAD) {
        const int k = threadIdx.x;
        partials[(size_t)blockIdx.x * TERMS_PAD + k] =
            k < TERMS ? (wave_sum[0][k] + wave_sum[1][k]) + (wave_sum[2][k] + wave_sum[3][k]) : 0.0;
    }
}

__global__ __launch_bounds__(64) void fit_close_kernel(FitState *__restrict__ st, const double *__restrict__ partials, int64_t n_blocks,
                                                       int pass, int max_iter, double rel_fitness, double rel_rmse,
                                                       double *__restrict__ trace) {
    if (st->done) return;
    __shared__ double pk[TERMS_PAD];
    if (threadIdx.x < TERMS_PAD) {
        double v = 0.0;
        for (int64_t b = 0; b < n_blocks; ++b) v += partials[(size_t)b * TERMS_PAD + threadIdx.x];   // the blocks in index order
        pk[threadIdx.x] = v;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    // sums that overflowed (a pose thrown far off by a rank-deficient solve): the fit ends on the last pass it could close
    for (int k = 0; k < TERMS; ++k)
        if (!(fabs(pk[k]) < pos_inf())) {
            for (int e = 0; e < 16; ++e) st->T[e] = st->T_closed[e];
            st->singular = 1; st->done = 1;
            return;
        }
    for (int k = 0; k < TERMS_PAD; ++k) st->packet[k] = pk[k];
    for (int e = 0; e < 16; ++e) st->T_closed[e] = st->T[e];
    const double K = pk[28], n_finite = pk[30];
    double fit = 0.0, rmse = 0.0;
    if (K > 0.0) { fit = K / n_finite; rmse = sqrt(pk[27] / K); }
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
    if (pass >= max_iter || !(K > 0.0)) { st->done = 1; return; }
    if (pass > 0 && fabs(st->prev_fitness - fit) < rel_fitness && fabs(st->prev_rmse - rmse) < rel_rmse) { st->done = 1; return; }
    double A[36], nb[6], x[6], upd[16], next[16];
    int k = 0;
    for (int a = 0; a < 6; ++a)
        for (int c = a; c < 6; ++c) { A[6 * a + c] = pk[k]; A[6 * c + a] = pk[k]; ++k; }
    for (int a = 0; a < 6; ++a) nb[a] = -pk[21 + a];
    bool ok = solve6_ldlt(A, nb, x);
    if (ok) {
        vec6_to_T(x, upd);
        mat4_mul_dev(upd, st->T, next);
        for (int e = 0; e < 16; ++e)
            if (!(fabs(next[e]) < pos_inf())) ok = false;   // (false for a NaN too)
    }
    if (!ok) { st->singular = 1; st->done = 1; return; }
    for (int e = 0; e < 16; ++e) st->T[e] = next[e];
}

// T (16 doubles) and the statistics (PEDP_FIT_STATS_DOUBLES) of the call, where the caller reads them
__global__ void fit_emit_kernel(const FitState *__restrict__ st, double *__restrict__ T_out, double *__restrict__ stats) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (T_out)
        for (int k = 0; k < 16; ++k) T_out[k] = st->T[k];
    if (stats) {
        stats[0] = st->fitness;
        stats[1] = st->rmse;
        stats[2] = (double)st->iters;
        stats[3] = st->packet[28];
        stats[4] = st->packet[29];
        stats[5] = (double)st->singular;
        stats[6] = st->packet[30];
        stats[7] = 0.0;
        for (int k = 0; k < 30; ++k) stats[8 + k] = st->packet[k];
        stats[38] = stats[39] = 0.0;
    }
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

extern "C" int pedp_fit_to_surface(pedp_ctx_t c, pedp_mesh_t mesh, const double *pts, int64_t N, int mem, const double *init, int loss,
                                   double scale, double gate, int max_iteration, double relative_fitness, double relative_rmse,
                                   double *T_out, double *stats_out, double *trace_out) {
    const char *who = "pedp_fit_to_surface";
    PEDP_REQUIRE(c && mesh, "%s: null context/mesh", who);
    PEDP_REQUIRE(mesh->ctx == c, "%s: the mesh belongs to another context", who);
    PEDP_REQUIRE(mem == PEDP_HOST || mem == PEDP_DEVICE, "%s: bad mem flag %d", who, mem);
    PEDP_REQUIRE(N >= 0 && N <= MAX_FIT_POINTS, "%s: N = %lld, at most %lld points", who, (long long)N, (long long)MAX_FIT_POINTS);
    PEDP_REQUIRE(loss == PEDP_FIT_L2 || loss == PEDP_FIT_HUBER || loss == PEDP_FIT_TUKEY, "%s: unknown loss %d", who, loss);
    PEDP_REQUIRE(loss == PEDP_FIT_L2 || scale > 0.0, "%s: a robust loss needs scale > 0, got %g", who, scale);
    PEDP_REQUIRE(gate >= 0.0, "%s: gate must not be negative (or NaN), got %g", who, gate);
    PEDP_REQUIRE(max_iteration >= 0 && max_iteration <= MAX_FIT_ITERATION, "%s: max_iteration = %d, 0 ... %d", who, max_iteration,
                 MAX_FIT_ITERATION);
    PEDP_REQUIRE(N == 0 || pts, "%s: null points", who);
    // the state of the fit and its sums live in the context's fit workspace, which a second fit would overwrite, and the
    // call's end waits on the stream (PEDP_HOST) that a pending registration owns until pedp_icp_end
    PEDP_REQUIRE(!c->icp_pending, "%s: a registration is pending on this context", who);
    Mat4 start;
    for (int k = 0; k < 16; ++k) start.m[k] = init ? init[k] : (k % 5 == 0 ? 1.0 : 0.0);
    for (int k = 0; k < 16; ++k) PEDP_REQUIRE(std::isfinite(start.m[k]), "%s: init[%d] is not finite", who, k);
    PEDP_HIP_CHECK(hipSetDevice(c->device));

    const size_t n = (size_t)N, n_blocks = (n + FT - 1) / FT, rows = (size_t)max_iteration + 1;
    const size_t o_state = 0, o_out = o_state + align256(sizeof(FitState)),
                 o_trace = o_out + align256(8 * (16 + PEDP_FIT_STATS_DOUBLES)), o_part = o_trace + align256(8 * 18 * rows),
                 o_cl = o_part + align256(8 * TERMS_PAD * n_blocks), o_d = o_cl + align256(24 * n), o_id = o_d + align256(8 * n),
                 ws_bytes = o_id + align256(4 * n);
    int rc = c->fit_ws.reserve(ws_bytes);
    if (rc) return rc;
    char *ws = (char *)c->fit_ws.ptr;
    FitState *st = (FitState *)(ws + o_state);
    double *d_out = (double *)(ws + o_out), *d_trace = (double *)(ws + o_trace), *d_part = (double *)(ws + o_part);
    double *d_cl = (double *)(ws + o_cl), *d_dist = (double *)(ws + o_d);
    uint32_t *d_prim = (uint32_t *)(ws + o_id);
    const double *d_pts = pts;
    if (mem == PEDP_HOST && N) {
        rc = c->fit_io.reserve(24 * n);
        if (rc) return rc;
        rc = pedp_upload(c, c->fit_io.ptr, pts, 24 * n);
        if (rc) return rc;
        d_pts = (const double *)c->fit_io.ptr;
    }
    double *k_trace = !trace_out ? nullptr : (mem == PEDP_DEVICE ? trace_out : d_trace);
    if (mem == PEDP_HOST && trace_out) PEDP_HIP_CHECK(hipMemsetAsync(d_trace, 0, 8 * 18 * rows, c->stream));

    hipLaunchKernelGGL(fit_init_kernel, dim3(1), dim3(64), 0, c->stream, st, start);
    PEDP_HIP_CHECK(hipGetLastError());
    for (int pass = 0; N && pass <= max_iteration; ++pass) {
        rc = pedp_closest_launch_posed(c, mesh, d_pts, N, st->T, &st->done, &st->pairs, d_cl, d_dist, d_prim);
        if (rc) return rc;
        hipLaunchKernelGGL(fit_rows_kernel, dim3((unsigned)n_blocks), dim3(FT), 0, c->stream, st, mesh->tri, d_pts, N, d_cl, d_dist,
                           d_prim, loss, scale, gate, d_part);
        hipLaunchKernelGGL(fit_close_kernel, dim3(1), dim3(64), 0, c->stream, st, d_part, (int64_t)n_blocks, pass, max_iteration,
                           relative_fitness, relative_rmse, k_trace);
        PEDP_HIP_CHECK(hipGetLastError());
    }
    const bool host = mem == PEDP_HOST;
    hipLaunchKernelGGL(fit_emit_kernel, dim3(1), dim3(64), 0, c->stream, st, host ? d_out : T_out, host ? d_out + 16 : stats_out);
    PEDP_HIP_CHECK(hipGetLastError());
    if (!host) return PEDP_OK;
    // the one read-back: T, the statistics and (behind them in the workspace) the trace
    const size_t bytes = trace_out ? o_trace - o_out + 8 * 18 * rows : 8 * (16 + PEDP_FIT_STATS_DOUBLES);
    const void *view = nullptr;
    rc = pedp_download_view(c, d_out, bytes, &view);
    if (rc) return rc;
    const double *got = (const double *)view;
    if (T_out) memcpy(T_out, got, 8 * 16);
    if (stats_out) memcpy(stats_out, got + 16, 8 * PEDP_FIT_STATS_DOUBLES);
    if (trace_out) memcpy(trace_out, (const char *)view + (o_trace - o_out), 8 * 18 * rows);
    return PEDP_OK;
}
