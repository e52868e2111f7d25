// Pose errors against a ground truth: ADD and ADD-S (Utils.py:232-253) for a batch of poses on the device.
//
//   add_kernel      one workgroup per chunk of 256 model points, pose and symmetry: both transforms of its points, the
//                   distances of the pairs, one partial sum
//   adds_kernel     the same grid; a thread holds two gt points in registers, every pred point passes through LDS in
//                   tiles of 256 (transformed as it is staged, all lanes read the same slot), the running minimum is of
//                   the squared distance
//   finish_kernel   one lane per pose: the partial sums in index order, the mean, the minimum over the symmetries
//
// Arithmetic: float64 with no contraction (-ffp-contract=off), every sum in the order written, no
// floating-point atomics.  The order of the mean depends on N alone; tests/_metrics_ref.py restates it in numpy.
#include "pedp_internal.h"
#include "metrics/plan.h"
#include <cmath>

namespace {

using namespace pedp_metrics;

// a value with no NaN / infinity in it, tested on the exponent bits
__device__ __forceinline__ bool finite1(double v) {
    const unsigned long long e = 0x7FF0000000000000ull;
    return ((unsigned long long)__double_as_longlong(v) & e) != e;
}

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7FF8000000000000ll); }

// rows 0 .. 2 of a row-major 4 x 4 pose (the bottom row is not read)
__device__ __forceinline__ void load_rows(const double *__restrict__ p, double M[12]) {
    for (int k = 0; k < 12; ++k) M[k] = p[k];
}

// rows 0 .. 2 of M . s: entry (i, j) = ((M_i0 s_0j + M_i1 s_1j) + M_i2 s_2j) + M_i3 s_3j
__device__ __forceinline__ void times_sym(double M[12], const double *__restrict__ s) {
    double R[12];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j)
            R[4 * i + j] = ((M[4 * i] * s[j] + M[4 * i + 1] * s[4 + j]) + M[4 * i + 2] * s[8 + j]) + M[4 * i + 3] * s[12 + j];
    for (int k = 0; k < 12; ++k) M[k] = R[k];
}

// q_k = ((R_k0 x + R_k1 y) + R_k2 z) + t_k; false if a coordinate of q is not finite
__device__ __forceinline__ bool xform(const double M[12], double x, double y, double z, double &qx, double &qy, double &qz) {
    qx = ((M[0] * x + M[1] * y) + M[2] * z) + M[3];
    qy = ((M[4] * x + M[5] * y) + M[6] * z) + M[7];
    qz = ((M[8] * x + M[9] * y) + M[10] * z) + M[11];
    return finite1(qx) && finite1(qy) && finite1(qz);
}

// The chunk's sum of one value per thread, valid in thread 0: the lanes of a wave by halving (lane k takes lane k + 32,
// then k + 16, ... k + 1), then the waves in order.
__device__ __forceinline__ double chunk_sum(double v, double *red) {
    const int t = threadIdx.x;
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_down(v, off, 64);
    if ((t & 63) == 0) red[t >> 6] = v;
    __syncthreads();
    double s = red[0];
    for (int w = 1; w < MT / 64; ++w) s = s + red[w];
    return s;
}

struct Args {
    const double *pts, *preds, *gts, *sym;
    int64_t n;
    int gstride;   // 0: one ground truth for all poses, 16: one per pose
    int chunks;
    double *partial;  // [pose of the slab][symmetry][chunk]
};

// prediction and ground truth of workgroup (chunk, pose, symmetry)
template <bool SYM>
__device__ __forceinline__ void poses_of(const Args &a, double P[12], double G[12]) {
    load_rows(a.preds + 16 * (size_t)blockIdx.y, P);
    if (SYM) times_sym(P, a.sym + 16 * (size_t)blockIdx.z);
    load_rows(a.gts + (size_t)a.gstride * blockIdx.y, G);
}

__device__ __forceinline__ void store_partial(const Args &a, double sum, int bad) {
    if (threadIdx.x == 0)
        a.partial[((size_t)blockIdx.y * gridDim.z + blockIdx.z) * (size_t)a.chunks + blockIdx.x] = bad ? quiet_nan() : sum;
}

// Thread t of chunk c holds points c * 256 + t and c * 256 + 128 + t; a point past the end adds +0.
template <bool SYM>
__global__ __launch_bounds__(MT) void add_kernel(Args a) {
    __shared__ double red[MT / 64];
    double P[12], G[12];
    poses_of<SYM>(a, P, G);
    int bad = 0;
    double term[QPT];
    for (int j = 0; j < QPT; ++j) {
        const int64_t i = (int64_t)blockIdx.x * CH + j * MT + threadIdx.x;
        term[j] = 0.0;
        if (i < a.n) {
            const double *p = a.pts + 3 * i;
            const double x = p[0], y = p[1], z = p[2];
            double ax, ay, az, bx, by, bz;
            const bool oka = xform(P, x, y, z, ax, ay, az), okb = xform(G, x, y, z, bx, by, bz);
            const double dx = ax - bx, dy = ay - by, dz = az - bz;
            term[j] = sqrt((dx * dx + dy * dy) + dz * dz);
            if (!(oka && okb)) bad = 1;
        }
    }
    bad = __syncthreads_or(bad);
    const double sum = chunk_sum(term[0] + term[1], red);
    store_partial(a, sum, bad);
}

template <bool SYM>
__global__ __launch_bounds__(MT) void adds_kernel(Args a) {
    __shared__ double sx[TP], sy[TP], sz[TP];
    __shared__ double red[MT / 64];
    const int t = threadIdx.x;
    double P[12], G[12];
    poses_of<SYM>(a, P, G);
    int bad = 0;
    double qx[QPT], qy[QPT], qz[QPT], best[QPT];
    bool valid[QPT];
    for (int j = 0; j < QPT; ++j) {
        const int64_t i = (int64_t)blockIdx.x * CH + j * MT + t;
        valid[j] = i < a.n;
        qx[j] = qy[j] = qz[j] = 0.0;
        best[j] = __longlong_as_double(0x7FF0000000000000ll);  // +inf: any pred point beats it
        if (valid[j]) {
            const double *p = a.pts + 3 * i;
            if (!xform(G, p[0], p[1], p[2], qx[j], qy[j], qz[j])) bad = 1;
        }
    }
    for (int64_t j0 = 0; j0 < a.n; j0 += TP) {
        const int cnt = (int)((a.n - j0) < TP ? (a.n - j0) : TP);
        __syncthreads();  // the tile before this one has been read
        for (int k = t; k < cnt; k += MT) {
            const double *p = a.pts + 3 * (j0 + k);
            double x, y, z;
            if (!xform(P, p[0], p[1], p[2], x, y, z)) bad = 1;
            sx[k] = x; sy[k] = y; sz[k] = z;
        }
        __syncthreads();
        // slots cnt .. TP - 1 hold nothing and are never read
#pragma unroll 4
        for (int k = 0; k < cnt; ++k) {
            const double x = sx[k], y = sy[k], z = sz[k];
            for (int j = 0; j < QPT; ++j) {
                const double dx = x - qx[j], dy = y - qy[j], dz = z - qz[j];
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                best[j] = d2 < best[j] ? d2 : best[j];  // d2 is a NaN only under `bad`, which overrides the sum
            }
        }
    }
    double term[QPT];
    for (int j = 0; j < QPT; ++j) term[j] = valid[j] ? sqrt(best[j]) : 0.0;
    bad = __syncthreads_or(bad);
    const double sum = chunk_sum(term[0] + term[1], red);
    store_partial(a, sum, bad);
}

// e_s = ((p_0 + p_1) + ... + p_{chunks-1}) / N; out = min over s, a NaN if any e_s is one
__global__ __launch_bounds__(64) void finish_kernel(const double *__restrict__ partial, int B, int S1, int chunks, double n,
                                                    double *__restrict__ out) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    double best = 0.0;
    bool nan = false;
    for (int s = 0; s < S1; ++s) {
        const double *p = partial + ((size_t)b * S1 + s) * (size_t)chunks;
        double sum = p[0];
        for (int c = 1; c < chunks; ++c) sum = sum + p[c];
        const double e = sum / n;
        if (e != e) nan = true;
        else if (s == 0 || e < best) best = e;
    }
    out[b] = nan ? quiet_nan() : best;
}

static_assert(QPT == 2, "the kernels add a thread's two terms as term[0] + term[1]");

}  // namespace

extern "C" {

int pedp_pose_errors(pedp_ctx_t c, const double *pts, int64_t N, const double *preds, int B, const double *gts, int G,
                     const double *sym, int S, int kind, int mem, double *out) {
    const char *who = "pedp_pose_errors";
    PEDP_REQUIRE(c, "%s: null context", who);
    PEDP_REQUIRE(mem == PEDP_HOST || mem == PEDP_DEVICE, "%s: bad mem flag %d", who, mem);
    PEDP_REQUIRE(kind == PEDP_ERR_ADD || kind == PEDP_ERR_ADDS, "%s: kind %d", who, kind);
    Plan pl;
    const char *wrong = plan(N, B, G, S, &pl);
    PEDP_REQUIRE(!wrong, "%s: %s (N = %lld, B = %d, G = %d, S = %d)", who, wrong, (long long)N, B, G, S);
    if (B == 0) return PEDP_OK;
    PEDP_REQUIRE(pts && preds && gts && out && (sym || S == 0), "%s: null array", who);
    // the partial sums have a workspace of their own; a host-memory call also goes through the context's staging
    // buffers and waits on its stream, which a pending registration (pedp_icp_begin) owns until pedp_icp_end
    PEDP_REQUIRE(mem == PEDP_DEVICE || !c->icp_pending, "%s: a registration is pending on this context (host-memory call)", who);
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    int rc = c->metrics_ws.reserve(pl.ws_bytes);
    if (rc) return rc;
    Args a;
    a.pts = pts; a.preds = preds; a.gts = gts; a.sym = sym;
    double *d_out = out;
    if (mem == PEDP_HOST) {
        rc = c->metrics_io.reserve(pl.io_bytes);
        if (rc) return rc;
        char *io = (char *)c->metrics_io.ptr;
        a.pts = (const double *)(io + pl.o_pts);
        a.preds = (const double *)(io + pl.o_preds);
        a.gts = (const double *)(io + pl.o_gts);
        a.sym = S ? (const double *)(io + pl.o_sym) : nullptr;
        d_out = (double *)(io + pl.o_out);
        rc = pedp_upload(c, (void *)a.pts, pts, 24 * (size_t)N);
        if (!rc) rc = pedp_upload(c, (void *)a.preds, preds, 128 * (size_t)B);
        if (!rc) rc = pedp_upload(c, (void *)a.gts, gts, 128 * (size_t)G);
        if (!rc && S) rc = pedp_upload(c, (void *)a.sym, sym, 128 * (size_t)S);
        if (rc) return rc;
    }
    a.n = N;
    a.gstride = G == 1 ? 0 : 16;
    a.chunks = pl.chunks;
    a.partial = (double *)c->metrics_ws.ptr;
    const double *preds0 = a.preds, *gts0 = a.gts;
    for (int b0 = 0; b0 < B; b0 += pl.slab) {
        const int nb = B - b0 < pl.slab ? B - b0 : pl.slab;
        a.preds = preds0 + 16 * (size_t)b0;
        a.gts = gts0 + (size_t)a.gstride * b0;
        const dim3 grid((unsigned)pl.chunks, (unsigned)nb, (unsigned)pl.S1);
        if (kind == PEDP_ERR_ADD) {
            if (S) hipLaunchKernelGGL(add_kernel<true>, grid, dim3(MT), 0, c->stream, a);
            else hipLaunchKernelGGL(add_kernel<false>, grid, dim3(MT), 0, c->stream, a);
        } else {
            if (S) hipLaunchKernelGGL(adds_kernel<true>, grid, dim3(MT), 0, c->stream, a);
            else hipLaunchKernelGGL(adds_kernel<false>, grid, dim3(MT), 0, c->stream, a);
        }
        PEDP_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(finish_kernel, dim3((unsigned)((nb + 63) / 64)), dim3(64), 0, c->stream, a.partial, nb, pl.S1,
                           pl.chunks, (double)N, d_out + b0);
        PEDP_HIP_CHECK(hipGetLastError());
    }
    if (mem == PEDP_HOST) rc = pedp_download(c, out, d_out, 8 * (size_t)B);
    return rc;
}

}  // extern "C"
