// FoundationPose's pose arithmetic on the device: the device half of estimator.py.
//
//   update_kernel     one lane per pose: the refiner's network output -> new pose (predict_pose_refine.py:195-231 with
//                     egocentric_delta_pose_to_pose, Utils.py:848-855)
//   pair_max_kernel   one workgroup per pair of 256-point tiles (upper triangle): the largest squared distance of the
//                     pair as one 64-bit atomicMax on its bit pattern (compute_mesh_diameter's dists.max(), Utils.py:559-574)
//
// Arithmetic: float32 with no contraction (-ffp-contract=off), every sum in the order written; tanh, sin
// and cos in float64, rounded once to float32.  The rotation formulas restate pytorch3d 0.7's so3_exp_map (eps 1e-4, the
// clamp on the squared norm) and rotation_6d_to_matrix; pytorch3d is not installed here, so parity with it is unpinned.
// tests/_pose_ref.py restates both kernels operation for operation.
#include "pedp_internal.h"
#include <cmath>

namespace {

constexpr int PB = 64;    // poses per workgroup
constexpr int TP = 256;   // points per tile = threads per workgroup of the pair maximum

struct UpdateArgs {
    int B, trans_rep, rot_rep, normalize;
    float tn[3], rot_norm, half_diameter;
};

__device__ __forceinline__ float tanh32(float x) { return (float)tanh((double)x); }

// pytorch3d _so3_exp_map(log_rot, eps=1e-4): R = (f1 K + f2 K^2) + I, K = hat(x)
__device__ inline void so3_exp(const float x[3], float R[9]) {
    const float n = (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2];
    const float th = sqrtf(n != n ? n : fmaxf(n, 1e-4f));  // torch.clamp keeps a NaN
    const float ti = 1.0f / th;
    const float f1 = ti * (float)sin((double)th);
    const float f2 = (ti * ti) * (1.0f - (float)cos((double)th));
    const float K[9] = {0.f, -x[2], x[1], x[2], 0.f, -x[0], -x[1], x[0], 0.f};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const float k2 = (K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j]) + K[3 * i + 2] * K[6 + j];
            R[3 * i + j] = (f1 * K[3 * i + j] + f2 * k2) + (i == j ? 1.f : 0.f);
        }
}

// F.normalize(v, dim=-1): v / max(|v|, 1e-12), |v| = sqrt((v0 v0 + v1 v1) + v2 v2)
__device__ __forceinline__ void normalize3(float v[3]) {
    const float nr = sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    const float d = nr == nr ? fmaxf(nr, 1e-12f) : nr;
    for (int k = 0; k < 3; ++k) v[k] = v[k] / d;
}

// pytorch3d rotation_6d_to_matrix: rows b1, b2, b3 (Gram-Schmidt, then the cross product)
__device__ inline void rot6d(const float a[6], float R[9]) {
    float b1[3] = {a[0], a[1], a[2]}, b2[3];
    normalize3(b1);
    const float dot = (b1[0] * a[3] + b1[1] * a[4]) + b1[2] * a[5];
    for (int k = 0; k < 3; ++k) b2[k] = a[3 + k] - dot * b1[k];
    normalize3(b2);
    R[0] = b1[0]; R[1] = b1[1]; R[2] = b1[2];
    R[3] = b2[0]; R[4] = b2[1]; R[5] = b2[2];
    R[6] = b1[1] * b2[2] - b1[2] * b2[1];
    R[7] = b1[2] * b2[0] - b1[0] * b2[2];
    R[8] = b1[0] * b2[1] - b1[1] * b2[0];
}

__global__ __launch_bounds__(PB) void update_kernel(UpdateArgs a, const float *__restrict__ trans, const float *__restrict__ rot,
                                                    const float *poseA, float *poses, float *__restrict__ tdelta,
                                                    float *__restrict__ rdelta) {
    const int b = blockIdx.x * PB + threadIdx.x;
    if (b >= a.B) return;
    float td[3], R[9], PA[16];
    for (int k = 0; k < 16; ++k) PA[k] = poseA[16 * (size_t)b + k];  // all of it first: poses may alias poseA
    for (int k = 0; k < 3; ++k) {
        const float o = trans[3 * (size_t)b + k];
        td[k] = (a.trans_rep == PEDP_TRANS_TRACKNET && !a.normalize) ? tanh32(o) * a.tn[k] : o;
        if (a.normalize) td[k] = td[k] * a.half_diameter;
    }
    if (a.rot_rep == PEDP_ROT_AXIS_ANGLE) {
        float x[3];
        for (int k = 0; k < 3; ++k) x[k] = tanh32(rot[3 * (size_t)b + k]) * a.rot_norm;
        so3_exp(x, R);
    } else {
        float r6[6];
        for (int k = 0; k < 6; ++k) r6[k] = rot[6 * (size_t)b + k];
        rot6d(r6, R);
    }
    float Rd[9];  // the reference's .permute(0, 2, 1)
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Rd[3 * i + j] = R[3 * j + i];
    float out[16];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j)
            out[4 * i + j] = (Rd[3 * i] * PA[j] + Rd[3 * i + 1] * PA[4 + j]) + Rd[3 * i + 2] * PA[8 + j];
        out[4 * i + 3] = PA[4 * i + 3] + td[i];
    }
    out[12] = 0.f; out[13] = 0.f; out[14] = 0.f; out[15] = 1.f;
    for (int k = 0; k < 16; ++k) poses[16 * (size_t)b + k] = out[k];
    if (tdelta)
        for (int k = 0; k < 3; ++k) tdelta[3 * (size_t)b + k] = td[k];
    if (rdelta)
        for (int k = 0; k < 9; ++k) rdelta[9 * (size_t)b + k] = Rd[k];
}

__device__ __forceinline__ bool finite3(const double *p) {
    return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]);
}

// Tile pair (blockIdx.x, blockIdx.y), x <= y: thread t holds point x*256 + t, tile y sits in LDS.  Every point is the
// thread point of its own diagonal pair, which is where non-finite coordinates are flagged.  Squared distances are
// non-negative (or +inf), so their bit patterns order as unsigned integers.
__global__ __launch_bounds__(TP) void pair_max_kernel(const double *__restrict__ pts, int64_t n,
                                                      unsigned long long *__restrict__ best, int *__restrict__ nan_flag) {
    const int ta = blockIdx.x, tb = blockIdx.y;
    if (tb < ta) return;  // lower triangle: covered by its mirror (d^2 is symmetric bit for bit)
    __shared__ double sx[TP], sy[TP], sz[TP];
    __shared__ unsigned long long red[TP / 64];
    const int t = threadIdx.x;
    const int64_t j0 = (int64_t)tb * TP;
    const int cnt = (int)((n - j0) < TP ? (n - j0) : TP);
    if (t < cnt) {
        const double *q = pts + 3 * (j0 + t);
        sx[t] = q[0]; sy[t] = q[1]; sz[t] = q[2];
    }
    __syncthreads();
    const int64_t i = (int64_t)ta * TP + t;
    unsigned long long m = 0;
    if (i < n) {
        const double *p = pts + 3 * i;
        const double px = p[0], py = p[1], pz = p[2];
        if (ta == tb && !finite3(p)) atomicOr(nan_flag, 1);
        double dm = 0.0;
        for (int k = 0; k < cnt; ++k) {
            const double dx = sx[k] - px, dy = sy[k] - py, dz = sz[k] - pz;
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            dm = d2 > dm ? d2 : dm;  // a NaN never wins; it is reported through the flag
        }
        m = (unsigned long long)__double_as_longlong(dm);
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_down(m, off, 64);
        m = o > m ? o : m;
    }
    if ((t & 63) == 0) red[t >> 6] = m;
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < TP / 64; ++w) m = red[w] > m ? red[w] : m;
        atomicMax(best, m);
    }
}

size_t a256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

extern "C" {

int pedp_pose_update(pedp_ctx_t c, const pedp_pose_update_params *prm, int B, const float *trans, const float *rot,
                     const float *poseA, int mem, float *poses, float *trans_delta, float *rot_mat_delta) {
    const char *who = "pedp_pose_update";
    PEDP_REQUIRE(c && prm, "%s: null context or parameters", who);
    PEDP_REQUIRE(mem == PEDP_HOST || mem == PEDP_DEVICE, "%s: bad mem flag %d", who, mem);
    PEDP_REQUIRE(prm->trans_rep == PEDP_TRANS_TRACKNET || prm->trans_rep == PEDP_TRANS_RAW, "%s: trans_rep %d", who,
                 prm->trans_rep);
    PEDP_REQUIRE(prm->rot_rep == PEDP_ROT_AXIS_ANGLE || prm->rot_rep == PEDP_ROT_6D, "%s: rot_rep %d", who, prm->rot_rep);
    PEDP_REQUIRE(B >= 0, "%s: B = %d", who, B);
    if (B == 0) return PEDP_OK;
    PEDP_REQUIRE(trans && rot && poseA && poses, "%s: null array", who);
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    UpdateArgs a;
    a.B = B;
    a.trans_rep = prm->trans_rep;
    a.rot_rep = prm->rot_rep;
    a.normalize = prm->normalize_xyz != 0;
    for (int k = 0; k < 3; ++k) a.tn[k] = prm->trans_normalizer[k];
    a.rot_norm = prm->rot_normalizer;
    a.half_diameter = (float)(prm->mesh_diameter / 2.0);
    const int rw = prm->rot_rep == PEDP_ROT_6D ? 6 : 3;
    const size_t bt = 12 * (size_t)B, br = 4 * (size_t)rw * B, bp = 64 * (size_t)B, bd = 36 * (size_t)B;
    const float *d_t = trans, *d_r = rot, *d_pa = poseA;
    float *d_p = poses, *d_td = trans_delta, *d_rd = rot_mat_delta;
    int rc = PEDP_OK;
    if (mem == PEDP_HOST) {
        rc = c->pose_io.reserve(a256(bt) + a256(br) + 2 * a256(bp) + a256(bt) + a256(bd));
        if (rc) return rc;
        char *p = (char *)c->pose_io.ptr;
        d_t = (const float *)p; p += a256(bt);
        d_r = (const float *)p; p += a256(br);
        d_pa = (const float *)p; p += a256(bp);
        d_p = (float *)p; p += a256(bp);
        d_td = trans_delta ? (float *)p : nullptr; p += a256(bt);
        d_rd = rot_mat_delta ? (float *)p : nullptr;
        rc = pedp_upload(c, (void *)d_t, trans, bt);
        if (!rc) rc = pedp_upload(c, (void *)d_r, rot, br);
        if (!rc) rc = pedp_upload(c, (void *)d_pa, poseA, bp);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(update_kernel, dim3((unsigned)((B + PB - 1) / PB)), dim3(PB), 0, c->stream, a, d_t, d_r, d_pa, d_p, d_td,
                       d_rd);
    PEDP_HIP_CHECK(hipGetLastError());
    if (mem == PEDP_HOST) {
        rc = pedp_download(c, poses, d_p, bp);
        if (!rc && trans_delta) rc = pedp_download(c, trans_delta, d_td, bt);
        if (!rc && rot_mat_delta) rc = pedp_download(c, rot_mat_delta, d_rd, bd);
    }
    return rc;
}

int pedp_max_pair_distance(pedp_ctx_t c, const double *pts, int64_t n, int mem, double *out) {
    const char *who = "pedp_max_pair_distance";
    PEDP_REQUIRE(c && out, "%s: null context or output", who);
    PEDP_REQUIRE(mem == PEDP_HOST || mem == PEDP_DEVICE, "%s: bad mem flag %d", who, mem);
    PEDP_REQUIRE(n > 0, "%s: no points", who);
    PEDP_REQUIRE(n <= (int64_t)65535 * TP, "%s: %lld points (at most %d)", who, (long long)n, 65535 * TP);
    PEDP_REQUIRE(pts, "%s: null points", who);
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    const size_t bytes = 24 * (size_t)n;
    int rc = c->pose_ws.reserve(256 + (mem == PEDP_HOST ? a256(bytes) : 0));
    if (rc) return rc;
    char *ws = (char *)c->pose_ws.ptr;
    unsigned long long *d_best = (unsigned long long *)ws;
    int *d_flag = (int *)(ws + 8);
    const double *d_pts = pts;
    if (mem == PEDP_HOST) {
        d_pts = (const double *)(ws + 256);
        rc = pedp_upload(c, (void *)d_pts, pts, bytes);
        if (rc) return rc;
    }
    PEDP_HIP_CHECK(hipMemsetAsync(ws, 0, 16, c->stream));
    const unsigned T = (unsigned)((n + TP - 1) / TP);
    hipLaunchKernelGGL(pair_max_kernel, dim3(T, T), dim3(TP), 0, c->stream, d_pts, n, d_best, d_flag);
    PEDP_HIP_CHECK(hipGetLastError());
    const void *view = nullptr;
    rc = pedp_download_view(c, ws, 16, &view);
    if (rc) return rc;
    unsigned long long bits;
    int flag;
    memcpy(&bits, view, 8);
    memcpy(&flag, (const char *)view + 8, 4);
    double d2;
    memcpy(&d2, &bits, 8);
    *out = flag ? std::nan("") : std::sqrt(d2);
    return PEDP_OK;
}

}  // extern "C"
