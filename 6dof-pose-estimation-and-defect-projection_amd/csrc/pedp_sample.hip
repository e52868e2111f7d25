// Surface sampling: a point cloud of a triangle mesh -- the model.ply that ICP and the pose errors start
// from -- drawn uniformly by area, and thinned to a spacing (the Poisson-disk rule).  Every result is a pure function of
// (mesh, seed, spacing) that tests/_sample_ref.py restates in numpy bit for bit:
//   * the generator is counter based (sample/philox.h): sample k is two Philox blocks of (k, seed), whoever draws it
//   * the face is chosen from an INTEGER prefix sum of 32-bit area weights (any scan shape gives the same sums) by a
//     64 x 64 -> high 64 multiply; the point is Open3D's (1 - sqrt u1, sqrt u1 (1 - u2), sqrt u1 u2) in float64
//   * the thinning keeps the one set that a visit in ascending (hashed) key order would keep; it is found in rounds of
//     final decisions, so neither the schedule nor the number of rounds can change it.  No kernel waits for another
//     workgroup; the host reads one small counter block per group of rounds.
// float64, no contraction, every expression in the order of the contract (include/pedp.h).  The only atomics are integer:
// the validation's minima, the largest area's bits, the cells' counts and the undecided counter.
#include "cloud/bounds.h"
#include "cloud/grid.h"
#include "mesh/record.h"
#include "sample/philox.h"
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#pragma clang fp contract(off)

struct pedp_mesh_sampler_s {
    pedp_ctx_t ctx = nullptr;
    int device = 0;
    int64_t V = 0, F = 0;
    double *v = nullptr;       // V x 3
    uint32_t *t = nullptr;     // F x 3
    double *vn = nullptr;      // V x 3 vertex normals, or null
    uint64_t *C = nullptr;     // F: the inclusive prefix sum of the faces' weights
    uint64_t W = 0;            // C[F - 1]
    double area = 0.0;         // the areas summed in face order
    double amax = 0.0;         // the largest finite area
    int64_t unsampled = 0;     // faces of weight 0
    // the last pedp_mesh_sample_disk: its draw and the kept samples' indices
    pedp_scratch draw, kept_buf, io;
    int64_t M = 0, K = 0;
    int disk_normals = 0;
    double *d_pts = nullptr, *d_bary = nullptr, *d_nrm = nullptr;
    int32_t *d_face = nullptr;
};

namespace {

constexpr int TT = 256;
constexpr int64_t MAX_FACES = 1 << 24;        // the weights' total stays below 2^57
constexpr int64_t MAX_VERTS = 0xFFFFFFFEll;
constexpr int64_t MAX_POINTS = 1 << 28;       // a thinning's points: int32 positions, 32-bit key indices
constexpr double CELL_CAP = 2097152.0;        // 2^21 grid cells at most
constexpr int GROUP = 6;                      // rounds enqueued between two reads of the undecided counters
constexpr uint32_t UNDECIDED = 0, KEPT = 1, REMOVED = 2;
constexpr uint32_t NONE = 0xFFFFFFFFu;

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + TT - 1) / TT); }

// ------------------------------------------------------------------ the sampler's tables
__global__ __launch_bounds__(TT) void check_tris_kernel(const uint32_t *__restrict__ tri, int64_t E, int64_t V, uint32_t *__restrict__ first) {
    const int64_t e = (int64_t)blockIdx.x * TT + threadIdx.x;
    if (e < E && (int64_t)tri[e] >= V) atomicMin(&first[0], (uint32_t)e);
}
__global__ __launch_bounds__(TT) void check_verts_kernel(const double *__restrict__ v, int64_t V, uint32_t *__restrict__ first) {
    const int64_t i = (int64_t)blockIdx.x * TT + threadIdx.x;
    if (i < V && !pedp_row_finite(v, i)) atomicMin(&first[1], (uint32_t)i);
}

__device__ __forceinline__ void load_face(const double *__restrict__ v, const uint32_t *__restrict__ tri, int64_t f, double p[3][3]) {
    for (int k = 0; k < 3; ++k) {
        const size_t i = tri[3 * f + k];
        p[k][0] = v[3 * i]; p[k][1] = v[3 * i + 1]; p[k][2] = v[3 * i + 2];
    }
}
// e1 x e2 of a face, e1 = v1 - v0, e2 = v2 - v0, and its length sqrt((x^2 + y^2) + z^2)
__device__ __forceinline__ double face_cross(const double p[3][3], double c[3]) {
    double e1[3], e2[3];
    for (int d = 0; d < 3; ++d) { e1[d] = p[1][d] - p[0][d]; e2[d] = p[2][d] - p[0][d]; }
    record::cross3(e1, e2, c);
    return sqrt(record::dot3(c, c));
}
__device__ __forceinline__ bool is_finite(double x) { return (__double_as_longlong(x) & 0x7FF0000000000000ll) != 0x7FF0000000000000ll; }

// a lane per face: its area, and the largest finite one (non-negative doubles order like their bits)
__global__ __launch_bounds__(TT) void area_kernel(const double *__restrict__ v, const uint32_t *__restrict__ tri, int64_t F,
                                                 double *__restrict__ area, unsigned long long *__restrict__ amax_bits) {
    const int64_t f = (int64_t)blockIdx.x * TT + threadIdx.x;
    if (f >= F) return;
    double p[3][3], c[3];
    load_face(v, tri, f, p);
    const double a = 0.5 * face_cross(p, c);
    area[f] = a;
    if (is_finite(a)) atomicMax(amax_bits, (unsigned long long)__double_as_longlong(a));
}
// w_f = floor((area_f / amax) * 2^32); 0 for a face without area or whose area is not finite
__global__ __launch_bounds__(TT) void weight_kernel(const double *__restrict__ area, int64_t F, const unsigned long long *__restrict__ amax_bits,
                                                   unsigned long long *__restrict__ w, unsigned *__restrict__ unsampled) {
    const int64_t f = (int64_t)blockIdx.x * TT + threadIdx.x;
    if (f >= F) return;
    const double amax = __longlong_as_double((long long)*amax_bits), a = area[f];
    unsigned long long x = 0;
    if (a > 0.0 && is_finite(a)) x = (unsigned long long)floor((a / amax) * 4294967296.0);
    w[f] = x;
    if (x == 0) atomicAdd(unsampled, 1u);
}

// ------------------------------------------------------------------ sampling
// A lane per sample k = first + i (mod 2^64): blocks x and y of (k, seed); t = mulhi64(x0:x1, W); the first face whose
// prefix sum exceeds t; the point, its barycentrics, on request a normal, and y2 -- the high word of its thinning key.
__global__ __launch_bounds__(TT) void sample_kernel(const double *__restrict__ v, const uint32_t *__restrict__ tri, const double *__restrict__ vn,
                                                   const unsigned long long *__restrict__ C, int64_t F, unsigned long long W,
                                                   unsigned long long seed, unsigned long long first, int64_t n, int mode,
                                                   double *__restrict__ pts, int32_t *__restrict__ face, double *__restrict__ bary,
                                                   double *__restrict__ nrm, uint32_t *__restrict__ z) {
    const int64_t i = (int64_t)blockIdx.x * TT + threadIdx.x;
    if (i >= n) return;
    const unsigned long long k = first + (unsigned long long)i;
    uint32_t x[4], y[4];
    philox::draw(k, 0u, seed, x);
    philox::draw(k, 1u, seed, y);
    const unsigned long long t = __umul64hi(((unsigned long long)x[0] << 32) | x[1], W);
    int64_t lo = 0, hi = F - 1;  // C[F - 1] = W > t: the answer lies in [lo, hi]
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (C[mid] > t) hi = mid; else lo = mid + 1;
    }
    const int64_t f = lo;
    const double u1 = (double)((((unsigned long long)x[2] << 32) | x[3]) >> 11) * 0x1p-53;
    const double u2 = (double)((((unsigned long long)y[0] << 32) | y[1]) >> 11) * 0x1p-53;
    const double s = sqrt(u1), a = 1.0 - s, b = s * (1.0 - u2), c = s * u2;
    double p[3][3];
    load_face(v, tri, f, p);
    for (int d = 0; d < 3; ++d) pts[3 * i + d] = (a * p[0][d] + b * p[1][d]) + c * p[2][d];
    if (face) face[i] = (int32_t)f;
    if (bary) { bary[3 * i] = a; bary[3 * i + 1] = b; bary[3 * i + 2] = c; }
    if (z) z[i] = y[2];
    if (mode == PEDP_SAMPLE_NORMALS_VERTEX) {
        double q[3][3];
        load_face(vn, tri, f, q);
        for (int d = 0; d < 3; ++d) nrm[3 * i + d] = (a * q[0][d] + b * q[1][d]) + c * q[2][d];
    } else if (mode == PEDP_SAMPLE_NORMALS_TRIANGLE) {
        double cr[3];
        const double len = face_cross(p, cr);
        for (int d = 0; d < 3; ++d) nrm[3 * i + d] = cr[d] / len;
    }
}

// ------------------------------------------------------------------ thinning
// key of point i: (z_i << 32) | (i mod 2^32); the lower key wins.  z_i: a mesh sample's y2, or word 0 of block 2 of (i, seed)
__global__ __launch_bounds__(TT) void key_kernel(const uint32_t *__restrict__ z, unsigned long long seed, int64_t M, unsigned long long *__restrict__ key) {
    const int64_t i = (int64_t)blockIdx.x * TT + threadIdx.x;
    if (i >= M) return;
    uint32_t zi;
    if (z) zi = z[i];
    else { uint32_t w[4]; philox::draw((unsigned long long)i, 2u, seed, w); zi = w[0]; }
    key[i] = ((unsigned long long)zi << 32) | (uint32_t)i;
}
__global__ __launch_bounds__(TT) void gather_key_kernel(const unsigned long long *__restrict__ key, const int *__restrict__ idx_sorted, int64_t M,
                                                       unsigned long long *__restrict__ key_s, uint32_t *__restrict__ state) {
    const int64_t q = (int64_t)blockIdx.x * TT + threadIdx.x;
    if (q >= M) return;
    key_s[q] = key[idx_sorted[q]];
    state[q] = UNDECIDED;
}
// One round, a lane per point of the cell-sorted order that is still undecided: REMOVED once a conflicting point of a
// lower key is KEPT, KEPT once every conflicting point of a lower key is REMOVED.  A state is written once and only by
// its own lane; a neighbour's state may be read from before or during the round -- decisions are final, so either is
// right.  i and j conflict iff ((dx^2 + dy^2) + dz^2) < r2, strictly.  The cells x0 .. x1 of one x row are one run.
__global__ __launch_bounds__(TT) void thin_round_kernel(Grid g, const double *__restrict__ sp, const unsigned long long *__restrict__ key_s,
                                                       const int *__restrict__ begin, int64_t M, double r2, uint32_t *state,
                                                       uint32_t *__restrict__ undecided) {
    const int64_t q = (int64_t)blockIdx.x * TT + threadIdx.x;
    if (q >= M) return;
    if (__atomic_load_n(&state[q], __ATOMIC_RELAXED) != UNDECIDED) return;
    const double p[3] = {sp[3 * q], sp[3 * q + 1], sp[3 * q + 2]};
    const unsigned long long kq = key_s[q];
    const int cx = grid_axis(p[0], g.lo[0], g.cell, g.dim[0]), cy = grid_axis(p[1], g.lo[1], g.cell, g.dim[1]),
              cz = grid_axis(p[2], g.lo[2], g.cell, g.dim[2]);
    const int x0 = max(cx - 1, 0), x1 = min(cx + 1, g.dim[0] - 1);
    bool removed = false, blocked = false;
    for (int zc = max(cz - 1, 0); zc <= min(cz + 1, g.dim[2] - 1) && !removed; ++zc)
        for (int yc = max(cy - 1, 0); yc <= min(cy + 1, g.dim[1] - 1) && !removed; ++yc) {
            const int base = g.dim[0] * (yc + g.dim[1] * zc);
            const int js = begin[base + x0], je = begin[base + x1 + 1];
            for (int j = js; j < je; ++j) {
                if (key_s[j] >= kq) continue;
                if (!(dist2(p, sp + 3 * (size_t)j) < r2)) continue;
                const uint32_t st = __atomic_load_n(&state[j], __ATOMIC_RELAXED);
                if (st == KEPT) { removed = true; break; }
                if (st == UNDECIDED) blocked = true;
            }
        }
    if (removed) __atomic_store_n(&state[q], REMOVED, __ATOMIC_RELAXED);
    else if (!blocked) __atomic_store_n(&state[q], KEPT, __ATOMIC_RELAXED);
    else atomicAdd(undecided, 1u);
}
// the kept flags in the points' own order; flag[M] = 0 closes the scan
__global__ __launch_bounds__(TT) void flag_kernel(const uint32_t *__restrict__ state, const int *__restrict__ idx_sorted, int64_t M, uint32_t *__restrict__ flag) {
    const int64_t q = (int64_t)blockIdx.x * TT + threadIdx.x;
    if (q > M) return;
    if (q == M) { flag[M] = 0; return; }
    flag[idx_sorted[q]] = state[q] == KEPT;
}
__global__ __launch_bounds__(TT) void fill_kernel(uint32_t *__restrict__ flag, int64_t M, uint32_t value) {
    const int64_t i = (int64_t)blockIdx.x * TT + threadIdx.x;
    if (i > M) return;
    flag[i] = i < M ? value : 0u;
}
__global__ __launch_bounds__(TT) void compact_kernel(const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pos, int64_t M, int64_t cap,
                                                    int32_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * TT + threadIdx.x;
    if (i < M && flag[i] && (int64_t)pos[i] < cap) out[pos[i]] = (int32_t)i;
}
// the kept points' keys, in the points' order (sorted next: the N lowest stay)
__global__ __launch_bounds__(TT) void kept_keys_kernel(const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pos,
                                                      const unsigned long long *__restrict__ key, int64_t M, unsigned long long *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * TT + threadIdx.x;
    if (i < M && flag[i]) out[pos[i]] = key[i];
}
__global__ __launch_bounds__(TT) void lowest_kernel(const unsigned long long *__restrict__ key, const unsigned long long *__restrict__ sorted, int64_t N,
                                                   int64_t M, uint32_t *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * TT + threadIdx.x;
    if (i < M) flag[i] = flag[i] && key[i] <= sorted[N - 1];
}
// rows idx[j] of a draw, j < K
__global__ __launch_bounds__(TT) void gather_rows_kernel(const int32_t *__restrict__ idx, int64_t K, const double *__restrict__ pts,
                                                        const int32_t *__restrict__ face, const double *__restrict__ bary, const double *__restrict__ nrm,
                                                        double *__restrict__ o_pts, int32_t *__restrict__ o_face, double *__restrict__ o_bary,
                                                        double *__restrict__ o_nrm) {
    const int64_t j = (int64_t)blockIdx.x * TT + threadIdx.x;
    if (j >= K) return;
    const size_t i = (size_t)idx[j];
    for (int d = 0; d < 3; ++d) {
        if (o_pts) o_pts[3 * j + d] = pts[3 * i + d];
        if (o_bary) o_bary[3 * j + d] = bary[3 * i + d];
        if (o_nrm) o_nrm[3 * j + d] = nrm[3 * i + d];
    }
    if (o_face) o_face[j] = face[i];
}

// ------------------------------------------------------------------ host side
int copy_in(pedp_ctx_t c, void *dst, const void *src, size_t bytes, int mem) {
    if (bytes == 0) return PEDP_OK;
    if (mem == PEDP_HOST) return pedp_upload(c, dst, src, bytes);
    PEDP_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream));
    return PEDP_OK;
}
int dev_alloc(void **p, size_t bytes, const char *who) {
    const hipError_t e = hipMalloc(p, bytes ? bytes : 256);
    if (e != hipSuccess) {
        *p = nullptr;
        pedp_set_error("%s: hipMalloc(%zu) -> %s", who, bytes, hipGetErrorString(e));
        return PEDP_ERR_HIP;
    }
    return PEDP_OK;
}

// One thinning's workspace, carved from the context's sample_ws: sized once for M points and the cell cap, so that the
// probes of a count form never move it.
struct ThinWs {
    unsigned *cell, *count, *cell_s;
    int *slot, *begin, *idx;
    double *sp, *part;
    unsigned long long *key_s, *sel, *sel_sorted;
    uint32_t *state, *counters, *flag, *pos;
    void *tmp;
    size_t tmp_bytes;
};
int thin_ws(pedp_ctx_t c, int64_t M, ThinWs &w) {
    const size_t m = (size_t)M, cells = (size_t)CELL_CAP + 1;
    size_t t_cells = 0, t_pts = 0, t_sort = 0;
    PEDP_ROCPRIM(rocprim::exclusive_scan(nullptr, t_cells, (uint32_t *)nullptr, (uint32_t *)nullptr, 0u, cells, rocprim::plus<uint32_t>(), c->stream));
    PEDP_ROCPRIM(rocprim::exclusive_scan(nullptr, t_pts, (uint32_t *)nullptr, (uint32_t *)nullptr, 0u, m + 1, rocprim::plus<uint32_t>(), c->stream));
    PEDP_ROCPRIM(rocprim::radix_sort_keys(nullptr, t_sort, (unsigned long long *)nullptr, (unsigned long long *)nullptr, m ? m : 1, 0, 64, c->stream));
    w.tmp_bytes = t_cells > t_pts ? t_cells : t_pts;
    if (t_sort > w.tmp_bytes) w.tmp_bytes = t_sort;
    w.tmp_bytes += 16 * m + 4096;  // a sort of fewer keys may merge instead, in buffers of its own
    const size_t bytes = 6 * a256(4 * m) + 2 * a256(4 * cells) + a256(24 * m) + a256(48 * BND_BLOCKS) + 3 * a256(8 * m) + a256(4 * GROUP) +
                         2 * a256(4 * (m + 1)) + a256(w.tmp_bytes) + 4096;
    PEDP_TRY(c->sample_ws.reserve(bytes));
    Carver k{(char *)c->sample_ws.ptr};
    w.cell = k.take<unsigned>(m); w.cell_s = k.take<unsigned>(m); w.slot = k.take<int>(m); w.idx = k.take<int>(m);
    w.state = k.take<uint32_t>(m);
    w.count = k.take<unsigned>(cells); w.begin = k.take<int>(cells);
    w.sp = k.take<double>(3 * m); w.part = k.take<double>(6 * BND_BLOCKS);
    w.key_s = k.take<unsigned long long>(m); w.sel = k.take<unsigned long long>(m); w.sel_sorted = k.take<unsigned long long>(m);
    w.counters = k.take<uint32_t>(GROUP);
    w.flag = k.take<uint32_t>(m + 1); w.pos = k.take<uint32_t>(m + 1);
    w.tmp = k.take<char>(w.tmp_bytes);
    return PEDP_OK;
}

// the workspace's scans and its sort: the scratch was sized for the largest of them, which each call checks
int scan_u32(pedp_ctx_t c, const ThinWs &w, const uint32_t *in, uint32_t *out, size_t n) {
    size_t need = 0;
    PEDP_ROCPRIM(rocprim::exclusive_scan(nullptr, need, in, out, 0u, n, rocprim::plus<uint32_t>(), c->stream));
    PEDP_REQUIRE(need <= w.tmp_bytes, "pedp_sample: a scan of %zu entries needs %zu bytes of scratch, %zu are there", n, need, w.tmp_bytes);
    PEDP_ROCPRIM(rocprim::exclusive_scan(w.tmp, need, in, out, 0u, n, rocprim::plus<uint32_t>(), c->stream));
    return PEDP_OK;
}
int sort_u64(pedp_ctx_t c, const ThinWs &w, const unsigned long long *in, unsigned long long *out, size_t n) {
    size_t need = 0;
    PEDP_ROCPRIM(rocprim::radix_sort_keys(nullptr, need, in, out, n, 0, 64, c->stream));
    PEDP_REQUIRE(need <= w.tmp_bytes, "pedp_sample: a sort of %zu keys needs %zu bytes of scratch, %zu are there", n, need, w.tmp_bytes);
    PEDP_ROCPRIM(rocprim::radix_sort_keys(w.tmp, need, in, out, n, 0, 64, c->stream));
    return PEDP_OK;
}

// the points' box (lo xyz, hi xyz); a non-finite coordinate is refused
int points_box(pedp_ctx_t c, const ThinWs &w, const double *d_pts, int64_t M, double box[6], const char *who) {
    hipLaunchKernelGGL(bounds_kernel, dim3(BND_BLOCKS), dim3(256), 0, c->stream, d_pts, M, w.part);
    PEDP_HIP_CHECK(hipGetLastError());
    std::vector<double> part(6 * BND_BLOCKS);
    PEDP_TRY(pedp_download(c, part.data(), w.part, 48 * BND_BLOCKS));
    for (int k = 0; k < 3; ++k) { box[k] = part[k]; box[3 + k] = part[3 + k]; }
    for (int b = 0; b < BND_BLOCKS; ++b) {
        PEDP_REQUIRE(part[6 * b] == part[6 * b], "%s: points has a non-finite coordinate", who);
        for (int k = 0; k < 3; ++k) {
            if (part[6 * b + k] < box[k]) box[k] = part[6 * b + k];
            if (part[6 * b + 3 + k] > box[3 + k]) box[3 + k] = part[6 * b + 3 + k];
        }
    }
    for (int k = 0; k < 3; ++k)
        PEDP_REQUIRE(std::isfinite(box[3 + k] - box[k]), "%s: the points' extent overflows float64", who);
    return PEDP_OK;
}

// The grid of a thinning at spacing r: cells a little wider than r (so that rounding in a point's cell index cannot
// put two conflicting points two cells apart), at least 2^-20 of the largest extent, doubled until they fit the cap.
Grid thin_grid(const double box[6], double r) {
    Grid g;
    double ext[3], emax = 0.0;
    for (int k = 0; k < 3; ++k) { g.lo[k] = box[k]; ext[k] = box[3 + k] - box[k]; if (ext[k] > emax) emax = ext[k]; }
    double cell = r * 1.0009765625;
    if (cell < emax * 0x1p-20) cell = emax * 0x1p-20;
    if (!(cell > 0.0)) cell = 1.0;
    while (true) {
        double cells = 1.0;
        for (int k = 0; k < 3; ++k) { g.dim[k] = (int)floor(ext[k] / cell) + 1; cells *= (double)g.dim[k]; }
        if (cells <= CELL_CAP) break;
        cell *= 2.0;
    }
    g.cell = cell;
    return g;
}

// S(r) of the M points d_pts under the keys d_key: w.flag[i] = 1 for a kept point (w.flag[M] = 0), w.pos its exclusive
// scan, *count = |S(r)|.  rounds (nullable) is ADDED to.
int thin_once(pedp_ctx_t c, const ThinWs &w, const double *d_pts, const unsigned long long *d_key, int64_t M, double r, const double box[6],
              int64_t *count, int32_t *rounds, const char *who) {
    hipStream_t s = c->stream;
    const double r2 = r * r;
    if (!(r2 > 0.0)) {  // nothing is closer than 0: every point stays
        hipLaunchKernelGGL(fill_kernel, dim3(blocks_for(M + 1)), dim3(TT), 0, s, w.flag, M, 1u);
    } else {
        const Grid g = thin_grid(box, r);
        const size_t cells = (size_t)g.dim[0] * g.dim[1] * g.dim[2];
        PEDP_HIP_CHECK(hipMemsetAsync(w.count, 0, 4 * (cells + 1), s));
        hipLaunchKernelGGL(grid_count_kernel, dim3(blocks_for(M)), dim3(TT), 0, s, d_pts, M, g, w.cell, w.slot, w.count);
        PEDP_TRY(scan_u32(c, w, w.count, (uint32_t *)w.begin, cells + 1));
        hipLaunchKernelGGL(grid_place_kernel, dim3(blocks_for(M)), dim3(TT), 0, s, d_pts, M, w.cell, w.slot, w.begin, w.sp, w.idx, w.cell_s);
        hipLaunchKernelGGL(gather_key_kernel, dim3(blocks_for(M)), dim3(TT), 0, s, d_key, w.idx, M, w.key_s, w.state);
        PEDP_HIP_CHECK(hipGetLastError());
        int64_t launched = 0;
        while (true) {
            PEDP_HIP_CHECK(hipMemsetAsync(w.counters, 0, 4 * GROUP, s));
            for (int k = 0; k < GROUP; ++k)
                hipLaunchKernelGGL(thin_round_kernel, dim3(blocks_for(M)), dim3(TT), 0, s, g, w.sp, w.key_s, w.begin, M, r2, w.state, w.counters + k);
            PEDP_HIP_CHECK(hipGetLastError());
            uint32_t left[GROUP];
            PEDP_TRY(pedp_download(c, left, w.counters, sizeof(left)));
            int k = 0;
            while (k < GROUP && left[k] != 0) ++k;
            if (k < GROUP) { if (rounds) *rounds += (int32_t)(launched + k + 1); break; }
            launched += GROUP;
            // a round decides at least the undecided point of the lowest key: M rounds always suffice
            PEDP_REQUIRE(launched <= M, "%s: %lld points are undecided after %lld rounds", who, (long long)left[GROUP - 1], (long long)launched);
        }
        hipLaunchKernelGGL(flag_kernel, dim3(blocks_for(M + 1)), dim3(TT), 0, s, w.state, w.idx, M, w.flag);
    }
    PEDP_TRY(scan_u32(c, w, w.flag, w.pos, (size_t)M + 1));
    PEDP_HIP_CHECK(hipGetLastError());
    uint32_t n = 0;
    PEDP_TRY(pedp_download(c, &n, w.pos + M, 4));
    *count = (int64_t)n;
    return PEDP_OK;
}

// The count form: r bisected on [0, r_hi] for 24 halvings towards the largest spacing that still keeps N of the M
// points; of S(r*) the N lowest keys, in ascending index, to d_out (N x int32).
int thin_to_count(pedp_ctx_t c, const ThinWs &w, const double *d_pts, const unsigned long long *d_key, int64_t M, int64_t N, double r_hi,
                  const double box[6], int32_t *d_out, double *spacing, int32_t *rounds, int32_t *probes, const char *who) {
    hipStream_t s = c->stream;
    double lo = 0.0, hi = r_hi;
    int64_t count = 0;
    int32_t n_probes = 0, last_rounds = 0;
    bool have_last = false;  // w.flag / w.pos hold S(lo)
    for (int it = 0; it < 24; ++it) {
        const double mid = 0.5 * (lo + hi);
        last_rounds = 0;
        PEDP_TRY(thin_once(c, w, d_pts, d_key, M, mid, box, &count, &last_rounds, who));
        ++n_probes;
        if (count >= N) { lo = mid; have_last = true; }
        else { hi = mid; have_last = false; }
    }
    if (!have_last) {
        last_rounds = 0;
        PEDP_TRY(thin_once(c, w, d_pts, d_key, M, lo, box, &count, &last_rounds, who));
        ++n_probes;
    }
    PEDP_REQUIRE(count >= N, "%s: the thinning at spacing %g kept %lld of %lld points, fewer than the %lld asked for", who, lo, (long long)count,
                 (long long)M, (long long)N);
    if (count > N) {
        hipLaunchKernelGGL(kept_keys_kernel, dim3(blocks_for(M)), dim3(TT), 0, s, w.flag, w.pos, d_key, M, w.sel);
        PEDP_TRY(sort_u64(c, w, w.sel, w.sel_sorted, (size_t)count));
        hipLaunchKernelGGL(lowest_kernel, dim3(blocks_for(M)), dim3(TT), 0, s, d_key, w.sel_sorted, N, M, w.flag);
        PEDP_TRY(scan_u32(c, w, w.flag, w.pos, (size_t)M + 1));
    }
    hipLaunchKernelGGL(compact_kernel, dim3(blocks_for(M)), dim3(TT), 0, s, w.flag, w.pos, M, N, d_out);
    PEDP_HIP_CHECK(hipGetLastError());
    if (spacing) *spacing = lo;
    if (rounds) *rounds = last_rounds;
    if (probes) *probes = n_probes;
    return PEDP_OK;
}

int sampler_build(pedp_mesh_sampler_s *m, const double *verts, const uint32_t *tris, const double *normals, int mem, const char *who) {
    pedp_ctx_t c = m->ctx;
    hipStream_t s = c->stream;
    const int64_t V = m->V, F = m->F, E = 3 * F;
    PEDP_TRY(dev_alloc((void **)&m->v, 24 * (size_t)V, who));
    PEDP_TRY(dev_alloc((void **)&m->t, 4 * (size_t)E, who));
    PEDP_TRY(dev_alloc((void **)&m->C, 8 * (size_t)F, who));
    if (normals) PEDP_TRY(dev_alloc((void **)&m->vn, 24 * (size_t)V, who));
    PEDP_TRY(copy_in(c, m->v, verts, 24 * (size_t)V, mem));
    PEDP_TRY(copy_in(c, m->t, tris, 4 * (size_t)E, mem));
    if (normals) PEDP_TRY(copy_in(c, m->vn, normals, 24 * (size_t)V, mem));
    size_t tmp_bytes = 0;
    PEDP_ROCPRIM(rocprim::inclusive_scan(nullptr, tmp_bytes, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (size_t)F,
                                         rocprim::plus<unsigned long long>(), s));
    PEDP_TRY(m->io.reserve(2 * a256(8 * (size_t)F) + a256(tmp_bytes) + 1024));
    Carver k{(char *)m->io.ptr};
    double *area = k.take<double>((size_t)F);
    unsigned long long *w = k.take<unsigned long long>((size_t)F);
    uint32_t *first = k.take<uint32_t>(2);
    unsigned long long *amax_bits = k.take<unsigned long long>(1);
    unsigned *unsampled = k.take<unsigned>(1);
    void *tmp = k.take<char>(tmp_bytes);
    // the arguments' check, before any kernel follows an index
    PEDP_HIP_CHECK(hipMemsetAsync(first, 0xFF, 8, s));
    hipLaunchKernelGGL(check_tris_kernel, dim3(blocks_for(E)), dim3(TT), 0, s, m->t, E, V, first);
    hipLaunchKernelGGL(check_verts_kernel, dim3(blocks_for(V)), dim3(TT), 0, s, m->v, V, first);
    PEDP_HIP_CHECK(hipGetLastError());
    uint32_t bad[2] = {NONE, NONE};
    PEDP_TRY(pedp_download(c, bad, first, sizeof(bad)));
    PEDP_REQUIRE(bad[0] == NONE, "%s: triangles: triangle %u names a vertex outside the %lld given", who, bad[0] / 3, (long long)V);
    PEDP_REQUIRE(bad[1] == NONE, "%s: vertices: vertex %u has a non-finite coordinate", who, bad[1]);
    // areas, the largest, the weights and their prefix sum
    PEDP_HIP_CHECK(hipMemsetAsync(amax_bits, 0, 8, s));
    PEDP_HIP_CHECK(hipMemsetAsync(unsampled, 0, 4, s));
    hipLaunchKernelGGL(area_kernel, dim3(blocks_for(F)), dim3(TT), 0, s, m->v, m->t, F, area, amax_bits);
    hipLaunchKernelGGL(weight_kernel, dim3(blocks_for(F)), dim3(TT), 0, s, area, F, amax_bits, w, unsampled);
    PEDP_ROCPRIM(rocprim::inclusive_scan(tmp, tmp_bytes, w, (unsigned long long *)m->C, (size_t)F, rocprim::plus<unsigned long long>(), s));
    PEDP_HIP_CHECK(hipGetLastError());
    std::vector<double> host_area((size_t)F);
    PEDP_TRY(pedp_download(c, host_area.data(), area, 8 * (size_t)F));
    unsigned long long bits = 0;
    unsigned zero = 0;
    PEDP_TRY(pedp_download(c, &bits, amax_bits, 8));
    PEDP_TRY(pedp_download(c, &zero, unsampled, 4));
    PEDP_TRY(pedp_download(c, &m->W, m->C + (F - 1), 8));
    memcpy(&m->amax, &bits, 8);
    m->unsampled = (int64_t)zero;
    double sum = 0.0;  // in face order: part of the contract (the count form's first bracket, the spacing form's draw)
    for (int64_t f = 0; f < F; ++f) sum = sum + host_area[(size_t)f];
    m->area = sum;
    PEDP_REQUIRE(m->W > 0, "%s: triangles: all %lld faces are degenerate (no face has an area)", who, (long long)F);
    return PEDP_OK;
}

// the output of a host-memory call: staged in `io`, downloaded behind the kernel
struct Out {
    void *user = nullptr, *dev = nullptr;
    size_t bytes = 0;
};
int stage_outputs(pedp_ctx_t c, pedp_scratch &io, Out *o, int n, int mem) {
    if (mem != PEDP_HOST) {
        for (int i = 0; i < n; ++i) o[i].dev = o[i].user;
        return PEDP_OK;
    }
    size_t total = 256;
    for (int i = 0; i < n; ++i) total += o[i].user ? a256(o[i].bytes) : 0;
    PEDP_TRY(io.reserve(total));
    size_t off = 0;
    for (int i = 0; i < n; ++i) {
        o[i].dev = o[i].user ? (char *)io.ptr + off : nullptr;
        off += o[i].user ? a256(o[i].bytes) : 0;
    }
    return PEDP_OK;
}
int fetch_outputs(pedp_ctx_t c, Out *o, int n, int mem) {
    if (mem != PEDP_HOST) return PEDP_OK;
    for (int i = 0; i < n; ++i)
        if (o[i].user) PEDP_TRY(pedp_download(c, o[i].user, o[i].dev, o[i].bytes));
    return PEDP_OK;
}

int check_mode(pedp_mesh_sampler_t m, int normals, const char *who) {
    PEDP_REQUIRE(normals == PEDP_SAMPLE_NORMALS_NONE || normals == PEDP_SAMPLE_NORMALS_VERTEX || normals == PEDP_SAMPLE_NORMALS_TRIANGLE,
                 "%s: normals = %d", who, normals);
    PEDP_REQUIRE(normals != PEDP_SAMPLE_NORMALS_VERTEX || m->vn, "%s: normals: the sampler was created without vertex normals", who);
    return PEDP_OK;
}

}  // namespace

extern "C" {

int pedp_mesh_sampler_create(pedp_ctx_t c, const double *verts, int64_t V, const uint32_t *tris, int64_t F, const double *vertex_normals,
                             int mem, pedp_mesh_sampler_t *out) {
    const char *who = "pedp_mesh_sampler_create";
    PEDP_REQUIRE(out, "%s: null out", who);
    *out = nullptr;
    PEDP_REQUIRE(c, "%s: null context", who);
    PEDP_REQUIRE(mem == PEDP_HOST || mem == PEDP_DEVICE, "%s: bad mem flag %d", who, mem);
    PEDP_REQUIRE(V >= 1 && V <= MAX_VERTS && F >= 1 && F <= MAX_FACES, "%s: V = %lld, F = %lld (at least one face, at most 2^24)", who,
                 (long long)V, (long long)F);
    PEDP_REQUIRE(verts && tris, "%s: null array", who);
    PEDP_REQUIRE(!c->icp_pending, "%s: a registration is pending on this context (the call waits for the stream)", who);
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    pedp_mesh_sampler_s *m = new pedp_mesh_sampler_s;
    m->ctx = c;
    m->device = c->device;
    m->V = V;
    m->F = F;
    const int rc = sampler_build(m, verts, tris, vertex_normals, mem, who);
    if (rc) {
        (void)hipStreamSynchronize(c->stream);
        pedp_mesh_sampler_destroy(m);
        return rc;
    }
    *out = m;
    return PEDP_OK;
}

int pedp_mesh_sampler_destroy(pedp_mesh_sampler_t m) {
    if (!m) return PEDP_OK;
    if (hipSetDevice(m->device) == hipSuccess) {
        if (m->v) (void)hipFree(m->v);  // waits for the device: nothing enqueued still uses it
        if (m->t) (void)hipFree(m->t);
        if (m->vn) (void)hipFree(m->vn);
        if (m->C) (void)hipFree(m->C);
        m->draw.release();
        m->kept_buf.release();
        m->io.release();
    }
    delete m;
    return PEDP_OK;
}

int pedp_mesh_sampler_info(pedp_mesh_sampler_t m, pedp_mesh_sampler_info_t *info) {
    PEDP_REQUIRE(m && info, "pedp_mesh_sampler_info: null %s", m ? "info" : "handle");
    info->vertices = m->V;
    info->faces = m->F;
    info->unsampled_faces = m->unsampled;
    info->total_weight = m->W;
    info->area = m->area;
    info->largest_area = m->amax;
    info->has_vertex_normals = m->vn != nullptr;
    return PEDP_OK;
}

int pedp_mesh_sample(pedp_mesh_sampler_t m, uint64_t seed, uint64_t first, int64_t n, int normals, int mem, double *points, int32_t *face_ids,
                     double *barycentric, double *normals_out) {
    const char *who = "pedp_mesh_sample";
    PEDP_REQUIRE(m, "%s: null handle", who);
    pedp_ctx_t c = m->ctx;
    PEDP_REQUIRE(mem == PEDP_HOST || mem == PEDP_DEVICE, "%s: bad mem flag %d", who, mem);
    PEDP_REQUIRE(n >= 0 && n <= MAX_POINTS, "%s: n = %lld (at most 2^28 samples a call)", who, (long long)n);
    PEDP_TRY(check_mode(m, normals, who));
    PEDP_REQUIRE(mem == PEDP_DEVICE || !c->icp_pending, "%s: a registration is pending on this context (host-memory call)", who);
    if (n == 0) return PEDP_OK;
    PEDP_REQUIRE(points, "%s: null points", who);
    PEDP_REQUIRE(normals == PEDP_SAMPLE_NORMALS_NONE || normals_out, "%s: normals asked for, null normals_out", who);
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    Out o[4] = {{points, nullptr, 24 * (size_t)n}, {face_ids, nullptr, 4 * (size_t)n}, {barycentric, nullptr, 24 * (size_t)n},
                {normals == PEDP_SAMPLE_NORMALS_NONE ? nullptr : normals_out, nullptr, 24 * (size_t)n}};
    PEDP_TRY(stage_outputs(c, m->io, o, 4, mem));
    hipLaunchKernelGGL(sample_kernel, dim3(blocks_for(n)), dim3(TT), 0, c->stream, m->v, m->t, m->vn, (const unsigned long long *)m->C, m->F,
                       (unsigned long long)m->W, (unsigned long long)seed, (unsigned long long)first, n, normals, (double *)o[0].dev,
                       (int32_t *)o[1].dev, (double *)o[2].dev, (double *)o[3].dev, (uint32_t *)nullptr);
    PEDP_HIP_CHECK(hipGetLastError());
    return fetch_outputs(c, o, 4, mem);
}

int pedp_points_thin(pedp_ctx_t c, const double *points, int64_t n, double spacing, uint64_t seed, int mem, int64_t capacity, int32_t *kept,
                     int64_t *count, int32_t *rounds) {
    const char *who = "pedp_points_thin";
    PEDP_REQUIRE(c, "%s: null context", who);
    PEDP_REQUIRE(count, "%s: null count", who);
    *count = 0;
    if (rounds) *rounds = 0;
    PEDP_REQUIRE(mem == PEDP_HOST || mem == PEDP_DEVICE, "%s: bad mem flag %d", who, mem);
    PEDP_REQUIRE(n >= 0 && n <= MAX_POINTS, "%s: n = %lld (at most 2^28 points)", who, (long long)n);
    PEDP_REQUIRE(spacing >= 0.0 && std::isfinite(spacing), "%s: spacing = %g must be a finite number >= 0", who, spacing);
    PEDP_REQUIRE(capacity >= 0 && (kept || capacity == 0), "%s: capacity = %lld, kept %s", who, (long long)capacity, kept ? "given" : "null");
    PEDP_REQUIRE(!c->icp_pending, "%s: a registration is pending on this context (the call waits for the stream)", who);
    if (n == 0) return PEDP_OK;
    PEDP_REQUIRE(points, "%s: null points", who);
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    const size_t m = (size_t)n;
    PEDP_TRY(c->sample_io.reserve(a256(24 * m) + a256(8 * m) + a256(4 * m) + 256));
    Carver k{(char *)c->sample_io.ptr};
    double *up = k.take<double>(3 * m);
    unsigned long long *key = k.take<unsigned long long>(m);
    int32_t *out = k.take<int32_t>(m);
    const double *d_pts = points;
    if (mem == PEDP_HOST) { PEDP_TRY(pedp_upload(c, up, points, 24 * m)); d_pts = up; }
    ThinWs w;
    PEDP_TRY(thin_ws(c, n, w));
    double box[6];
    PEDP_TRY(points_box(c, w, d_pts, n, box, who));
    hipLaunchKernelGGL(key_kernel, dim3(blocks_for(n)), dim3(TT), 0, c->stream, (const uint32_t *)nullptr, (unsigned long long)seed, n, key);
    PEDP_TRY(thin_once(c, w, d_pts, key, n, spacing, box, count, rounds, who));
    const int64_t fit = *count < capacity ? *count : capacity;  // short of capacity: the count says what to come back with
    if (fit == 0) return PEDP_OK;
    int32_t *d_out = mem == PEDP_HOST ? out : kept;
    hipLaunchKernelGGL(compact_kernel, dim3(blocks_for(n)), dim3(TT), 0, c->stream, w.flag, w.pos, n, fit, d_out);
    PEDP_HIP_CHECK(hipGetLastError());
    if (mem == PEDP_HOST) return pedp_download(c, kept, out, 4 * (size_t)fit);
    return PEDP_OK;
}

int pedp_points_thin_count(pedp_ctx_t c, const double *points, int64_t n, int64_t number_of_points, double spacing_max, uint64_t seed, int mem,
                           int32_t *kept, double *spacing, int32_t *rounds, int32_t *probes) {
    const char *who = "pedp_points_thin_count";
    PEDP_REQUIRE(c, "%s: null context", who);
    PEDP_REQUIRE(mem == PEDP_HOST || mem == PEDP_DEVICE, "%s: bad mem flag %d", who, mem);
    PEDP_REQUIRE(n >= 1 && n <= MAX_POINTS, "%s: n = %lld (1 ... 2^28 points)", who, (long long)n);
    PEDP_REQUIRE(number_of_points >= 1 && number_of_points <= n, "%s: number_of_points = %lld must lie in 1 ... %lld, the points given", who,
                 (long long)number_of_points, (long long)n);
    PEDP_REQUIRE(spacing_max >= 0.0 && std::isfinite(spacing_max), "%s: spacing_max = %g must be a finite number >= 0", who, spacing_max);
    PEDP_REQUIRE(points && kept, "%s: null array", who);
    PEDP_REQUIRE(!c->icp_pending, "%s: a registration is pending on this context (the call waits for the stream)", who);
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    const size_t m = (size_t)n;
    PEDP_TRY(c->sample_io.reserve(a256(24 * m) + a256(8 * m) + a256(4 * m) + 256));
    Carver k{(char *)c->sample_io.ptr};
    double *up = k.take<double>(3 * m);
    unsigned long long *key = k.take<unsigned long long>(m);
    int32_t *out = k.take<int32_t>(m);
    const double *d_pts = points;
    if (mem == PEDP_HOST) { PEDP_TRY(pedp_upload(c, up, points, 24 * m)); d_pts = up; }
    ThinWs w;
    PEDP_TRY(thin_ws(c, n, w));
    double box[6];
    PEDP_TRY(points_box(c, w, d_pts, n, box, who));
    hipLaunchKernelGGL(key_kernel, dim3(blocks_for(n)), dim3(TT), 0, c->stream, (const uint32_t *)nullptr, (unsigned long long)seed, n, key);
    int32_t *d_out = mem == PEDP_HOST ? out : kept;
    PEDP_TRY(thin_to_count(c, w, d_pts, key, n, number_of_points, spacing_max, box, d_out, spacing, rounds, probes, who));
    if (mem == PEDP_HOST) return pedp_download(c, kept, out, 4 * (size_t)number_of_points);
    return PEDP_OK;
}

int pedp_mesh_sample_disk(pedp_mesh_sampler_t m, uint64_t seed, int64_t number_of_points, double spacing, int64_t init_factor, int normals,
                          int64_t *count, int64_t *drawn, double *spacing_out, int32_t *rounds, int32_t *probes) {
    const char *who = "pedp_mesh_sample_disk";
    PEDP_REQUIRE(m, "%s: null handle", who);
    pedp_ctx_t c = m->ctx;
    PEDP_REQUIRE(count, "%s: null count", who);
    *count = 0;
    m->M = m->K = 0;
    const bool by_count = number_of_points != 0;
    PEDP_REQUIRE(number_of_points >= 0, "%s: number_of_points = %lld must be at least 1", who, (long long)number_of_points);
    PEDP_REQUIRE(by_count != (spacing >= 0.0 || spacing != spacing), "%s: give number_of_points (and spacing < 0) or spacing (and number_of_points 0), got %lld and %g",
                 who, (long long)number_of_points, spacing);
    PEDP_REQUIRE(by_count || (spacing > 0.0 && std::isfinite(spacing)), "%s: spacing = %g must be a positive finite number", who, spacing);
    PEDP_REQUIRE(init_factor >= 1, "%s: init_factor = %lld must be at least 1", who, (long long)init_factor);
    PEDP_TRY(check_mode(m, normals, who));
    PEDP_REQUIRE(std::isfinite(m->area) && m->area > 0.0, "%s: the mesh's area %g is not a positive finite number", who, m->area);
    PEDP_REQUIRE(!c->icp_pending, "%s: a registration is pending on this context (the call waits for the stream)", who);
    double want = by_count ? (double)init_factor * (double)number_of_points : ceil(((double)init_factor * m->area) / (spacing * spacing));
    if (want < 1.0) want = 1.0;
    PEDP_REQUIRE(want <= (double)MAX_POINTS, "%s: %s draws %.0f samples (at most 2^28)", who, by_count ? "number_of_points x init_factor" : "this spacing", want);
    const int64_t M = (int64_t)want;
    const size_t mm = (size_t)M;
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    PEDP_TRY(m->draw.reserve(3 * a256(24 * mm) + 2 * a256(4 * mm) + a256(8 * mm) + 256));
    PEDP_TRY(m->kept_buf.reserve(a256(4 * mm) + 256));
    Carver k{(char *)m->draw.ptr};
    m->d_pts = k.take<double>(3 * mm);
    m->d_bary = k.take<double>(3 * mm);
    m->d_nrm = k.take<double>(3 * mm);
    m->d_face = k.take<int32_t>(mm);
    uint32_t *z = k.take<uint32_t>(mm);
    unsigned long long *key = k.take<unsigned long long>(mm);
    int32_t *d_kept = (int32_t *)m->kept_buf.ptr;
    hipLaunchKernelGGL(sample_kernel, dim3(blocks_for(M)), dim3(TT), 0, c->stream, m->v, m->t, m->vn, (const unsigned long long *)m->C, m->F,
                       (unsigned long long)m->W, (unsigned long long)seed, 0ull, M, normals, m->d_pts, m->d_face, m->d_bary, m->d_nrm, z);
    hipLaunchKernelGGL(key_kernel, dim3(blocks_for(M)), dim3(TT), 0, c->stream, z, 0ull, M, key);
    PEDP_HIP_CHECK(hipGetLastError());
    ThinWs w;
    PEDP_TRY(thin_ws(c, M, w));
    double box[6];
    PEDP_TRY(points_box(c, w, m->d_pts, M, box, who));
    int64_t K = 0;
    int32_t n_rounds = 0, n_probes = 1;
    double r = spacing;
    if (by_count) {
        K = number_of_points;
        PEDP_TRY(thin_to_count(c, w, m->d_pts, key, M, K, 2.0 * sqrt(m->area / (double)number_of_points), box, d_kept, &r, &n_rounds, &n_probes, who));
    } else {
        PEDP_TRY(thin_once(c, w, m->d_pts, key, M, spacing, box, &K, &n_rounds, who));
        hipLaunchKernelGGL(compact_kernel, dim3(blocks_for(M)), dim3(TT), 0, c->stream, w.flag, w.pos, M, K, d_kept);
        PEDP_HIP_CHECK(hipGetLastError());
    }
    m->M = M;
    m->K = K;
    m->disk_normals = normals;
    *count = K;
    if (drawn) *drawn = M;
    if (spacing_out) *spacing_out = r;
    if (rounds) *rounds = n_rounds;
    if (probes) *probes = n_probes;
    return PEDP_OK;
}

int pedp_mesh_sample_disk_read(pedp_mesh_sampler_t m, int mem, double *points, int32_t *face_ids, double *barycentric, double *normals_out,
                               int32_t *sample_index) {
    const char *who = "pedp_mesh_sample_disk_read";
    PEDP_REQUIRE(m, "%s: null handle", who);
    pedp_ctx_t c = m->ctx;
    PEDP_REQUIRE(mem == PEDP_HOST || mem == PEDP_DEVICE, "%s: bad mem flag %d", who, mem);
    PEDP_REQUIRE(!normals_out || m->disk_normals != PEDP_SAMPLE_NORMALS_NONE, "%s: normals_out given, the last pedp_mesh_sample_disk drew no normals", who);
    PEDP_REQUIRE(mem == PEDP_DEVICE || !c->icp_pending, "%s: a registration is pending on this context (host-memory call)", who);
    const int64_t K = m->K;
    if (K == 0) return PEDP_OK;
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    Out o[5] = {{points, nullptr, 24 * (size_t)K}, {face_ids, nullptr, 4 * (size_t)K}, {barycentric, nullptr, 24 * (size_t)K},
                {normals_out, nullptr, 24 * (size_t)K}, {sample_index, nullptr, 4 * (size_t)K}};
    PEDP_TRY(stage_outputs(c, m->io, o, 5, mem));
    const int32_t *d_kept = (const int32_t *)m->kept_buf.ptr;
    hipLaunchKernelGGL(gather_rows_kernel, dim3(blocks_for(K)), dim3(TT), 0, c->stream, d_kept, K, m->d_pts, m->d_face, m->d_bary, m->d_nrm,
                       (double *)o[0].dev, (int32_t *)o[1].dev, (double *)o[2].dev, (double *)o[3].dev);
    if (o[4].dev) PEDP_HIP_CHECK(hipMemcpyAsync(o[4].dev, d_kept, 4 * (size_t)K, hipMemcpyDeviceToDevice, c->stream));
    PEDP_HIP_CHECK(hipGetLastError());
    return fetch_outputs(c, o, 5, mem);
}

}  // extern "C"
