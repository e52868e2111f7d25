// What the coverage map (pedp_coverage.hip) shares with the view planner laid over it
// (pedp_viewplan.hip): the per-pixel rule, the per-face state and its criteria, the sums in s4.17's
// block-and-butterfly order, and the handle.  Internal linkage: each including file gets its own copy.
#pragma once
#include "../defectmap/shared.h"
#include "../camera/pixel_ray.h"
#include "../mesh/record.h"
#include <cmath>

namespace {
namespace coverage {

using namespace defectmap;

constexpr int64_t MAX_PIXELS = (int64_t)1 << 31;
constexpr int SUM_BLOCK = 4096;  // faces one wave sums (64 per lane): pedp_defectmap.hip's block
constexpr int SUM_WPB = DT / 64;
constexpr unsigned long long NEVER = ~0ull;  // min_footprint's bits of a face never seen

enum : int { MASKED = 0, MISS = 1, NO_DEPTH = 2, OCCLUDED = 3, BEHIND = 4, GRAZING = 5, SEEN = 6, N_CLASSES = 7 };

// one view: the cast, the sensor's images and the parameters that give a pixel its class
struct View {
    const float *t;
    const uint32_t *id;
    const float *depth;   // nullable
    const uint8_t *mask;  // nullable
    const float *tri;     // the mesh's records as posed
    int64_t n, F;
    camera::Cam cam;
    double fxfy, depth_scale, depth_tol, min_cos;
    float z_min;
};

// The class of pixel i (the table of pedp.h, first rule that holds); for OCCLUDED and SEEN the face, for SEEN the key
// of the cosine and the bits of the footprint (NEVER: a NaN footprint, t = 0 on an edge-on face, takes no part).
__device__ __forceinline__ int classify(const View &a, int64_t i, uint32_t &f, unsigned long long &key, unsigned long long &fp) {
    if (a.mask && a.mask[i] == 0) return MASKED;
    const uint32_t id = a.id[i];
    const float tf = a.t[i];
    if ((int64_t)id >= a.F || (__float_as_uint(tf) & 0x7F800000u) == 0x7F800000u) return MISS;
    float dm = 0.0f;
    if (a.depth) {
        dm = a.depth[i];
        if (!(dm >= a.z_min) || dm == __builtin_inff()) return NO_DEPTH;
    }
    double d[3];
    camera::pixel_direction(a.cam, i, d);
    for (int k = 0; k < 3; ++k) d[k] = (double)(float)d[k];  // the ray that was cast
    const double z_hit = (double)tf * d[2];
    f = id;
    if (a.depth) {
        const double diff = (double)dm * a.depth_scale - z_hit;
        if (diff < -a.depth_tol) return OCCLUDED;
        if (diff > a.depth_tol) return BEHIND;
    }
    double cosine = 0.0;  // a record no ray can hit, or a normal that is NaN: edge on
    record::Tri tr;
    if (record::load_tri(a.tri + (size_t)id * PEDP_TRI_STRIDE, tr)) {
        double n[3];
        record::unit_normal(tr, n);
        const double dp = fabs(record::dot3(n, d));
        if (dp > 0.0) cosine = dp < 1.0 ? dp : 1.0;
    }
    if (cosine < a.min_cos) return GRAZING;
    const double foot = ((z_hit * z_hit) * d[2]) / (a.fxfy * cosine);
    key = key_of(cosine);
    fp = is_nan_bits(bits_of(foot)) ? NEVER : bits_of(foot);
    return SEEN;
}

// the per-face state: the coverage map's own, or a planner's working copy (blocked: the map's alone)
struct State {
    const unsigned long long *pixels, *blocked, *best, *minfp;
    const int32_t *views;
};
__device__ __forceinline__ double cos_of_key(unsigned long long key) { return key ? value_of(key) : 0.0; }
__device__ __forceinline__ double footprint_of_bits(unsigned long long b) { return b == NEVER ? record::pos_inf() : double_of(b); }
__device__ __forceinline__ double best_cos_of(const State &s, int64_t f) { return cos_of_key(s.best[f]); }
__device__ __forceinline__ double min_footprint_of(const State &s, int64_t f) { return footprint_of_bits(s.minfp[f]); }
__device__ __forceinline__ bool is_covered(const State &s, const pedp_coverage_criteria &c, int64_t f) {
    return s.views[f] >= c.min_views && (int64_t)s.pixels[f] >= c.min_pixels && best_cos_of(s, f) >= c.min_cos &&
           min_footprint_of(s, f) <= c.max_footprint;
}

// The summary's two areas in s4.17's block-and-butterfly order over the faces in face order: a wave per block of
// SUM_BLOCK consecutive faces, lane l adds faces l, l + 64, ... of the block one after the other, the butterfly adds the
// 64 lanes; then one wave adds the block sums l, l + 64, ... the same way.
struct Sums {
    double covered_area, total_area;
    int64_t covered;
};
__device__ __forceinline__ double butterfly_sum(double a) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) a = a + double_of(shfl_xor_u64(bits_of(a), off));
    return a;
}
__device__ __forceinline__ int64_t butterfly_sum(int64_t a) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) a += (int64_t)shfl_xor_u64((uint64_t)a, off);
    return a;
}
__device__ __forceinline__ void sums_butterfly(Sums &a) {
    a.covered_area = butterfly_sum(a.covered_area);
    a.total_area = butterfly_sum(a.total_area);
    a.covered = butterfly_sum(a.covered);
}
__global__ __launch_bounds__(DT) void summary_block_kernel(State s, pedp_coverage_criteria c, const double *__restrict__ area, int64_t F,
                                                          int64_t n_blocks, Sums *__restrict__ part) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * SUM_WPB + (threadIdx.x >> 6);
    if (w >= n_blocks) return;  // wave-uniform
    const int64_t f0 = w * SUM_BLOCK, f1 = f0 + SUM_BLOCK < F ? f0 + SUM_BLOCK : F;
    Sums a{0.0, 0.0, 0};
    for (int64_t f = f0 + lane; f < f1; f += 64) {
        const double ar = area[f];
        a.total_area = a.total_area + ar;
        if (is_covered(s, c, f)) {
            a.covered_area = a.covered_area + ar;
            a.covered += 1;
        }
    }
    sums_butterfly(a);
    if (lane == 0) part[w] = a;
}
__global__ __launch_bounds__(64) void summary_total_kernel(const Sums *__restrict__ part, int64_t n_blocks, Sums *__restrict__ out) {
    const int lane = threadIdx.x;
    Sums a{0.0, 0.0, 0};
    for (int64_t b = lane; b < n_blocks; b += 64) {
        a.covered_area = a.covered_area + part[b].covered_area;
        a.total_area = a.total_area + part[b].total_area;
        a.covered += part[b].covered;
    }
    sums_butterfly(a);
    if (lane == 0) *out = a;
}
// both kernels on `stream`: the totals of state `s` into *total (device); part: room for n_blocks rows
inline void launch_summary(hipStream_t stream, const State &s, const pedp_coverage_criteria &c, const double *area, int64_t F, Sums *part,
                           Sums *total) {
    const int64_t n_blocks = (F + SUM_BLOCK - 1) / SUM_BLOCK;
    hipLaunchKernelGGL(summary_block_kernel, dim3((unsigned)((n_blocks + SUM_WPB - 1) / SUM_WPB)), dim3(DT), 0, stream, s, c, area, F, n_blocks,
                       part);
    hipLaunchKernelGGL(summary_total_kernel, dim3(1), dim3(64), 0, stream, part, n_blocks, total);
}

const pedp_coverage_criteria DEFAULT_CRITERIA = {1, 1, 0.0, HUGE_VAL};

}  // namespace coverage
}  // namespace

struct pedp_coverage_s {
    pedp_defect_map_s *map = nullptr;  // borrowed: it must outlive this handle
    pedp_ctx_t ctx = nullptr;
    int device = 0;
    int64_t F = 0;
    char *store = nullptr;  // one allocation: everything below
    unsigned long long *pixels = nullptr, *blocked = nullptr, *best = nullptr, *minfp = nullptr, *counters = nullptr;
    int32_t *views = nullptr;
    uint32_t *stamp = nullptr;
    size_t zero_bytes = 0, ones_off = 0, ones_bytes = 0;  // what clear sets to 0 and to all ones (minfp)
    int64_t n_views = 0;
    pedp_scratch io;  // staging of host-memory calls; the summary's block sums
    coverage::State state() const { return coverage::State{pixels, blocked, best, minfp, views}; }
};
