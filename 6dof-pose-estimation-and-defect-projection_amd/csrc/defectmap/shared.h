// What the defect map (pedp_defectmap.hip) shares with the coverage map laid over its faces
// (pedp_coverage.hip): the handle, the order-preserving key, the in-wave combine of runs of equal face
// ids, and the regions' body behind the marking.  The helpers have internal linkage: each including file gets its own copy.
#pragma once
#include "../pedp_internal.h"

namespace {
namespace defectmap {

constexpr int DT = 256;                  // threads per block of the lane-per-item kernels
constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr int MAX_GROW = 64;

inline size_t a256(size_t b) { return (b + 255) & ~(size_t)255; }
inline unsigned blocks_for(int64_t n) { return (unsigned)((n + DT - 1) / DT); }

struct Carver {
    char *base;
    size_t off = 0;
    template <class T> T *take(size_t n) {
        T *p = (T *)(base + off);
        off = a256(off + sizeof(T) * n);
        return p;
    }
};

// ------------------------------------------------------------------ the order-preserving key of a double
// key(x) < key(y) <=> x < y for non-NaN x, y, with -0 below +0; no non-NaN value has key 0 (-inf has 0x000F...F), so
// 0 stands for "nothing yet".
__host__ __device__ inline uint64_t bits_of(double x) { uint64_t b; memcpy(&b, &x, 8); return b; }
__host__ __device__ inline double double_of(uint64_t b) { double x; memcpy(&x, &b, 8); return x; }
__host__ __device__ inline bool is_nan_bits(uint64_t b) { return (b & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull; }
__host__ __device__ inline uint64_t key_of(double x) {
    const uint64_t b = bits_of(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__host__ __device__ inline double value_of(uint64_t k) { return double_of((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k); }
constexpr uint64_t KEY_PINF = 0xFFF0000000000000ull;  // key_of(+inf)
constexpr uint64_t KEY_NINF = 0x000FFFFFFFFFFFFFull;  // key_of(-inf)

// ------------------------------------------------------------------ runs of equal face ids in neighbouring lanes
// Rows arrive in row-major pixel order, so neighbouring lanes often carry one face.  A run is a maximal stretch of
// neighbouring lanes of one wave with the same id; a lane with NONE takes no part and ends the run before it.  The run's
// first lane (head) speaks for lanes [lane, end] and is the only one that goes to the atomics.
__device__ __forceinline__ unsigned long long shfl_down_u64(unsigned long long v, int off) {
    const unsigned lo = __shfl_down((unsigned)v, off, 64), hi = __shfl_down((unsigned)(v >> 32), off, 64);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int off) {
    const unsigned lo = __shfl_xor((unsigned)v, off, 64), hi = __shfl_xor((unsigned)(v >> 32), off, 64);
    return ((uint64_t)hi << 32) | lo;
}
struct LaneRun {
    bool head;  // this lane opens a run
    bool wide;  // wave-uniform: some run of the wave is longer than one lane (else nothing needs combining)
    int end;    // the last lane of this lane's run
    // the lanes [lane, end] as a mask: a ballot and a popcount count the run's lanes of a kind
    __device__ __forceinline__ unsigned long long lanes(int lane) const {
        return (end == 63 ? ~0ull : ((1ull << (end + 1)) - 1)) & (~0ull << lane);
    }
};
__device__ __forceinline__ LaneRun lane_run(uint32_t fid, int lane) {
    const uint32_t prev = __shfl_up(fid, 1, 64);
    const bool used = fid != NONE;
    LaneRun r;
    r.head = used && (lane == 0 || prev != fid);
    const unsigned long long bounds = __builtin_amdgcn_ballot_w64(r.head || !used);
    r.wide = bounds != ~0ull;
    const unsigned long long above = lane == 63 ? 0ull : (bounds >> (lane + 1)) << (lane + 1);
    r.end = above ? __builtin_ctzll(above) - 1 : 63;
    return r;
}
// the maximum / minimum of `v` over the lanes [lane, end] of a run; every lane of the wave calls it
__device__ __forceinline__ unsigned long long run_max(unsigned long long v, int lane, int end) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long v2 = shfl_down_u64(v, off);
        if (lane + off <= end) v = v2 > v ? v2 : v;
    }
    return v;
}
__device__ __forceinline__ unsigned long long run_min(unsigned long long v, int lane, int end) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long v2 = shfl_down_u64(v, off);
        if (lane + off <= end) v = v2 < v ? v2 : v;
    }
    return v;
}
// the sum (modulo 2^64, so two's complement sums too) of `v` over the lanes [lane, end] of a run: step `off` adds the sum
// of the lanes [lane + off, min(lane + 2 off - 1, end)], so every lane of the run is added once
__device__ __forceinline__ unsigned long long run_sum(unsigned long long v, int lane, int end) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long v2 = shfl_down_u64(v, off);
        if (lane + off <= end) v += v2;
    }
    return v;
}

}  // namespace defectmap
}  // namespace

struct pedp_defect_map_s {
    pedp_ctx_t ctx = nullptr;
    int device = 0;
    int64_t V = 0, F = 0;
    char *store = nullptr;  // one allocation: everything below
    double *area = nullptr, *cen = nullptr, *box = nullptr;
    int32_t *pos_face = nullptr, *pos_run = nullptr, *face_run = nullptr;  // 3 F each
    unsigned long long *peak = nullptr, *hits = nullptr, *counters = nullptr;
    int32_t *frames = nullptr;
    uint32_t *stamp = nullptr;
    size_t state_off = 0, state_bytes = 0;  // peak ... counters: what pedp_defect_map_clear zeroes
    int64_t observations = 0;
    int64_t ignored_host = 0;  // F = 0: the ignored rows (there are no device counters)
    pedp_scratch ws;   // regions: marks, the union-find, the scans, the sorted order
    pedp_scratch io;   // staging of host-memory calls; regions: the block sums and a host-memory call's table
};

// ------------------------------------------------------------------ regions of a marking (pedp_defectmap.hip)
// The regions' workspace, carved from the map's `ws`.  A caller fills seed and mark[0] (F bytes each, the same marking)
// on the context's stream between the two calls below.
struct pedp_region_ws {
    uint8_t *seed = nullptr, *mark[2] = {nullptr, nullptr};
    uint32_t *run_first, *is_root, *rank, *n_blocks, *block_off;
    int32_t *parent, *root, *label, *order, *begin, *end;
    void *tmp;
    size_t tmp_bytes;
};
// the three per-face columns that a region's row sums up besides the geometry: hits (a row's `hits` is their sum),
// frames (`max_frames`) and the key whose maximum over the faces with hits is `peak`
struct pedp_region_columns {
    const unsigned long long *peak_key, *hits;
    const int32_t *frames;
};
// The argument checks of a regions call (`who` names it) and the workspace.  *n_regions is set to 0.  A map without
// faces returns PEDP_OK with w.seed == nullptr: there is nothing to do.
int pedp_defect_regions_begin(pedp_defect_map_s *m, const char *who, int32_t grow, int mem, int64_t capacity, const pedp_defect_region *table,
                              int64_t *n_regions, pedp_region_ws &w);
// Growth, union-find, ranking, the (label, face) sort, the block sums and the rows: everything behind the marking.
int pedp_defect_regions_finish(pedp_defect_map_s *m, const char *who, const pedp_region_ws &w, const pedp_region_columns &col, int32_t grow,
                               int mem, int32_t *labels, int64_t capacity, pedp_defect_region *table, int64_t *n_regions);
