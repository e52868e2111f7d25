// The defect map: what the projected heat maps of many frames say about the CAD model itself.
//   * per FACE, in the model frame: the peak intensity, the number of hits and the number of observations (frames)
//     that hit it.  Triangle indices keep the input's order in every mesh handle whatever the pose, so the map is a
//     constant-size object that never needs a transform (run.py:61, :119, :196-201 keeps a growing list of hit clouds
//     and moves every one of them at every detection).
//   * regions: the connected components of the marked faces under the welded edge adjacency, with their sizes.
// No floating-point atomic anywhere: the maximum goes through an order-preserving 64-bit integer key, the counts are
// integers, and a region's floating-point sums are formed in a fixed order (below), so every output is a function of
// the inputs alone.
#include "defectmap/shared.h"
#include "mesh/topology.h"
#include <cmath>
#include <rocprim/device/device_scan.hpp>

namespace {

using namespace defectmap;

constexpr int64_t MAX_FACES = 1 << 28;   // 3 F edge slots are sorted with int32 positions
constexpr int64_t MAX_ROWS = (int64_t)1 << 31;
constexpr int SUM_BLOCK = 4096;          // faces of a region one wave sums (64 per lane); longer runs are split

#define PEDP_ROCPRIM(expr)                                                                     \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) {                                                                \
            pedp_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(e_)); \
            return PEDP_ERR_HIP;                                                               \
        }                                                                                      \
    } while (0)

// ------------------------------------------------------------------ creation
// area, centroid and box of every face; float64, no contraction, in the order of the contract
__global__ __launch_bounds__(DT) void face_geometry_kernel(const double *__restrict__ v, const uint32_t *__restrict__ tri, int64_t F,
                                                          double *__restrict__ area, double *__restrict__ cen, double *__restrict__ box) {
    const int64_t f = (int64_t)blockIdx.x * DT + threadIdx.x;
    if (f >= F) return;
    double p[3][3];
    for (int k = 0; k < 3; ++k) {
        const size_t i = tri[3 * f + k];
        p[k][0] = v[3 * i]; p[k][1] = v[3 * i + 1]; p[k][2] = v[3 * i + 2];
    }
    const double ab[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
    const double ac[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
    const double n0 = ab[1] * ac[2] - ab[2] * ac[1], n1 = ab[2] * ac[0] - ab[0] * ac[2], n2 = ab[0] * ac[1] - ab[1] * ac[0];
    area[f] = 0.5 * sqrt((n0 * n0 + n1 * n1) + n2 * n2);
    for (int d = 0; d < 3; ++d) {
        cen[3 * f + d] = ((p[0][d] + p[1][d]) + p[2][d]) / 3.0;
        uint64_t lo = KEY_PINF, hi = KEY_NINF;  // a NaN coordinate takes no part; none left: +inf / -inf
        for (int k = 0; k < 3; ++k) {
            if (is_nan_bits(bits_of(p[k][d]))) continue;
            const uint64_t key = key_of(p[k][d]);
            lo = key < lo ? key : lo;
            hi = key > hi ? key : hi;
        }
        box[6 * f + d] = value_of(lo);
        box[6 * f + 3 + d] = value_of(hi);
    }
}

// position p of the sorted slots opens a run of equal keys: its own position, else 0 (an inclusive max scan turns
// these into every position's run start)
__global__ __launch_bounds__(DT) void run_head_kernel(const unsigned long long *__restrict__ key, const int32_t *__restrict__ perm, int64_t E,
                                                     int32_t *__restrict__ head) {
    const int64_t p = (int64_t)blockIdx.x * DT + threadIdx.x;
    if (p >= E) return;
    head[p] = (p > 0 && key[perm[p]] != key[perm[p - 1]]) ? (int32_t)p : 0;
}
// per sorted position: its face and its run (-1: no edge); per edge slot of a face: the run it is in
__global__ __launch_bounds__(DT) void run_fill_kernel(const unsigned long long *__restrict__ key, const int32_t *__restrict__ perm,
                                                     const int32_t *__restrict__ start, int64_t E, int32_t *__restrict__ pos_face,
                                                     int32_t *__restrict__ pos_run, int32_t *__restrict__ face_run) {
    const int64_t p = (int64_t)blockIdx.x * DT + threadIdx.x;
    if (p >= E) return;
    const int32_t e = perm[p];
    const int32_t r = key[e] == ~0ull ? -1 : start[p];
    pos_face[p] = e / 3;
    pos_run[p] = r;
    face_run[e] = r;
}

// ------------------------------------------------------------------ accumulating
// One observation's rows.  Integer atomics only: the key's maximum, the 64-bit count, and the observation stamp whose
// maximum tells the first arrival of this observation on a face (the one that sees an older stamp come back) from the rest.
__global__ __launch_bounds__(DT) void add_kernel(const uint32_t *__restrict__ id, const double *__restrict__ inten, int64_t n, int64_t F,
                                                uint32_t obs, unsigned long long *__restrict__ peak, unsigned long long *__restrict__ hits,
                                                int32_t *__restrict__ frames, uint32_t *__restrict__ stamp,
                                                unsigned long long *__restrict__ counters) {
    const int64_t i = (int64_t)blockIdx.x * DT + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool live = false, used = false;
    uint32_t f = NONE;
    unsigned long long key = 0, count = 1;
    if (i < n) {
        live = true;
        f = id[i];
        const double x = inten[i];
        used = (int64_t)f < F && !is_nan_bits(bits_of(x));
        key = key_of(x);
    }
    // Hits arrive in row-major pixel order, so neighbouring lanes often carry one face: a run of equal ids in
    // neighbouring lanes sends its maximum and its length through its first lane alone.  Measured: a frame's 35,863
    // hits take the same 12 us either way, 368,640 rows piled onto 64 faces 0.08 ms in the place of 2.5 ms.
    const LaneRun run = lane_run(used ? f : NONE, lane);
    if (run.wide) {
        key = run_max(key, lane, run.end);
        count = (unsigned long long)(run.end - lane + 1);
    }
    if (run.head) {
        atomicMax(&peak[f], key);
        atomicAdd(&hits[f], count);
        if (atomicMax(&stamp[f], obs) < obs) atomicAdd(&frames[f], 1);
    }
    const int n_used = __builtin_popcountll(__builtin_amdgcn_ballot_w64(used));
    const int n_ign = __builtin_popcountll(__builtin_amdgcn_ballot_w64(live && !used));
    if (lane == 0) {
        if (n_used) atomicAdd(&counters[0], (unsigned long long)n_used);
        if (n_ign) atomicAdd(&counters[1], (unsigned long long)n_ign);
    }
}

__global__ __launch_bounds__(DT) void faces_kernel(const unsigned long long *__restrict__ peak_key, const unsigned long long *__restrict__ hits,
                                                  const int32_t *__restrict__ frames, int64_t F, double *__restrict__ peak,
                                                  int64_t *__restrict__ out_hits, int32_t *__restrict__ out_frames) {
    const int64_t f = (int64_t)blockIdx.x * DT + threadIdx.x;
    if (f >= F) return;
    if (peak) peak[f] = hits[f] ? value_of(peak_key[f]) : 0.0;
    if (out_hits) out_hits[f] = (int64_t)hits[f];
    if (out_frames) out_frames[f] = frames[f];
}

// ------------------------------------------------------------------ regions
__global__ __launch_bounds__(DT) void seed_kernel(const unsigned long long *__restrict__ peak_key, const unsigned long long *__restrict__ hits,
                                                 const int32_t *__restrict__ frames, int64_t F, double threshold, int32_t min_frames,
                                                 uint8_t *__restrict__ seed, uint8_t *__restrict__ mark) {
    const int64_t f = (int64_t)blockIdx.x * DT + threadIdx.x;
    if (f >= F) return;
    const uint8_t m = hits[f] > 0 && value_of(peak_key[f]) > threshold && frames[f] >= min_frames;
    seed[f] = m;
    mark[f] = m;
}
// every run learns the first of its positions whose face is marked (none: NONE)
__global__ __launch_bounds__(DT) void run_first_kernel(const int32_t *__restrict__ pos_face, const int32_t *__restrict__ pos_run, int64_t E,
                                                      const uint8_t *__restrict__ mark, uint32_t *__restrict__ run_first) {
    const int64_t p = (int64_t)blockIdx.x * DT + threadIdx.x;
    if (p >= E) return;
    const int32_t r = pos_run[p];
    if (r >= 0 && mark[pos_face[p]]) atomicMin(&run_first[r], (uint32_t)p);
}
// one round of growth: a face is marked if it was, or if one of its edges' runs holds a marked face
__global__ __launch_bounds__(DT) void grow_kernel(const int32_t *__restrict__ face_run, const uint32_t *__restrict__ run_first, int64_t F,
                                                 const uint8_t *__restrict__ mark, uint8_t *__restrict__ out) {
    const int64_t f = (int64_t)blockIdx.x * DT + threadIdx.x;
    if (f >= F) return;
    uint8_t m = mark[f];
    for (int k = 0; k < 3; ++k) {
        const int32_t r = face_run[3 * f + k];
        if (r >= 0 && run_first[r] != NONE) m = 1;
    }
    out[f] = m;
}
__global__ __launch_bounds__(DT) void parent_init_kernel(const uint8_t *__restrict__ mark, int64_t F, int32_t *__restrict__ parent) {
    const int64_t f = (int64_t)blockIdx.x * DT + threadIdx.x;
    if (f < F) parent[f] = mark[f] ? (int32_t)f : -1;
}

// Union-find as pedp_cloudops.hip's DBSCAN keeps it: parent[x] <= x names a member of x's component, only a root is
// ever hooked (compare-and-swap on parent[root] == root, the larger root under the smaller), and a find halves its
// path with stores of ancestors.  The root is then the component's lowest face.
__device__ __forceinline__ int32_t uf_load(int32_t *parent, int32_t x) { return __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int32_t uf_find(int32_t *parent, int32_t a) {
    int32_t r = a;
    while (true) {
        const int32_t p = uf_load(parent, r);
        if (p == r) return r;
        const int32_t gp = uf_load(parent, p);
        if (gp != p) __hip_atomic_store(&parent[r], gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        r = p;
    }
}
// every marked face of a run is united with the run's first marked one
__global__ __launch_bounds__(DT) void union_kernel(const int32_t *__restrict__ pos_face, const int32_t *__restrict__ pos_run, int64_t E,
                                                  const uint8_t *__restrict__ mark, const uint32_t *__restrict__ run_first,
                                                  int32_t *__restrict__ parent) {
    const int64_t p = (int64_t)blockIdx.x * DT + threadIdx.x;
    if (p >= E) return;
    const int32_t r = pos_run[p];
    if (r < 0) return;
    const int32_t f = pos_face[p];
    if (!mark[f]) return;
    const uint32_t q = run_first[r];
    if (q == (uint32_t)p) return;
    int32_t a = uf_find(parent, f), b = uf_find(parent, pos_face[q]);
    while (a != b) {
        if (a < b) { const int32_t t = a; a = b; b = t; }
        if (atomicCAS(&parent[a], a, b) == a) break;
        a = uf_find(parent, a);
        b = uf_find(parent, b);
    }
}
__global__ __launch_bounds__(DT) void root_kernel(const uint8_t *__restrict__ mark, int64_t F, int32_t *__restrict__ parent, int32_t *__restrict__ root,
                                                 uint32_t *__restrict__ is_root /* F + 1 */) {
    const int64_t f = (int64_t)blockIdx.x * DT + threadIdx.x;
    if (f > F) return;
    if (f == F) { is_root[F] = 0; return; }
    const int32_t r = mark[f] ? uf_find(parent, (int32_t)f) : -1;
    root[f] = r;
    is_root[f] = r == (int32_t)f;
}
// the label of a face: the rank of its root among the roots in face order; also the key of the (label, face) sort
__global__ __launch_bounds__(DT) void label_kernel(const int32_t *__restrict__ root, const uint32_t *__restrict__ rank, int64_t F,
                                                  int32_t *__restrict__ label, int32_t *__restrict__ label_out) {
    const int64_t f = (int64_t)blockIdx.x * DT + threadIdx.x;
    if (f >= F) return;
    const int32_t r = root[f];
    const int32_t l = r < 0 ? -1 : (int32_t)rank[r];
    label[f] = l;
    if (label_out) label_out[f] = l;
}
__global__ __launch_bounds__(DT) void label_key_kernel(const int32_t *__restrict__ label, int64_t F, unsigned long long *__restrict__ key) {
    const int64_t f = (int64_t)blockIdx.x * DT + threadIdx.x;
    if (f < F) key[f] = (uint32_t)label[f];  // -1 sorts last
}
// the run [begin, end) of every region among the faces sorted by (label, face), and its number of summing blocks
__global__ __launch_bounds__(DT) void region_range_kernel(const int32_t *__restrict__ label, const int32_t *__restrict__ order, int64_t F,
                                                         int32_t *__restrict__ begin, int32_t *__restrict__ end) {
    const int64_t p = (int64_t)blockIdx.x * DT + threadIdx.x;
    if (p >= F) return;
    const int32_t l = label[order[p]];
    if (l < 0) return;
    if (p == 0 || label[order[p - 1]] != l) begin[l] = (int32_t)p;
    if (p == F - 1 || label[order[p + 1]] != l) end[l] = (int32_t)p + 1;
}
__global__ __launch_bounds__(DT) void region_blocks_kernel(const int32_t *__restrict__ begin, const int32_t *__restrict__ end, int64_t R,
                                                          uint32_t *__restrict__ n_blocks /* R + 1 */) {
    const int64_t r = (int64_t)blockIdx.x * DT + threadIdx.x;
    if (r > R) return;
    n_blocks[r] = r == R ? 0u : (uint32_t)((end[r] - begin[r] + SUM_BLOCK - 1) / SUM_BLOCK);
}

// What one wave knows of a region or of one block of it.  The two floating-point sums take their terms in a fixed
// order (below); everything else is an integer sum or a maximum / minimum of keys, which no order can change.
struct Part {
    double area, m[3];
    uint64_t peak, lo[3], hi[3];
    int64_t hits;
    int32_t n_seed, max_frames;
};
__device__ __forceinline__ void part_init(Part &a) {
    a.area = 0.0; a.hits = 0; a.n_seed = 0; a.max_frames = 0; a.peak = 0;
    for (int d = 0; d < 3; ++d) { a.m[d] = 0.0; a.lo[d] = KEY_PINF; a.hi[d] = KEY_NINF; }
}
// this lane's value and its partner's of the butterfly step `off`: a + b is the same on both sides, bit for bit
__device__ __forceinline__ void part_butterfly(Part &a) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        a.area = a.area + double_of(shfl_xor_u64(bits_of(a.area), off));
        a.hits += (int64_t)shfl_xor_u64((uint64_t)a.hits, off);
        a.n_seed += __shfl_xor(a.n_seed, off, 64);
        const int32_t mf = __shfl_xor(a.max_frames, off, 64);
        a.max_frames = mf > a.max_frames ? mf : a.max_frames;
        const uint64_t pk = shfl_xor_u64(a.peak, off);
        a.peak = pk > a.peak ? pk : a.peak;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            a.m[d] = a.m[d] + double_of(shfl_xor_u64(bits_of(a.m[d]), off));
            const uint64_t lo = shfl_xor_u64(a.lo[d], off), hi = shfl_xor_u64(a.hi[d], off);
            a.lo[d] = lo < a.lo[d] ? lo : a.lo[d];
            a.hi[d] = hi > a.hi[d] ? hi : a.hi[d];
        }
    }
}
__device__ __forceinline__ void part_merge(Part &a, const Part &b) {
    a.area = a.area + b.area;
    a.hits += b.hits;
    a.n_seed += b.n_seed;
    a.max_frames = b.max_frames > a.max_frames ? b.max_frames : a.max_frames;
    a.peak = b.peak > a.peak ? b.peak : a.peak;
    for (int d = 0; d < 3; ++d) {
        a.m[d] = a.m[d] + b.m[d];
        a.lo[d] = b.lo[d] < a.lo[d] ? b.lo[d] : a.lo[d];
        a.hi[d] = b.hi[d] > a.hi[d] ? b.hi[d] : a.hi[d];
    }
}

struct SumArgs {
    const int32_t *order, *begin, *end;
    const uint32_t *block_off;  // R + 1: exclusive scan of the regions' block counts
    int64_t R;
    const double *area, *cen, *box;
    const unsigned long long *peak_key, *hits;
    const int32_t *frames;
    const uint8_t *seed;
    Part *part;
};
// First pass, a wave per block of SUM_BLOCK consecutive positions of a region's run: lane l adds positions l, l + 64,
// l + 128, ... of the block one after the other, then the butterfly adds the 64 lanes.
constexpr int SUM_WPB = DT / 64;
__global__ __launch_bounds__(DT) void region_block_sum_kernel(SumArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * SUM_WPB + (threadIdx.x >> 6);
    if (w >= (int64_t)a.block_off[a.R]) return;  // wave-uniform
    int64_t lo_r = 0, hi_r = a.R;                // the region of block w: the last r with block_off[r] <= w
    while (hi_r - lo_r > 1) {
        const int64_t mid = (lo_r + hi_r) >> 1;
        if ((int64_t)a.block_off[mid] <= w) lo_r = mid; else hi_r = mid;
    }
    const int64_t r = lo_r;
    const int64_t p0 = (int64_t)a.begin[r] + (w - (int64_t)a.block_off[r]) * SUM_BLOCK;
    const int64_t p1 = p0 + SUM_BLOCK < (int64_t)a.end[r] ? p0 + SUM_BLOCK : (int64_t)a.end[r];
    Part s;
    part_init(s);
    for (int64_t p = p0 + lane; p < p1; p += 64) {
        const size_t f = (size_t)a.order[p];
        const double ar = a.area[f];
        s.area = s.area + ar;
        for (int d = 0; d < 3; ++d) {
            s.m[d] = s.m[d] + ar * a.cen[3 * f + d];
            const double bl = a.box[6 * f + d], bh = a.box[6 * f + 3 + d];
            const uint64_t kl = key_of(bl), kh = key_of(bh);
            s.lo[d] = kl < s.lo[d] ? kl : s.lo[d];
            s.hi[d] = kh > s.hi[d] ? kh : s.hi[d];
        }
        const unsigned long long h = a.hits[f];
        s.hits += (int64_t)h;
        if (h) s.peak = a.peak_key[f] > s.peak ? a.peak_key[f] : s.peak;
        s.n_seed += a.seed[f];
        s.max_frames = a.frames[f] > s.max_frames ? a.frames[f] : s.max_frames;
    }
    part_butterfly(s);
    if (lane == 0) a.part[w] = s;
}
// Second pass, a wave per region: lane l adds the region's block sums l, l + 64, ... in that order, then the same
// butterfly; lane 0 writes the row.
__global__ __launch_bounds__(DT) void region_row_kernel(SumArgs a, pedp_defect_region *__restrict__ table) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * SUM_WPB + (threadIdx.x >> 6);
    if (r >= a.R) return;  // wave-uniform
    Part s;
    part_init(s);
    for (int64_t b = (int64_t)a.block_off[r] + lane; b < (int64_t)a.block_off[r + 1]; b += 64) part_merge(s, a.part[b]);
    part_butterfly(s);
    if (lane != 0) return;
    pedp_defect_region row;
    row.first_face = a.order[a.begin[r]];
    row.n_faces = a.end[r] - a.begin[r];
    row.n_seed_faces = s.n_seed;
    row.max_frames = s.max_frames;
    row.hits = s.hits;
    row.area = s.area;
    row.peak = s.peak ? value_of(s.peak) : 0.0;
    for (int d = 0; d < 3; ++d) {
        row.moment[d] = s.m[d];
        row.centroid[d] = s.m[d] / s.area;
        if (!(s.area > 0.0) && !is_nan_bits(bits_of(s.area))) row.centroid[d] = double_of(0x7FF8000000000000ull);
        row.lo[d] = value_of(s.lo[d]);
        row.hi[d] = value_of(s.hi[d]);
    }
    table[r] = row;
}

}  // namespace

namespace {

using RegionWs = pedp_region_ws;
int region_ws(pedp_defect_map_s *m, RegionWs &w) {
    const size_t F = (size_t)m->F, E = 3 * F;
    size_t t1 = 0, t2 = 0;
    PEDP_ROCPRIM(rocprim::exclusive_scan(nullptr, t1, (uint32_t *)nullptr, (uint32_t *)nullptr, 0u, F + 1, rocprim::plus<uint32_t>(),
                                         m->ctx->stream));
    PEDP_ROCPRIM(rocprim::inclusive_scan(nullptr, t2, (int32_t *)nullptr, (int32_t *)nullptr, E, rocprim::maximum<int32_t>(),
                                         m->ctx->stream));
    w.tmp_bytes = t1 > t2 ? t1 : t2;
    const size_t need = 3 * a256(F) + a256(4 * E) + 4 * a256(4 * (F + 1)) + 6 * a256(4 * F) + a256(w.tmp_bytes) + 4096;
    const int rc = m->ws.reserve(need);
    if (rc) return rc;
    Carver cv{(char *)m->ws.ptr};
    w.seed = cv.take<uint8_t>(F); w.mark[0] = cv.take<uint8_t>(F); w.mark[1] = cv.take<uint8_t>(F);
    w.run_first = cv.take<uint32_t>(E);
    w.is_root = cv.take<uint32_t>(F + 1); w.rank = cv.take<uint32_t>(F + 1);
    w.n_blocks = cv.take<uint32_t>(F + 1); w.block_off = cv.take<uint32_t>(F + 1);
    w.parent = cv.take<int32_t>(F); w.root = cv.take<int32_t>(F); w.label = cv.take<int32_t>(F);
    w.order = cv.take<int32_t>(F); w.begin = cv.take<int32_t>(F); w.end = cv.take<int32_t>(F);
    w.tmp = cv.take<char>(w.tmp_bytes);
    return PEDP_OK;
}

int build_adjacency(pedp_defect_map_s *m, const uint32_t *d_tri, const uint32_t *d_w) {
    pedp_ctx_t c = m->ctx;
    const int64_t E = 3 * m->F;
    // scratch of the build in the map's workspace (the regions' layout takes it over afterwards)
    size_t tmp_bytes = 0;
    PEDP_ROCPRIM(rocprim::inclusive_scan(nullptr, tmp_bytes, (int32_t *)nullptr, (int32_t *)nullptr, (size_t)E, rocprim::maximum<int32_t>(),
                                         c->stream));
    int rc = m->ws.reserve(a256(8 * (size_t)E) + 3 * a256(4 * (size_t)E) + a256(tmp_bytes) + 1024);
    if (rc) return rc;
    Carver cv{(char *)m->ws.ptr};
    unsigned long long *key_copy = cv.take<unsigned long long>((size_t)E);
    int32_t *perm = cv.take<int32_t>((size_t)E), *head = cv.take<int32_t>((size_t)E), *start = cv.take<int32_t>((size_t)E);
    void *tmp = cv.take<char>(tmp_bytes);
    rc = topology::sort_edges(c, d_tri, d_w, E, key_copy, perm);
    if (rc) return rc;
    hipLaunchKernelGGL(run_head_kernel, dim3(blocks_for(E)), dim3(DT), 0, c->stream, key_copy, perm, E, head);
    PEDP_ROCPRIM(rocprim::inclusive_scan(tmp, tmp_bytes, head, start, (size_t)E, rocprim::maximum<int32_t>(), c->stream));
    hipLaunchKernelGGL(run_fill_kernel, dim3(blocks_for(E)), dim3(DT), 0, c->stream, key_copy, perm, start, E, m->pos_face, m->pos_run,
                       m->face_run);
    PEDP_HIP_CHECK(hipGetLastError());
    return PEDP_OK;
}

}  // namespace

extern "C" {

int pedp_defect_map_create(pedp_ctx_t c, const double *verts, int64_t V, const uint32_t *tris, int64_t F, pedp_defect_map_t *out) {
    const char *who = "pedp_defect_map_create";
    PEDP_REQUIRE(c && out, "%s: null context/out", who);
    PEDP_REQUIRE(V >= 0 && V < ((int64_t)1 << 32) - 1 && F >= 0 && F <= MAX_FACES, "%s: V = %lld, F = %lld (at most 2^28 faces)", who,
                 (long long)V, (long long)F);
    PEDP_REQUIRE((verts || V == 0) && (tris || F == 0), "%s: null array", who);
    PEDP_REQUIRE(!c->icp_pending, "%s: a registration is pending on this context (the call waits for the stream)", who);
    for (int64_t i = 0; i < 3 * F; ++i)
        PEDP_REQUIRE((int64_t)tris[i] < V, "%s: triangle %lld names vertex %u of %lld", who, (long long)(i / 3), tris[i], (long long)V);
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    pedp_defect_map_s *m = new pedp_defect_map_s;
    m->ctx = c;
    m->device = c->device;
    m->V = V;
    m->F = F;
    *out = m;
    if (F == 0) return PEDP_OK;
    const size_t f = (size_t)F, E = 3 * f;
    size_t off = 0;
    auto place = [&](size_t bytes) { const size_t o = off; off += a256(bytes); return o; };
    const size_t o_area = place(8 * f), o_cen = place(24 * f), o_box = place(48 * f), o_pf = place(4 * E), o_pr = place(4 * E),
                 o_fr = place(4 * E);
    m->state_off = off;
    const size_t o_peak = place(8 * f), o_hits = place(8 * f), o_frames = place(4 * f), o_stamp = place(4 * f), o_cnt = place(16);
    m->state_bytes = off - m->state_off;
    int rc = PEDP_OK;
    hipError_t e = hipMalloc((void **)&m->store, off);
    if (e != hipSuccess) {
        pedp_set_error("%s: hipMalloc(%zu) -> %s", who, off, hipGetErrorString(e));
        rc = PEDP_ERR_HIP;
    }
    if (!rc) {
        m->area = (double *)(m->store + o_area); m->cen = (double *)(m->store + o_cen); m->box = (double *)(m->store + o_box);
        m->pos_face = (int32_t *)(m->store + o_pf); m->pos_run = (int32_t *)(m->store + o_pr); m->face_run = (int32_t *)(m->store + o_fr);
        m->peak = (unsigned long long *)(m->store + o_peak); m->hits = (unsigned long long *)(m->store + o_hits);
        m->frames = (int32_t *)(m->store + o_frames); m->stamp = (uint32_t *)(m->store + o_stamp);
        m->counters = (unsigned long long *)(m->store + o_cnt);
        // the vertices, the triangles, the weld's table and ids: needed by the build alone
        const uint64_t slots = topology::weld_slots(V);
        const size_t b_v = a256(24 * (size_t)V), b_t = a256(4 * E), b_s = a256(4 * slots), b_w = a256(4 * (size_t)V);
        rc = m->io.reserve(b_v + b_t + b_s + b_w);
        if (!rc) {
            char *io = (char *)m->io.ptr;
            double *d_v = (double *)io;
            uint32_t *d_t = (uint32_t *)(io + b_v), *d_s = (uint32_t *)(io + b_v + b_t), *d_w = (uint32_t *)(io + b_v + b_t + b_s);
            rc = pedp_upload(c, d_v, verts, 24 * (size_t)V);
            if (!rc) rc = pedp_upload(c, d_t, tris, 4 * E);
            if (!rc && hipMemsetAsync(m->store + m->state_off, 0, m->state_bytes, c->stream) != hipSuccess) rc = PEDP_ERR_HIP;
            if (!rc) {
                hipLaunchKernelGGL(face_geometry_kernel, dim3(blocks_for(F)), dim3(DT), 0, c->stream, d_v, d_t, F, m->area, m->cen, m->box);
                rc = topology::weld(c, d_v, V, d_s, d_w);
                if (!rc) rc = build_adjacency(m, d_t, d_w);
            }
            if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) {
                pedp_set_error("%s: the build failed on the device", who);
                rc = PEDP_ERR_HIP;
            }
        }
    }
    if (rc) {
        pedp_defect_map_destroy(m);
        *out = nullptr;
    }
    return rc;
}

int pedp_defect_map_destroy(pedp_defect_map_t m) {
    if (!m) return PEDP_OK;
    if (hipSetDevice(m->device) == hipSuccess) {
        if (m->store) (void)hipFree(m->store);  // waits for the device: nothing enqueued still uses it
        m->ws.release();
        m->io.release();
    }
    delete m;
    return PEDP_OK;
}

int pedp_defect_map_size(pedp_defect_map_t m, int64_t *V, int64_t *F) {
    PEDP_REQUIRE(m, "pedp_defect_map_size: null map");
    if (V) *V = m->V;
    if (F) *F = m->F;
    return PEDP_OK;
}

int pedp_defect_map_add(pedp_defect_map_t m, const uint32_t *prim_id, const double *intensity, int64_t n, int mem) {
    const char *who = "pedp_defect_map_add";
    PEDP_REQUIRE(m, "%s: null map", who);
    pedp_ctx_t c = m->ctx;
    PEDP_REQUIRE(mem == PEDP_HOST || mem == PEDP_DEVICE, "%s: bad mem flag %d", who, mem);
    PEDP_REQUIRE(n >= 0 && n < MAX_ROWS, "%s: n = %lld", who, (long long)n);
    PEDP_REQUIRE(n == 0 || (prim_id && intensity), "%s: null array", who);
    PEDP_REQUIRE(mem == PEDP_DEVICE || !c->icp_pending, "%s: a registration is pending on this context (host-memory call)", who);
    PEDP_REQUIRE(m->observations < 0xFFFFFFFEll, "%s: 2^32 - 2 observations since the last clear", who);
    m->observations += 1;
    if (n == 0) return PEDP_OK;
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    if (m->F == 0) {  // a map without faces ignores every row: counted on the host
        m->ignored_host += n;
        return PEDP_OK;
    }
    const uint32_t *d_id = prim_id;
    const double *d_x = intensity;
    if (mem == PEDP_HOST) {
        int rc = m->io.reserve(a256(4 * (size_t)n) + a256(8 * (size_t)n));
        if (rc) return rc;
        char *io = (char *)m->io.ptr;
        rc = pedp_upload(c, io, prim_id, 4 * (size_t)n);
        if (!rc) rc = pedp_upload(c, io + a256(4 * (size_t)n), intensity, 8 * (size_t)n);
        if (rc) return rc;
        d_id = (const uint32_t *)io;
        d_x = (const double *)(io + a256(4 * (size_t)n));
    }
    hipLaunchKernelGGL(add_kernel, dim3(blocks_for(n)), dim3(DT), 0, c->stream, d_id, d_x, n, m->F, (uint32_t)m->observations, m->peak,
                       m->hits, m->frames, m->stamp, m->counters);
    PEDP_HIP_CHECK(hipGetLastError());
    if (mem == PEDP_HOST) PEDP_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PEDP_OK;
}

int pedp_defect_map_clear(pedp_defect_map_t m) {
    PEDP_REQUIRE(m, "pedp_defect_map_clear: null map");
    m->observations = 0;
    m->ignored_host = 0;
    if (m->F == 0) return PEDP_OK;
    PEDP_HIP_CHECK(hipSetDevice(m->device));
    PEDP_HIP_CHECK(hipMemsetAsync(m->store + m->state_off, 0, m->state_bytes, m->ctx->stream));
    return PEDP_OK;
}

int pedp_defect_map_faces(pedp_defect_map_t m, int mem, double *peak, int64_t *hits, int32_t *frames) {
    const char *who = "pedp_defect_map_faces";
    PEDP_REQUIRE(m, "%s: null map", who);
    pedp_ctx_t c = m->ctx;
    PEDP_REQUIRE(mem == PEDP_HOST || mem == PEDP_DEVICE, "%s: bad mem flag %d", who, mem);
    PEDP_REQUIRE(mem == PEDP_DEVICE || !c->icp_pending, "%s: a registration is pending on this context (host-memory call)", who);
    if (m->F == 0 || (!peak && !hits && !frames)) return PEDP_OK;
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    const size_t f = (size_t)m->F;
    double *d_peak = peak;
    int64_t *d_hits = hits;
    int32_t *d_frames = frames;
    if (mem == PEDP_HOST) {
        const int rc = m->io.reserve(2 * a256(8 * f) + a256(4 * f));
        if (rc) return rc;
        char *io = (char *)m->io.ptr;
        d_peak = peak ? (double *)io : nullptr;
        d_hits = hits ? (int64_t *)(io + a256(8 * f)) : nullptr;
        d_frames = frames ? (int32_t *)(io + 2 * a256(8 * f)) : nullptr;
    }
    hipLaunchKernelGGL(faces_kernel, dim3(blocks_for(m->F)), dim3(DT), 0, c->stream, m->peak, m->hits, m->frames, m->F, d_peak, d_hits,
                       d_frames);
    PEDP_HIP_CHECK(hipGetLastError());
    int rc = PEDP_OK;
    if (mem == PEDP_HOST) {
        if (peak) rc = pedp_download(c, peak, d_peak, 8 * f);
        if (!rc && hits) rc = pedp_download(c, hits, d_hits, 8 * f);
        if (!rc && frames) rc = pedp_download(c, frames, d_frames, 4 * f);
    }
    return rc;
}

int pedp_defect_map_stats(pedp_defect_map_t m, int64_t *observations, int64_t *rows_added, int64_t *rows_ignored) {
    const char *who = "pedp_defect_map_stats";
    PEDP_REQUIRE(m, "%s: null map", who);
    pedp_ctx_t c = m->ctx;
    if (observations) *observations = m->observations;
    if (!rows_added && !rows_ignored) return PEDP_OK;
    unsigned long long v[2] = {0, 0};
    if (m->F == 0) v[1] = (unsigned long long)m->ignored_host;
    else {
        PEDP_REQUIRE(!c->icp_pending, "%s: a registration is pending on this context (the call waits for the stream)", who);
        PEDP_HIP_CHECK(hipSetDevice(c->device));
        const int rc = pedp_download(c, v, m->counters, sizeof(v));
        if (rc) return rc;
    }
    if (rows_added) *rows_added = (int64_t)v[0];
    if (rows_ignored) *rows_ignored = (int64_t)v[1];
    return PEDP_OK;
}

int pedp_defect_map_regions(pedp_defect_map_t m, double threshold, int32_t min_frames, int32_t grow, int mem, int32_t *labels,
                            int64_t capacity, pedp_defect_region *table, int64_t *n_regions) {
    const char *who = "pedp_defect_map_regions";
    pedp_region_ws w;
    const int rc = pedp_defect_regions_begin(m, who, grow, mem, capacity, table, n_regions, w);
    if (rc || !w.seed) return rc;
    hipLaunchKernelGGL(seed_kernel, dim3(blocks_for(m->F)), dim3(DT), 0, m->ctx->stream, m->peak, m->hits, m->frames, m->F, threshold,
                       min_frames, w.seed, w.mark[0]);
    const pedp_region_columns col{m->peak, m->hits, m->frames};
    return pedp_defect_regions_finish(m, who, w, col, grow, mem, labels, capacity, table, n_regions);
}

}  // extern "C"

int pedp_defect_regions_begin(pedp_defect_map_s *m, const char *who, int32_t grow, int mem, int64_t capacity, const pedp_defect_region *table,
                              int64_t *n_regions, pedp_region_ws &w) {
    PEDP_REQUIRE(m && n_regions, "%s: null map / n_regions", who);
    pedp_ctx_t c = m->ctx;
    PEDP_REQUIRE(mem == PEDP_HOST || mem == PEDP_DEVICE, "%s: bad mem flag %d", who, mem);
    PEDP_REQUIRE(grow >= 0 && grow <= MAX_GROW, "%s: grow = %d, 0 ... %d", who, grow, MAX_GROW);
    PEDP_REQUIRE(capacity >= 0 && (table || capacity == 0), "%s: capacity %lld with %s table", who, (long long)capacity,
                 table ? "a" : "no");
    PEDP_REQUIRE(!c->icp_pending, "%s: a registration is pending on this context (the call waits for the stream)", who);
    *n_regions = 0;
    w.seed = nullptr;
    if (m->F == 0) return PEDP_OK;
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    return region_ws(m, w);
}

int pedp_defect_regions_finish(pedp_defect_map_s *m, const char *who, const pedp_region_ws &w, const pedp_region_columns &col, int32_t grow,
                               int mem, int32_t *labels, int64_t capacity, pedp_defect_region *table, int64_t *n_regions) {
    pedp_ctx_t c = m->ctx;
    const int64_t F = m->F, E = 3 * F;
    int rc = PEDP_OK;
    size_t tmp_bytes = w.tmp_bytes;  // rocprim takes it by reference
    hipStream_t s = c->stream;
    const dim3 gF(blocks_for(F)), gE(blocks_for(E)), bt(DT);
    int cur = 0;
    for (int round = 0; round <= grow; ++round) {  // the last fill of run_first serves the union
        PEDP_HIP_CHECK(hipMemsetAsync(w.run_first, 0xFF, 4 * (size_t)E, s));
        hipLaunchKernelGGL(run_first_kernel, gE, bt, 0, s, m->pos_face, m->pos_run, E, w.mark[cur], w.run_first);
        if (round == grow) break;
        hipLaunchKernelGGL(grow_kernel, gF, bt, 0, s, m->face_run, w.run_first, F, w.mark[cur], w.mark[cur ^ 1]);
        cur ^= 1;
    }
    const uint8_t *mark = w.mark[cur];
    hipLaunchKernelGGL(parent_init_kernel, gF, bt, 0, s, mark, F, w.parent);
    hipLaunchKernelGGL(union_kernel, gE, bt, 0, s, m->pos_face, m->pos_run, E, mark, w.run_first, w.parent);
    hipLaunchKernelGGL(root_kernel, dim3(blocks_for(F + 1)), bt, 0, s, mark, F, w.parent, w.root, w.is_root);
    PEDP_ROCPRIM(rocprim::exclusive_scan(w.tmp, tmp_bytes, w.is_root, w.rank, 0u, (size_t)F + 1, rocprim::plus<uint32_t>(), s));
    int32_t *d_labels = mem == PEDP_DEVICE ? labels : nullptr;
    hipLaunchKernelGGL(label_kernel, gF, bt, 0, s, w.root, w.rank, F, w.label, d_labels);
    PEDP_HIP_CHECK(hipGetLastError());
    uint32_t R32 = 0;
    rc = pedp_download(c, &R32, w.rank + F, sizeof(R32));
    if (rc) return rc;
    const int64_t R = R32;
    *n_regions = R;
    if (labels && mem == PEDP_HOST) {
        rc = pedp_download(c, labels, w.label, 4 * (size_t)F);
        if (rc) return rc;
    }
    PEDP_REQUIRE(R <= capacity || !table, "%s: %lld regions, room for %lld", who, (long long)R, (long long)capacity);
    if (!table || R == 0) return PEDP_OK;
    // the faces by (label, face): a stable sort of the face order on the label
    unsigned long long *keys = nullptr;
    rc = pedp_sort_keys64_exact_begin(c, F, 32, &keys);
    if (rc) return rc;
    hipLaunchKernelGGL(label_key_kernel, gF, bt, 0, s, w.label, F, keys);
    rc = pedp_sort_keys64_exact_run(c, F, 32, w.order);
    if (rc) return rc;
    hipLaunchKernelGGL(region_range_kernel, gF, bt, 0, s, w.label, w.order, F, w.begin, w.end);
    hipLaunchKernelGGL(region_blocks_kernel, dim3(blocks_for(R + 1)), bt, 0, s, w.begin, w.end, R, w.n_blocks);
    PEDP_ROCPRIM(rocprim::exclusive_scan(w.tmp, tmp_bytes, w.n_blocks, w.block_off, 0u, (size_t)R + 1, rocprim::plus<uint32_t>(), s));
    SumArgs a;
    a.order = w.order; a.begin = w.begin; a.end = w.end; a.block_off = w.block_off; a.R = R;
    a.area = m->area; a.cen = m->cen; a.box = m->box; a.peak_key = col.peak_key; a.hits = col.hits; a.frames = col.frames; a.seed = w.seed;
    const int64_t blocks_max = F / SUM_BLOCK + R;  // every region has at most one block that is not full
    // the block sums and a host-memory call's table, sized by R: in the staging scratch
    rc = m->io.reserve(a256(sizeof(Part) * (size_t)blocks_max) + a256(sizeof(pedp_defect_region) * (size_t)R));
    if (rc) return rc;
    a.part = (Part *)m->io.ptr;
    pedp_defect_region *ws_table = (pedp_defect_region *)((char *)m->io.ptr + a256(sizeof(Part) * (size_t)blocks_max));
    hipLaunchKernelGGL(region_block_sum_kernel, dim3((unsigned)((blocks_max + SUM_WPB - 1) / SUM_WPB)), bt, 0, s, a);
    pedp_defect_region *d_table = mem == PEDP_DEVICE ? table : ws_table;
    hipLaunchKernelGGL(region_row_kernel, dim3((unsigned)((R + SUM_WPB - 1) / SUM_WPB)), bt, 0, s, a, d_table);
    PEDP_HIP_CHECK(hipGetLastError());
    if (mem == PEDP_HOST) return pedp_download(c, table, d_table, sizeof(pedp_defect_region) * (size_t)R);
    PEDP_HIP_CHECK(hipStreamSynchronize(s));
    return PEDP_OK;
}
