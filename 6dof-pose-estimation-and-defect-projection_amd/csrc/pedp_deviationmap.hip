// The deviation map: per-face statistics of the signed deviation of the measured surface from the CAD
// solid, over every frame the camera took.
//   * per ROW (one depth point): the face the closest-point search found and the signed distance d, quantised to
//     q = rint(d 2^20); rows with a bad id or a NaN are ignored, rows beyond the call's gate are gated.
//   * per FACE, laid over the faces of a defect map: the count n, the sums S1 = sum q and S2 = sum q^2 (exact: two
//     64-bit words), the extremes of q and the frames.  Integer atomics only, as in pedp_defectmap.hip: sums are exact
//     and associative, the extremes go through a biased unsigned key, so the state is a function of the rows alone.
//   * read out: mean, standard deviation (from the exact integer n S2 - S1^2), marking by mean, sign and significance,
//     regions through the defect map's body with the volume of excess or missing material, and the totals.
// The areas, the adjacency and the regions' body are the defect map's (defectmap/shared.h); the sign of a point is the
// signed query's routine (solid/shared.h), so a frame's points go into the map with one search.
#include "defectmap/shared.h"
#include "solid/shared.h"
#include <cmath>
#include <cstdlib>

namespace {

using namespace defectmap;

typedef unsigned __int128 u128;

constexpr int64_t MAX_ROWS = (int64_t)1 << 31;
constexpr int SUM_BLOCK = 4096;  // faces one wave sums (64 per lane): pedp_defectmap.hip's block
constexpr int SUM_WPB = DT / 64;
constexpr int COUNTER_SLOTS = 64;  // copies of the row counters: a block adds to copy blockIdx % 64
enum : int { TAKEN = 0, IGNORED = 1, GATED = 2, BACKFACING = 3, N_KINDS = 4 };
constexpr double Q_SCALE = 1048576.0;            // 2^20
constexpr double Q_UNIT = 1.0 / 1048576.0;       // 2^-20
constexpr double Q_UNIT2 = Q_UNIT * Q_UNIT;      // 2^-40
constexpr double MAX_GATE = 1024.0;
constexpr unsigned long long BIAS = 1ull << 63;  // q ^ BIAS: an unsigned key in the order of q
constexpr unsigned long long NEVER = ~0ull;      // qmin's key of a face without rows (qmax's: 0)
static_assert(solid::ST == DT, "one block size serves the fused kernel");

struct State {
    unsigned long long *n, *s1, *s2lo, *s2hi, *qmin, *qmax, *counters;
    int32_t *frames;
    uint32_t *stamp;
};

// ------------------------------------------------------------------ accumulating
__device__ __forceinline__ int row_kind(uint32_t f, double d, int64_t F, double gate) {
    if ((int64_t)f >= F || is_nan_bits(bits_of(d))) return IGNORED;
    return fabs(d) <= gate ? TAKEN : GATED;
}

// One row per lane, every lane of the block (kind -1: beyond the rows).  Depth pixels arrive in row-major order, so
// whole waves fall on one face: a run of equal ids in neighbouring lanes (defectmap/shared.h) sends its count, its three
// sums and its extremes through its first lane alone.  Integer sums are exact and associative: `combine` changes no bit.
__device__ __forceinline__ void accumulate(const State &s, uint32_t f, double d, int kind, uint32_t obs, int combine, unsigned *block_count) {
    const int lane = threadIdx.x & 63;
    if (threadIdx.x < N_KINDS) block_count[threadIdx.x] = 0;
    __syncthreads();
    const bool taken = kind == TAKEN;
    unsigned long long cnt = 1, s1 = 0, lo = 0, hi = 0, kmin = NEVER, kmax = 0;
    if (taken) {
        const long long q = (long long)__builtin_rint(d * Q_SCALE);  // |q| <= 2^30: q q < 2^61
        const unsigned long long qq = (unsigned long long)(q * q);
        s1 = (unsigned long long)q;
        lo = qq & 0xFFFFFFFFull;
        hi = qq >> 32;
        kmin = kmax = (unsigned long long)q ^ BIAS;
    }
    bool head = taken;
    if (combine) {  // uniform over the launch
        const LaneRun run = lane_run(taken ? f : NONE, lane);
        if (run.wide) {
            cnt = (unsigned long long)(run.end - lane + 1);
            s1 = run_sum(s1, lane, run.end);
            lo = run_sum(lo, lane, run.end);
            hi = run_sum(hi, lane, run.end);
            kmin = run_min(kmin, lane, run.end);
            kmax = run_max(kmax, lane, run.end);
        }
        head = run.head;
    }
    if (head) {
        atomicAdd(&s.n[f], cnt);
        atomicAdd(&s.s1[f], s1);
        atomicAdd(&s.s2lo[f], lo);
        atomicAdd(&s.s2hi[f], hi);
        atomicMin(&s.qmin[f], kmin);
        atomicMax(&s.qmax[f], kmax);
        if (atomicMax(&s.stamp[f], obs) < obs) atomicAdd(&s.frames[f], 1);
    }
    // the row counters as the coverage map keeps its classes: a wave's counts meet in LDS, the block adds each once
#pragma unroll
    for (int k = 0; k < N_KINDS; ++k) {
        const int c = __builtin_popcountll(__builtin_amdgcn_ballot_w64(kind == k));
        if (lane == 0 && c) atomicAdd(&block_count[k], (unsigned)c);
    }
    __syncthreads();
    if (threadIdx.x < N_KINDS && block_count[threadIdx.x])
        atomicAdd(&s.counters[(blockIdx.x % COUNTER_SLOTS) * N_KINDS + threadIdx.x], (unsigned long long)block_count[threadIdx.x]);
}

__global__ __launch_bounds__(DT) void deviation_add_kernel(State s, const uint32_t *__restrict__ id, const double *__restrict__ d, int64_t n,
                                                          int64_t F, double gate, uint32_t obs, int combine) {
    __shared__ unsigned block_count[N_KINDS];
    const int64_t i = (int64_t)blockIdx.x * DT + threadIdx.x;
    int kind = -1;
    uint32_t f = NONE;
    double x = 0.0;
    if (i < n) {
        f = id[i];
        x = d[i];
        kind = row_kind(f, x, F, gate);
    }
    accumulate(s, f, x, kind, obs, combine, block_count);
}

struct PointArgs {
    solid::SignArgs sign;
    const double *pts, *closest, *dist;
    const uint32_t *prim;
    const uint8_t *region;
    int64_t n, F;
    double gate, origin[3];
    int has_origin, combine;
    uint32_t obs;
};
// a frame's points: the sign of every point against its closest feature (the signed query's routine), the test against
// the camera centre, and the row into the state without leaving the registers
__global__ __launch_bounds__(DT) void deviation_points_kernel(State s, PointArgs a) {
    __shared__ unsigned block_count[N_KINDS];
    const int64_t i = (int64_t)blockIdx.x * DT + threadIdx.x;
    int kind = -1;
    uint32_t f = NONE;
    double sd = 0.0;
    if (i < a.n) {
        f = a.prim[i];
        sd = a.dist[i];
        double N[3];
        const double p[3] = {a.pts[3 * i], a.pts[3 * i + 1], a.pts[3 * i + 2]};
        const double c[3] = {a.closest[3 * i], a.closest[3 * i + 1], a.closest[3 * i + 2]};
        const int feature = solid::sign_of_point(a.sign, f, a.region[i], p, c, sd, N);
        kind = row_kind(f, sd, a.F, a.gate);
        if (kind != IGNORED && a.has_origin && feature != solid::FEATURE_NONE) {
            const double r[3] = {a.origin[0] - c[0], a.origin[1] - c[1], a.origin[2] - c[2]};
            if (!(record::dot3(r, N) * a.sign.orientation > 0.0)) kind = BACKFACING;
        }
    }
    accumulate(s, f, sd, kind, a.obs, a.combine, block_count);
}

// ------------------------------------------------------------------ reading
// The double nearest to x, ties to even: the leading 64 bits, a sticky bit for what lies below them, one rounding.
__device__ __forceinline__ double double_of_u128(u128 x) {
    const uint64_t hi = (uint64_t)(x >> 64), lo = (uint64_t)x;
    if (hi == 0) return (double)lo;
    const int shift = 64 - __builtin_clzll(hi);  // 1 ... 64 bits lie below the leading 64
    uint64_t top = shift == 64 ? hi : (hi << (64 - shift)) | (lo >> shift);
    const uint64_t below = shift == 64 ? lo : lo & ((1ull << shift) - 1);
    top |= below != 0;  // bit 0 of 64 lies below the 53 that stay: it only breaks a tie
    return ldexp((double)top, shift);
}
__device__ __forceinline__ u128 mul_64x64(uint64_t a, uint64_t b) { return ((u128)__umul64hi(a, b) << 64) | (u128)(a * b); }

struct Face {
    unsigned long long n;
    long long s1;
    uint64_t s2_hi, s2_lo;
    double mean, sd;  // NaN without rows
};
__device__ __forceinline__ Face face_of(const State &s, int64_t f) {
    Face v;
    v.n = s.n[f];
    v.s1 = (long long)s.s1[f];
    const u128 s2 = ((u128)s.s2hi[f] << 32) + (u128)s.s2lo[f];
    v.s2_hi = (uint64_t)(s2 >> 64);
    v.s2_lo = (uint64_t)s2;
    v.mean = v.sd = record::quiet_nan();
    if (v.n == 0) return v;
    v.mean = ((double)v.s1 / (double)v.n) * Q_UNIT;
    if (v.n < (1ull << 33)) {  // n S2 < 2^126, S1^2 < 2^126
        const uint64_t a = v.s1 < 0 ? (uint64_t)0 - (uint64_t)v.s1 : (uint64_t)v.s1;
        const u128 ns2 = mul_64x64(v.n, v.s2_lo) + ((u128)(v.n * v.s2_hi) << 64);
        const u128 num = ns2 - mul_64x64(a, a);  // n^2 times the variance of q: never negative
        const double var = (double_of_u128(num) / ((double)v.n * (double)v.n)) * Q_UNIT2;
        v.sd = sqrt(var);
    }
    return v;
}
__device__ __forceinline__ bool is_marked(const Face &v, int32_t frames, const pedp_deviation_criteria &c) {
    if ((long long)v.n < c.min_samples || frames < c.min_frames) return false;
    const bool far = c.sign == 0 ? fabs(v.mean) > c.threshold : (c.sign > 0 ? v.mean > c.threshold : v.mean < -c.threshold);
    if (!far) return false;  // a face without rows: its NaN mean fails every test
    if (c.z > 0.0) return fabs(v.mean) * sqrt((double)v.n) > c.z * v.sd;
    return true;
}
__device__ __forceinline__ bool is_measured(const Face &v, const pedp_deviation_criteria &c) {
    return v.n > 0 && (long long)v.n >= c.min_samples;
}

struct FaceOut {
    int64_t *n, *s1;
    int32_t *frames;
    uint64_t *s2_hi, *s2_lo;
    double *min, *max, *mean, *sd;
};
__global__ __launch_bounds__(DT) void deviation_faces_kernel(State s, int64_t F, FaceOut o) {
    const int64_t f = (int64_t)blockIdx.x * DT + threadIdx.x;
    if (f >= F) return;
    const Face v = face_of(s, f);
    if (o.n) o.n[f] = (int64_t)v.n;
    if (o.frames) o.frames[f] = s.frames[f];
    if (o.s1) o.s1[f] = v.s1;
    if (o.s2_hi) o.s2_hi[f] = v.s2_hi;
    if (o.s2_lo) o.s2_lo[f] = v.s2_lo;
    if (o.min) o.min[f] = v.n ? (double)(long long)(s.qmin[f] ^ BIAS) * Q_UNIT : record::quiet_nan();
    if (o.max) o.max[f] = v.n ? (double)(long long)(s.qmax[f] ^ BIAS) * Q_UNIT : record::quiet_nan();
    if (o.mean) o.mean[f] = v.mean;
    if (o.sd) o.sd[f] = v.sd;
}

// the marking of a regions call, and the two columns the rows need: the key of |mean| (the body's peak) and the mean
__global__ __launch_bounds__(DT) void deviation_seed_kernel(State s, pedp_deviation_criteria c, int64_t F, uint8_t *__restrict__ seed,
                                                           uint8_t *__restrict__ mark, unsigned long long *__restrict__ abs_key,
                                                           double *__restrict__ mean) {
    const int64_t f = (int64_t)blockIdx.x * DT + threadIdx.x;
    if (f >= F) return;
    const Face v = face_of(s, f);
    const uint8_t m = is_marked(v, s.frames[f], c);
    seed[f] = m;
    mark[f] = m;
    abs_key[f] = v.n ? key_of(fabs(v.mean)) : 0;
    mean[f] = v.mean;
}

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
__device__ __forceinline__ uint64_t butterfly_max(uint64_t a) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint64_t b = shfl_xor_u64(a, off);
        a = b > a ? b : a;
    }
    return a;
}
__device__ __forceinline__ uint64_t butterfly_min(uint64_t a) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint64_t b = shfl_xor_u64(a, off);
        a = b < a ? b : a;
    }
    return a;
}

// ---- a region's measured area and volume, in the order in which the body sums `area` (s4.17): a wave per block of
// SUM_BLOCK positions of the region's run of the sorted faces, lane l adds positions l, l + 64, ... one after the other,
// the butterfly adds the lanes; then a wave per region adds the block sums l, l + 64, ... the same way.
struct VolumePart {
    double area, volume;
    uint64_t lo, hi;  // keys of the smallest and the largest mean
};
struct VolumeArgs {
    const int32_t *order, *begin, *end;
    const uint32_t *block_off;
    int64_t R;
    const double *area, *mean;
    const unsigned long long *n;
    VolumePart *part;
};
__global__ __launch_bounds__(DT) void deviation_volume_block_kernel(VolumeArgs a) {
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
    VolumePart s{0.0, 0.0, KEY_PINF, KEY_NINF};
    for (int64_t p = p0 + lane; p < p1; p += 64) {
        const size_t f = (size_t)a.order[p];
        if (a.n[f] == 0) continue;
        const double ar = a.area[f], m = a.mean[f];
        s.area = s.area + ar;
        s.volume = s.volume + ar * m;
        const uint64_t k = key_of(m);
        s.lo = k < s.lo ? k : s.lo;
        s.hi = k > s.hi ? k : s.hi;
    }
    s.area = butterfly_sum(s.area);
    s.volume = butterfly_sum(s.volume);
    s.lo = butterfly_min(s.lo);
    s.hi = butterfly_max(s.hi);
    if (lane == 0) a.part[w] = s;
}
__global__ __launch_bounds__(DT) void deviation_volume_row_kernel(VolumeArgs a, const pedp_defect_region *__restrict__ body,
                                                                 pedp_deviation_region *__restrict__ table) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * SUM_WPB + (threadIdx.x >> 6);
    if (r >= a.R) return;  // wave-uniform
    VolumePart s{0.0, 0.0, KEY_PINF, KEY_NINF};
    for (int64_t b = (int64_t)a.block_off[r] + lane; b < (int64_t)a.block_off[r + 1]; b += 64) {
        const VolumePart q = a.part[b];
        s.area = s.area + q.area;
        s.volume = s.volume + q.volume;
        s.lo = q.lo < s.lo ? q.lo : s.lo;
        s.hi = q.hi > s.hi ? q.hi : s.hi;
    }
    s.area = butterfly_sum(s.area);
    s.volume = butterfly_sum(s.volume);
    s.lo = butterfly_min(s.lo);
    s.hi = butterfly_max(s.hi);
    if (lane != 0) return;
    pedp_deviation_region row;
    row.region = body[r];
    const bool any = s.hi >= s.lo;  // some face of the region has rows
    row.measured_area = s.area;
    row.volume = s.volume;
    row.mean = any ? s.volume / s.area : record::quiet_nan();
    row.min_mean = any ? value_of(s.lo) : record::quiet_nan();
    row.max_mean = any ? value_of(s.hi) : record::quiet_nan();
    table[r] = row;
}

// ---- the totals, in the order of pedp_coverage_summary's sums: a wave per block of SUM_BLOCK consecutive faces, then
// one wave over the block sums
struct Sums {
    double total_area, measured_area, marked_area, s1, s2;  // s1, s2: sum of area mean, of area mean^2
    int64_t measured, marked, max_face;
    uint64_t max_key;  // key of the largest |mean|; 0: no measured face
};
__device__ __forceinline__ void sums_init(Sums &a) {
    a.total_area = a.measured_area = a.marked_area = a.s1 = a.s2 = 0.0;
    a.measured = a.marked = 0;
    a.max_face = -1;
    a.max_key = 0;
}
__device__ __forceinline__ void sums_peak(Sums &a, uint64_t key, int64_t face) {  // the larger key, then the lower face
    if (key > a.max_key || (key == a.max_key && key && face < a.max_face)) { a.max_key = key; a.max_face = face; }
}
__device__ __forceinline__ void sums_butterfly(Sums &a) {
    a.total_area = butterfly_sum(a.total_area);
    a.measured_area = butterfly_sum(a.measured_area);
    a.marked_area = butterfly_sum(a.marked_area);
    a.s1 = butterfly_sum(a.s1);
    a.s2 = butterfly_sum(a.s2);
    a.measured = butterfly_sum(a.measured);
    a.marked = butterfly_sum(a.marked);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint64_t k = shfl_xor_u64(a.max_key, off);
        const int64_t f = (int64_t)shfl_xor_u64((uint64_t)a.max_face, off);
        sums_peak(a, k, f);
    }
}
__global__ __launch_bounds__(DT) void deviation_summary_block_kernel(State s, pedp_deviation_criteria c, const double *__restrict__ area,
                                                                    int64_t F, int64_t n_blocks, Sums *__restrict__ part) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * SUM_WPB + (threadIdx.x >> 6);
    if (w >= n_blocks) return;  // wave-uniform
    const int64_t f0 = w * SUM_BLOCK, f1 = f0 + SUM_BLOCK < F ? f0 + SUM_BLOCK : F;
    Sums a;
    sums_init(a);
    for (int64_t f = f0 + lane; f < f1; f += 64) {
        const double ar = area[f];
        a.total_area = a.total_area + ar;
        const Face v = face_of(s, f);
        if (is_measured(v, c)) {
            a.measured_area = a.measured_area + ar;
            a.s1 = a.s1 + ar * v.mean;
            a.s2 = a.s2 + ar * (v.mean * v.mean);
            a.measured += 1;
            sums_peak(a, key_of(fabs(v.mean)), f);
        }
        if (is_marked(v, s.frames[f], c)) {
            a.marked_area = a.marked_area + ar;
            a.marked += 1;
        }
    }
    sums_butterfly(a);
    if (lane == 0) part[w] = a;
}
__global__ __launch_bounds__(64) void deviation_summary_total_kernel(const Sums *__restrict__ part, int64_t n_blocks, Sums *__restrict__ out) {
    const int lane = threadIdx.x;
    Sums a;
    sums_init(a);
    for (int64_t b = lane; b < n_blocks; b += 64) {
        const Sums q = part[b];
        a.total_area = a.total_area + q.total_area;
        a.measured_area = a.measured_area + q.measured_area;
        a.marked_area = a.marked_area + q.marked_area;
        a.s1 = a.s1 + q.s1;
        a.s2 = a.s2 + q.s2;
        a.measured += q.measured;
        a.marked += q.marked;
        sums_peak(a, q.max_key, q.max_face);
    }
    sums_butterfly(a);
    if (lane == 0) *out = a;
}

const pedp_deviation_criteria DEFAULT_CRITERIA = {0.0, 0.0, 1, 1, 0};

// the switch of the in-wave combine, read once per process: PEDP_DEVIATION_COMBINE=0 sends every row to the atomics
// itself (the A/B of profiles/deviation_map_time.json); the state is the same either way
int combine_switch() {
    static const int on = getenv("PEDP_DEVIATION_COMBINE") ? atoi(getenv("PEDP_DEVIATION_COMBINE")) != 0 : 1;
    return on;
}

}  // namespace

struct pedp_deviation_map_s {
    pedp_defect_map_s *map = nullptr;  // borrowed: it must outlive this handle
    pedp_ctx_t ctx = nullptr;
    int device = 0;
    int64_t F = 0;
    char *store = nullptr;  // one allocation: everything below
    State st = {};
    unsigned long long *abs_key = nullptr;  // F: a regions call's column of |mean| keys
    double *mean = nullptr;                 // F: a regions call's means
    size_t zero_bytes = 0, ones_off = 0, ones_bytes = 0;  // what clear sets to 0 and to all ones (qmin)
    int64_t observations = 0;
    int64_t ignored_host = 0;  // F = 0: the ignored rows (there are no device counters)
    pedp_scratch ws;  // add_points: the vertex table and the search's outputs
    pedp_scratch io;  // staging of host-memory calls; the summary's block sums; a regions call's rows
};

namespace {

int clear_state(pedp_deviation_map_s *v) {
    if (!v->store) return PEDP_OK;
    PEDP_HIP_CHECK(hipMemsetAsync(v->store, 0, v->zero_bytes, v->ctx->stream));
    PEDP_HIP_CHECK(hipMemsetAsync(v->store + v->ones_off, 0xFF, v->ones_bytes, v->ctx->stream));
    return PEDP_OK;
}

int check_criteria(const char *who, const pedp_deviation_criteria &k) {
    PEDP_REQUIRE(k.sign >= -1 && k.sign <= 1, "%s: sign = %d, one of -1, 0, +1", who, k.sign);
    PEDP_REQUIRE(k.threshold == k.threshold && k.z == k.z, "%s: threshold = %g, z = %g (NaN)", who, k.threshold, k.z);
    return PEDP_OK;
}

// what every observation checks before it is counted
int check_observation(const char *who, pedp_deviation_map_s *v, double gate) {
    PEDP_REQUIRE(gate >= 0.0 && gate <= MAX_GATE, "%s: gate = %g, 0 ... %g", who, gate, MAX_GATE);
    PEDP_REQUIRE(v->observations < 0xFFFFFFFEll, "%s: 2^32 - 2 observations since the last clear", who);
    return PEDP_OK;
}

}  // namespace

extern "C" {

int pedp_deviation_map_create(pedp_defect_map_t map, pedp_deviation_map_t *out) {
    const char *who = "pedp_deviation_map_create";
    PEDP_REQUIRE(map && out, "%s: null map/out", who);
    pedp_ctx_t c = map->ctx;
    PEDP_REQUIRE(!c->icp_pending, "%s: a registration is pending on this context (the call allocates device memory)", who);
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    pedp_deviation_map_s *v = new pedp_deviation_map_s;
    v->map = map;
    v->ctx = c;
    v->device = c->device;
    v->F = map->F;
    *out = v;
    if (v->F == 0) return PEDP_OK;
    const size_t f = (size_t)v->F;
    size_t off = 0;
    auto place = [&](size_t bytes) { const size_t o = off; off += a256(bytes); return o; };
    const size_t o_n = place(8 * f), o_s1 = place(8 * f), o_lo = place(8 * f), o_hi = place(8 * f), o_max = place(8 * f),
                 o_frames = place(4 * f), o_stamp = place(4 * f), o_cnt = place(8 * N_KINDS * COUNTER_SLOTS);
    v->zero_bytes = off;
    v->ones_off = place(8 * f);
    v->ones_bytes = off - v->ones_off;
    const size_t o_key = place(8 * f), o_mean = place(8 * f);
    hipError_t e = hipMalloc((void **)&v->store, off);
    if (e != hipSuccess) {
        pedp_set_error("%s: hipMalloc(%zu) -> %s", who, off, hipGetErrorString(e));
        delete v;
        *out = nullptr;
        return PEDP_ERR_HIP;
    }
    auto at = [&](size_t o) { return (unsigned long long *)(v->store + o); };
    v->st.n = at(o_n); v->st.s1 = at(o_s1); v->st.s2lo = at(o_lo); v->st.s2hi = at(o_hi); v->st.qmax = at(o_max);
    v->st.qmin = at(v->ones_off); v->st.counters = at(o_cnt);
    v->st.frames = (int32_t *)(v->store + o_frames); v->st.stamp = (uint32_t *)(v->store + o_stamp);
    v->abs_key = at(o_key); v->mean = (double *)(v->store + o_mean);
    const int rc = clear_state(v);  // enqueued: every later use is behind it on the context's stream
    if (rc) {
        pedp_deviation_map_destroy(v);
        *out = nullptr;
        return rc;
    }
    return PEDP_OK;
}

int pedp_deviation_map_destroy(pedp_deviation_map_t v) {
    if (!v) return PEDP_OK;
    if (hipSetDevice(v->device) == hipSuccess) {
        if (v->store) (void)hipFree(v->store);  // waits for the device: nothing enqueued still uses it
        v->ws.release();
        v->io.release();
    }
    delete v;
    return PEDP_OK;
}

int pedp_deviation_map_clear(pedp_deviation_map_t v) {
    PEDP_REQUIRE(v, "pedp_deviation_map_clear: null handle");
    v->observations = 0;
    v->ignored_host = 0;
    PEDP_HIP_CHECK(hipSetDevice(v->device));
    return clear_state(v);
}

int pedp_deviation_map_add(pedp_deviation_map_t v, const uint32_t *prim_id, const double *d, int64_t n, double gate, int mem) {
    const char *who = "pedp_deviation_map_add";
    PEDP_REQUIRE(v, "%s: null handle", who);
    pedp_ctx_t c = v->ctx;
    PEDP_REQUIRE(mem == PEDP_HOST || mem == PEDP_DEVICE, "%s: bad mem flag %d", who, mem);
    PEDP_REQUIRE(n >= 0 && n < MAX_ROWS, "%s: n = %lld", who, (long long)n);
    PEDP_REQUIRE(n == 0 || (prim_id && d), "%s: null array", who);
    PEDP_REQUIRE(mem == PEDP_DEVICE || !c->icp_pending, "%s: a registration is pending on this context (host-memory call)", who);
    int rc = check_observation(who, v, gate);
    if (rc) return rc;
    if (n == 0 || v->F == 0) {  // no rows, or a map without faces, which ignores every row: counted on the host
        v->observations += 1;
        v->ignored_host += v->F == 0 ? n : 0;
        return PEDP_OK;
    }
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    const uint32_t *d_id = prim_id;
    const double *d_x = d;
    if (mem == PEDP_HOST) {
        rc = v->io.reserve(a256(4 * (size_t)n) + a256(8 * (size_t)n));
        if (rc) return rc;
        char *io = (char *)v->io.ptr;
        rc = pedp_upload(c, io, prim_id, 4 * (size_t)n);
        if (!rc) rc = pedp_upload(c, io + a256(4 * (size_t)n), d, 8 * (size_t)n);
        if (rc) return rc;
        d_id = (const uint32_t *)io;
        d_x = (const double *)(io + a256(4 * (size_t)n));
    }
    hipLaunchKernelGGL(deviation_add_kernel, dim3(blocks_for(n)), dim3(DT), 0, c->stream, v->st, d_id, d_x, n, v->F, gate,
                       (uint32_t)(v->observations + 1), combine_switch());
    PEDP_HIP_CHECK(hipGetLastError());
    v->observations += 1;  // behind the launch's check: an observation that was not enqueued is not counted
    if (mem == PEDP_HOST) PEDP_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PEDP_OK;
}

int pedp_deviation_map_add_points(pedp_deviation_map_t v, pedp_mesh_t mesh, pedp_solid_t solid, const double *pts, int64_t N, int mem,
                                  double gate, const double *origin) {
    const char *who = "pedp_deviation_map_add_points";
    PEDP_REQUIRE(v, "%s: null handle", who);
    pedp_ctx_t c = v->ctx;
    int rc = solid::check_query(who, c, mesh, solid, N, mem);
    if (rc) return rc;
    PEDP_REQUIRE(mesh->F == v->F, "%s: the mesh has %lld faces, the map %lld", who, (long long)mesh->F, (long long)v->F);
    PEDP_REQUIRE(N == 0 || pts, "%s: null points", who);
    PEDP_REQUIRE(!origin || (std::isfinite(origin[0]) && std::isfinite(origin[1]) && std::isfinite(origin[2])),
                 "%s: the origin must be finite", who);
    rc = check_observation(who, v, gate);
    if (rc) return rc;
    if (N == 0 || v->F == 0) {
        v->observations += 1;
        v->ignored_host += v->F == 0 ? N : 0;
        return PEDP_OK;
    }
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    const pedp_solid_info &info = solid->info;
    const int64_t V = info.V;
    const size_t n = (size_t)N;
    // the vertex table, the search's outputs, the flag of the index comparison: the handle's own workspace
    const size_t o_table = 0, o_cl = o_table + a256(24 * (size_t)V), o_d = o_cl + a256(24 * n), o_id = o_d + a256(8 * n),
                 o_reg = o_id + a256(4 * n), o_flag = o_reg + a256(n), ws_bytes = o_flag + 256;
    rc = v->ws.reserve(ws_bytes);
    if (rc) return rc;
    char *ws = (char *)v->ws.ptr;
    rc = solid::verify_indices(who, c, mesh, solid, (uint32_t *)(ws + o_flag));
    if (rc) return rc;
    const double *d_pts = pts;
    if (mem == PEDP_HOST) {
        rc = v->io.reserve(a256(24 * n));
        if (rc) return rc;
        rc = pedp_upload(c, v->io.ptr, pts, 24 * n);
        if (rc) return rc;
        d_pts = (const double *)v->io.ptr;
    }
    PointArgs a;
    a.sign.rec = mesh->tri;
    a.sign.table = (double *)(ws + o_table);
    a.sign.wid = solid->wid; a.sign.twin = solid->twin;
    a.sign.orientation = info.orientation < 0 ? -1.0 : 1.0;
    a.pts = d_pts;
    a.closest = (double *)(ws + o_cl); a.dist = (double *)(ws + o_d); a.prim = (uint32_t *)(ws + o_id); a.region = (uint8_t *)(ws + o_reg);
    a.n = N; a.F = v->F;
    a.gate = gate;
    a.has_origin = origin != nullptr;
    for (int k = 0; k < 3; ++k) a.origin[k] = origin ? origin[k] : 0.0;
    a.combine = combine_switch();
    a.obs = (uint32_t)(v->observations + 1);
    rc = pedp_closest_launch(c, mesh, d_pts, N, (double *)a.closest, (double *)a.dist, (uint32_t *)a.prim, nullptr, nullptr,
                             (uint8_t *)a.region);
    if (rc) return rc;
    hipLaunchKernelGGL(solid::vertex_normal_kernel, dim3(solid::blocks_for(V)), dim3(solid::ST), 0, c->stream, mesh->tri, solid->vstart,
                       solid->vcount, solid->corner, V, (double *)a.sign.table);
    hipLaunchKernelGGL(deviation_points_kernel, dim3(blocks_for(N)), dim3(DT), 0, c->stream, v->st, a);
    PEDP_HIP_CHECK(hipGetLastError());
    v->observations += 1;  // behind the launches' check: an observation that was not enqueued is not counted
    if (mem == PEDP_HOST) PEDP_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PEDP_OK;
}

int pedp_deviation_map_faces(pedp_deviation_map_t v, int mem, int64_t *n, int32_t *frames, int64_t *s1, uint64_t *s2_hi, uint64_t *s2_lo,
                             double *min, double *max, double *mean, double *std) {
    const char *who = "pedp_deviation_map_faces";
    PEDP_REQUIRE(v, "%s: null handle", who);
    pedp_ctx_t c = v->ctx;
    PEDP_REQUIRE(mem == PEDP_HOST || mem == PEDP_DEVICE, "%s: bad mem flag %d", who, mem);
    PEDP_REQUIRE(mem == PEDP_DEVICE || !c->icp_pending, "%s: a registration is pending on this context (host-memory call)", who);
    void *const user[9] = {n, s1, s2_hi, s2_lo, min, max, mean, std, frames};  // eight 8-byte columns, then the 4-byte one
    bool any = false;
    for (int k = 0; k < 9; ++k) any = any || user[k];
    if (v->F == 0 || !any) return PEDP_OK;
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    const size_t f = (size_t)v->F, b8 = a256(8 * f);
    void *dev[9];
    for (int k = 0; k < 9; ++k) dev[k] = user[k];
    if (mem == PEDP_HOST) {
        const int rc = v->io.reserve(8 * b8 + a256(4 * f));
        if (rc) return rc;
        for (int k = 0; k < 9; ++k) dev[k] = user[k] ? (char *)v->io.ptr + k * b8 : nullptr;
    }
    const FaceOut o{(int64_t *)dev[0], (int64_t *)dev[1],  (int32_t *)dev[8], (uint64_t *)dev[2], (uint64_t *)dev[3],
                    (double *)dev[4],  (double *)dev[5],   (double *)dev[6],  (double *)dev[7]};
    hipLaunchKernelGGL(deviation_faces_kernel, dim3(blocks_for(v->F)), dim3(DT), 0, c->stream, v->st, v->F, o);
    PEDP_HIP_CHECK(hipGetLastError());
    int rc = PEDP_OK;
    if (mem == PEDP_HOST)
        for (int k = 0; k < 9 && !rc; ++k)
            if (user[k]) rc = pedp_download(c, user[k], dev[k], (k == 8 ? 4 : 8) * f);
    return rc;
}

int pedp_deviation_map_stats(pedp_deviation_map_t v, int64_t *observations, int64_t *rows_taken, int64_t *rows_ignored,
                             int64_t *rows_gated, int64_t *rows_backfacing) {
    const char *who = "pedp_deviation_map_stats";
    PEDP_REQUIRE(v, "%s: null handle", who);
    pedp_ctx_t c = v->ctx;
    if (observations) *observations = v->observations;
    if (!rows_taken && !rows_ignored && !rows_gated && !rows_backfacing) return PEDP_OK;
    int64_t kinds[N_KINDS] = {0, v->ignored_host, 0, 0};
    if (v->F > 0) {
        PEDP_REQUIRE(!c->icp_pending, "%s: a registration is pending on this context (the call waits for the stream)", who);
        PEDP_HIP_CHECK(hipSetDevice(c->device));
        unsigned long long cnt[COUNTER_SLOTS * N_KINDS];
        const int rc = pedp_download(c, cnt, v->st.counters, sizeof(cnt));
        if (rc) return rc;
        for (int slot = 0; slot < COUNTER_SLOTS; ++slot)
            for (int k = 0; k < N_KINDS; ++k) kinds[k] += (int64_t)cnt[slot * N_KINDS + k];
    }
    if (rows_taken) *rows_taken = kinds[TAKEN];
    if (rows_ignored) *rows_ignored = kinds[IGNORED];
    if (rows_gated) *rows_gated = kinds[GATED];
    if (rows_backfacing) *rows_backfacing = kinds[BACKFACING];
    return PEDP_OK;
}

int pedp_deviation_map_summary(pedp_deviation_map_t v, const pedp_deviation_criteria *crit, pedp_deviation_totals *out) {
    const char *who = "pedp_deviation_map_summary";
    PEDP_REQUIRE(v && out, "%s: null handle/out", who);
    pedp_ctx_t c = v->ctx;
    const pedp_deviation_criteria k = crit ? *crit : DEFAULT_CRITERIA;
    int rc = check_criteria(who, k);
    if (rc) return rc;
    PEDP_REQUIRE(!c->icp_pending, "%s: a registration is pending on this context (the call waits for the stream)", who);
    *out = pedp_deviation_totals{v->F, 0, 0, -1, 0.0, 0.0, 0.0, NAN, NAN, NAN};
    if (v->F == 0) return PEDP_OK;
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    const int64_t n_blocks = (v->F + SUM_BLOCK - 1) / SUM_BLOCK;
    rc = v->io.reserve(a256(sizeof(Sums) * (size_t)(n_blocks + 1)));
    if (rc) return rc;
    Sums *part = (Sums *)v->io.ptr, *total = part + n_blocks;
    hipLaunchKernelGGL(deviation_summary_block_kernel, dim3((unsigned)((n_blocks + SUM_WPB - 1) / SUM_WPB)), dim3(DT), 0, c->stream, v->st, k,
                       v->map->area, v->F, n_blocks, part);
    hipLaunchKernelGGL(deviation_summary_total_kernel, dim3(1), dim3(64), 0, c->stream, part, n_blocks, total);
    PEDP_HIP_CHECK(hipGetLastError());
    Sums s;
    rc = pedp_download(c, &s, total, sizeof(s));
    if (rc) return rc;
    out->measured_faces = s.measured;
    out->marked_faces = s.marked;
    out->max_face = s.max_face;
    out->total_area = s.total_area;
    out->measured_area = s.measured_area;
    out->marked_area = s.marked_area;
    if (s.measured > 0) {
        out->mean = s.s1 / s.measured_area;
        out->rms = sqrt(s.s2 / s.measured_area);
        out->max_abs_mean = value_of(s.max_key);
    }
    return PEDP_OK;
}

int pedp_deviation_map_regions(pedp_deviation_map_t v, const pedp_deviation_criteria *crit, int32_t grow, int mem, int32_t *labels,
                               int64_t capacity, pedp_deviation_region *table, int64_t *n_regions) {
    const char *who = "pedp_deviation_map_regions";
    PEDP_REQUIRE(v, "%s: null handle", who);
    pedp_defect_map_s *m = v->map;
    pedp_ctx_t c = v->ctx;
    const pedp_deviation_criteria k = crit ? *crit : DEFAULT_CRITERIA;
    int rc = check_criteria(who, k);
    if (rc) return rc;
    pedp_region_ws w;
    rc = pedp_defect_regions_begin(m, who, grow, mem, capacity, (const pedp_defect_region *)table, n_regions, w);
    if (rc || !w.seed) return rc;
    const int64_t F = v->F;
    // The body writes its rows and labels to device memory of this handle; the rows of this call are made from them.
    const int64_t rows = !table ? 0 : (capacity < F ? capacity : F);
    const int64_t blocks_max = F / SUM_BLOCK + rows;  // every region has at most one block that is not full
    const size_t o_body = 0, o_part = o_body + a256(sizeof(pedp_defect_region) * (size_t)rows),
                 o_rows = o_part + a256(sizeof(VolumePart) * (size_t)blocks_max),
                 o_labels = o_rows + a256(sizeof(pedp_deviation_region) * (size_t)rows), bytes = o_labels + a256(4 * (size_t)F);
    rc = v->io.reserve(bytes);
    if (rc) return rc;
    char *io = (char *)v->io.ptr;
    pedp_defect_region *body = rows ? (pedp_defect_region *)(io + o_body) : nullptr;
    int32_t *d_labels = mem == PEDP_DEVICE ? labels : (labels ? (int32_t *)(io + o_labels) : nullptr);
    hipLaunchKernelGGL(deviation_seed_kernel, dim3(blocks_for(F)), dim3(DT), 0, c->stream, v->st, k, F, w.seed, w.mark[0], v->abs_key,
                       v->mean);
    const pedp_region_columns col{v->abs_key, v->st.n, v->st.frames};
    rc = pedp_defect_regions_finish(m, who, w, col, grow, PEDP_DEVICE, d_labels, rows, body, n_regions);
    if (mem == PEDP_HOST && labels && (rc == PEDP_OK || (rc == PEDP_ERR_BAD_ARG && *n_regions > rows))) {
        const int rc2 = pedp_download(c, labels, d_labels, 4 * (size_t)F);
        if (rc2) return rc2;
    }
    const int64_t R = *n_regions;
    if (rc) return rc;
    // a table with capacity 0 went to the body as no table (rows = 0), which skips the body's own check: made here
    PEDP_REQUIRE(R <= capacity || !table, "%s: %lld regions, room for %lld", who, (long long)R, (long long)capacity);
    if (!table || R == 0) return PEDP_OK;
    VolumeArgs a;
    a.order = w.order; a.begin = w.begin; a.end = w.end; a.block_off = w.block_off; a.R = R;
    a.area = m->area; a.mean = v->mean; a.n = v->st.n;
    a.part = (VolumePart *)(io + o_part);
    pedp_deviation_region *d_table = mem == PEDP_DEVICE ? table : (pedp_deviation_region *)(io + o_rows);
    hipLaunchKernelGGL(deviation_volume_block_kernel, dim3((unsigned)((blocks_max + SUM_WPB - 1) / SUM_WPB)), dim3(DT), 0, c->stream, a);
    hipLaunchKernelGGL(deviation_volume_row_kernel, dim3((unsigned)((R + SUM_WPB - 1) / SUM_WPB)), dim3(DT), 0, c->stream, a, body, d_table);
    PEDP_HIP_CHECK(hipGetLastError());
    if (mem == PEDP_HOST) return pedp_download(c, table, d_table, sizeof(pedp_deviation_region) * (size_t)R);
    PEDP_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PEDP_OK;
}

}  // extern "C"
