// ICP, shared by every stage: build switches, the diagnostic stamp macros, the constants of the
// segmented path, the device state of a registration and the correctly rounded float64 helpers.
#pragma once
#include "../pedp_internal.h"
#include <cmath>
#include <cstddef>
#include <type_traits>

#ifndef PEDP_NN_EXPERIMENT
#define PEDP_NN_EXPERIMENT 0
#endif

#ifndef PEDP_ICP_STAMPS
#define PEDP_ICP_STAMPS 0
#endif
#if PEDP_ICP_STAMPS
// Diagnostic build only (tools/icp_stamps.py): s_memtime at the phase boundaries of the fused
// pass's kernels, written to a buffer nothing else reads.  [kernel 0..2][workgroup or wave][8]
__device__ long long g_icp_stamps[3][4096][8];
#define PEDP_STAMP(kern, unit, slot)                                                   \
    do {                                                                               \
        if ((unit) < 4096) g_icp_stamps[kern][unit][slot] = (long long)__builtin_amdgcn_s_memtime(); \
    } while (0)
extern "C" int pedp_debug_icp_stamps(long long *out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_icp_stamps), sizeof(long long) * 3 * 4096 * 8) == hipSuccess ? 0 : -3;
}
// s_memrealtime (100 MHz, one clock for the whole device) per pass and workgroup of the pass kernel:
// [0] entry, [1] state read, [2] chunks done, [3] ticket returned, [4] pass closed (last workgroup only); the head close of the
// pass before: [5] partial sums' loads back, [6] sums done, [7] U published
__device__ long long g_icp_rt[32][512][8];
// per wave of the pass kernel (last pass that ran): [0] start [1] slots ready [2] culled+swept [3] selected [4] sums done (s_memtime),
// [5] words << 32 | batches << 16 | wide << 8 | slots, [6] tiles
__device__ long long g_icp_wave[512][8][16];
#define PEDP_WV(slot, val)                                                                         \
    do {                                                                                           \
        if ((threadIdx.x & 63) == 0 && blockIdx.x < 512 && blockIdx.y == 0)                        \
            g_icp_wave[blockIdx.x][threadIdx.x >> 6][slot] = (long long)(val);                     \
    } while (0)
extern "C" int pedp_debug_icp_wave(long long *out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_icp_wave), sizeof(long long) * 512 * 8 * 16) == hipSuccess ? 0 : -3;
}
#define PEDP_RT(pass, slot)                                                                     \
    do {                                                                                        \
        if (threadIdx.x == 0 && (pass) < 32 && blockIdx.x < 512 && blockIdx.y == 0)             \
            g_icp_rt[pass][blockIdx.x][slot] = (long long)__builtin_amdgcn_s_memrealtime();     \
    } while (0)
extern "C" int pedp_debug_icp_rt(long long *out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_icp_rt), sizeof(long long) * 32 * 512 * 8) == hipSuccess ? 0 : -3;
}
#else
#define PEDP_STAMP(kern, unit, slot) do {} while (0)
#define PEDP_RT(pass, slot) do {} while (0)
#define PEDP_WV(slot, val) do {} while (0)
#endif

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int PACKET = 29;  // doubles per partial-sum packet
constexpr int NN_SB = 8;    // scene blocks of 16 points per wave
constexpr int NN_WAVES = 4;
constexpr int NN_PTS_PER_WG = NN_SB * 16 * NN_WAVES;  // 512
constexpr int NN_TU = 4;    // rows are padded to multiples of 16 * NN_TU (= the largest unit)
// A target UNIT is QT MFMA tiles (16 QT rows): the granularity of culling, of the sweep's
// fold-and-compare epilogue and of the exact re-scoring.  QT = 1 inside a registration with a
// finite radius (finest culling), QT = 4 for dense sweeps (3 instead of 6 VALU ops per MFMA).
constexpr int NN_LIST_TILES = 2048; // most MFMA tiles one sweep wave walks (its unit list lives in LDS)
constexpr int SEG_MIN_TILES = 64;   // MFMA tiles per sweep segment at least
constexpr int CULL_WORDS = 8;       // 64-unit mask words one cull wave fills
constexpr int SORT_BITS = 16;         // spatial sort: 65536^3 Hilbert-ordered cells over the cloud's own bounding box
constexpr int SORT_KEY_BITS = 3 * SORT_BITS + 1;  // + the bucket of points without a cell (non-finite coordinates)
constexpr int NN_TILE_PAD = 2 * NN_TU;  // readable pad tiles behind the last real tile
constexpr int ACC_BLOCKS = 256;
constexpr int ACC_THREADS = 256;

struct IcpState {
    double T[16];
    double upd[16];
    double fitness, rmse, prev_fitness, prev_rmse;
    double centroid[3];
    int done;
    int iters;
    int fb_count;
    int n_cand;   // slots of the compacted candidate list this pass (128 per scene block)
    int n_blocks; // scene blocks (one per transform wave with at least one candidate)
    int n_segs, seg_len;       // sweep segments of this pass and their length in tiles
    int n_lane;                // closes of this registration whose 6x6 solve ran a row per lane (solve_lanes.h; statistics, as n_wide;
                               // the word was padding in front of the 8-byte counters: the state did not grow)
    long long sum_tiles;       // surviving (scene block, target tile) pairs, summed over passes
    long long sum_cand;  // statistics over the passes of this registration
    long long sum_fb;
    // fused pass: the live chunk set is rebuilt from the whole scene when `rebuild` is set (pass 0,
    // and whenever the accumulated motion could have carried an outside point into reach)
    int rebuild;
    int n_rebuilds;
    int n_live;                // entries of the live list (written by icp_finish_kernel)
    // parameters of this registration that the fused pass reads from here rather than from kernel
    // arguments, so that one captured graph serves start poses with different radii and criteria
    double r2, r2cut, r2live;  // r^2; rounding-safe r^2 of the box test; (r + margin)^2 of the live test
    double reachE, margin;     // motion bound: r + margin + rho, margin
    double rel_fitness, rel_rmse, n_source;
    float r1, r_search, wide_radius, r2f;
    int pass, max_iter;        // the pass the fused kernels are in (advanced by icp_finish_kernel), and the limit
    double mu_theta, mu_tau;   // sum of |R - I|_F and of |t + (R - I) c| since the last rebuild
    // tickets and sign-offs are counted on from launch to launch (nothing to reset at the end of a pass): what the
    // counters read when this launch began
    unsigned ticket_base, idle_base;
    int n_planned;             // passes of this registration that ran under a visit plan (statistics)
    int nonce;                 // of this registration (<< 16 in the tags of the visit plan: entries of an earlier registration never match)
    int n_wide;                // passes of this registration closed by the wide close (statistics: tests check it was in force)
    int n_head;                // passes of this registration closed at the head of the next launch (statistics, as n_wide)
    int n_steady;              // passes of this registration run inside a steady launch (steady_pass.h; statistics)
    int n_followed;            // workgroups that followed a closer in the last steady launch (statistics; the word was a spare one:
                               // the state did not grow, and only the launch's service workgroup writes it, once, at exit)
    double T_init[16];         // the start transformation: slot 0 of the update history (arrives with the state, no copy of its own)
    long long sum_cert, sum_searched;  // candidate slots whose search a certificate replaced / that searched, summed over passes (statistics)
};
static_assert(sizeof(IcpState) == 83 * sizeof(double), "the state moves as 83 8-byte words; a new statistic takes a spare word");

// Certificates (fused pass, single registration): a chunk's count of certified and of searching slots shares the
// free 32nd double of its partial, searching slots scaled by CERT_PACK (exact while a pass has fewer than 2^26 of either)
constexpr double CERT_PACK = 67108864.0;
// a slot that searches does so within KAPPA times the distance to last pass's neighbour: the margin its certificate lives on
// (bench registration, one MI355X: 1.25 -- 0.531 ms, 1.5 -- 0.548, 2 -- 0.543, 3 -- 0.542; the certified share is the same)
#ifndef PEDP_ICP_KAPPA
#define PEDP_ICP_KAPPA 1.25f
#endif
// Rows a lane did not re-score are bounded from below through fp32 g: d^2 >= g + S - (CERT_SLACK eps + 4.8e-7 S).  eps bounds
// every j-dependent error of one g (the selection window g_min + 2 eps rests on the same bound), 4.8e-7 S the
// rounding of S.  The `maybe` test's generous 4 eps is a third of a typical gap between first and second neighbour at bench
// size and left 42 % of the slots certifiable; 1 eps certifies all of them from pass 6 on.
#ifndef PEDP_ICP_CERT_SLACK
#define PEDP_ICP_CERT_SLACK 1.0f
#endif

__device__ __forceinline__ double dmul(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ double dadd(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ double dsub(double a, double b) { return __dsub_rn(a, b); }

// the oracle's dist2(): (dx*dx + dy*dy) + dz*dz, no FMA
__device__ __forceinline__ double dist2(double ax, double ay, double az, double bx, double by, double bz) {
    double dx = dsub(ax, bx), dy = dsub(ay, by), dz = dsub(az, bz);
    return dadd(dadd(dmul(dx, dx), dmul(dy, dy)), dmul(dz, dz));
}

// Pointers that reach a kernel through the argument block parked in LDS have no address space the compiler
// could infer: every access through them came out as a FLAT operation, which counts on the LDS counter as
// well as on the memory counter -- each LDS read of a list entry then waited for the loads still in flight
// (`s_waitcnt vmcnt(0) lgkmcnt(0)` in front of the sweep's MFMAs), so nothing was prefetched at all.  The
// pass kernel states the address space where it dereferences them.
#define PEDP_GLOBAL __attribute__((address_space(1)))
template <typename T>
__device__ __forceinline__ PEDP_GLOBAL T *as_global(T *p) {
    return (PEDP_GLOBAL T *)(uintptr_t)p;
}

}  // namespace
