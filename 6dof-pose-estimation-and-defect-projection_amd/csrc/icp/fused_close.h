// ICP, fused pass: its overview and constants, the argument blocks, and the close of a pass (sum, solve,
// update, live list) as the body the pass kernel runs in-launch and as icp_finish_kernel.
#pragma once
#include "common.h"
#include "live_list.h"
#include "solve.h"
#include "solve_lanes.h"

namespace {

// ================================================================== fused pass
// Radius-limited registrations (unit size 1) run ONE launch per correspondence pass:
//   icp_pass_kernel    one workgroup (8 waves) per live scene chunk.  Every WAVE owns one 16-slot
//                      sub-block of the chunk from the transform to the partial sums and never
//                      waits for another wave on the way: transform, box test, compaction into the
//                      wave's slots, the sub-block's bounding sphere, two-level culling of the target
//                      tiles against THAT sphere, MFMA sweep of the survivors (one MFMA per tile,
//                      the two best tiles per lane in registers), exact float64 selection, the
//                      sub-block's partial sums of J^T J / J^T r by a fixed shuffle tree.  The eight
//                      waves meet once, to add their sums in order.  The workgroup that finishes
//                      last (a ticket) adds the live chunks' partial sums in ascending chunk order,
//                      solves the 6x6 system, updates the pose, the convergence test, the motion
//                      bound and the live list (icp_finish_body).
//   icp_finish_kernel  the same body as a launch of its own: only where an exchange step (scene
//                      sharded over ranks) sits between the sum and the solve.
// Round 2 ran the chunk as eight cooperating waves with ten workgroup barriers, its triples and tile
// lists in LDS, and the finish as a second launch: 36 + 10 us per pass of which a few hundred
// nanoseconds were arithmetic.
//
// A chunk is 128 consecutive entries of the scene's spatial order.  Only LIVE chunks are visited:
// those that had a point within r + margin of the target's bounding box when the live set was
// last rebuilt.  A rebuild pass walks the whole scene and recomputes every point from the source
// through the history of updates -- the same float64 operations, in the same order, as applying
// them pass by pass, so a point's coordinates do not depend on when its chunk became live.
// Between rebuilds a point outside the live chunks is farther than r + margin from the box; an
// update (R, t) moves a point x by at most |R - I| |x - c| + |t + (R - I) c| (c = box centre), and
// with e = (distance to the box) + rho (rho = half diagonal), E = r + margin + rho:
//   e_new >= e (1 - theta) - tau   =>   e_n >= E - (Theta E + Tau) = E - mu,
// so no such point can come within r while mu < margin; the finish requests a rebuild at
// mu >= 0.95 margin.  Chunk ids, slot order, tile order and the order of the partial sums depend
// only on the data, never on execution order: results are run-to-run bit-stable.
//
// Hand-over of the partial sums inside the launch (MI355X: per-XCD L2s are not coherent, a CU's L1
// is never refreshed): every partial is stored write-through (sc1), every storing wave drains its
// stores (s_waitcnt vmcnt(0)), the workgroup meets at a barrier, ONE lane takes an agent-scope
// ticket; the workgroup whose ticket is the last reads every partial with sc1 loads (they bypass
// its L1).  No fence: a release fence per workgroup writes the XCD's L2 back and took the pass from
// 36 to 92 us in round 2.  The live mask words are only ever touched by agent-scope atomics.
constexpr int CH = NN_SB * 16;   // 128 scene points per chunk = slots per scene block
constexpr int BK_W = 8;          // waves of a pass workgroup = sub-blocks of a chunk
constexpr int BK_WCAP = BK_W * 64;  // mask words (64 tiles each) the fused pass handles: 524,288 target points
constexpr int PSTRIDE = 32;      // doubles per chunk in the partials: packet, [29] wave-tiles swept, [30] exact searches, [31] certified slots (single registration)
constexpr int LIVE_CAP = 8192;   // live chunks the finish kernel lists in LDS (1M scene points)
constexpr int FIN_THREADS = 1024; // threads of icp_finish_kernel

// ---- the 6x6 solve of the close
// The same pivoted LDLT as solve6_ldlt (and oracle/icp.c), operation for operation, with the
// matrix in registers: every index is a compile-time constant after unrolling and the pivot
// exchange of step k is a chain of predicated swaps, one per candidate row.
__device__ __forceinline__ void swap_if(bool c, double &x, double &y) {
    const double t = x;
    x = c ? y : x;
    y = c ? t : y;
}
__device__ bool solve6_ldlt_reg(const double *__restrict__ Ain, const double *__restrict__ b, double *__restrict__ x) {
    // ONE thread runs this; its pivot index is made wave-uniform (readfirstlane: the only active lane), so the
    // exchange of step k is a scalar branch to the one pair of rows and columns concerned instead of a
    // predicated swap for every candidate row (5 + 4 + 3 + 2 + 1 times 12 swaps: a third of the solve).
    double A[6][6], y[6];
    int tr[6];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) A[i][j] = Ain[6 * i + j];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        int p = k;
        double big = fabs(A[k][k]);
#pragma unroll
        for (int i = k + 1; i < 6; ++i)
            if (fabs(A[i][i]) > big) { big = fabs(A[i][i]); p = i; }
        p = __builtin_amdgcn_readfirstlane(p);
        tr[k] = p;
#pragma unroll
        for (int q = k + 1; q < 6; ++q) {
            if (p == q) {  // scalar branch
#pragma unroll
                for (int j = 0; j < 6; ++j) { const double t = A[k][j]; A[k][j] = A[q][j]; A[q][j] = t; }
#pragma unroll
                for (int i = 0; i < 6; ++i) { const double t = A[i][k]; A[i][k] = A[i][q]; A[i][q] = t; }
            }
        }
        if (k > 0) {
            double tmp[6];
#pragma unroll
            for (int j = 0; j < k; ++j) tmp[j] = A[j][j] * A[k][j];
            double sacc = 0.0;
#pragma unroll
            for (int j = 0; j < k; ++j) sacc += A[k][j] * tmp[j];
            A[k][k] -= sacc;
#pragma unroll
            for (int i = k + 1; i < 6; ++i) {
                double u = 0.0;
#pragma unroll
                for (int j = 0; j < k; ++j) u += A[i][j] * tmp[j];
                A[i][k] -= u;
            }
        }
        const double akk = A[k][k];
        if (fabs(akk) > 0.0) {
#pragma unroll
            for (int i = k + 1; i < 6; ++i) A[i][k] /= akk;
        }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) y[i] = b[i];
#pragma unroll
    for (int k = 0; k < 6; ++k)
#pragma unroll
        for (int q = k + 1; q < 6; ++q)
            if (tr[k] == q) { const double t = y[k]; y[k] = y[q]; y[q] = t; }
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < i; ++j) y[i] -= A[i][j] * y[j];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        if (fabs(A[i][i]) > 2.2250738585072014e-308) y[i] /= A[i][i];
        else y[i] = 0.0;
    }
#pragma unroll
    for (int i = 5; i >= 0; --i)
#pragma unroll
        for (int j = i + 1; j < 6; ++j) y[i] -= A[j][i] * y[j];
#pragma unroll
    for (int k = 5; k >= 0; --k)
#pragma unroll
        for (int q = k + 1; q < 6; ++q)
            if (tr[k] == q) { const double t = y[k]; y[k] = y[q]; y[q] = t; }
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        x[i] = y[i];
        if (not_finite64(y[i])) ok = false;  // (NaN or infinite)
    }
    // (a solution that is not finite comes back as zeros: what a NaN's sign and payload are depends on the instructions the
    // compiler picked, and no caller uses such a solution)
#pragma unroll
    for (int i = 0; i < 6; ++i) x[i] = ok ? x[i] : 0.0;
    return ok;
}


__device__ __forceinline__ void xform(const double *__restrict__ M, double &x, double &y, double &z) {
    const double nx = dadd(dadd(dadd(dmul(M[0], x), dmul(M[1], y)), dmul(M[2], z)), M[3]);
    const double ny = dadd(dadd(dadd(dmul(M[4], x), dmul(M[5], y)), dmul(M[6], z)), M[7]);
    const double nz = dadd(dadd(dadd(dmul(M[8], x), dmul(M[9], y)), dmul(M[10], z)), M[11]);
    x = nx; y = ny; z = nz;
}

__device__ __forceinline__ float4 gload4(const float4 *p) {
    typedef float v4 __attribute__((ext_vector_type(4)));
    const v4 v = *(const PEDP_GLOBAL v4 *)(uintptr_t)p;
    return make_float4(v[0], v[1], v[2], v[3]);
}
template <typename P>
__device__ __forceinline__ void xform_g(P M, double &x, double &y, double &z) {  // xform through a global pointer
    const double nx = dadd(dadd(dadd(dmul(M[0], x), dmul(M[1], y)), dmul(M[2], z)), M[3]);
    const double ny = dadd(dadd(dadd(dmul(M[4], x), dmul(M[5], y)), dmul(M[6], z)), M[7]);
    const double nz = dadd(dadd(dadd(dmul(M[8], x), dmul(M[9], y)), dmul(M[10], z)), M[11]);
    x = nx; y = ny; z = nz;
}

struct PassArgs {
    // scene
    const double *src;          // N x 3 source points
    const int32_t *perm;        // spatial order
    int64_t N;
    int n_chunks;
    double *hist;               // [pass + 1][16]: init, then the update of every pass so far
    double *Pk;                 // 2 x N_pad x 3: transformed points in spatial order (live chunks); pass p reads copy p & 1, writes the other
    double *Tprev;              // 2 x N_pad x 3: last pass's nearest neighbour of the point at that position (x = NaN: none); likewise
    size_t pp_stride;           // doubles between the two copies
    unsigned long long *live;   // live mask (n_lw words), behind it the mask before the last rebuild (n_lw words)
    const double *chunk_sph;    // [chunk][8][4]: bounding spheres of the chunk's eight 16-point runs in the source frame
    int32_t *live_list;         // live chunks ascending (valid outside rebuild passes)
    // target
    const float *tgtf;          // sorted target operand, 64 floats per 16-row tile
    int n_tiles, n_words;
    const float4 *tile_sph, *word_sph;
    const double *tgt_s;        // sorted target rows, float64 x 6: x y z nx ny nz
    const int32_t *tperm;       // sorted row -> target index
    int64_t Nt;
    const double *tgt, *nrm;
    // parameters (the radius-dependent ones live in IcpState)
    float Tn, T2;
    double lo[3], hi[3];
    int estimator;
    int32_t *idx_out;
    double *partials;           // n_chunks x PSTRIDE: by chunk id in a rebuild pass, by live rank otherwise
    // Several start poses of one (scene, target) pair share a launch: pose b = blockIdx.y owns the
    // state and the per-pose buffers (Pk, Tprev, live, live_list, hist, idx_out, partials, packet)
    // b * pose_stride bytes behind pose 0's.
    size_t pose_stride;
    // the finish inside the launch (fuse != 0)
    int fuse, n_lw;
    unsigned *ticket;           // workgroups of the running launch that are through (the last one closes the pass); a line of its own:
                                // 512 atomics on the state's line held up every wave's reads of the state
    double *packet, *trace;
    double bc[3];               // centre of the target's box (motion bound)
    // Which workgroup visits which live chunk (single registration only).  With more live chunks than CUs the
    // dispatcher puts workgroups n_cu + k and k on one CU, and two workgroups on a CU run a third slower than one
    // alone: the pass ended with the pairs.  The workgroup that is through FIRST (ticket 0; it has ten microseconds
    // to spare) ranks the chunks by the durations the pass before measured and hands the lightest 2 (n_live - n_cu)
    // of them to the positions that share a CU, the lightest with the heaviest of those.  Only who works on a chunk
    // changes -- partial sums stay indexed by live rank, so no result bit does.
    int4 *visit;                // [2][visit_cap]: (live rank, chunk, pass + 1 it is meant for, n_live) for workgroup b of pass p at [p & 1][b]
    int2 *dur;                  // [2][visit_cap]: (cycles, pass + 1 that measured them) by live rank, at [p & 1][rank]
    int visit_cap, n_cu;
    // the closing workgroup that ends the registration (it sets `done`) also writes the final state here, into the
    // executor's page-locked block: no copy follows the last pass (single registration; null: the host copies)
    unsigned long long *down;
    int serial_close;           // PEDP_ICP_SERIAL_CLOSE=1: the close as it was, everything after the sums on one lane
    int lane_solve;             // the wide close's 6x6 solve with a row per lane (solve_lanes.h; PEDP_ICP_LANE_SOLVE=0: on lane 0 alone).
                                // The HOST reads it: it launches the kernels' LANES instantiations, which hold that form alone.
    // Head close (single registration, fused, wide close, final state written by the device; PEDP_ICP_HEAD_CLOSE=0: off).
    // A steady pass ends with its partial sums; the NEXT launch closes it, in every workgroup, before it transforms its
    // chunk.  The state has two slots by pass parity (slot p & 1 holds the state pass p starts from); `launch` is the
    // index of this launch = the pass it runs.  The grid has one workgroup more than chunks can fill: the first
    // workgroup without a chunk (the service workgroup) writes what a head close leaves behind.
    int head, launch;
    // Head close: pass p stores its partial sums into copy p & 1 (part_stride doubles apart).  The head of launch L reads
    // pass L - 1's while workgroups of launch L that are through already store pass L's: not into the same buffer.
    size_t part_stride;
    // Certificates (single registration closed in its launches; PEDP_ICP_CERT=0: off -- null).  One float per scene
    // position, two copies by pass parity like Pk: a lower bound on the distance from the point as pass p left it to
    // every target point other than the neighbour pass p found (0: none).  While the point's motion since leaves the
    // old neighbour strictly inside the bound, the next pass takes it over without a search (fused_pass.h).
    float *cert;
    size_t cert_stride;         // floats between the two copies
};

template <typename T>
__device__ __host__ __forceinline__ T *pose_ptr(T *p, size_t bytes) {
    return (T *)((char *)p + bytes);
}
template <typename T>
__device__ __host__ __forceinline__ const T *pose_ptr(const T *p, size_t bytes) {
    return (const T *)((const char *)p + bytes);
}

// ------------------------------------------------------------------ finish
// phase 0: sum the live chunks' partials, solve, update (one GPU); phase 1: sum only (the packet
// then goes through the all-reduce); phase 2: solve from the summed packet.
// Order of the sum: 32 contiguous ranges of the live chunks, ascending inside a range, then the
// ranges in order -- a function of the live set alone, whatever the number of threads.
struct FinishArgs {
    unsigned long long *live;
    int32_t *live_list;
    int n_lw;
    const double *partials;
    double *packet;
    int phase, estimator;
    double *trace, *hist;
    double bcx, bcy, bcz;
    // in-launch finish: sixteen counters (32 words apart) on which the launch's workgroups without a chunk sign off;
    // the state is rewritten only once all n_idle of them have
    unsigned *idle = nullptr;
    int n_idle = 0, n_busy = 0;
    // in-launch finish: what the closing workgroup read of the state when the launch began (pass, rebuild flag, live
    // count do not change inside a pass) -- no second, dependent read in front of the partial sums' loads
    int known = 0, k_pass = 0, k_rebuild = 0, k_n_live = 0;
    // in-launch finish: where the final state goes once `done` is set (page-locked host memory; null: nowhere)
    unsigned long long *down = nullptr;
    // 0: the wide close -- the first look at the sign-off counters travels with the partial sums' loads, and behind the
    // solve the three sincos run on three lanes, the sixteen entries of the new pose on sixteen; 1: all of it on lane 0,
    // one step after the other, as it was.  Every output is computed by the same sequence of float64 operations.
    int serial = 0;
    // the wide close's point-to-plane solve: 0 -- solve6_ldlt_reg on lane 0; else solve6_ldlt_lanes on wave 0, a row per lane.
    // The same float64 operations per output either way.
    int lane = 0;
    // the mask the rebuild pass before this close read "was live" from (today: the copy the closer makes aside when it
    // asks for a rebuild; gen_masks: the other of two masks used in turn, rebuild g ORs into mask g & 1 -- its closer
    // zeroes the other one, nothing is copied aside when a rebuild is asked for)
    unsigned long long *live_old = nullptr;
    int gen_masks = 0;
};
template <int NT, int LCAP>
struct FinishLds {
    double slice[32][32], pk[32];
    int scan[NT], lst[LCAP];
    int do_rebuild, n_live_s, stopped;
    double t0[16];  // the pose the pass started from
};
// lane 0's value in every lane of a wave whose lanes are all active
__device__ __forceinline__ double bcast0(double v) {
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}
// (COHERENT loads, the g_u64 / g_i32 / g_u32 pointer types and load_live: live_list.h)
__device__ __forceinline__ double load_sc1(const double *p) {
    return __longlong_as_double((long long)__hip_atomic_load((g_u64 *)(uintptr_t)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ int load_sc1(const int32_t *p) {
    return __hip_atomic_load((g_i32 *)(uintptr_t)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void store_sc1(double *p, double v) {
    __hip_atomic_store((g_u64 *)(uintptr_t)p, (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool COHERENT>
__device__ __forceinline__ double load_partial(const double *p) {
    return COHERENT ? load_sc1(p) : *p;
}

// MODE 0: `st` is the state in memory.  MODE 1: `st` is the workgroup's copy of the state in LDS; the caller writes it
// out (and the final state to f.down's block) behind the body.  MODE 2: the head close -- as 1, and every workgroup of
// the launch runs it: nothing is written to memory here (the service workgroup does that from LDS), no live list, no
// sign-off poll, no live-mask upkeep.  MODE 3: the head close inside a launch that goes on (steady_pass.h) -- as 2, but the
// partial sums were stored in THIS launch: they are read coherently, entry by entry.
// the close's stamps (diagnostic build): of a head close, which every workgroup runs, workgroup 0's only
#ifndef PEDP_ICP_STAMP_CLOSE_PASS
#define PEDP_ICP_STAMP_CLOSE_PASS 5  // the pass whose close is stamped phase by phase (diagnostic build; 0 or 1: a rebuild pass's, with its listing)
#endif
#define PEDP_STAMP_CLOSE(unit, slot) do { if (!HEAD || blockIdx.x == 0) PEDP_STAMP(2, unit, slot); } while (0)
template <int NT, int LCAP, bool COHERENT, int MODE = 0>
__device__ __forceinline__ void icp_finish_body(IcpState *st, const FinishArgs &f, FinishLds<NT, LCAP> &L, const int tid) {
    constexpr bool LOCAL = MODE != 0, HEAD = MODE >= 2;
    static_assert(MODE != 2 || !COHERENT, "the head close reads what the launch before stored");
    static_assert(MODE != 3 || COHERENT, "the close inside a steady launch reads what that launch stored");
    // (a state in LDS comes back in vector registers: the parameters, the same in every lane, are made scalar again)
    auto uni = [](double v) { return LOCAL ? bcast0(v) : v; };
    const int pass = f.known ? f.k_pass : st->pass, max_iter = LOCAL ? __builtin_amdgcn_readfirstlane(st->max_iter) : st->max_iter;
    const double n_source = uni(st->n_source), rel_fitness = uni(st->rel_fitness), rel_rmse = uni(st->rel_rmse), reachE = uni(st->reachE),
                 margin = uni(st->margin);
    constexpr int PARTS = 32, TPARTS = NT / 32, PPT = PARTS / TPARTS;  // ranges; ranges in flight; ranges per thread
    static_assert(NT % 32 == 0 && PARTS % TPARTS == 0, "thread count");
    const bool wide = f.serial == 0;
    if (tid == 0) { L.do_rebuild = 0; L.stopped = 0; }
    if (tid == 0) PEDP_STAMP_CLOSE(0, 0);
    if (tid == 0 && pass == PEDP_ICP_STAMP_CLOSE_PASS) PEDP_STAMP_CLOSE(3, 0);
    // The first look at the sign-off counters is requested here, with the partial sums' loads, and evaluated where
    // the poll stands: the counters only grow, so a look that is complete now is complete then, and only a look that
    // comes back short enters the spin.  (With fewer live chunks than workgroups there are idle workgroups in every
    // pass, so the look -- a device-scope round trip -- used to be paid behind the sum's two barriers, every pass.)
    const bool early_look = wide && COHERENT && f.n_idle > 0;
    unsigned look0 = 0u, idle_base0 = 0u;
    if (early_look && tid < 64) {
        if (tid < 16) look0 = __hip_atomic_load((g_u32 *)(uintptr_t)(f.idle + 32 * tid), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        idle_base0 = st->idle_base;  // (rewritten only by this workgroup, further down)
    }
    // a rebuild pass's close lists the live chunks anew: its mask words are requested here as well (every workgroup with a
    // chunk has taken its ticket: the mask is final)
    const bool listing = f.phase != 2 && !HEAD && (f.known ? f.k_rebuild != 0 : st->rebuild != 0);
    LiveWords lw = {0, 0, 0, 0ull};
    if (listing) lw = live_words_load<NT, COHERENT>(f.live, f.n_lw, tid);
    // what the solving thread needs of the state is requested now, ahead of the sums; the pose is parked in LDS, an
    // entry per lane (the barriers of the sums lie between this store and its readers): held in lane 0's registers
    // through the sums and the solve it was thirty-two registers of a kernel at its cap, spilled and fetched back
    double fit0 = 0.0, rmse0 = 0.0, mu_th0 = 0.0, mu_ta0 = 0.0;
    int n_wide0 = 0;
    if (tid < 16) L.t0[tid] = st->T[tid];
    if (tid == 0) {
        fit0 = st->fitness; rmse0 = st->rmse; mu_th0 = st->mu_theta; mu_ta0 = st->mu_tau;
        if (wide) n_wide0 = st->n_wide;
    }
#if PEDP_ICP_STAMPS
    if (tid == 0 && (!HEAD || blockIdx.x == 0)) { g_icp_stamps[2][1][0] = (long long)__builtin_amdgcn_s_memtime(); g_icp_stamps[2][1][1] = (long long)__builtin_amdgcn_s_memrealtime(); }
#endif
    if (f.phase != 2) {
        // Partial sums are indexed by chunk id in a rebuild pass and by live rank otherwise; either
        // way they are summed in ascending chunk order.
        int n_live = f.known ? f.k_n_live : st->n_live;
        bool listed = true;
        if (listing) {
            // the new live list, ascending (live_list.h; the waves' totals go through the head of L.scan)
            n_live = live_list_build<NT, LCAP, COHERENT>(lw, f.live, f.live_list, L.lst, L.scan, tid);
            listed = n_live <= LCAP;
            if (tid == 0 && pass == PEDP_ICP_STAMP_CLOSE_PASS) PEDP_STAMP_CLOSE(3, 7);  // the list stands
        }
        // PARTS contiguous ranges of the live chunks, ascending inside a range, then the ranges in
        // order.  Sixteen loads in flight per thread and range; branch-free (an entry beyond the range
        // reads the range's last chunk again and is not added), the three ways to a chunk's position in
        // the partials -- live rank; list in LDS; list in memory, written a moment ago by this workgroup:
        // read past L1 -- are told apart outside the loops.
        const int k = tid & 31;
        const int lper = (n_live + PARTS - 1) / PARTS;
        auto sum_ranges = [&](auto position) {
            if constexpr (PPT == 2) {
                // 512 threads, 32 ranges x 32 entries: a thread takes TWO ENTRIES OF ONE range (not one entry of two
                // ranges, one range after the other): every load of the pass's sum is requested in one go -- one round
                // trip past the L2 instead of two -- with the registers the two-range form used (ten loads per entry and
                // round: a range is 9 chunks at the bench frame's 281 live chunks; each entry's additions in the same order)
                constexpr int BW = 10;
                const int part = tid >> 4, k0 = (tid & 15) * 2, k1 = k0 + 1;
                const bool has1 = k1 < PACKET + (LOCAL ? 3 : 2);  // (entry 31, the certificates' count: only a single registration's pass kernel writes it)
                const int l_lo = part * lper < n_live ? part * lper : n_live, l_hi = l_lo + lper < n_live ? l_lo + lper : n_live;
                double v0 = 0.0, v1 = 0.0;
                for (int q = l_lo; q < l_hi; q += BW) {
                    int at[BW];
                    double x0[BW], x1[BW];
#pragma unroll
                    for (int u = 0; u < BW; ++u) at[u] = position(q + u < l_hi ? q + u : l_hi - 1);
#pragma unroll
                    for (int u = 0; u < BW; ++u) {
                        if constexpr (HEAD && !COHERENT) {  // k0 is even and PSTRIDE is 32: the two entries are one aligned 16-byte load
                            typedef double v2d __attribute__((ext_vector_type(2)));
                            const v2d t = *(const PEDP_GLOBAL v2d *)(uintptr_t)&f.partials[(size_t)at[u] * PSTRIDE + k0];
                            x0[u] = t[0];
                            x1[u] = has1 ? t[1] : 0.0;
                        } else {
                            x0[u] = load_partial<COHERENT>(&f.partials[(size_t)at[u] * PSTRIDE + k0]);
                            x1[u] = has1 ? load_partial<COHERENT>(&f.partials[(size_t)at[u] * PSTRIDE + k1]) : 0.0;
                        }
                    }
#pragma unroll
                    for (int u = 0; u < BW; ++u) {
                        v0 = q + u < l_hi ? v0 + x0[u] : v0;
                        v1 = q + u < l_hi ? v1 + x1[u] : v1;
                    }
                }
                L.slice[part][k0] = v0;
                L.slice[part][k1] = v1;
                return;
            }
#pragma unroll
            for (int pp = 0; pp < PPT; ++pp) {
                const int part = (tid >> 5) + pp * TPARTS;
                const int l_lo = part * lper < n_live ? part * lper : n_live, l_hi = l_lo + lper < n_live ? l_lo + lper : n_live;
                double v = 0.0;
                // loads per round: inside a steady launch (1,024 threads, a thread per entry and range) ten, as above -- a
                // range is 9 chunks at the bench frame's 281 live chunks, and the CU's sixteen waves queue their loads on one
                // vector memory path: every load past the range's end is waited for by all of them
                constexpr int BW1 = MODE == 3 ? 10 : 16;
                if (k < PACKET + (LOCAL ? 3 : 2)) {  // (entry 31: as above)
                    for (int q = l_lo; q < l_hi; q += BW1) {
                        int at[BW1];
                        double x[BW1];
#pragma unroll
                        for (int u = 0; u < BW1; ++u) at[u] = position(q + u < l_hi ? q + u : l_hi - 1);
#pragma unroll
                        for (int u = 0; u < BW1; ++u) x[u] = load_partial<COHERENT>(&f.partials[(size_t)at[u] * PSTRIDE + k]);
#pragma unroll
                        for (int u = 0; u < BW1; ++u) v = q + u < l_hi ? v + x[u] : v;
                    }
                }
                L.slice[part][k] = v;
            }
        };
        if (!listing) sum_ranges([&](int q) { return q; });
        else if (listed) sum_ranges([&](int q) { return L.lst[q]; });
        else sum_ranges([&](int q) { return load_sc1(&f.live_list[q]); });
        if (tid == 0 && pass == PEDP_ICP_STAMP_CLOSE_PASS) PEDP_STAMP_CLOSE(3, 1);
        if (HEAD) PEDP_RT(pass + 1, 5);  // head close: this workgroup's loads of the partial sums are back
        if (tid == 0) L.n_live_s = n_live;
        __syncthreads();
        if (tid == 0 && pass == PEDP_ICP_STAMP_CLOSE_PASS) PEDP_STAMP_CLOSE(3, 2);
        if (tid < 32) {
            double t = 0.0;
            for (int q = 0; q < PARTS; ++q) t += L.slice[q][tid];
            L.pk[tid] = t;
            if (!HEAD && tid < PACKET) as_global(f.packet)[tid] = t;
        }
        __syncthreads();
        if (HEAD) PEDP_RT(pass + 1, 6);  // head close: the sums are done
        if (tid == 0 && f.phase == 1) {  // (phase 0 writes these further down, with the rest of the state)
            st->sum_tiles += (long long)L.pk[PACKET];
            st->sum_fb += (long long)L.pk[PACKET + 1];
            st->n_live = L.n_live_s;
        }
        if (tid == 0) {
#if PEDP_ICP_STAMPS
            if (!HEAD || blockIdx.x == 0) { g_icp_stamps[2][1][2] = (long long)__builtin_amdgcn_s_memtime(); g_icp_stamps[2][1][3] = (long long)__builtin_amdgcn_s_memrealtime(); }
#endif
        }
        if (f.phase == 1) return;
    } else {
        if (tid < PACKET) L.pk[tid] = as_global(f.packet)[tid];
        __syncthreads();
    }
    if (COHERENT && f.n_idle > 0 && tid < 64) {  // normally true at the first look
        for (unsigned spins = 0;; ++spins) {
            unsigned c = look0;  // (the wide close's first look is back already)
            if (!early_look || spins > 0)
                c = tid < 16 ? __hip_atomic_load((g_u32 *)(uintptr_t)(f.idle + 32 * tid), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
#pragma unroll
            for (int off = 8; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
            if (__shfl(c, 0, 64) - (early_look ? idle_base0 : st->idle_base) >= (unsigned)f.n_idle) break;
            if (spins > (1u << 22)) {  // bounded: a lost workgroup must not hang the device -- but the pass is NOT closed over
                if (tid == 0) L.do_rebuild = -1;   // workgroups that may still read the old state: the registration fails loudly
                break;
            }
            __builtin_amdgcn_s_sleep(8);
        }
    }
    if (COHERENT && f.n_idle > 0) {
        __syncthreads();
        if (L.do_rebuild == -1) {  // (workgroup-uniform)
            if (tid == 0) {
                st->done = -1;   // icp_collect / the batch driver turn this into PEDP_ERR_HIP
                if (!LOCAL && f.down) *(int *)((char *)f.down + offsetof(IcpState, done)) = -1;  // (where icp_collect looks when no copy follows)
            }
            return;
        }
    }
    // Everything from here to the state's last store is one dependent chain that 255 CUs wait for.  The serial close
    // runs all of it on lane 0.  The wide close keeps lane 0 for what is one chain by nature (criteria, the pivoted
    // solve, the motion bound) and gives wave 0's other lanes what is several independent pieces: a lane per angle
    // for the three sincos, a lane per entry for upd x T0 and for the stores of both matrices.  Each output is
    // computed by the sequence of float64 operations the serial close uses (sincos_to_T; mat4_mul_dev's sum).
    if (wide ? tid < 64 : tid == 0) {
        const bool l0 = tid == 0;
        int stop_i = 0, angles_i = 0;  // angles: the update is made from x (point-to-plane, the solve succeeded)
        int solve_i = 0;               // lane 0 found the pass in need of the point-to-plane solve and left it to the wave
        const bool lane_form = wide && f.lane != 0;
        double upd[16], x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        ident4(upd);
        if (l0) {
            PEDP_STAMP_CLOSE(0, 1);
            if (pass == PEDP_ICP_STAMP_CLOSE_PASS) PEDP_STAMP_CLOSE(3, 3);
            if (COHERENT) { st->ticket_base += (unsigned)f.n_busy; st->idle_base += (unsigned)f.n_idle; }
            if (f.phase == 0) {
                st->sum_tiles += (long long)L.pk[PACKET];
                st->sum_fb += (long long)L.pk[PACKET + 1];
                st->n_live = L.n_live_s;
                if constexpr (LOCAL) {
                    const long long searched = (long long)(L.pk[PACKET + 2] / CERT_PACK);  // (the division by 2^26 is exact)
                    st->sum_searched += searched;
                    st->sum_cert += (long long)(L.pk[PACKET + 2] - (double)searched * CERT_PACK);
                }
            }
            L.do_rebuild = 0;
            const double *pk = L.pk;
            const double K = pk[28];
            double fit = 0.0, rmse = 0.0;
            if (K > 0.0) { fit = K / n_source; rmse = sqrt(pk[27] / K); }
            st->prev_fitness = fit0;
            st->prev_rmse = rmse0;
            st->fitness = fit;
            st->rmse = rmse;
            if (!HEAD && f.trace) {
                PEDP_GLOBAL double *tr = as_global(f.trace) + 18 * pass;
                tr[0] = fit; tr[1] = rmse;
                for (int k = 0; k < 16; ++k) tr[2 + k] = L.t0[k];
            }
            st->iters = pass;
            if (wide) st->n_wide = n_wide0 + 1;
            if (HEAD) st->n_head = st->n_head + 1;
            bool stop = pass >= max_iter;
            if (pass > 0 && fabs(fit0 - fit) < rel_fitness && fabs(rmse0 - rmse) < rel_rmse) stop = true;
            if (stop) {
                st->done = 1;
                if (!LOCAL && COHERENT && f.down) {  // the final state goes to the host from here (below): this lane's stores have left first
                    L.stopped = 1;
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
                stop_i = 1;
            } else {
                PEDP_STAMP_CLOSE(2, 0);
                if (pass == PEDP_ICP_STAMP_CLOSE_PASS) PEDP_STAMP_CLOSE(3, 4);
                if (K > 0.0) {
                    if (f.estimator == PEDP_POINT_TO_PLANE && lane_form) {
                        solve_i = 1;  // (wave 0 solves below, a row per lane)
                    } else if (f.estimator == PEDP_POINT_TO_PLANE) {
                        double A[36], nb[6];
                        int k = 0;
#pragma unroll
                        for (int u = 0; u < 6; ++u)
#pragma unroll
                            for (int v = u; v < 6; ++v) { A[6 * u + v] = pk[k]; A[6 * v + u] = pk[k]; ++k; }
#pragma unroll
                        for (int u = 0; u < 6; ++u) nb[u] = -pk[21 + u];
                        const bool ok = solve6_ldlt_reg(A, nb, x);
                        PEDP_STAMP_CLOSE(2, 1);
                        if (ok) {
                            if (wide) angles_i = 1;
                            else vec6_to_T(x, upd);
                        }
                        if (!wide) PEDP_STAMP_CLOSE(2, 2);
                    } else {
                        const double *c = st->centroid;
                        double ms[3], mt[3], sig[9];
                        for (int u = 0; u < 3; ++u) { ms[u] = pk[u] / K; mt[u] = pk[3 + u] / K; }
                        for (int u = 0; u < 3; ++u)
                            for (int v = 0; v < 3; ++v) sig[3 * u + v] = pk[6 + 3 * u + v] / K - mt[u] * ms[v];
                        double U[9], w[3], V[9];
                        svd3_dev(sig, U, w, V);
                        const double sgn = (det3_dev(U) * det3_dev(V) < 0.0) ? -1.0 : 1.0;
                        double R[9];
                        for (int u = 0; u < 3; ++u)
                            for (int v = 0; v < 3; ++v)
                                R[3 * u + v] = U[3 * u] * V[3 * v] + U[3 * u + 1] * V[3 * v + 1] + sgn * U[3 * u + 2] * V[3 * v + 2];
                        for (int u = 0; u < 3; ++u) {
                            for (int v = 0; v < 3; ++v) upd[4 * u + v] = R[3 * u + v];
                            const double msa[3] = {ms[0] + c[0], ms[1] + c[1], ms[2] + c[2]};
                            upd[4 * u + 3] = (mt[u] + c[u]) - (R[3 * u] * msa[0] + R[3 * u + 1] * msa[1] + R[3 * u + 2] * msa[2]);
                        }
                    }
                }
            }
        }
        if (wide) {  // (all 64 lanes of wave 0 are here: lane 0 is the first)
            stop_i = __builtin_amdgcn_readfirstlane(stop_i);
            angles_i = __builtin_amdgcn_readfirstlane(angles_i);
        }
        if (lane_form) {
            // "point-to-plane, K > 0, not stopping" is lane 0's finding, made wave-uniform.  The lanes read their entries of
            // the symmetric matrix out of the packet's upper triangle, and -b.
            solve_i = __builtin_amdgcn_readfirstlane(solve_i);
            if (solve_i) {
                const double *pk = L.pk;
                const bool ok = solve6_ldlt_lanes(
                    [pk](int a, int b) {
                        const int u = a < b ? a : b, v = a < b ? b : a;  // entry (u, v), u <= v, of the packed triangle
                        return pk[6 * u - u * (u - 1) / 2 + (v - u)];
                    },
                    [pk](int u) { return -pk[21 + u]; }, x, tid & 63);
                if (l0) {
                    PEDP_STAMP_CLOSE(2, 1);
                    st->n_lane = st->n_lane + 1;
                }
                if (ok) angles_i = 1;
            }
        }
        if (!stop_i) {
            if (wide) {
                if (angles_i) {  // wave-uniform
                    if (!lane_form) {  // (the lane solve's x is the same in every lane as it comes)
#pragma unroll
                        for (int k = 0; k < 6; ++k) x[k] = bcast0(x[k]);
                    }
                    double s, c;
                    sincos(tid == 0 ? x[0] : (tid == 1 ? x[1] : x[2]), &s, &c);  // one angle per lane
                    const double sa = __shfl(s, 0, 64), ca = __shfl(c, 0, 64), sb = __shfl(s, 1, 64), cb = __shfl(c, 1, 64),
                                 sc = __shfl(s, 2, 64), cc = __shfl(c, 2, 64);
                    sincos_to_T(sa, ca, sb, cb, sc, cc, x, upd);
                    if (l0) PEDP_STAMP_CLOSE(2, 2);
                } else {
#pragma unroll
                    for (int k = 0; k < 16; ++k) upd[k] = bcast0(upd[k]);
                }
                if (l0) PEDP_STAMP_CLOSE(0, 2);
                if (l0 && pass == PEDP_ICP_STAMP_CLOSE_PASS) PEDP_STAMP_CLOSE(3, 5);
                // lane k = 4 i + j holds entry (i, j) of the update and of upd x T0 (mat4_mul_dev's sum) and stores both
                const int i = (tid >> 2) & 3, j = tid & 3;
                double tn = 0.0, u_ij = 0.0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double a = i == 0 ? upd[k] : (i == 1 ? upd[4 + k] : (i == 2 ? upd[8 + k] : upd[12 + k]));
                    const double b = L.t0[4 * k + j];
                    tn += a * b;
                    u_ij = j == k ? a : u_ij;
                }
                if (tid < 16) {
                    st->upd[tid] = u_ij;
                    if (!HEAD) as_global(f.hist)[16 * (pass + 1) + tid] = u_ij;
                    st->T[tid] = tn;
                }
            } else {
                PEDP_STAMP_CLOSE(0, 2);
                if (pass == PEDP_ICP_STAMP_CLOSE_PASS) PEDP_STAMP_CLOSE(3, 5);
                for (int k = 0; k < 16; ++k) { st->upd[k] = upd[k]; if (!HEAD) as_global(f.hist)[16 * (pass + 1) + k] = upd[k]; }
                double Tn[16];
                mat4_mul_dev(upd, L.t0, Tn);
                for (int k = 0; k < 16; ++k) st->T[k] = Tn[k];
            }
            if (l0) {
                // how far this update can move a point near the target: |R - I|_F (>= the spectral norm) and
                // |t + (R - I) c| about the box centre c
                double th2 = 0.0, tv[3];
                for (int u = 0; u < 3; ++u) {
                    tv[u] = upd[4 * u + 3];
                    const double cc[3] = {f.bcx, f.bcy, f.bcz};
                    for (int v = 0; v < 3; ++v) {
                        const double dlt = upd[4 * u + v] - (u == v ? 1.0 : 0.0);
                        th2 += dlt * dlt;
                        tv[u] += dlt * cc[v];
                    }
                }
                double mu_th = mu_th0 + sqrt(th2), mu_ta = mu_ta0 + sqrt(tv[0] * tv[0] + tv[1] * tv[1] + tv[2] * tv[2]);
                const double mu = mu_th * reachE + mu_ta;
                if (!(mu < 0.95 * margin)) {  // also when mu is NaN
                    L.do_rebuild = 1;
                    mu_th = 0.0;
                    mu_ta = 0.0;
                    st->n_rebuilds += 1;
                }
                st->mu_theta = mu_th;
                st->mu_tau = mu_ta;
                st->rebuild = L.do_rebuild;
                st->pass = pass + 1;
                PEDP_STAMP_CLOSE(2, 3);
                if (pass == PEDP_ICP_STAMP_CLOSE_PASS) PEDP_STAMP_CLOSE(3, 6);
            }
        }
        if (l0) PEDP_STAMP_CLOSE(0, 3);
    }
    __syncthreads();
    if (!HEAD && !f.gen_masks && L.do_rebuild)  // the next pass lists the live chunks anew; it resets what the old ones leave behind
        for (int wi = tid; wi < f.n_lw; wi += NT) { as_global(f.live_old)[wi] = load_live<COHERENT>(&f.live[wi]); as_global(f.live)[wi] = 0ull; }
    if (!HEAD && f.gen_masks && f.known && f.k_rebuild)  // this rebuild pass is over (all have signed off): the next one ORs into the other mask
        for (int wi = tid; wi < f.n_lw; wi += NT) as_global(f.live_old)[wi] = 0ull;
    // The registration ends here: its final state goes straight into the executor's page-locked block (read past this
    // CU's L1: lane 0's stores have reached L2, see above), so that no copy follows the last pass.
    if (!LOCAL && COHERENT && f.down && L.stopped)
        for (int i = tid; i < (int)(sizeof(IcpState) / sizeof(double)); i += NT) ((double *)f.down)[i] = load_sc1((const double *)st + i);
}

__global__ __launch_bounds__(FIN_THREADS) void icp_finish_kernel(IcpState *st, unsigned long long *live, int32_t *live_list,
                                                         int n_lw, const double *partials, double *packet, int phase, int estimator,
                                                         double *__restrict__ trace, double *__restrict__ hist,
                                                         double bcx, double bcy, double bcz, size_t pose_stride, int serial, int lane) {
    {   // pose b = blockIdx.x of a batch: its state and buffers are b * pose_stride bytes behind pose 0's
        const size_t off = (size_t)blockIdx.x * pose_stride;
        st = pose_ptr(st, off); live = pose_ptr(live, off); live_list = pose_ptr(live_list, off);
        partials = pose_ptr(partials, off); packet = pose_ptr(packet, off); hist = pose_ptr(hist, off);
    }
    if (st->done) return;
    __shared__ FinishLds<FIN_THREADS, LIVE_CAP> L;
    FinishArgs f;
    f.live = live; f.live_list = live_list; f.n_lw = n_lw; f.partials = partials; f.packet = packet; f.phase = phase;
    f.estimator = estimator; f.trace = trace; f.hist = hist; f.bcx = bcx; f.bcy = bcy; f.bcz = bcz;
    f.serial = serial; f.lane = lane; f.live_old = live + n_lw;
    icp_finish_body<FIN_THREADS, LIVE_CAP, false>(st, f, L, threadIdx.x);
}

// Both forms of the close's solve on systems of the caller's (pedp_debug_solve6): the row-per-lane form, a wave per
// system, and the one-lane form, a thread per system.
__global__ __launch_bounds__(256) void solve6_lanes_debug_kernel(const double *__restrict__ A, const double *__restrict__ b, int64_t n,
                                                                 double *__restrict__ x_out, int32_t *__restrict__ ok_out) {
    const int lane = threadIdx.x & 63;
    const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= n) return;  // (wave-uniform)
    double x[6];
    const double *As = A + 36 * s, *bs = b + 6 * s;
    const bool ok = solve6_ldlt_lanes([As](int u, int v) { return As[6 * u + v]; }, [bs](int u) { return bs[u]; }, x, lane);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) x_out[6 * s + k] = x[k];
        ok_out[s] = ok ? 1 : 0;
    }
}
// (one thread per system and per WAVE: solve6_ldlt_reg counts on being its wave's only active lane)
__global__ __launch_bounds__(256) void solve6_one_debug_kernel(const double *__restrict__ A, const double *__restrict__ b, int64_t n,
                                                               double *__restrict__ x_out, int32_t *__restrict__ ok_out) {
    const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= n || (threadIdx.x & 63) != 0) return;
    double x[6];
    const bool ok = solve6_ldlt_reg(A + 36 * s, b + 6 * s, x);
#pragma unroll
    for (int k = 0; k < 6; ++k) x_out[6 * s + k] = x[k];
    ok_out[s] = ok ? 1 : 0;
}

}  // namespace
