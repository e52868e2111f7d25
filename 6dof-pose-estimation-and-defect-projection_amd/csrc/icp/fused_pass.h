// ICP, fused pass: one launch per correspondence pass (icp_pass_kernel), and the three kernels that move
// registration states into and out of the workspace.
#pragma once
#include "fused_close.h"
#include "segmented_sweep.h"

namespace {

// ------------------------------------------------------------------ pass
constexpr int WTL = 1024;        // tiles a wave lists before it sweeps them
constexpr int L2_WORDS = 8;      // mask words whose tile spheres a wave requests at once
constexpr int SW_G = 8;          // tiles per group of the sweep (A fragments fetched one group ahead)

// exact float64 scan of the rows of the tiles in `near` (one bit per lane's tile), 64 rows per trip
// (icp_steady_kernel has a copy of this loop that also tracks the second-smallest d^2: keep the two alike)
__device__ __forceinline__ void scan_near_tiles(unsigned long long near, int unit_of_lane, const PassArgs &a, double qx,
                                                double qy, double qz, int lane, double &bd, int &bj) {
    while (near != 0ull) {  // wave-uniform: 64 lanes = 64 rows = 4 tiles per trip
        int unit = -1;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            if (near != 0ull) {
                const int bit = __builtin_ctzll(near);
                near &= near - 1ull;
                const int u = __shfl(unit_of_lane, bit, 64);
                if (g == (lane >> 4)) unit = u;
            }
        }
        const int64_t row = (int64_t)unit * 16 + (lane & 15);
        if (unit >= 0 && row < a.Nt)
            lexmin(bd, bj, dist2(qx, qy, qz, as_global(a.tgt_s)[6 * row], as_global(a.tgt_s)[6 * row + 1], as_global(a.tgt_s)[6 * row + 2]), as_global(a.tperm)[row]);
    }
}

// Butterfly partner inside a row of 16 lanes by DPP -- a modifier on a move, no round trip through the LDS
// crossbar like ds_bpermute.  LEVEL 0: lane ^ 1, 1: lane ^ 2 (quad permutes); 2, 3: lane 7 - i of the half row /
// 15 - i of the row, i.e. SOME lane of the partner's group: in a symmetric reduction every lane of that group
// holds what the partner holds once the lower levels are done, so the result is the xor butterfly's, bit for bit.
template <int LEVEL>
__device__ __forceinline__ int row_partner(int v) {
    constexpr int ctrl = LEVEL == 0 ? 0xB1 : (LEVEL == 1 ? 0x4E : (LEVEL == 2 ? 0x141 : 0x140));
    return __builtin_amdgcn_update_dpp(v, v, ctrl, 0xF, 0xF, false);
}
template <int LEVEL>
__device__ __forceinline__ float row_partner(float v) { return __int_as_float(row_partner<LEVEL>(__float_as_int(v))); }
template <int LEVEL>
__device__ __forceinline__ double row_partner(double v) {
    return __hiloint2double(row_partner<LEVEL>(__double2hiint(v)), row_partner<LEVEL>(__double2loint(v)));
}
template <int LEVEL>
__device__ __forceinline__ double row_sum_step(double v) { return v + row_partner<LEVEL>(v); }

// The MFMA loop of one wave over the n tiles of its LDS list against ITS sub-block (B operand b):
// per lane -- slot lane & 15, target rows 4 (lane >> 4) .. + 3 of every tile -- the two best tiles
// (value, tile) and the third-best value.  One MFMA per tile; the A fragments of the next SW_G tiles
// are requested before this group's MFMAs are issued (as GLOBAL loads: while they were flat, every LDS
// read of a list entry waited for them).  SW_PAD pad tiles (rows that never win) follow the
// list's last entry.  (Three groups in flight with the winners kept as list positions measured slower:
// 0.738 against 0.714 ms per registration, round 4.)
constexpr int SW_PAD = 2 * SW_G;
__device__ __forceinline__ void sweep_sub_block(const unsigned *__restrict__ list, int n, const PEDP_GLOBAL float *__restrict__ tgtf,
                                                int frag, float b, float &b1, int &t1, float &b2, int &t2, float &b3) {
    if (n <= 0) return;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    float a[SW_G];
    unsigned un[SW_G];
#pragma unroll
    for (int g = 0; g < SW_G; ++g) {
        un[g] = list[g];
        a[g] = tgtf[(size_t)un[g] * 64 + frag];
    }
    for (int k = 0; k < n; k += SW_G) {
        float an[SW_G];
        unsigned unn[SW_G];
#pragma unroll
        for (int g = 0; g < SW_G; ++g) {
            unn[g] = list[k + SW_G + g];  // pad tiles follow the last real one
            an[g] = tgtf[(size_t)unn[g] * 64 + frag];
        }
        f32x4 acc[SW_G];
#pragma unroll
        for (int g = 0; g < SW_G; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g], b, zero, 0, 0, 0);
#pragma unroll
        for (int g = 0; g < SW_G; ++g) {
            const float v = fminf(fminf(fminf(acc[g][0], acc[g][1]), acc[g][2]), acc[g][3]);
            const int tile = (int)un[g];
            const bool lt1 = v < b1, lt2 = v < b2;
            t2 = lt1 ? t1 : (lt2 ? tile : t2);
            t1 = lt1 ? tile : t1;
            b3 = __builtin_amdgcn_fmed3f(b2, b3, v);  // b2 <= b3: the third smallest of the four
            b2 = __builtin_amdgcn_fmed3f(b1, b2, v);  // b1 <= b2
            b1 = fminf(b1, v);
        }
#pragma unroll
        for (int g = 0; g < SW_G; ++g) { a[g] = an[g]; un[g] = unn[g]; }
    }
}

// BATCH: the launch carries several poses (grid.y); a separate instantiation, so that a kernel
// trace tells the single registration's launches from a batch's
// LANES: the close solves its 6x6 system a row per lane (solve_lanes.h) and is the wide close -- the host launches this
// instantiation only where neither PEDP_ICP_LANE_SOLVE=0 nor PEDP_ICP_SERIAL_CLOSE=1 is set, so the one-lane solve and its
// 72 registers of matrix are not in the kernel at all; the other instantiation is the kernel as it was.
template <int W, bool BATCH, bool LANES>
__global__ __launch_bounds__(W * 64, 4) void icp_pass_kernel(IcpState *st0, const PassArgs a0) {
    static_assert(W == 8 && CH == 128, "a chunk is two halves of four 16-slot sub-blocks");
    const size_t pose_off = BATCH ? (size_t)blockIdx.y * a0.pose_stride : 0;
    IcpState *st = pose_ptr(st0, pose_off);
    // A single registration works on a copy of its state in LDS (one 8-byte word per thread, requested with everything
    // else at entry): what a pass reads of it comes from there, a close writes it there, and the closing workgroup --
    // or, behind a head close, the service workgroup -- stores it as one block.  A batch reads its pose's state in memory.
    __shared__ IcpState cur;
    typedef double __attribute__((may_alias)) state_word;
    constexpr int SWORDS = (int)(sizeof(IcpState) / sizeof(double));
#define PEDP_ST (*(BATCH ? st : &cur))
    // The argument block (with this pose's pointers) is parked in LDS and read from there where it is
    // used: held in scalar registers for the whole kernel its 40-odd fields overflow the SGPR file,
    // and the spills -- executed at entry by EVERY launched workgroup -- left tens of MB of dirty
    // scratch for the kernel boundary to write back.
    __shared__ PassArgs sa;
    __shared__ FinishLds<W * 64, 2048> fin;
    // a wave's slots (its sub-block): written and read by that wave only
    __shared__ double wp[W][3][16], accsh[W][PSTRIDE];
    __shared__ float wcs[W][3][16], weps[W][16], wS[W][16], wrho[W][16];
    __shared__ int wpi[W][16], wkk[W][16], misc[8];
    __shared__ unsigned wtl[W][WTL + SW_PAD];
    __shared__ float4 wnode[W][16], wsph0[64];
    __shared__ double rbs[16];  // rebuild passes: the pose so far (3 x 4), its norm bound, the reach
    __shared__ float wnode_r[W][16];
    // certificates (single registration): per slot, the bound carried over (certified: the search is not needed),
    // the neighbour it keeps and its squared distance
    __shared__ float wcert[BATCH ? 1 : W][16];
    __shared__ int wfj[BATCH ? 1 : W][16];
    __shared__ double wfd[BATCH ? 1 : W][16];
    if (threadIdx.x == 0) {
        PassArgs t = a0;
        t.Pk = pose_ptr(a0.Pk, pose_off); t.Tprev = pose_ptr(a0.Tprev, pose_off); t.live = pose_ptr(a0.live, pose_off);
        t.live_list = pose_ptr(a0.live_list, pose_off); t.hist = pose_ptr(a0.hist, pose_off);
        t.idx_out = pose_ptr(a0.idx_out, pose_off); t.partials = pose_ptr(a0.partials, pose_off);
        t.packet = pose_ptr(a0.packet, pose_off); t.ticket = pose_ptr(a0.ticket, pose_off);
        sa = t;
    }
    const PassArgs &a = sa;
#if PEDP_ICP_STAMPS
    const long long rt_entry = (long long)__builtin_amdgcn_s_memrealtime();
#endif
    // the first unit's live-list entry is requested together with the state (the list has one entry
    // per chunk, so the index is always inside it; the value is used only when it is valid)
    int chunk_next = pose_ptr(a0.live_list, pose_off)[blockIdx.x < (unsigned)a0.n_chunks ? blockIdx.x : 0];
    // both parities of this workgroup's entry of the visit plan, requested before the pass number is known
    typedef int v4i __attribute__((ext_vector_type(4)));
    v4i vis0 = {0, 0, 0, 0}, vis1 = {0, 0, 0, 0};
    if (!BATCH && a0.visit && blockIdx.x < (unsigned)a0.visit_cap) {
        vis0 = ((const v4i *)a0.visit)[blockIdx.x];
        vis1 = ((const v4i *)a0.visit)[(size_t)a0.visit_cap + blockIdx.x];
    }
    // word spheres do not depend on the chunk: the first 64 are requested before anything else and parked in LDS
    if (threadIdx.x < 64) wsph0[threadIdx.x] = a0.word_sph[(int)threadIdx.x < a0.n_words ? threadIdx.x : 0];
    // Head close: launch L asks for both state slots and decides from their fields alone.  Slot (L - 1) & 1 holds pass
    // L - 1, not done and left open (no rebuild pass, not the last): close it here, then run pass L.  Else slot L & 1 holds
    // pass L: it was closed in the launch before (or this is pass 0) -- run the pass.  Else the registration is over.
    const bool head = !BATCH && a0.head != 0;
    bool close_here = false;
    if constexpr (!BATCH) {
        IcpState *sA = st0 + (head ? (a0.launch & 1) : 0), *sB = st0 + (head ? ((a0.launch + 1) & 1) : 0);
        double wA = 0.0, wB = 0.0;
        if (threadIdx.x < SWORDS) {
            wA = ((const state_word *)sA)[threadIdx.x];
            if (head) wB = ((const state_word *)sB)[threadIdx.x];
        }
        if (head) {
            // Slot (L - 1) & 1 is looked at FIRST: nobody writes it before every workgroup of this launch has read it (only
            // an in-launch closer of pass L does, behind all tickets and sign-offs).  Slot L & 1 is being rewritten by the
            // service workgroup while a workgroup that starts late reads it -- so it counts only where no head close happens.
            if (a0.launch > 0 && sB->pass == a0.launch - 1 && sB->done == 0 && sB->rebuild == 0 && sB->pass < sB->max_iter) close_here = true;
            else if (sA->pass != a0.launch || sA->done) return;
        } else if (sA->done) return;
        if (threadIdx.x < SWORDS) ((state_word *)&cur)[threadIdx.x] = close_here ? wB : wA;
        __syncthreads();  // the state (and the argument block) is in LDS
    } else {
        if (st->done) return;
    }
    if (close_here) {
        // ---- the close of pass L - 1, by every workgroup of launch L: same inputs, same float64 sequence, same bits.
        // Plain loads: the launch boundary made the partial sums visible.  The new state stays in LDS.
        FinishArgs f;
        f.live = nullptr; f.live_list = nullptr; f.n_lw = 0; f.partials = a0.partials + (size_t)((a0.launch - 1) & 1) * a0.part_stride; f.packet = nullptr; f.phase = 0;
        f.estimator = a0.estimator; f.trace = nullptr; f.hist = nullptr; f.bcx = a0.bc[0]; f.bcy = a0.bc[1]; f.bcz = a0.bc[2];
        f.serial = 0; f.lane = LANES ? 1 : 0;
        f.known = 1; f.k_pass = a0.launch - 1; f.k_rebuild = 0; f.k_n_live = cur.n_live;
        icp_finish_body<W * 64, 2048, false, 2>(&cur, f, fin, threadIdx.x);  // (ends behind a barrier: U and the new state are published)
        PEDP_RT(a0.launch, 7);
    }
    // (what comes out of LDS is made scalar again: these live through the whole kernel)
    auto uni = [](int v) { return BATCH ? v : __builtin_amdgcn_readfirstlane(v); };
    auto unid = [](double v) { return BATCH ? v : bcast0(v); };
    auto unif = [](float v) { return BATCH ? v : __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); };
    const bool rebuild = uni(PEDP_ST.rebuild) != 0;
    const int n_live = uni(PEDP_ST.n_live), pass = uni(PEDP_ST.pass);
    const unsigned ticket_base = (unsigned)uni((int)PEDP_ST.ticket_base);
    const v4i vis = (pass & 1) ? vis1 : vis0;
    const int tag_now = uni(PEDP_ST.nonce) + pass + 1;  // (a registration runs well under 65,535 passes; beyond that no plan is made)
    bool planned = !BATCH && !rebuild && vis[2] == tag_now && vis[3] == n_live;  // (all workgroups with a chunk agree: the plan is written whole)
    // a pass left open: no ticket, no sign-off, no close in this launch
    const bool stopped_here = close_here && uni(PEDP_ST.done) != 0;  // the head close ended the registration
    const bool open = head && !rebuild && pass < uni(PEDP_ST.max_iter) && !stopped_here;
    const int gdim = (int)gridDim.x - (head ? 1 : 0);  // workgroups the chunks are dealt to
    // rebuild g ORs into live mask g & 1 and reads "was live" from the other (head close); else: the mask, and the copy made aside
    const int mask_gen = head ? (uni(PEDP_ST.n_rebuilds) & 1) : 0;
#define PEDP_MASK_CUR (sa.live + (size_t)mask_gen * sa.n_lw)
#define PEDP_MASK_OLD (sa.live + (size_t)(mask_gen ^ 1) * sa.n_lw)
    // Workgroups with chunks take a ticket when they are through; the one that draws the last closes the
    // pass.  The others leave at once -- but sign off first (a counter of sixteen, each on a line of its own:
    // hundreds of atomics on one word in the first microsecond held up everybody's loads), and the closing
    // workgroup rewrites the state only after all of them have: a batch's grid is not resident at once, a
    // workgroup that starts late must not find the next pass's state.
    int n_wg = rebuild ? a0.n_chunks : n_live;
    n_wg = n_wg < gdim ? n_wg : gdim;
    n_wg = n_wg < 1 ? 1 : n_wg;  // (no live chunk at all: workgroup 0 still closes the pass)
    // The plan of the pass after this one: the first workgroup through writes it (a pass closed in its launch), or the
    // service workgroup (a pass left open: nobody takes a ticket).  All of it, valid or void.
    auto write_next_plan = [&]() {
        typedef int v2i __attribute__((ext_vector_type(2)));
        const int tid = threadIdx.x, n_cu = sa.n_cu, extra = n_live - n_cu;
        PEDP_GLOBAL v4i *plan = (PEDP_GLOBAL v4i *)(uintptr_t)sa.visit + (size_t)((pass + 1) & 1) * sa.visit_cap;
        const bool want = !rebuild && pass < 65000 && extra > 0 && n_live <= 2 * n_cu && n_live <= gdim && n_live <= W * 64 && n_live <= sa.visit_cap;
        int d = 0x7FFFFFFF, mine_ok = 1;
        if (want && tid < n_live) {
            const v2i e = ((const PEDP_GLOBAL v2i *)(uintptr_t)sa.dur)[(size_t)((pass + 1) & 1) * sa.visit_cap + tid];  // pass - 1 wrote this copy
            mine_ok = e[1] == tag_now - 1;
            d = e[0];
        }
        const int chunk_of_rank = (want && tid < n_live) ? as_global(sa.live_list)[tid] : 0;
        if (__syncthreads_and(mine_ok) && want) {
            fin.scan[tid] = d;
            __syncthreads();
            if (tid < n_live) {
                int r = 0;  // rank of this chunk by (duration, live rank)
                for (int q = 0; q < n_live; ++q) {
                    const int dq = fin.scan[q];
                    r += (dq < d || (dq == d && q < tid)) ? 1 : 0;
                }
                const int pos = r < extra ? r : (r < 2 * extra ? n_cu + (2 * extra - 1 - r) : r - extra);
                const v4i e = {tid, chunk_of_rank, tag_now + 1, n_live};
                plan[pos] = e;
            }
        } else {
            const v4i none = {0, 0, 0, 0};
            const int n = (int)gridDim.x < sa.visit_cap ? (int)gridDim.x : sa.visit_cap;
            for (int i = tid; i < n; i += W * 64) plan[i] = none;
        }
    };
    if (head) {
        // A planned pass is counted when its state is made: by the head close in front of it.  (A pass whose state an
        // in-launch close made follows a rebuild pass, or is one: never planned.)  The service workgroup has no entry
        // of its own in the plan: it looks at entry 0.
        const bool service = (int)blockIdx.x == n_wg;
        if (close_here && service && !rebuild && sa.visit && sa.visit_cap > 0) {
            const v4i e0 = ((const PEDP_GLOBAL v4i *)(uintptr_t)sa.visit)[(size_t)(pass & 1) * sa.visit_cap];
            planned = e0[2] == tag_now && e0[3] == n_live;
        }
        if (close_here && planned && !stopped_here && threadIdx.x == 0) cur.n_planned += 1;
        if (service) {
            // ---- the service workgroup: the first without a chunk.  What the head close leaves behind: the state
            // into its slot (the final one into the page-locked block too), the row of the trace, the history slot,
            // the packet, and the plan of the next pass.
            __syncthreads();
            const int tid = threadIdx.x;
            if (close_here) {
                const int prev = a0.launch - 1;
                const bool stopped = cur.done != 0;
                if (tid < SWORDS) {
                    const double wd = ((const state_word *)&cur)[tid];
                    ((PEDP_GLOBAL state_word *)(uintptr_t)(st0 + (a0.launch & 1)))[tid] = wd;
                    if (stopped && sa.down) ((state_word *)sa.down)[tid] = wd;
                }
                if (sa.trace && tid < 18)
                    as_global(sa.trace)[18 * prev + tid] = tid == 0 ? cur.fitness : (tid == 1 ? cur.rmse : fin.t0[tid >= 2 ? tid - 2 : 0]);
                if (!stopped && tid < 16) as_global(sa.hist)[16 * (prev + 1) + tid] = cur.upd[tid];
                if (open && tid < PACKET) as_global(sa.packet)[tid] = fin.pk[tid];  // (the closer of this launch's pass writes its own)
            }
            if (open && sa.visit) write_next_plan();
        }
        if (stopped_here) return;  // the head close ended the registration: nobody runs a pass
    }
    if ((int)blockIdx.x >= n_wg) {
        if (open) return;
        if (a0.fuse && threadIdx.x == 0)
            __hip_atomic_fetch_add((g_u32 *)(uintptr_t)(pose_ptr(a0.ticket, pose_off) + 32 * (1 + (blockIdx.x & 15))), 1u, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
#if PEDP_ICP_STAMPS
    if (threadIdx.x == 0 && pass < 32 && blockIdx.x < 512 && blockIdx.y == 0) g_icp_rt[pass][blockIdx.x][0] = rt_entry;
#endif
    PEDP_RT(pass, 1);
    // certificates are kept by a single registration that closes its passes itself, and never by a rebuild pass
    // (its points are recomputed through the history; it writes certificates, the pass behind it reads them)
    const bool certify = !BATCH && a0.cert != nullptr;
    const float inf = __uint_as_float(0x7F800000u);
    const double dinf = __longlong_as_double(0x7FF0000000000000ll);
    const double dnan = __longlong_as_double(0x7FF8000000000000ll);
    // (a batch keeps these in scalar registers; a single registration reads them from the state in LDS where they are used)
    const double ccx_b = BATCH ? st->centroid[0] : 0.0, ccy_b = BATCH ? st->centroid[1] : 0.0, ccz_b = BATCH ? st->centroid[2] : 0.0;
    const float r_search_b = BATCH ? st->r_search : 0.f;
#define PEDP_CC(k, b) (BATCH ? (b) : bcast0(cur.centroid[k]))
    // A rebuild pass asks the chunks' bounding spheres first (8 of this workgroup's chunks per round, a lane per
    // run sphere, every wave for itself): a sphere moved by the pose so far that stays farther than r + margin
    // from the target's box holds no live point -- the chunk is not touched (only, if it was live before,
    // its points' correspondences are withdrawn).  The others are decided point by point as before.
    unsigned long long todo = 0ull;  // wave-uniform: chunks of the current round still to visit
    int todo_base = -8, it = 0;
#if PEDP_ICP_STAMPS
    bool rt_first = true;
#endif
    if (rebuild && threadIdx.x == 0) {
        double Rs[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) { Rs[k] = PEDP_ST.T[k]; rbs[k] = Rs[k]; }
        // |R x| <= rscale |x|: the square root of the largest row sum of |R^T R| bounds the spectral norm
        double m = 0.0;
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            double row = 0.0;
#pragma unroll
            for (int v = 0; v < 3; ++v) row += fabs(Rs[u] * Rs[v] + Rs[4 + u] * Rs[4 + v] + Rs[8 + u] * Rs[8 + v]);
            m = row > m ? row : m;
        }
        rbs[12] = sqrt(m) * (1.0 + 1e-9);
        rbs[13] = sqrt(PEDP_ST.r2live) * (1.0 + 1e-9);
    }
    __syncthreads();  // the argument block, the word spheres (and the rebuild constants) are in LDS
    for (;;) {
        // The thread index is made opaque per chunk: everything derived from it (LDS addresses, lane
        // masks, role predicates) is then computed where it is used instead of being hoisted out of
        // this loop and kept alive -- spilled -- through every phase.
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        const int lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
        const int half = wv >> 2, q4 = wv & 3;   // the wave's half of the chunk (64 points), its quarter of the half's slots
        const int j = lane & 15, g = lane >> 4;  // MFMA layout: slot of the sub-block, row group / component
        const int frag = j * 4 + g;              // float offset inside a 16-point target tile
        const unsigned long long lt = (1ull << lane) - 1ull;
        // a rebuild pass visits chunks (unit = chunk id), other passes the live list (unit = rank);
        // `unit` also indexes the chunk's partial sums (see icp_finish_body)
        const PEDP_GLOBAL double *Pk_in = as_global(a.Pk) + (size_t)(pass & 1) * a.pp_stride, *Tp_in = as_global(a.Tprev) + (size_t)(pass & 1) * a.pp_stride;
        PEDP_GLOBAL double *Pk_out = as_global(a.Pk) + (size_t)((pass + 1) & 1) * a.pp_stride, *Tp_out = as_global(a.Tprev) + (size_t)((pass + 1) & 1) * a.pp_stride;
        int chunk, unit;
        if (rebuild) {
            bool more = true;
            while (todo == 0ull) {  // wave-uniform
                // A round decides eight chunks: lane 8 c + s takes run sphere s of the round's c-th chunk, and its 32 bytes
                // and the old mask's word are requested before anything is looked at -- one round trip per round.  (A lane
                // per chunk that walked the eight spheres, each behind a branch on its radius, was sixteen.)
                todo_base += 8;
                if ((long long)blockIdx.x + (long long)todo_base * (long long)gdim >= (long long)a.n_chunks) { more = false; break; }
                const long long u = (long long)blockIdx.x + (long long)(todo_base + (lane >> 3)) * (long long)gdim;
                const bool inside = u < (long long)a.n_chunks;
                const long long uc = inside ? u : 0;  // (a lane without a chunk reads chunk 0's sphere and uses nothing of it)
                typedef double v2d __attribute__((ext_vector_type(2)));
                const PEDP_GLOBAL v2d *sp8 = (const PEDP_GLOBAL v2d *)(uintptr_t)(a.chunk_sph + (size_t)(8 * uc + (lane & 7)) * 4);
                const v2d sxy = sp8[0], szr = sp8[1];
                const unsigned long long old_word = as_global(PEDP_MASK_OLD)[uc >> 6];
                bool near_box;
                {
                    double Rs[12];
#pragma unroll
                    for (int k = 0; k < 12; ++k) Rs[k] = rbs[k];
                    const double rscale = rbs[12], reach = rbs[13];
                    const double cx = sxy[0], cy = sxy[1], cz = szr[0], cr = szr[1];
                    const double tx = Rs[0] * cx + Rs[1] * cy + Rs[2] * cz + Rs[3], ty = Rs[4] * cx + Rs[5] * cy + Rs[6] * cz + Rs[7],
                                 tz = Rs[8] * cx + Rs[9] * cy + Rs[10] * cz + Rs[11];
                    // (box_dist2 of slot_math.h, written out: the call moved instructions of this kernel)
                    const double ex = fmax(fmax(a.lo[0] - tx, tx - a.hi[0]), 0.0), ey = fmax(fmax(a.lo[1] - ty, ty - a.hi[1]), 0.0),
                                 ez = fmax(fmax(a.lo[2] - tz, tz - a.hi[2]), 0.0);
                    const double lim = cr * rscale + reach + 1e-9 * (fabs(tx) + fabs(ty) + fabs(tz) + 1.0);
                    // (the sentinel is looked at LAST: with it in front the compiler requests the centre only behind its test, a second
                    // round trip.  Also when anything is NaN.)
                    near_box = inside && !(ex * ex + ey * ey + ez * ez > lim * lim) && !(cr < 0.0);
                }
                // a chunk is visited where any of its eight spheres says so; chunk c's bit of `todo` and `wd` is bit 8 c
                const unsigned long long nb = __builtin_amdgcn_ballot_w64(near_box);
                const bool visit = ((nb >> (lane & 56)) & 0xFFull) != 0ull;
                const bool was_live = (old_word >> (uc & 63)) & 1ull;
                const bool withdraw = inside && !visit && (was_live || pass == 0);  // pass 0: every chunk's correspondences start at "none"
                todo = __builtin_amdgcn_ballot_w64(visit && (lane & 7) == 0);
                const unsigned long long wd = __builtin_amdgcn_ballot_w64(withdraw && (lane & 7) == 0);
                if (wd != 0ull) {  // pass 0: most chunks; later: a chunk that was live and no longer is
                    // Withdrawals, four chunks at a time over the workgroup's eight waves (every wave runs the rounds for itself
                    // and finds the same `wd`): wave w takes half w & 1 of the (w >> 1)-th and the (4 + (w >> 1))-th chunk to
                    // withdraw, and both entries of the order are requested before the first store.
                    int64_t kq[2];
                    int pq[2];
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        unsigned long long rest = wd;
                        for (int s = 0; s < 4 * q + (wv >> 1); ++s) rest &= rest - 1ull;  // (wave-uniform)
                        kq[q] = rest != 0ull ? ((int64_t)blockIdx.x + (int64_t)(todo_base + (__builtin_ctzll(rest) >> 3)) * gdim) * CH + (tid & (CH - 1))
                                             : a.N;
                        pq[q] = kq[q] < a.N ? as_global(a.perm)[kq[q]] : 0;
                    }
#pragma unroll
                    for (int q = 0; q < 2; ++q)
                        if (kq[q] < a.N) as_global(a.idx_out)[pq[q]] = -1;
                }
            }
            if (!more) break;
            const int i = __builtin_ctzll(todo) >> 3;
            todo &= todo - 1ull;
            unit = (int)(blockIdx.x + (unsigned)(todo_base + i) * (unsigned)gdim);
            chunk = unit;
        } else {
            unit = (int)(blockIdx.x + (unsigned)it * (unsigned)gdim);
            ++it;
            if (unit >= n_live) break;
            if (planned && it == 1) { unit = vis[0]; chunk = vis[1]; }
            else chunk = unit == (int)blockIdx.x ? chunk_next : as_global(a.live_list)[unit];
        }
        long long t_chunk0 = 0;
        if (!BATCH && !rebuild) t_chunk0 = (long long)__builtin_amdgcn_s_memtime();
        if (tid == 0) PEDP_STAMP(1, blockIdx.x, 0);
#if PEDP_ICP_STAMPS
        // the workgroup's FIRST chunk on the device-wide clock (slot 5 is the head close's otherwise: a launch has one or the other)
        if (!close_here && rt_first) PEDP_RT(pass, 5);
        rt_first = false;
#endif
        PEDP_WV(0, __builtin_amdgcn_s_memtime());
        PEDP_WV(9, pass);
        PEDP_WV(10, __builtin_amdgcn_s_memrealtime());
        PEDP_WV(12, ((long long)__builtin_amdgcn_s_getreg(63508) << 32) | (unsigned)__builtin_amdgcn_s_getreg(63492));  // XCC_ID, HW_ID
        // ---- 1. every wave transforms the 64 points of its half (the four waves of a half do the same
        // arithmetic and get the same ballots; quarter 0 stores), box test, compaction of the candidates:
        // the half's candidates in ascending position take the half's slots 0.., the wave keeps those
        // whose rank falls into its quarter
        int nsl;  // real slots of this wave's sub-block
        bool skip = false;  // wave-uniform: every one of them is certified
        {
            bool cand = false, near = false, certd = false;
            int pi = -1, jprev = -1;
            float c_new = 0.f;
            double x = 0.0, y = 0.0, z = 0.0, dprev = dnan, d2prev = dnan;
            const int64_t k = (int64_t)chunk * CH + half * 64 + lane;
            const bool valid = k < a.N;
            if (valid) {
                pi = as_global(a.perm)[k];
                if (rebuild) {
                    x = as_global(a.src)[3 * (int64_t)pi]; y = as_global(a.src)[3 * (int64_t)pi + 1]; z = as_global(a.src)[3 * (int64_t)pi + 2];
                    xform(PEDP_ST.T_init, x, y, z);
                    // (behind a head close the last step is not in the history yet: it is the update in LDS)
                    for (int q = 1; q <= (close_here ? pass - 1 : pass); ++q) xform_g(as_global(a.hist) + 16 * q, x, y, z);
                    if (close_here) xform(PEDP_ST.upd, x, y, z);
                    // a chunk that was live in the pass before has that pass's neighbours (every point of a live
                    // chunk gets one, or NaN): the search radii need not start from r again
                    if ((as_global(PEDP_MASK_OLD)[chunk >> 6] >> (chunk & 63)) & 1ull)
                        dprev = sqrt(dist2(x, y, z, Tp_in[3 * k], Tp_in[3 * k + 1], Tp_in[3 * k + 2]));
                } else {
                    x = Pk_in[3 * k]; y = Pk_in[3 * k + 1]; z = Pk_in[3 * k + 2];
                    const double ux = Tp_in[3 * k], uy = Tp_in[3 * k + 1], uz = Tp_in[3 * k + 2];
                    float c_in = 0.f;
                    if constexpr (!BATCH) {
                        if (certify) {
                            c_in = (as_global(a.cert) + (size_t)(pass & 1) * a.cert_stride)[k];
                            jprev = as_global(a.idx_out)[pi];  // (rewritten in this pass by the slot's own wave only, behind this read)
                        }
                    }
                    const double x0 = x, y0 = y, z0 = z;
                    xform(PEDP_ST.upd, x, y, z);
                    // Temporal coherence: last pass's neighbour is still a target point, so the new nearest
                    // neighbour is no farther than it is now.  NaN (no neighbour last pass) fails the
                    // comparison below and leaves the full radius.
                    d2prev = dist2(x, y, z, ux, uy, uz);
                    dprev = sqrt(d2prev);
                    if constexpr (!BATCH) {
                        if (certify) {
                            // the certificate, less the point's motion m: does last pass's neighbour stay proven?  (slot_math.h)
                            const double m = sqrt(dist2(x, y, z, x0, y0, z0));
                            c_new = cert_moved(c_in, m);
                            const bool fin = cert_finite(d2prev, m, c_new);
                            certd = fin && jprev >= 0 && c_new > 0.f && cert_inside(dprev, c_new);
                            if (!certd) c_new = 0.f;
                        }
                    }
                }
                const double d2box = box_dist2(x, y, z, a.lo, a.hi);
                cand = d2box <= unid(PEDP_ST.r2cut);   // r2cut = r^2 (1 + 1e-12): rounding-safe
                near = d2box <= unid(PEDP_ST.r2live);
            }
            const unsigned long long mc = __builtin_amdgcn_ballot_w64(cand), mn = __builtin_amdgcn_ballot_w64(near);
            const int wc = __builtin_popcountll(mc);
            if (q4 == 0) {  // (the other copy: a wave of this half that comes late still reads this pass's inputs)
                if (lane == 0) misc[half] = mn != 0ull;
                if (valid) {  // (a rebuild pass stores every visited chunk's coordinates; only the live ones are read again)
                    if (!cand) { as_global(a.idx_out)[pi] = -1; store_nan(&Tp_out[3 * k]); }
                    if constexpr (!BATCH) {
                        if (certify && !cand) (as_global(a.cert) + (size_t)((pass + 1) & 1) * a.cert_stride)[k] = 0.f;
                    }
                    Pk_out[3 * k] = x; Pk_out[3 * k + 1] = y; Pk_out[3 * k + 2] = z;
                }
            }
            const int sl = __builtin_popcountll(mc & lt) - 16 * q4;
            if constexpr (!BATCH) {
                // (a) a wave whose slots are all certified has nothing to search for
                if (certify) {  // wave-uniform
                    const bool mine = cand && sl >= 0 && sl < 16;
                    skip = __builtin_amdgcn_ballot_w64(mine && !certd) == 0ull;
                    if (mine) { wcert[wv][sl] = c_new; wfj[wv][sl] = jprev; wfd[wv][sl] = d2prev; }
                }
            }
            if (cand && sl >= 0 && sl < 16) {
                const float sx = (float)(x - PEDP_CC(0, ccx_b)), sy = (float)(y - PEDP_CC(1, ccy_b)), sz = (float)(z - PEDP_CC(2, ccz_b));
                // error bound of the fp32 surrogate against the float64 distance
                const float s1 = fabsf(sx) + fabsf(sy) + fabsf(sz);
                const float Mi = 2.0f * s1 * a.Tn + a.T2;
                weps[wv][sl] = 1.1920929e-7f * (5.0f * Mi + 2.0f * fminf(unif(PEDP_ST.r1), s1 + a.Tn) * (a.Tn + s1)) * 1.0001f;
                wS[wv][sl] = sx * sx + sy * sy + sz * sz;
                wpi[wv][sl] = pi;
                wkk[wv][sl] = half * 64 + lane;
                wp[wv][0][sl] = x; wp[wv][1][sl] = y; wp[wv][2][sl] = z;
                wcs[wv][0][sl] = sx; wcs[wv][1][sl] = sy; wcs[wv][2][sl] = sz;
                // search radius of the slot: the distance to last pass's neighbour, rounded up, at most r
                float rp = slot_radius(dprev, s1);
                if constexpr (!BATCH) {
                    // with certificates: KAPPA times that.  Any radius not below the true nearest distance gives the same
                    // result; the wider one leaves a margin between the neighbour and the bound the certificate is made from
                    if (certify) rp = slot_radius_kappa(dprev, s1);
                }
                const float r_search = BATCH ? r_search_b : unif(cur.r_search);
                wrho[wv][sl] = rp < r_search ? rp : r_search;
            }
            nsl = wc - 16 * q4;
            nsl = nsl < 0 ? 0 : (nsl > 16 ? 16 : nsl);
            __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): this wave's LDS writes have landed
        }
        if (rebuild) {  // is the chunk live?  (both halves' flags)
            __syncthreads();
            const bool is_live = (misc[0] | misc[1]) != 0;
            if (!is_live) {  // workgroup-uniform: the chunk stays outside the live set
                __syncthreads();  // (the flags are rewritten by the next chunk)
                continue;
            }
            if (tid == 0) __hip_atomic_fetch_or((g_u64 *)(uintptr_t)&PEDP_MASK_CUR[chunk >> 6], 1ull << (chunk & 63), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (tid == 0) PEDP_STAMP(1, blockIdx.x, 1);
        PEDP_WV(1, __builtin_amdgcn_s_memtime());
        const bool real = j < nsl;
        double fd = dinf;      // the slot's result: squared distance, target index (-1: none), neighbour and normal
        int fj = -1;
        double wt[3] = {0.0, 0.0, 0.0}, wn[3] = {0.0, 0.0, 0.0};
        bool have_tn = false;
        int ntl_w = 0, nfb_w = 0;
        // (the slot's certificate for the next pass waits in wcert: a certified slot's is there already)
        if (skip) {  // wave-uniform (nothing happens for nsl == 0)
            if (real) { fj = wfj[wv][j]; fd = wfd[wv][j]; }  // neighbour and normal are fetched by index below
        } else if (nsl > 0) {  // wave-uniform
            // ---- 2. what the target's spheres are tested against: a COVER of the sub-block's slots by bounding
            // spheres (centred fp32 coordinates), each with the largest search radius of its slots.  The slots'
            // binary tree -- pairs, quads, octets, all sixteen: the levels of a butterfly reduction -- is cut
            // where a node's sphere is no wider than r.  A compact sub-block is one node; 16 consecutive points
            // of the spatial order that straddle a jump of the curve (a WIDE sub-block) come out as the few
            // compact groups they really are, down to single points, instead of one huge ball whose tiles
            // would all have to be swept.  Nodes live in the wave's LDS; the first also in registers.
            const float px = real ? wcs[wv][0][j] : 0.f, py = real ? wcs[wv][1][j] : 0.f, pz = real ? wcs[wv][2][j] : 0.f;
            const float rho_j = real ? wrho[wv][j] : 0.f;
            int nn;  // nodes of the cover
            {
                const float big = 3e38f, wr = unif(PEDP_ST.wide_radius);
                float lx = real ? px : big, hx = real ? px : -big, ly = real ? py : big, hy = real ? py : -big,
                      lz = real ? pz : big, hz = real ? pz : -big, rmx = rho_j;
                // level 0: the point itself, widened by the rounding of its centred coordinates
                float4 node = make_float4(px, py, pz, point_slack(px, py, pz));
                float node_r = rho_j;
                bool open = real;   // no level of this lane's chain is in the cover yet
                bool mine = false;  // this lane holds a node of the cover
                int cut = 0;        // a chain inside this lane's current node has been closed
                auto level = [&](auto LV) {
                    constexpr int lv = decltype(LV)::value;  // butterfly level 0..3: nodes of 2 << lv slots
                    constexpr int off = 1 << lv;
                    lx = fminf(lx, row_partner<lv>(lx)); hx = fmaxf(hx, row_partner<lv>(hx));
                    ly = fminf(ly, row_partner<lv>(ly)); hy = fmaxf(hy, row_partner<lv>(hy));
                    lz = fminf(lz, row_partner<lv>(lz)); hz = fmaxf(hz, row_partner<lv>(hz));
                    rmx = fmaxf(rmx, row_partner<lv>(rmx));
                    const float mx = 0.5f * (lx + hx), my = 0.5f * (ly + hy), mz = 0.5f * (lz + hz);
                    const float ex = hx - mx, ey = hy - my, ez = hz - mz;
                    const float rad = sqrtf(ex * ex + ey * ey + ez * ez) * 1.0001f + 1e-6f * (fabsf(mx) + fabsf(my) + fabsf(mz)) + 1e-30f;
                    // a node is cut where its sphere is wider than r -- or where a part of it has been cut already
                    // (so that rounding can never leave a slot outside the cover); lanes of one node agree
                    cut |= row_partner<lv>(cut);
                    const bool wide_here = rad > wr || cut != 0;
                    // the level below is in the cover where this level is cut: its nodes close their chains
                    if (open && wide_here) { mine = (j & (off - 1)) == 0; open = false; cut = 1; }
                    if (open) { node = make_float4(mx, my, mz, rad); node_r = rmx; }
                };
                level(std::integral_constant<int, 0>{});
                level(std::integral_constant<int, 1>{});
                level(std::integral_constant<int, 2>{});
                level(std::integral_constant<int, 3>{});
                if (open) mine = j == 0;  // the whole sub-block is one node
                const unsigned long long nm = __builtin_amdgcn_ballot_w64(mine && g == 0);
                nn = __builtin_popcountll(nm);
                if (mine && g == 0) {
                    const int at = __builtin_popcountll(nm & lt);
                    wnode[wv][at] = node;
                    wnode_r[wv][at] = node_r;
                }
                __builtin_amdgcn_s_waitcnt(0xC07F);
            }
            PEDP_WV(7, __builtin_amdgcn_s_memtime());
            const float4 node0 = wnode[wv][0];
            const float node0_r = wnode_r[wv][0];
            // Can a target sphere ts (a tile's, or a whole mask word's) hold the nearest neighbour of a slot
            // of this sub-block?  Every slot has a search radius rho <= r, a node the largest of its slots'.
            auto near_sb = [&](const float4 &ts) -> bool {
                const float dx = ts.x - node0.x, dy = ts.y - node0.y, dz = ts.z - node0.z;
                const float lim = node0_r + node0.w + ts.w;
                bool any = !offset_beyond(dx, dy, dz, lim);
#pragma nounroll
                for (int i = 1; i < nn; ++i) {  // wave-uniform; broadcast reads
                    const float4 nd = wnode[wv][i];
                    const float ex = ts.x - nd.x, ey = ts.y - nd.y, ez = ts.z - nd.z;
                    const float li = wnode_r[wv][i] + nd.w + ts.w;
                    any |= !offset_beyond(ex, ey, ez, li);
                }
                return any && ts.w >= 0.f;
            };
            // MFMA B operand of the sub-block: (-2x', -2y', -2z', 1) per slot, dummies (0, 0, 0, 1)
            const float bfrag = g == 3 ? 1.0f : (real ? -2.0f * wcs[wv][g < 3 ? g : 0][j] : 0.f);
            float b1 = inf, b2 = inf, b3 = inf;
            int t1 = a.n_tiles, t2 = a.n_tiles;
#if PEDP_ICP_STAMPS
            int dbg_words = 0, dbg_batches = 0;
#endif
            // ---- 3. culling and sweep.  Level 1: lane l tests the sphere of mask word l (64 tiles = 1,024
            // sorted rows).  Level 2, eight surviving words per round of loads: lane l tests tile 64 word + l,
            // the ballot is the word's tile mask; the survivors of ALL words go to the wave's LDS list, which is
            // then swept in one go (the list is swept early only if the next round might not fit).
            int n = 0;
            for (int R = 0; R * 64 < a.n_words; ++R) {
                const int wi = R * 64 + lane;
                const float4 wsR = R == 0 ? wsph0[lane] : gload4(a.word_sph + (wi < a.n_words ? wi : 0));
                unsigned long long km = __builtin_amdgcn_ballot_w64(wi < a.n_words && near_sb(wsR));
#if PEDP_ICP_STAMPS
                dbg_words += __builtin_popcountll(km);
#endif
                while (km != 0ull) {  // wave-uniform
#if PEDP_ICP_STAMPS
                    ++dbg_batches;
#endif
                    if (n + L2_WORDS * 64 > WTL) {  // rare: a dense neighbourhood
                        if (lane < SW_PAD) wtl[wv][n + lane] = (unsigned)a.n_tiles;  // pad tiles: rows that never win
                        __builtin_amdgcn_s_waitcnt(0xC07F);
                        sweep_sub_block(wtl[wv], n, as_global(a.tgtf), frag, bfrag, b1, t1, b2, t2, b3);
                        ntl_w += n;
                        n = 0;
                    }
                    int word[L2_WORDS];
                    float4 ts[L2_WORDS];
#pragma unroll
                    for (int u = 0; u < L2_WORDS; ++u) {
                        word[u] = -1;
                        if (km != 0ull) {
                            word[u] = R * 64 + __builtin_ctzll(km);
                            km &= km - 1ull;
                        }
                        const int tile = word[u] * 64 + lane;
                        ts[u] = gload4(a.tile_sph + ((word[u] >= 0 && tile < a.n_tiles) ? tile : 0));
                    }
                    // the batch's spheres against the cover, node by node: a node is read from LDS once per
                    // batch (the next one requested before this one's tests), not once per sphere -- a wide
                    // sub-block's four or five nodes used to cost a dependent LDS round trip per (sphere, node)
                    unsigned nearbits = 0u;
                    {
                        float4 nd = node0;
                        float nd_r = node0_r;
                        for (int i = 0; i < nn; ++i) {  // wave-uniform
                            float4 ndn = nd;
                            float ndn_r = nd_r;
                            if (i + 1 < nn) { ndn = wnode[wv][i + 1]; ndn_r = wnode_r[wv][i + 1]; }
#pragma unroll
                            for (int u = 0; u < L2_WORDS; ++u) {
                                const float ex = ts[u].x - nd.x, ey = ts[u].y - nd.y, ez = ts[u].z - nd.z;
                                const float li = nd_r + nd.w + ts[u].w;
                                if (!offset_beyond(ex, ey, ez, li)) nearbits |= 1u << u;
                            }
                            nd = ndn;
                            nd_r = ndn_r;
                        }
                    }
#pragma unroll
                    for (int u = 0; u < L2_WORDS; ++u) {
                        if (word[u] < 0) continue;
                        const int tile = word[u] * 64 + lane;
                        const bool keep = tile < a.n_tiles && (nearbits >> u & 1u) != 0u && ts[u].w >= 0.f;
                        const unsigned long long m = __builtin_amdgcn_ballot_w64(keep);
                        if (keep) wtl[wv][n + __builtin_popcountll(m & lt)] = (unsigned)tile;
                        n += __builtin_popcountll(m);
                    }
                }
            }
            PEDP_WV(8, __builtin_amdgcn_s_memtime());
            if (lane < SW_PAD) wtl[wv][n + lane] = (unsigned)a.n_tiles;  // pad tiles: rows that never win
            __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
            sweep_sub_block(wtl[wv], n, as_global(a.tgtf), frag, bfrag, b1, t1, b2, t2, b3);
            ntl_w += n;
            if (tid == 0) PEDP_STAMP(1, blockIdx.x, 2);
            PEDP_WV(2, __builtin_amdgcn_s_memtime());
            PEDP_WV(5, ((long long)dbg_words << 32) | ((long long)dbg_batches << 16) | ((long long)nn << 8) | nsl);
            PEDP_WV(6, ntl_w);
            // ---- 4. exact selection.  fp32 g is a filter: with the slot's error bound e the true nearest
            // neighbour lies in a tile whose value is within 2 e of the slot's minimum.  A lane re-scores the
            // four rows it saw of its best tile (and of its second best, if that is inside the window too) in
            // float64 with the oracle's formula, lexicographic (d^2, index); a third tile of one lane inside
            // the window sends the slot to the exact search.
            auto load_rows = [&](int tile, double (&rw)[4][6], int (&ri)[4]) {
                const int64_t row0 = (int64_t)tile * 16 + 4 * g;  // this lane's rows of the tile
                // four rows of 48 B lie one behind the other, 16-B aligned: twelve 16-B loads (the sorted rows are
                // allocated and zero-filled up to the pad tiles, so rows beyond Nt are readable; they are not scored)
                typedef double v2d __attribute__((ext_vector_type(2)));
                const PEDP_GLOBAL v2d *rows = (const PEDP_GLOBAL v2d *)(uintptr_t)(a.tgt_s + 6 * row0);
#pragma unroll
                for (int q = 0; q < 12; ++q) {
                    const v2d t = rows[q];
                    rw[q / 3][2 * (q % 3)] = t[0];
                    rw[q / 3][2 * (q % 3) + 1] = t[1];
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) ri[r] = as_global(a.tperm)[row0 + r < a.Nt ? row0 + r : 0];
            };
            const float e = real ? weps[wv][j] : 0.f, Si = real ? wS[wv][j] : 3e38f;
            const double qx = wp[wv][0][j], qy = wp[wv][1][j], qz = wp[wv][2][j];
            float mg = fminf(b1, __shfl_xor(b1, 16, 64));
            mg = fminf(mg, __shfl_xor(mg, 32, 64));
            const bool maybe = real && mg + Si <= unif(PEDP_ST.r2f) + 4.0f * e + 4.8e-7f * Si;  // else certainly farther than r
            const float win = mg + 2.0f * e;
            double bd = dinf, bd2 = dinf;  // (bd2: the second smallest exact d^2 this lane has seen, ties counted -- certificates only)
            int bj = 0x7FFFFFFF;
            auto eval_rows = [&](int tile, const double (&rw)[4][6], const int (&ri)[4]) {
                const int64_t row0 = (int64_t)tile * 16 + 4 * g;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (row0 + r < a.Nt) {
                        const double d = dist2(qx, qy, qz, rw[r][0], rw[r][1], rw[r][2]);
                        if constexpr (!BATCH) bd2 = (d < bd || (d == bd && ri[r] < bj)) ? bd : (d < bd2 ? d : bd2);
                        if (d < bd || (d == bd && ri[r] < bj)) {
                            bd = d; bj = ri[r];
                            wt[0] = rw[r][0]; wt[1] = rw[r][1]; wt[2] = rw[r][2];
                            wn[0] = rw[r][3]; wn[1] = rw[r][4]; wn[2] = rw[r][5];
                        }
                    }
                }
            };
            if (maybe && b1 <= win) {
                double rw1[4][6];
                int ri1[4];
                load_rows(t1, rw1, ri1);
                eval_rows(t1, rw1, ri1);
            }
            if (__builtin_amdgcn_ballot_w64(maybe && b2 <= win) != 0ull) {  // (about one lane in a hundred)
                if (maybe && b2 <= win) {
                    double rw2[4][6];
                    int ri2[4];
                    load_rows(t2, rw2, ri2);
                    eval_rows(t2, rw2, ri2);
                }
            }
            // the slot's winner over its four lanes; the lane that holds it hands neighbour and normal over
            fd = bd;
            int fjj = bj;
            double f2 = bd2;  // second smallest exact d^2 over the slot's four lanes
#pragma unroll
            for (int off = 16; off <= 32; off <<= 1) {
                const double od = __shfl_xor(fd, off, 64);
                const int oj = __shfl_xor(fjj, off, 64);
                if constexpr (!BATCH) {
                    const double o2 = __shfl_xor(f2, off, 64);
                    const double hi = fd < od ? od : fd, lo2 = f2 < o2 ? f2 : o2;
                    f2 = hi < lo2 ? hi : lo2;
                }
                lexmin(fd, fjj, od, oj);
            }
            const bool found = maybe && fjj != 0x7FFFFFFF;
            {
                int gw = (found && bj == fjj) ? g : 0;  // target indices are unique: one lane of the four at most
                gw |= __shfl_xor(gw, 16, 64);
                gw |= __shfl_xor(gw, 32, 64);
                const int srcl = j + 16 * gw;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    wt[c] = __shfl(wt[c], srcl, 64);
                    wn[c] = __shfl(wn[c], srcl, 64);
                }
            }
            fj = found ? fjj : -1;
            fd = found ? fd : dinf;
            have_tn = found;
            // ---- 5. ambiguous slots (three tiles of one lane inside the window): exact float64 search over
            // the tiles within the slot's own search radius, the whole wave per slot
            unsigned amb = (unsigned)__builtin_amdgcn_ballot_w64(maybe && b3 <= win);
            {
                const unsigned long long am = __builtin_amdgcn_ballot_w64(maybe && b3 <= win);
                amb = (unsigned)((am | (am >> 16) | (am >> 32) | (am >> 48)) & 0xFFFFull);
            }
            if constexpr (!BATCH) {
                if (certify) {
                    // ---- the slot's certificate: a lower bound L on the distance to every target point but the winner.
                    // Unlisted tiles: farther than rho (less the rounding allowance rho was given on top of the distance it
                    // stands for).  Rows this lane re-scored: exact, f2 is the best of them behind the winner.  Its other rows:
                    // g + S - (CERT_SLACK eps + 4.8e-7 S) bounds d^2 from below wherever d <= r1 (common.h), and the smallest g
                    // among them is b1, b2 or b3 -- the first tile the lane did NOT re-score.  An ambiguous slot, one without
                    // a neighbour and anything non-finite get 0.
                    const bool rs1 = maybe && b1 <= win, rs2 = maybe && b2 <= win;
                    float nr = !rs1 ? b1 : (!rs2 ? b2 : b3);
                    nr = fminf(nr, __shfl_xor(nr, 16, 64));
                    nr = fminf(nr, __shfl_xor(nr, 32, 64));
                    const float s1c = fabsf(wcs[wv][0][j]) + fabsf(wcs[wv][1][j]) + fabsf(wcs[wv][2][j]);
                    const double rho = cert_rho_s1(wrho[wv][j], s1c);
                    const double Lg = ((double)nr + (double)Si) - (double)(PEDP_ICP_CERT_SLACK * e + 4.8e-7f * Si) * 1.000001;
                    const double Le = f2 * (1.0 - 1e-12);
                    double L2 = rho * rho;
                    L2 = Lg < L2 ? Lg : L2;
                    L2 = Le < L2 ? Le : L2;
                    const bool ok = found && rho > 0.0 && (amb >> j & 1u) == 0u && (__float_as_int(nr) & 0x7FFFFFFF) <= 0x7F800000 && L2 > 0.0 &&
                                    (__double2hiint(L2) & 0x7FF00000) != 0x7FF00000;
                    if (g == 0 && real) wcert[wv][j] = ok ? cert_bound(L2) : 0.f;  // (over phase 1's entry; this lane reads it back in phase 6)
                }
            }
            if (tid == 0) PEDP_STAMP(1, blockIdx.x, 3);
            while (amb != 0u) {  // wave-uniform, rare
                const int s = __builtin_ctz(amb);
                amb &= amb - 1u;
                ++nfb_w;
                const double sx64 = wp[wv][0][s], sy64 = wp[wv][1][s], sz64 = wp[wv][2][s];
                const float sx = wcs[wv][0][s], sy = wcs[wv][1][s], sz = wcs[wv][2][s], rho_s = wrho[wv][s];
                const float slack = point_slack(sx, sy, sz);
                auto near_pt = [&](const float4 &ts) -> bool { return sphere_near_slot(ts, sx, sy, sz, rho_s, slack); };
                double xd = dinf;
                int xj = 0x7FFFFFFF;
                for (int R = 0; R * 64 < a.n_words; ++R) {
                    const int wi = R * 64 + lane;
                    const float4 wsR = R == 0 ? wsph0[lane] : gload4(a.word_sph + (wi < a.n_words ? wi : 0));
                    unsigned long long km = __builtin_amdgcn_ballot_w64(wi < a.n_words && near_pt(wsR));
                    while (km != 0ull) {
                        const int word = R * 64 + __builtin_ctzll(km);
                        km &= km - 1ull;
                        const int tile = word * 64 + lane;
                        const float4 ts = gload4(a.tile_sph + (tile < a.n_tiles ? tile : 0));
                        const bool keep = tile < a.n_tiles && near_pt(ts);
                        scan_near_tiles(__builtin_amdgcn_ballot_w64(keep), tile, a, sx64, sy64, sz64, lane, xd, xj);
                    }
                }
#pragma unroll
                for (int off = 1; off <= 32; off <<= 1) {
                    const double od = __shfl_xor(xd, off, 64);
                    const int oj = __shfl_xor(xj, off, 64);
                    lexmin(xd, xj, od, oj);
                }
                if (j == s) {
                    fd = xj == 0x7FFFFFFF ? dinf : xd;
                    fj = xj == 0x7FFFFFFF ? -1 : xj;
                    have_tn = false;  // neighbour and normal are fetched by index below
                }
            }
        }
        if (tid == 0) PEDP_STAMP(1, blockIdx.x, 4);
        PEDP_WV(3, __builtin_amdgcn_s_memtime());
        // ---- 6. the sub-block's partial sums (layout: see icp_accumulate_kernel).  Four lanes per slot,
        // lane group g owns the packet entries k = g (mod 4); entries are summed over the wave's 16
        // slots by a shuffle tree, then over the waves in order: a fixed tree.
        {
            double acc[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[k] = 0.0;
            const int i = real ? wpi[wv][j] : -1;
            int jn = fj;
            const double dd = fd;
            if (i >= 0) {
                if (jn >= 0 && !(dd < unid(PEDP_ST.r2))) jn = -1;  // strict, as SearchHybrid's lower_bound
                const int64_t kp = (int64_t)chunk * CH + wkk[wv][j];
                if (g == 0) {
                    as_global(a.idx_out)[i] = jn;
                    if (jn < 0) store_nan(&Tp_out[3 * kp]);
                    if constexpr (!BATCH) {
                        if (certify) (as_global(a.cert) + (size_t)((pass + 1) & 1) * a.cert_stride)[kp] = jn >= 0 ? wcert[wv][j] : 0.f;
                    }
                }
                if (jn >= 0) {
                    const double sx = wp[wv][0][j], sy = wp[wv][1][j], sz = wp[wv][2][j];
                    double tx = wt[0], ty = wt[1], tz = wt[2], nx = wn[0], ny = wn[1], nz = wn[2];
                    if (!have_tn) {  // rare: the exact search returns an index
                        tx = as_global(a.tgt)[3 * (int64_t)jn]; ty = as_global(a.tgt)[3 * (int64_t)jn + 1]; tz = as_global(a.tgt)[3 * (int64_t)jn + 2];
                        if (a.estimator == PEDP_POINT_TO_PLANE) {
                            nx = as_global(a.nrm)[3 * (int64_t)jn]; ny = as_global(a.nrm)[3 * (int64_t)jn + 1]; nz = as_global(a.nrm)[3 * (int64_t)jn + 2];
                        }
                    }
                    if (g == 0) { Tp_out[3 * kp] = tx; Tp_out[3 * kp + 1] = ty; Tp_out[3 * kp + 2] = tz; }
                    // entry k of the packet goes to lane group g = k % 4, accumulator k / 4
                    // (icp_steady_kernel has a copy of these entries, steady_pass.h: keep the two alike)
#define PEDP_PUT(K, V)                                   \
    do {                                                 \
        const double v_ = (V);                           \
        if (g == ((K) & 3)) acc[(K) >> 2] = v_;          \
    } while (0)
                    if (a.estimator == PEDP_POINT_TO_PLANE) {
                        const double r = (sx - tx) * nx + (sy - ty) * ny + (sz - tz) * nz;
                        const double J[6] = {sy * nz - sz * ny, sz * nx - sx * nz, sx * ny - sy * nx, nx, ny, nz};
                        int k = 0;
#pragma unroll
                        for (int u = 0; u < 6; ++u)
#pragma unroll
                            for (int v = u; v < 6; ++v) { PEDP_PUT(k, J[u] * J[v]); ++k; }
#pragma unroll
                        for (int u = 0; u < 6; ++u) PEDP_PUT(21 + u, J[u] * r);
                    } else {
                        const double ccx = PEDP_CC(0, ccx_b), ccy = PEDP_CC(1, ccy_b), ccz = PEDP_CC(2, ccz_b);
                        const double s3[3] = {sx - ccx, sy - ccy, sz - ccz}, t3[3] = {tx - ccx, ty - ccy, tz - ccz};
#pragma unroll
                        for (int u = 0; u < 3; ++u) { PEDP_PUT(u, s3[u]); PEDP_PUT(3 + u, t3[u]); }
#pragma unroll
                        for (int u = 0; u < 3; ++u)
#pragma unroll
                            for (int v = 0; v < 3; ++v) PEDP_PUT(6 + 3 * u + v, t3[u] * s3[v]);
                    }
                    PEDP_PUT(27, dd);
                    PEDP_PUT(28, 1.0);
#undef PEDP_PUT
                }
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                double v = acc[k];
#pragma unroll
                for (int once = 0; once < 1; ++once) v = row_sum_step<3>(row_sum_step<2>(row_sum_step<1>(row_sum_step<0>(v))));
                if (j == 0) accsh[wv][4 * k + g] = v;
            }
            // (entries 29, 30 of the tree are zero: the statistics replace them)
            __builtin_amdgcn_s_waitcnt(0xC07F);
            if (lane == 0) { accsh[wv][PACKET] = (double)ntl_w; accsh[wv][PACKET + 1] = (double)nfb_w; }
            if constexpr (!BATCH) {
                if (lane == 0) accsh[wv][PACKET + 2] = !certify ? 0.0 : (skip ? (double)nsl : CERT_PACK * (double)nsl);
            }
        }
        PEDP_WV(4, __builtin_amdgcn_s_memtime());
        PEDP_WV(11, __builtin_amdgcn_s_memrealtime());
        __syncthreads();
        if (tid < PSTRIDE) {
            double v = 0.0;
#pragma unroll
            for (int w = 0; w < W; ++w) v += accsh[w][tid];
            double *dst = &a.partials[(head ? (size_t)(pass & 1) * a.part_stride : 0) + (size_t)unit * PSTRIDE + tid];
            if (a.fuse && !open) store_sc1(dst, v);  // (an open pass: the launch boundary hands the sums over)
            else *as_global(dst) = v;
        }
        if (!BATCH && !rebuild && tid == 0 && a.dur && unit < a.visit_cap) {
            // what this chunk cost, for the plan after next; a workgroup that shared its CU ran about a third slower
            long long d = (long long)__builtin_amdgcn_s_memtime() - t_chunk0;
            const int extra = n_live - a.n_cu;
            if (extra > 0 && ((int)blockIdx.x < extra || (int)blockIdx.x >= a.n_cu)) d = d * 3 / 4;
            typedef int v2i __attribute__((ext_vector_type(2)));
            const v2i e = {(int)(d < 0x7FFFFFFF ? d : 0x7FFFFFFF), tag_now};
            ((PEDP_GLOBAL v2i *)(uintptr_t)a.dur)[(size_t)(pass & 1) * a.visit_cap + unit] = e;
        }
        if (tid == 0) PEDP_STAMP(1, blockIdx.x, 5);
#if PEDP_ICP_STAMPS
        if (tid == 1 && blockIdx.x < 4096) g_icp_stamps[1][blockIdx.x][7] = ((long long)ntl_w << 32) | (long long)(nfb_w << 16) | nsl;
#endif
        __syncthreads();  // the waves' sums are reused by the next chunk
    }
    PEDP_RT(pass, 2);
    if (!a.fuse || open) return;
    // ---- the pass is closed by the workgroup that finishes last
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every wave: its stores have left
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned prev = __hip_atomic_fetch_add((g_u32 *)(uintptr_t)a.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        misc[4] = prev - ticket_base == (unsigned)(n_wg - 1);
        misc[5] = prev == ticket_base;
    }
    __syncthreads();
    PEDP_RT(pass, 3);
    if (!BATCH && misc[5] && !misc[4] && a.visit) {
        // ---- the first workgroup through writes the next pass's visit plan
        write_next_plan();
        return;
    }
    if (!misc[4]) return;

    if (threadIdx.x == 0) PEDP_STAMP(1, blockIdx.x, 6);
    FinishArgs f;
    f.live = PEDP_MASK_CUR; f.live_old = PEDP_MASK_OLD; f.gen_masks = head ? 1 : 0; f.live_list = a.live_list; f.n_lw = a.n_lw; f.partials = a.partials + (head ? (size_t)(pass & 1) * a.part_stride : 0); f.packet = a.packet; f.phase = 0;
    f.estimator = a.estimator; f.trace = a.trace; f.hist = a.hist; f.bcx = a.bc[0]; f.bcy = a.bc[1]; f.bcz = a.bc[2];
    f.idle = a.ticket + 32;
    f.n_idle = (int)gridDim.x - n_wg;
    f.n_busy = n_wg;
    if (!BATCH && !head && planned && threadIdx.x == 0) cur.n_planned += 1;  // (head close: counted where the pass's state was made)
    f.down = BATCH ? nullptr : a.down; f.serial = LANES ? 0 : a.serial_close; f.lane = LANES ? 1 : 0;
    f.known = 1; f.k_pass = pass; f.k_rebuild = rebuild ? 1 : 0; f.k_n_live = n_live;
    if constexpr (BATCH) {
        icp_finish_body<W * 64, 2048, true>(st, f, fin, threadIdx.x);
    } else {
        // the close works on the state in LDS; the state goes to its slot -- with the head close the one pass + 1 names -- as
        // one block, and, when the registration ends here, into the executor's page-locked block as well
        icp_finish_body<W * 64, 2048, true, 1>(&cur, f, fin, threadIdx.x);
        __syncthreads();
        IcpState *out = head ? st0 + ((pass + 1) & 1) : st0;
        if (threadIdx.x < SWORDS) {
            const double wd = ((const state_word *)&cur)[threadIdx.x];
            ((PEDP_GLOBAL state_word *)(uintptr_t)out)[threadIdx.x] = wd;
            if (cur.done != 0 && a.down) ((state_word *)a.down)[threadIdx.x] = wd;
        }
    }
    PEDP_RT(pass, 4);
#undef PEDP_ST
#undef PEDP_CC
#undef PEDP_MASK_CUR
#undef PEDP_MASK_OLD
}

// Start states of a batch's group: from the page-locked block straight into the poses' state slots (G blocks
// pose_stride apart), and each pose's tickets, sign-off counters and live masks zeroed -- one launch instead of a
// 2-D copy and a 2-D fill (hipMemcpy2DAsync measured 73 us per call in the frame chain's hip trace, eight calls a frame).
__global__ __launch_bounds__(256) void batch_state_scatter_kernel(const unsigned long long *__restrict__ up, char *st0, size_t pose_stride,
                                                                  int state_words, char *zero0, int zero_words) {
    const unsigned long long *src = up + (size_t)blockIdx.x * state_words;
    unsigned long long *dst = (unsigned long long *)(st0 + (size_t)blockIdx.x * pose_stride);
    for (int i = threadIdx.x; i < state_words; i += blockDim.x) dst[i] = src[i];
    unsigned long long *z = (unsigned long long *)(zero0 + (size_t)blockIdx.x * pose_stride);
    for (int i = threadIdx.x; i < zero_words; i += blockDim.x) z[i] = 0ull;
}
// ... and the final states back into the page-locked block (a zero-copy write; the host reads after the stream has finished)
__global__ __launch_bounds__(256) void batch_state_gather_kernel(const char *__restrict__ st0, size_t pose_stride, int state_words,
                                                                 unsigned long long *__restrict__ down) {
    const unsigned long long *src = (const unsigned long long *)(st0 + (size_t)blockIdx.x * pose_stride);
    unsigned long long *dst = down + (size_t)blockIdx.x * state_words;
    for (int i = threadIdx.x; i < state_words; i += blockDim.x) dst[i] = src[i];
}

// A single registration's start: the state from the page-locked block into its slot, tickets, sign-off counters and
// live masks zeroed, and both parities of the visit plan and of the duration table too -- those are valid by tag
// alone, and zeroing them here means that no bit of a registration rests on what earlier users left in the workspace.
// One launch in front of pass 0 instead of a copy and a fill.
__global__ __launch_bounds__(256) void icp_state_start_kernel(const unsigned long long *__restrict__ up, unsigned long long *__restrict__ st,
                                                              int state_words, unsigned long long *__restrict__ zero, int zero_words,
                                                              unsigned long long *__restrict__ plan, int plan_words, int slots) {
    for (int i = threadIdx.x; i < state_words; i += blockDim.x) {
        unsigned long long v = up[i];
        st[i] = v;
        if (slots > 1) {  // the second slot of the state: the same parameters, and no pass (-1)
            if (i == (int)(offsetof(IcpState, pass) / 8)) v |= 0xFFFFFFFFull << (8 * (offsetof(IcpState, pass) % 8));
            st[state_words + i] = v;
        }
    }
    for (int i = threadIdx.x; i < zero_words; i += blockDim.x) zero[i] = 0ull;
    for (int i = threadIdx.x; i < plan_words; i += blockDim.x) plan[i] = 0ull;
}

}  // namespace
