// ICP, steady passes: consecutive non-rebuild passes of ONE fused registration in one launch (icp_steady_kernel).
//
// Once every slot of a pass is certified (fused_pass.h), a pass is a transform, a certificate check, a fetch by index
// and the sums: a few microseconds of work between launch boundaries that cost several times as much.  This kernel
// keeps a resident grid through such passes and replaces the launch boundary by a bounded device-wide hand-over:
//
//   per pass p   every workgroup with a rank runs phases 1 and 6 of its chunks (the float64 sequences of
//                icp_pass_kernel, same wave / half / quarter / slot layout, same sum tree), stores its partial sums
//                write-through (sc1) into copy p & 1, drains its stores, meets at a barrier; one lane adds 1 to one of
//                sixteen counters (a line each; the sign-off counters of the generic kernel, cumulative, base in the
//                state); lanes 0-15 poll them with sc1 loads and s_sleep until all have arrived -- at most
//                STEADY_SPIN_CAP looks, then the registration fails loudly (done = -1).  No fence.
//   the close    the ranks below C = min(ranks, closers) -- the CLOSERS; `closers` is the device's CU count unless
//                PEDP_ICP_STEADY_CLOSERS says otherwise -- then close pass p themselves: icp_finish_body in its coherent
//                head mode (MODE 3) -- the head close's sequence on sc1 loads of the partials -- and go on with pass
//                p + 1 from the state in their LDS.  The last closer also writes what a head close leaves behind: the
//                row of the trace, the history slot, the packet.
//   followers    The other ranks FOLLOW: with more ranks than CUs the dispatcher puts rank n_cu + k on the CU of rank k,
//                and a second close there pulls the same partial sums through the same vector memory path and runs the
//                same solve for the same bits, late for both.  A closer that has a follower (rank + C is a rank)
//                publishes what it goes on with -- the state in its LDS and the searched / certified word -- before it
//                begins its chunk: write-through stores by one wave, which drains them, then the tag (nonce + pass + 1),
//                write-through as well.  No fence.  Follower r polls the tag of closer r % C (sc1 loads, s_sleep, the
//                same cap and the same failure), copies the record into its LDS with sc1 loads and takes the branches
//                the closer took.  Where the dispatcher places a workgroup decides the gain only, never the result.
//   two copies   of the partial sums suffice: a workgroup stores pass p + 2 only after all have arrived for p + 1,
//                which they do after reading p.
//   wave groups  icp_steady_kernel<2>: a workgroup is TWO wave groups of eight waves, sixteen waves in all, and a rank is a
//                wave group: in round `it` of a pass group g of workgroup b holds unit b + (2 it + g) G (G workgroups).  A
//                group works on its unit exactly as the eight waves of icp_steady_kernel<1> do -- layout from the wave's
//                index in its group, the same float64 sequences and 16-slot tree, its eight waves added in order behind
//                the chunk's barrier, the partial stored at the unit's own index -- so no bit depends on GROUPS.  The
//                chunk loop and its barriers are the workgroup's: a group whose unit is not a live chunk skips the
//                work and meets the barriers.  The hand-over counts WORKGROUPS (one lane adds one arrival behind the
//                barrier behind both groups' drained stores), the close runs once per closing workgroup on all 1,024
//                threads (a range's 32 entries a thread each), and closer or follower is the workgroup's role, by its
//                group-0 rank.  What `followers` are to workgroups a second group gets for nothing: it goes on from the
//                `cur` its own workgroup's close -- or copy of a record -- left in LDS, no trip through memory.  With a
//                workgroup per CU group 1 of workgroup k holds rank n_cu + k: the rank the dispatcher put on that CU as
//                a second workgroup, and the position the visit plan hands the lightest chunks to.
//
// A slot that is not certified runs the exact search of the ambiguous-slot fallback (word spheres, tile spheres, the
// float64 scan of the near tiles, lexmin) within its own radius rho, the whole wave per slot, and leaves the
// certificate min(rho^2, e2) of DESIGN 4.2 (e2: the second smallest exact d^2 the scan saw, ties counted).  There is
// no cover, no sweep and no selection here.
//
// A chunk is worked on by the same workgroup in every pass of a launch, so what one pass stores of it (points,
// neighbours, certificates, indices: plain stores, written through this CU's L1 to its XCD's L2) the next pass of the
// same workgroup reads back with sc1 loads -- past the L1, which is never refreshed inside a launch.  A wave group's
// first chunk is also kept in LDS from its first pass on and read from there; the global buffers are written in every
// pass all the same, so there is nothing to write back at exit.
//
// The launch ends when the registration does (final state into the page-locked block, as the head close does), or hands
// back to the generic kernel: when a close asks for a rebuild, or when more than 1/8 of a pass's candidate slots
// searched.  The state then lies in the slot its pass names exactly as an in-launch close leaves it, the other slot
// names no pass, and the page-locked block carries a copy marked done = STEADY_HANDBACK for the host.
//
// The state's slots are rewritten only after a device-wide hand-over that counts EVERY workgroup of the grid once
// (those without a rank sign off when they have read the state and leave): nobody that starts late reads a slot while
// it changes.
//
// Residency, one group: 512 threads, 128 VGPRs (launch bounds: four waves per SIMD), 36.8 KB of LDS -- two workgroups per
// CU by registers and waves, four by LDS -- and the host sizes the grid from hipOccupancyMaxActiveBlocksPerMultiprocessor x
// CUs, at most 2 x CUs.  Two groups: 1,024 threads at 128 VGPRs are a CU's registers, 62.9 KB of LDS (per-wave arrays and
// the resident chunk once per group) -- one workgroup per CU, the grid is the CU count.  Every workgroup of the grid is
// resident at once, however many of them have a rank.  Which of the two a registration gets: steady_shape, pedp_icp.hip.
#pragma once
#include "fused_pass.h"

namespace {

// (diagnostic build) the stamps of a steady launch, a row per RANK: the first lane of each wave group that has one (n_ranks
// of the kernel) writes its group's
#if PEDP_ICP_STAMPS
#define PEDP_RT_RANK(pass, slot)                                                                                          \
    do {                                                                                                                  \
        const unsigned row_ = blockIdx.x + threadIdx.x / (BK_W * 64) * gridDim.x;                                         \
        if (threadIdx.x % (BK_W * 64) == 0 && (pass) < 32 && row_ < 512 && row_ < (unsigned)n_ranks)                      \
            g_icp_rt[pass][row_][slot] = (long long)__builtin_amdgcn_s_memrealtime();                                     \
    } while (0)
#else
#define PEDP_RT_RANK(pass, slot) do {} while (0)
#endif

constexpr unsigned STEADY_SPIN_CAP = 1u << 21;  // looks at the counters before a hand-over gives up
constexpr int STEADY_HANDBACK = 2;              // `done` of the page-locked copy of a state that was handed back
// A closer's record for its followers: the state (SWORDS doubles), the searched / certified word behind it, and the tag in
// a line of its own.  Each closer has one slot in each of two copies by the parity of the pass the record closes.  Two
// copies suffice, as for the partial sums: a closer writes copy (p + 1) & 1 only behind the hand-over of pass p + 1; that
// hand-over counts its followers; and the followers arrive there only after they have read copy p & 1 -- so nobody still
// reads the copy of pass p - 1 that the record of pass p + 1 replaces.  The tag names the registration (its nonce) and
// the pass: a record that an earlier registration or an earlier pass left in the slot never matches.
constexpr int FOLLOW_STRIDE = 128;  // doubles per slot
constexpr int FOLLOW_TAG = 112;     // the tag's double inside the slot (byte 896: the slot's last 128-byte line)
static_assert(sizeof(IcpState) / sizeof(double) + 1 <= FOLLOW_TAG, "the record ends in front of the tag's line");

__device__ __forceinline__ float load_sc1(const float *p) {
    return __uint_as_float(__hip_atomic_load((g_u32 *)(uintptr_t)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// A follower's close: wave 0 polls the tag of its closer's record, then the workgroup copies the record -- the state into
// `cur`, the searched / certified word to where the close leaves it.  false: the tag did not come within the cap.
// (Inlined: as a function of its own it cost the kernel more spilled registers than it saved)
__device__ __forceinline__ bool steady_follow(IcpState *cur, double *word, int *failed, const double *rec, unsigned tag) {
    constexpr int SWORDS = (int)(sizeof(IcpState) / sizeof(double));
    typedef double __attribute__((may_alias)) state_word;
    if (threadIdx.x < 64) {
        for (unsigned spins = 0;; ++spins) {
            const unsigned t = (unsigned)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load((g_u32 *)(uintptr_t)(rec + FOLLOW_TAG), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            if (t == tag) break;
            if (spins > STEADY_SPIN_CAP) {  // bounded, as the hand-over is
                if (threadIdx.x == 0) *failed = 1;
                break;
            }
            __builtin_amdgcn_s_sleep(2);
        }
    }
    __syncthreads();
    if (*failed != 0) return false;  // (workgroup-uniform)
    if (threadIdx.x <= SWORDS) {
        const double v = load_sc1(&rec[threadIdx.x]);
        if (threadIdx.x < SWORDS) ((state_word *)cur)[threadIdx.x] = v;
        else *word = v;
    }
    __syncthreads();
    return true;
}

// a0.launch: the first pass this launch may run (what a generic launch of that index would run)
// follow: the closers' records, [2][follow_cap] slots (null: every rank closes); closers: see above (< 1: every rank)
// GROUPS: wave groups of eight waves per workgroup, each with a rank of its own (1: a workgroup is a rank)
// LANES: the close's 6x6 solve a row per lane, and no one-lane solve in the kernel (as icp_pass_kernel's LANES)
template <int GROUPS, bool LANES>
__global__ __launch_bounds__(GROUPS * BK_W * 64, 4) void icp_steady_kernel(IcpState *st0, const PassArgs a0, double *follow, int follow_cap, int closers) {
    constexpr int W = BK_W, GW = GROUPS * W;
    static_assert(W == 8 && CH == 128, "a chunk is two halves of four 16-slot sub-blocks");
    static_assert(GROUPS == 1 || GROUPS == 2, "one workgroup is at most a CU's sixteen waves at 128 registers");
    __shared__ IcpState cur;
    typedef double __attribute__((may_alias)) state_word;
    typedef int v4i __attribute__((ext_vector_type(4)));
    constexpr int SWORDS = (int)(sizeof(IcpState) / sizeof(double));
    __shared__ PassArgs sa;
    __shared__ FinishLds<GW * 64, 1> fin;
    // per wave, group-major: wave 8 g + w is wave w of group g
    __shared__ double wp[GW][3][16], accsh[GW][PSTRIDE], wfd[GW][16];
    __shared__ float wcs[GW][3][16], wrho[GW][16], wcert[GW][16];
    __shared__ int wpi[GW][16], wkk[GW][16], wfj[GW][16], misc[4];
    __shared__ float4 wsph0[64];
    __shared__ double *role_rec[2];  // this workgroup's record in either copy: its own (a closer) or its closer's (a follower)
    // A group's first chunk stays resident from its first pass in this launch on, by position in the chunk: the
    // point (two copies by pass parity, like Pk: the four waves of a half read a pass's input while quarter 0 writes
    // its output), last pass's neighbour with its normal, the certificate, the neighbour's and the point's index.  Of
    // the last four a wave uses only its own slots' entries, which it alone rewrites, behind its own reads.
    __shared__ double rP[GROUPS][2][3][CH], rT[GROUPS][3][CH], rN[GROUPS][3][CH];
    __shared__ float rc[GROUPS][CH];
    __shared__ int rj[GROUPS][CH], rpi[GROUPS][CH];
    if (threadIdx.x == 0) { sa = a0; misc[0] = 0; }
    const PassArgs &a = sa;
    const int G = (int)gridDim.x;
    // this wave's group's first unit: workgroup b's group g starts at b + g G -- with a workgroup per CU, where a second
    // workgroup of the CU would start, and where the visit plan puts the lightest chunks
    const unsigned rank0 = GROUPS == 1 ? blockIdx.x : blockIdx.x + (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / (W * 64))) * gridDim.x;
    const int chunk_first = a0.live_list[rank0 < (unsigned)a0.n_chunks ? rank0 : 0];
    v4i vis = {0, 0, 0, 0};
    if (a0.visit && rank0 < (unsigned)a0.visit_cap) vis = ((const v4i *)a0.visit)[(size_t)(a0.launch & 1) * a0.visit_cap + rank0];
    // (the same entry in every lane: kept in scalar registers through the launch)
    for (int k = 0; k < 4; ++k) vis[k] = __builtin_amdgcn_readfirstlane(vis[k]);
    if (threadIdx.x < 64) wsph0[threadIdx.x] = a0.word_sph[(int)threadIdx.x < a0.n_words ? threadIdx.x : 0];
    // which slot holds what: the head of a generic launch of this index decides the same way (fused_pass.h)
    bool need_close = false;
    {
        IcpState *sA = st0 + (a0.launch & 1), *sB = st0 + ((a0.launch + 1) & 1);
        double wA = 0.0, wB = 0.0;
        if (threadIdx.x < SWORDS) {
            wA = ((const state_word *)sA)[threadIdx.x];
            wB = ((const state_word *)sB)[threadIdx.x];
        }
        if (a0.launch > 0 && sB->pass == a0.launch - 1 && sB->done == 0 && sB->rebuild == 0 && sB->pass < sB->max_iter) need_close = true;
        else if (sA->pass != a0.launch || sA->done) return;  // the registration is over (every workgroup sees that: nobody writes)
        if (threadIdx.x < SWORDS) ((state_word *)&cur)[threadIdx.x] = need_close ? wB : wA;
        __syncthreads();  // the state, the argument block and the word spheres are in LDS
    }
    auto uni = [](int v) { return __builtin_amdgcn_readfirstlane(v); };
    auto unif = [](float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); };
    const int n_live = uni(cur.n_live), max_iter = uni(cur.max_iter);
    const unsigned base0 = (unsigned)uni((int)cur.idle_base);
    int n_part = n_live < G ? n_live : G;
    n_part = n_part < 1 ? 1 : n_part;  // workgroups with a rank (no live chunk at all: workgroup 0 still closes the passes)
    const int n_ranks = GROUPS == 1 ? n_part : (n_live < GROUPS * G ? (n_live < 1 ? 1 : n_live) : GROUPS * G);  // wave groups with one
    g_u32 *const counters = (g_u32 *)(uintptr_t)(a0.ticket + 32);
    if ((int)blockIdx.x >= n_part) {  // no rank: this workgroup has read the state -- it signs off and leaves
        if (threadIdx.x == 0) __hip_atomic_fetch_add(counters + 32 * (blockIdx.x & 15), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    // Closer or follower, and where this workgroup's record lies: decided once and parked in LDS -- the kernel is at its
    // register cap, and a close needs these once per pass.  The role is the WORKGROUP's, by its group-0 rank: a second
    // group goes on from the state its workgroup's close, or its copy of a record, left in LDS.
    bool service;
    {
        int C = follow != nullptr && closers >= 1 && closers < n_part ? closers : n_part;
        C = C > follow_cap ? n_part : C;  // (the host sizes the slots for every grid it launches)
        const bool closer = (int)blockIdx.x < C;
        const bool publishes = closer && (int)blockIdx.x + C < n_part;  // some follower's rank % C is this rank
        service = (int)blockIdx.x == C - 1;  // (a closer: what it writes comes out of the close's LDS)
        if (threadIdx.x == 0) {
            misc[1] = (closer ? 1 : 0) | (publishes ? 2 : 0);
            misc[2] = n_ranks - C;  // ranks that did not close: following workgroups' groups, and every second group
            for (int k = 0; k < 2; ++k)
                role_rec[k] = C < n_part ? follow + ((size_t)k * follow_cap + (size_t)((int)blockIdx.x % C)) * FOLLOW_STRIDE : nullptr;
        }
        __syncthreads();
    }
    // the visit plan of the launch's first pass, where there is one, holds for all of them (one chunk per workgroup)
    // (wave-uniform: a group reads its own entry; the entries of one pass agree)
    const bool planned = a0.visit != nullptr && n_live <= GROUPS * G && vis[2] == uni(cur.nonce) + a0.launch + 1 && vis[3] == n_live;
    const double dinf = __longlong_as_double(0x7FF0000000000000ll);
    const double dnan = __longlong_as_double(0x7FF8000000000000ll);
    // The device-wide hand-over counts workgroups.  Arrivals so far in this launch: the first counts the whole grid, the
    // others the workgroups with a rank.
    unsigned arrivals = 0u;
    int handovers = 0;
    // (diagnostic build, g_icp_rt of pass p: [0] chunks begun, [2] chunks done, [3] arrived, [4] all seen to have arrived; the
    // close of pass p - 1 in front of it: [5] partial sums' loads back, [6] sums done, [7] U published)
    auto hand_over = [&](int p_stamp) -> bool {
        (void)p_stamp;
        PEDP_RT_RANK(p_stamp, 2);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every wave: its stores have left
        __syncthreads();  // (the whole workgroup: every group's)
        if (threadIdx.x == 0) __hip_atomic_fetch_add(counters + 32 * (blockIdx.x & 15), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        PEDP_RT_RANK(p_stamp, 3);
        arrivals += handovers == 0 ? (unsigned)G : (unsigned)n_part;
        ++handovers;
        if (threadIdx.x < 64) {
            for (unsigned spins = 0;; ++spins) {
                unsigned c = threadIdx.x < 16 ? __hip_atomic_load(counters + 32 * threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
#pragma unroll
                for (int off = 8; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
                if (__shfl(c, 0, 64) - base0 >= arrivals) break;
                if (spins > STEADY_SPIN_CAP) {  // bounded: a lost workgroup must not hang the device
                    if (threadIdx.x == 0) misc[0] = 1;
                    break;
                }
                __builtin_amdgcn_s_sleep(8);
            }
        }
        PEDP_RT_RANK(p_stamp, 4);
        __syncthreads();
        if (misc[0] != 0) {  // (workgroup-uniform) the registration fails loudly; the others give up the same way
            if (threadIdx.x == 0 && a0.down) *(int *)((char *)a0.down + offsetof(IcpState, done)) = -1;
            return false;
        }
        return true;
    };
    // What the launch leaves behind (the service workgroup, behind at least one hand-over): the state into the slot its
    // pass names -- a final state into the page-locked block too, a state handed back there marked as such -- and "no
    // pass" into the other slot, so that the head of the next generic launch does not close a pass again.
    auto leave = [&](bool handback) {
        if (!service) return;
        const int tid = threadIdx.x;
        if (tid == 0) cur.n_followed = misc[2];
        __syncthreads();
        const int next = uni(cur.done) != 0 ? uni(cur.pass) + 1 : uni(cur.pass);  // (a stop leaves `pass` at the pass it closed)
        if (tid < SWORDS) ((PEDP_GLOBAL state_word *)(uintptr_t)(st0 + (next & 1)))[tid] = ((const state_word *)&cur)[tid];
        if (tid == 0 && handback) as_global(&(st0 + ((next + 1) & 1))->pass)[0] = -1;
        if (!a0.down) return;
        __syncthreads();
        if (tid == 0 && handback) cur.done = STEADY_HANDBACK;
        __syncthreads();
        if (tid < SWORDS) ((state_word *)a0.down)[tid] = ((const state_word *)&cur)[tid];
    };

    bool ran = false;  // a pass of this launch has filled the resident copy of the first chunk
    for (int p = a0.launch;; ++p) {
        if (need_close) {
            // ---- the close of pass p - 1, by every closing workgroup, on all its threads: same inputs, same float64
            // sequence, same bits (at 1,024 threads a range's 32 entries have a thread each: fused_close.h)
            const int q = p - 1;
            const bool closer = (uni(misc[1]) & 1) != 0;
            if (closer) {
                FinishArgs f;
                f.live = nullptr; f.live_list = nullptr; f.n_lw = 0; f.partials = a0.partials + (size_t)(q & 1) * a0.part_stride; f.packet = nullptr; f.phase = 0;
                f.estimator = a0.estimator; f.trace = nullptr; f.hist = nullptr; f.bcx = a0.bc[0]; f.bcy = a0.bc[1]; f.bcz = a0.bc[2];
                f.serial = 0; f.lane = LANES ? 1 : 0;
                f.known = 1; f.k_pass = q; f.k_rebuild = 0; f.k_n_live = n_live;
                icp_finish_body<GW * 64, 1, true, 3>(&cur, f, fin, threadIdx.x);  // (ends behind a barrier)
            } else if (!steady_follow(&cur, &fin.pk[PACKET + 2], &misc[0], role_rec[q & 1], (unsigned)(uni(cur.nonce) + q + 1))) {
                if (threadIdx.x == 0 && a0.down) *(int *)((char *)a0.down + offsetof(IcpState, done)) = -1;
                return;
            }
            PEDP_RT_RANK(p, 7);
            // candidate slots of pass q that searched / that a certificate served (all workgroups agree: the same sums)
            const double pk31 = fin.pk[PACKET + 2];
            const long long searched = (long long)(pk31 / CERT_PACK);
            const long long certified = (long long)(pk31 - (double)searched * CERT_PACK);
            const bool stopped = uni(cur.done) != 0;
            // (a pass a generic launch ran counts its slots by waves -- a wave with one uncertified slot searches all sixteen --
            // and says little about the next pass here: the share decides only behind a pass of this launch)
            const bool handback = !stopped && (uni(cur.rebuild) != 0 || (q >= a0.launch && searched * 8 > searched + certified));
            if (closer && threadIdx.x == 0) {  // (a follower's state has all of this in it)
                if (q >= a0.launch) cur.n_steady += 1;  // (the pass ran in this launch)
                if (q >= max_iter) cur.n_head -= 1;  // the last pass counts as closed in its launch, as it is without this kernel
                cur.idle_base = base0 + arrivals;
                if (planned && !stopped && !handback) cur.n_planned += 1;  // (counted where the pass's state is made)
            }
            if (service) {
                const int tid = threadIdx.x;
                if (sa.trace && tid < 18)
                    as_global(sa.trace)[18 * q + tid] = tid == 0 ? cur.fitness : (tid == 1 ? cur.rmse : fin.t0[tid >= 2 ? tid - 2 : 0]);
                if (!stopped && tid < 16) as_global(sa.hist)[16 * (q + 1) + tid] = cur.upd[tid];
                if (!stopped && tid < PACKET) as_global(sa.packet)[tid] = fin.pk[tid];
            }
            __syncthreads();
            if ((uni(misc[1]) & 2) != 0 && threadIdx.x < 64) {  // one wave: the record, its drain, the tag
                double *const rec = role_rec[q & 1];
                const unsigned tag = (unsigned)(uni(cur.nonce) + q + 1);
                for (int k = threadIdx.x; k <= SWORDS; k += 64) store_sc1(&rec[k], k < SWORDS ? ((const state_word *)&cur)[k] : pk31);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                if (threadIdx.x == 0) __hip_atomic_store((g_u32 *)(uintptr_t)(rec + FOLLOW_TAG), tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (stopped || handback) {
                if (handovers == 0 && !hand_over(31)) return;
                if (threadIdx.x == 0) cur.idle_base = base0 + arrivals;
                __syncthreads();
                leave(handback);
                return;
            }
        } else if (uni(cur.rebuild) != 0) {  // the pass this launch was to start with is a rebuild pass: not ours
            if (!hand_over(31)) return;
            if (threadIdx.x == 0) cur.idle_base = base0 + arrivals;
            __syncthreads();
            leave(true);
            return;
        }
        need_close = true;
        // ---- pass p
        PEDP_RT_RANK(p, 0);
        for (int it = 0;; ++it) {
            // (the thread index is made opaque per chunk, as in icp_pass_kernel)
            int tid = threadIdx.x;
            asm volatile("" : "+v"(tid));
            // wave wv = 8 gr + wl: wave wl of wave group gr; thread ltid of the group's 512
            const int lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
            const int gr = GROUPS == 1 ? 0 : wv >> 3, wl = GROUPS == 1 ? wv : wv & 7, ltid = GROUPS == 1 ? tid : tid & (W * 64 - 1);
            const int half = wl >> 2, q4 = wl & 3;
            const int j = lane & 15, g = lane >> 4;
            const unsigned long long lt = (1ull << lane) - 1ull;
            const double *Pk_in = a.Pk + (size_t)(p & 1) * a.pp_stride, *Tp_in = a.Tprev + (size_t)(p & 1) * a.pp_stride;
            PEDP_GLOBAL double *Pk_out = as_global(a.Pk) + (size_t)((p + 1) & 1) * a.pp_stride, *Tp_out = as_global(a.Tprev) + (size_t)((p + 1) & 1) * a.pp_stride;
            const float *cert_in = a.cert + (size_t)(p & 1) * a.cert_stride;
            PEDP_GLOBAL float *cert_out = as_global(a.cert) + (size_t)((p + 1) & 1) * a.cert_stride;
            // round `it`: group gr holds unit b + (GROUPS it + gr) G; the loop ends for the workgroup as a whole
            int unit = (int)(blockIdx.x + (unsigned)(GROUPS * it) * (unsigned)G), chunk;
            if (unit >= n_live) break;
            if (GROUPS > 1) unit += gr * G;
            const bool active = GROUPS == 1 || unit < n_live;  // (wave-uniform) a group without a unit only meets the barriers
            if (it == 0) {
                chunk = chunk_first;
                if (planned) { unit = vis[0]; chunk = vis[1]; }
            } else {
                chunk = active ? as_global(a.live_list)[unit] : 0;
            }
            const bool res = ran && it == 0;  // (workgroup-uniform) the group's chunk has its inputs in LDS
            if (active) {  // (wave-uniform; a group without a unit goes straight to the chunk's barrier)
                // ---- 1. transform, certificate check, box test, compaction (icp_pass_kernel's phase 1 of a steady pass)
                int nsl;
                {
                    bool cand = false, certd = false;
                    int pi = -1, jprev = -1;
                    float c_new = 0.f;
                    double x = 0.0, y = 0.0, z = 0.0, dprev = dnan, d2prev = dnan;
                    const int64_t k = (int64_t)chunk * CH + half * 64 + lane;
                    const bool valid = k < a.N;
                    const int pos = half * 64 + lane;
                    if (valid) {
                        double ux, uy, uz;
                        float c_in;
                        if (res) {
                            pi = rpi[gr][pos];
                            x = rP[gr][p & 1][0][pos]; y = rP[gr][p & 1][1][pos]; z = rP[gr][p & 1][2][pos];
                            ux = rT[gr][0][pos]; uy = rT[gr][1][pos]; uz = rT[gr][2][pos];
                            c_in = rc[gr][pos];
                            jprev = rj[gr][pos];
                        } else {
                            pi = as_global(a.perm)[k];
                            x = load_sc1(&Pk_in[3 * k]); y = load_sc1(&Pk_in[3 * k + 1]); z = load_sc1(&Pk_in[3 * k + 2]);
                            ux = load_sc1(&Tp_in[3 * k]); uy = load_sc1(&Tp_in[3 * k + 1]); uz = load_sc1(&Tp_in[3 * k + 2]);
                            c_in = load_sc1(&cert_in[k]);
                            jprev = load_sc1(&a.idx_out[pi]);  // (rewritten in this pass by the slot's own wave only, behind this read)
                        }
                        const double x0 = x, y0 = y, z0 = z;
                        xform(cur.upd, x, y, z);
                        d2prev = dist2(x, y, z, ux, uy, uz);
                        dprev = sqrt(d2prev);
                        const double m = sqrt(dist2(x, y, z, x0, y0, z0));
                        c_new = cert_moved(c_in, m);
                        const bool fin_ = cert_finite(d2prev, m, c_new);
                        certd = fin_ && jprev >= 0 && c_new > 0.f && cert_inside(dprev, c_new);
                        if (!certd) c_new = 0.f;
                        const double d2box = box_dist2(x, y, z, a.lo, a.hi);
                        cand = d2box <= bcast0(cur.r2cut);
                    }
                    const unsigned long long mc = __builtin_amdgcn_ballot_w64(cand);
                    const int wc = __builtin_popcountll(mc);
                    if (q4 == 0 && valid) {
                        if (!cand) { as_global(a.idx_out)[pi] = -1; store_nan(&Tp_out[3 * k]); cert_out[k] = 0.f; }
                        Pk_out[3 * k] = x; Pk_out[3 * k + 1] = y; Pk_out[3 * k + 2] = z;
                        if (it == 0) {
                            rpi[gr][pos] = pi;
                            rP[gr][(p + 1) & 1][0][pos] = x; rP[gr][(p + 1) & 1][1][pos] = y; rP[gr][(p + 1) & 1][2][pos] = z;
                            if (!cand) { rj[gr][pos] = -1; lds_nan(&rT[gr][0][pos]); rc[gr][pos] = 0.f; }
                        }
                    }
                    const int sl = __builtin_popcountll(mc & lt) - 16 * q4;
                    if (cand && sl >= 0 && sl < 16) {
                        wcert[wv][sl] = c_new; wfj[wv][sl] = jprev; wfd[wv][sl] = d2prev;
                        const float sx = (float)(x - bcast0(cur.centroid[0])), sy = (float)(y - bcast0(cur.centroid[1])), sz = (float)(z - bcast0(cur.centroid[2]));
                        const float s1 = fabsf(sx) + fabsf(sy) + fabsf(sz);
                        wpi[wv][sl] = pi;
                        wkk[wv][sl] = half * 64 + lane;
                        wp[wv][0][sl] = x; wp[wv][1][sl] = y; wp[wv][2][sl] = z;
                        wcs[wv][0][sl] = sx; wcs[wv][1][sl] = sy; wcs[wv][2][sl] = sz;
                        // the slot's search radius, as a searching slot of icp_pass_kernel gets it under certificates
                        const float rp = slot_radius_kappa(dprev, s1);
                        const float r_search = unif(cur.r_search);
                        wrho[wv][sl] = rp < r_search ? rp : r_search;
                    }
                    nsl = wc - 16 * q4;
                    nsl = nsl < 0 ? 0 : (nsl > 16 ? 16 : nsl);
                    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): this wave's LDS writes have landed
                }
                const bool real = j < nsl;
                double fd = dinf;
                int fj = -1;
                if (real) { fj = wfj[wv][j]; fd = wfd[wv][j]; }
                // ---- the exact search of the slots no certificate serves, the whole wave per slot
                unsigned amb = (unsigned)(__builtin_amdgcn_ballot_w64(real && g == 0 && __float_as_int(wcert[wv][j]) == 0) & 0xFFFFull);
                const int n_search = __builtin_popcount(amb);
                while (amb != 0u) {  // wave-uniform
                    const int s = __builtin_ctz(amb);
                    amb &= amb - 1u;
                    const double sx64 = wp[wv][0][s], sy64 = wp[wv][1][s], sz64 = wp[wv][2][s];
                    const float sx = wcs[wv][0][s], sy = wcs[wv][1][s], sz = wcs[wv][2][s], rho_s = wrho[wv][s];
                    const float slack = point_slack(sx, sy, sz);
                    auto near_pt = [&](const float4 &ts) -> bool { return sphere_near_slot(ts, sx, sy, sz, rho_s, slack); };
                    double xd = dinf, x2 = dinf;  // smallest and second smallest exact d^2 this lane has seen (ties counted)
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
                            unsigned long long near = __builtin_amdgcn_ballot_w64(tile < a.n_tiles && near_pt(ts));
                            // (fused_pass.h's scan_near_tiles, with the second-smallest d^2 tracked: keep the two alike)
                            while (near != 0ull) {  // wave-uniform: 64 lanes = 64 rows = 4 tiles per trip
                                int t = -1;
#pragma unroll
                                for (int gg = 0; gg < 4; ++gg) {
                                    if (near != 0ull) {
                                        const int bit = __builtin_ctzll(near);
                                        near &= near - 1ull;
                                        const int u = __shfl(tile, bit, 64);
                                        if (gg == g) t = u;
                                    }
                                }
                                const int64_t row = (int64_t)t * 16 + j;
                                if (t >= 0 && row < a.Nt) {
                                    const double d = dist2(sx64, sy64, sz64, as_global(a.tgt_s)[6 * row], as_global(a.tgt_s)[6 * row + 1], as_global(a.tgt_s)[6 * row + 2]);
                                    const int ri = as_global(a.tperm)[row];
                                    const bool wins = d < xd || (d == xd && ri < xj);
                                    x2 = wins ? xd : (d < x2 ? d : x2);
                                    xd = wins ? d : xd;
                                    xj = wins ? ri : xj;
                                }
                            }
                        }
                    }
#pragma unroll
                    for (int off = 1; off <= 32; off <<= 1) {
                        const double od = __shfl_xor(xd, off, 64), o2 = __shfl_xor(x2, off, 64);
                        const int oj = __shfl_xor(xj, off, 64);
                        const double hi = xd < od ? od : xd, lo2 = x2 < o2 ? x2 : o2;
                        x2 = hi < lo2 ? hi : lo2;
                        lexmin(xd, xj, od, oj);
                    }
                    if (j == s) {
                        const bool found = xj != 0x7FFFFFFF;
                        fd = found ? xd : dinf;
                        fj = found ? xj : -1;
                        // the certificate the slot leaves: every target point but the winner is farther than rho (less the rounding
                        // allowance rho carries) or was scanned, and the best of those behind the winner is x2
                        const double rho = cert_rho(rho_s, slack);
                        const double Le = x2 * (1.0 - 1e-12);
                        double L2 = rho * rho;
                        L2 = Le < L2 ? Le : L2;
                        const bool ok = found && rho > 0.0 && L2 > 0.0 && (__double2hiint(L2) & 0x7FF00000) != 0x7FF00000;
                        if (g == 0) wcert[wv][s] = ok ? cert_bound(L2) : 0.f;
                    }
                }
                // ---- 6. the sub-block's partial sums (icp_pass_kernel's phase 6; neighbour and normal by index)
                {
                    double acc[8];
#pragma unroll
                    for (int k = 0; k < 8; ++k) acc[k] = 0.0;
                    const int i = real ? wpi[wv][j] : -1;
                    int jn = fj;
                    const double dd = fd;
                    if (i >= 0) {
                        if (jn >= 0 && !(dd < bcast0(cur.r2))) jn = -1;  // strict, as SearchHybrid's lower_bound
                        const int pos = wkk[wv][j];
                        const int64_t kp = (int64_t)chunk * CH + pos;
                        // a resident slot that keeps last pass's neighbour has its row and normal in LDS: no fetch by index
                        const bool kept = res && jn >= 0 && jn == rj[gr][pos];
                        if (g == 0) {
                            as_global(a.idx_out)[i] = jn;
                            if (jn < 0) store_nan(&Tp_out[3 * kp]);
                            const float c_out = jn >= 0 ? wcert[wv][j] : 0.f;
                            cert_out[kp] = c_out;
                            if (it == 0) {
                                rj[gr][pos] = jn; rc[gr][pos] = c_out;
                                if (jn < 0) lds_nan(&rT[gr][0][pos]);
                            }
                        }
                        if (jn >= 0) {
                            const double sx = wp[wv][0][j], sy = wp[wv][1][j], sz = wp[wv][2][j];
                            double tx, ty, tz, nx = 0.0, ny = 0.0, nz = 0.0;
                            if (kept) {
                                tx = rT[gr][0][pos]; ty = rT[gr][1][pos]; tz = rT[gr][2][pos];
                                if (a.estimator == PEDP_POINT_TO_PLANE) { nx = rN[gr][0][pos]; ny = rN[gr][1][pos]; nz = rN[gr][2][pos]; }
                            } else {
                                tx = as_global(a.tgt)[3 * (int64_t)jn]; ty = as_global(a.tgt)[3 * (int64_t)jn + 1]; tz = as_global(a.tgt)[3 * (int64_t)jn + 2];
                                if (a.estimator == PEDP_POINT_TO_PLANE) {
                                    nx = as_global(a.nrm)[3 * (int64_t)jn]; ny = as_global(a.nrm)[3 * (int64_t)jn + 1]; nz = as_global(a.nrm)[3 * (int64_t)jn + 2];
                                }
                            }
                            if (g == 0) {
                                Tp_out[3 * kp] = tx; Tp_out[3 * kp + 1] = ty; Tp_out[3 * kp + 2] = tz;
                                if (it == 0 && !kept) {
                                    rT[gr][0][pos] = tx; rT[gr][1][pos] = ty; rT[gr][2][pos] = tz;
                                    rN[gr][0][pos] = nx; rN[gr][1][pos] = ny; rN[gr][2][pos] = nz;
                                }
                            }
                            // (the packet entries of icp_pass_kernel's phase 6, fused_pass.h: keep the two alike)
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
                                const double ccx = bcast0(cur.centroid[0]), ccy = bcast0(cur.centroid[1]), ccz = bcast0(cur.centroid[2]);
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
                        const double v = row_sum_step<3>(row_sum_step<2>(row_sum_step<1>(row_sum_step<0>(acc[k]))));
                        if (j == 0) accsh[wv][4 * k + g] = v;
                    }
                    // (entries 29, 30 of the tree are zero: the statistics replace them -- nothing is swept here)
                    __builtin_amdgcn_s_waitcnt(0xC07F);
                    if (lane == 0) {
                        accsh[wv][PACKET] = 0.0;
                        accsh[wv][PACKET + 1] = (double)n_search;
                        accsh[wv][PACKET + 2] = (double)(nsl - n_search) + CERT_PACK * (double)n_search;
                    }
                }
            }
            __syncthreads();
            if (active && ltid < PSTRIDE) {  // the group's eight waves, in order, into the unit's own partial
                double v = 0.0;
#pragma unroll
                for (int w = 0; w < W; ++w) v += accsh[gr * W + w][ltid];
                store_sc1(&a.partials[(size_t)(p & 1) * a.part_stride + (size_t)unit * PSTRIDE + ltid], v);
            }
            __syncthreads();  // the waves' sums are reused by the next chunk
        }
        ran = true;
        if (!hand_over(p)) return;
    }
}

}  // namespace
