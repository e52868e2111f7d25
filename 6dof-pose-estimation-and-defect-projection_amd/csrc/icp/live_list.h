// ICP, fused pass: the live list of a rebuild pass's close -- the set bits of the live mask, ascending -- by a wave scan.
// Used by the close inside a pass launch (512 threads), by icp_finish_kernel (1,024) and by pedp_debug_live_list.
#pragma once
#include "common.h"

namespace {

// COHERENT: the partial sums and the live mask were written earlier in THIS launch by other
// workgroups (sc1 stores / atomics): read them past this CU's L1 -- global_load ... sc1, never a
// flat_ load (the pointers come out of the LDS-parked argument block, so the address space is
// stated here).
typedef __attribute__((address_space(1))) unsigned long long g_u64;
typedef __attribute__((address_space(1))) int g_i32;
typedef __attribute__((address_space(1))) unsigned g_u32;
template <bool COHERENT>
__device__ __forceinline__ unsigned long long load_live(unsigned long long *p) {
    if (COHERENT) return __hip_atomic_fetch_or((g_u64 *)(uintptr_t)p, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return *p;
}

// Thread t owns a contiguous range of `per` mask words.  What it knows of them before the scan: how many bits they hold,
// and the first word itself (per == 1 for scenes up to 64 NT chunks: the word is read once).
struct LiveWords {
    int w_lo, w_hi, mine;
    unsigned long long first;
};
// The loads of a thread's words: requested where the close begins, with whatever else it asks for first.
template <int NT, bool COHERENT>
__device__ __forceinline__ LiveWords live_words_load(unsigned long long *live, int n_lw, int tid) {
    const int per = (n_lw + NT - 1) / NT;
    LiveWords w;
    w.w_lo = tid * per < n_lw ? tid * per : n_lw;
    w.w_hi = w.w_lo + per < n_lw ? w.w_lo + per : n_lw;
    w.mine = 0;
    w.first = 0ull;
    for (int wi = w.w_lo; wi < w.w_hi; ++wi) {
        const unsigned long long word = load_live<COHERENT>(&live[wi]);
        if (wi == w.w_lo) w.first = word;
        w.mine += __builtin_popcountll(word);
    }
    return w;
}
// The list from the threads' counts: an inclusive scan inside every wave (six shuffle steps, no barrier), the waves' totals
// (NT / 64 of them) through `wave_tot` in LDS and ONE barrier, behind which every thread adds the totals of the waves before
// its own; then each thread expands its words from its position on.  The list goes to `live_list` in memory and, where it
// fits (n_live <= LCAP), to `lst` in LDS.  Returns n_live; ends behind a second barrier: `lst` is whole.
// (The 512-thread Hillis-Steele scan over LDS this replaces met at nineteen barriers.)
template <int NT, int LCAP, bool COHERENT>
__device__ __forceinline__ int live_list_build(const LiveWords &w, unsigned long long *live, int32_t *live_list, int *lst, int *wave_tot,
                                               int tid) {
    static_assert(NT % 64 == 0, "whole waves");
    const int lane = tid & 63, wave = tid >> 6;
    int incl = w.mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(incl, off, 64);
        incl += lane >= off ? t : 0;
    }
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    int before = 0, n_live = 0;
#pragma unroll
    for (int q = 0; q < NT / 64; ++q) {
        const int t = wave_tot[q];
        before += q < wave ? t : 0;
        n_live += t;
    }
    const bool listed = n_live <= LCAP;
    int at = before + incl - w.mine;
    for (int wi = w.w_lo; wi < w.w_hi; ++wi) {
        unsigned long long word = wi == w.w_lo ? w.first : load_live<COHERENT>(&live[wi]);
        while (word != 0ull) {
            const int chunk = wi * 64 + __builtin_ctzll(word);
            word &= word - 1ull;
            if (listed) lst[at] = chunk;
            as_global(live_list)[at] = chunk;
            ++at;
        }
    }
    __syncthreads();
    return n_live;
}

// The listing on mask words of the caller's (pedp_debug_live_list): one workgroup, with the thread count, the LDS list and
// the kind of load of the close that runs at that size -- 512: inside a pass launch, 1,024: icp_finish_kernel.
template <int NT, int LCAP, bool COHERENT>
__global__ __launch_bounds__(NT) void live_list_debug_kernel(unsigned long long *live, int n_lw, int32_t *list_out, int32_t *n_live_out) {
    __shared__ int lst[LCAP], wave_tot[NT / 64];
    const LiveWords w = live_words_load<NT, COHERENT>(live, n_lw, threadIdx.x);
    const int n_live = live_list_build<NT, LCAP, COHERENT>(w, live, list_out, lst, wave_tot, threadIdx.x);
    if (threadIdx.x == 0) *n_live_out = n_live;
}

}  // namespace
