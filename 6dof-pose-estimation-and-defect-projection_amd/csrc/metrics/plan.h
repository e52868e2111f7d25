// Host half of pedp_pose_errors (pedp_metrics.hip): the argument bounds, the launch grid and the sizes of the two
// workspaces.  Plain C++ with no HIP in it, so that a stand-alone host program can include it.
#pragma once
#include <cstddef>
#include <cstdint>

namespace pedp_metrics {

constexpr int MT = 128;                    // threads of a workgroup
constexpr int QPT = 2;                     // points held by a thread
constexpr int CH = MT * QPT;               // points of a chunk: one workgroup, one partial sum
constexpr int TP = 256;                    // pred points of an LDS tile
constexpr int64_t MAX_N = (int64_t)1 << 22;
constexpr int MAX_B = 65535, MAX_S = 65535;
constexpr size_t WS_BUDGET = (size_t)64 << 20;   // partial sums of one slab of poses

struct Plan {
    int chunks = 0;      // ceil(N / CH): depends on N alone, and with it the order of every sum
    int S1 = 1;          // max(S, 1): effective poses per prediction
    int slab = 0;        // poses per pair of launches
    size_t ws_bytes = 0; // partial sums: slab x S1 x chunks doubles
    // host-memory calls: offsets of the copies inside the i/o block, and its size
    size_t o_pts = 0, o_preds = 0, o_gts = 0, o_sym = 0, o_out = 0, io_bytes = 0;
};

inline size_t a256(size_t b) { return (b + 255) & ~(size_t)255; }

// nullptr and a filled plan, or what is wrong with the arguments.  B = 0 is accepted (the caller returns at once).
inline const char *plan(int64_t N, int B, int G, int S, Plan *p) {
    if (N <= 0) return "no points";
    if (N > MAX_N) return "more than 2^22 points";
    if (B < 0 || B > MAX_B) return "B outside 0 ... 65535";
    if (S < 0 || S > MAX_S) return "S outside 0 ... 65535";
    if (B > 0 && G != 1 && G != B) return "G is neither 1 nor B";
    p->chunks = (int)((N + CH - 1) / CH);
    p->S1 = S > 0 ? S : 1;
    const size_t per_pose = (size_t)p->S1 * (size_t)p->chunks * sizeof(double);
    size_t slab = WS_BUDGET / per_pose;
    if (slab < 1) slab = 1;
    if (slab > (size_t)(B > 0 ? B : 1)) slab = (size_t)(B > 0 ? B : 1);
    p->slab = (int)slab;
    p->ws_bytes = slab * per_pose;
    size_t o = 0;
    p->o_pts = o;   o += a256(24 * (size_t)N);
    p->o_preds = o; o += a256(128 * (size_t)B);
    p->o_gts = o;   o += a256(128 * (size_t)(G > 0 ? G : 0));
    p->o_sym = o;   o += a256(128 * (size_t)S);
    p->o_out = o;   o += a256(8 * (size_t)B);
    p->io_bytes = o;
    return nullptr;
}

}  // namespace pedp_metrics
