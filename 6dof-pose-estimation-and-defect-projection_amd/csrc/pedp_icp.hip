// ICP (registration_icp) for gfx950 (MI355X).
//
// Replaces o3d.pipelines.registration.registration_icp as called by
// src/pose_estimation.py:519-521 (refine_registration) and :654-660 (z search, one
// iteration).  Semantics contract: oracle/icp.c (float64; exact nearest neighbour,
// strict d^2 < r^2, point-to-plane 6x6 / point-to-point Umeyama update, Open3D's
// convergence rule).
//
// Kernels per correspondence pass (all on the context's stream, no host round trip: a
// device-side `done` flag turns the remaining passes into no-ops):
//   icp_transform_pack   P <- U * P in float64 (the oracle's operation order).  Points farther
//                        than r from the target's bounding box cannot be inliers and are
//                        dropped here; the others are compacted (wave-aggregated atomic) into
//                        the float32 MFMA operand array, (-2x', -2y', -2z', 1) in coordinates
//                        centred on the target centroid.
//   nn_sweep             the one dense contraction.  v_mfma_f32_16x16x4_f32 evaluates
//                        g(i,j) = |t'_j|^2 - 2 s'_i . t'_j for 16 target x 16 scene
//                        points per instruction (A = target tile (x,y,z,|t|^2), B = scene
//                        block); a wave keeps 8 scene blocks (128 points) as B operands in
//                        registers and streams a chunk of target tiles as coalesced 256-B
//                        fragments; the grid is (scene blocks) x (target chunks), sized on
//                        the device from the candidate count so small problems still fill
//                        the chip.  The loop is software-pipelined: the MFMA of tile k+1 is
//                        issued before the 6-op VALU epilogue of tile k (best tile value,
//                        its tile, second-best tile value per lane), so one wave alone keeps
//                        the matrix pipe busy.
//   nn_select            exact selection from the per-(point, lane group, chunk) triples.
//                        fp32 g is only a FILTER: with a proven error bound eps_i the true
//                        nearest neighbour lies in the tiles whose value is within
//                        2 eps_i of the minimum; those <= 16 points are re-scored in
//                        float64 in the oracle's exact formula; if a second tile of one
//                        lane group is inside the window the point goes to nn_fallback.
//   nn_fallback          exact float64 brute force for the (rare) ambiguous points.
//   icp_accumulate       float64 J^T J / J^T r (or Umeyama moments), fixed partition and
//                        fixed reduction tree: run-to-run bit-stable.
//   icp_reduce + icp_solve   29-double packet (optionally summed over ranks by the
//                        caller's hook), pivoted LDLT 6x6 / Jacobi SVD 3x3, T <- U * T,
//                        fitness / rmse / convergence.
//
// Source map.  This file is one translation unit: the kernels live in headers under icp/, included below in
// their order of definition, and the host orchestration follows them here.
//   icp/live_list.h          the live list of a rebuild pass's close by a wave scan: live_words_load, live_list_build, live_list_debug_kernel
//   icp/common.h             build switches (PEDP_NN_EXPERIMENT, PEDP_ICP_STAMPS), constants, IcpState, dmul/dadd/dsub, dist2
//   icp/prep.h               hilbert3, cell_key_kernel, chunk_sphere_kernel, pack_target_kernel, sort_rows_kernel,
//                            tile_sphere_kernel
//   icp/target_order.h       the compact row order of a target pack: tord_init_kernel, tord_block_box_kernel,
//                            tord_key_kernel, tord_leaf_kernel
//   icp/slot_math.h          what several kernels must compute alike: candidate tests, search radii, the certificate's steps
//   icp/segmented_sweep.h    icp_transform_pack_kernel, nn_cull_kernel, nn_segment_kernel, nn_sweep_kernel,
//                            pack_target_bf16_kernel, nn_sweep_bf16_kernel, nn_bf16_debug_kernel
//   icp/segmented_select.h   nn_select_kernel, nn_fallback_kernel, icp_accumulate_kernel, icp_reduce_kernel
//   icp/solve.h              solve6_ldlt, svd3_dev, icp_solve_kernel
//   icp/ransac.h             ransac_hypothesis_kernel
//   icp/solve_lanes.h        solve6_ldlt_lanes: the close's 6x6 solve with a row per lane
//   icp/fused_close.h        the fused pass's overview and constants, solve6_ldlt_reg, PassArgs, FinishArgs,
//                            icp_finish_body, icp_finish_kernel, solve6_lanes_debug_kernel, solve6_one_debug_kernel
//   icp/fused_pass.h         sweep_sub_block, icp_pass_kernel, batch_state_scatter_kernel, batch_state_gather_kernel,
//                            icp_state_start_kernel
//   icp/steady_pass.h        icp_steady_kernel: fully certified passes of a single registration in one resident launch
// Host side, here: icp_switches (the one reader of the environment), icp_decide_path (the one decision of a registration's
// way), then workspace, enqueue, stage / start / collect, the graph and batch forms and the C entry points.
#include "pedp_internal.h"
#include <atomic>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <new>

// The in-launch close of a pass hands data from workgroup to workgroup without fences: relaxed agent-scope
// atomics, sc1 loads and stores past the CU's L1, s_waitcnt for "my stores have left".  That is sound on
// gfx950's cache hierarchy and has been checked on nothing else.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "pedp_icp.hip: the fence-free close of a pass rests on gfx950's caches; build with --offload-arch=gfx950 only"
#endif

#include "icp/common.h"
#include "icp/prep.h"
#include "icp/target_order.h"
#include "icp/segmented_sweep.h"
#include "icp/segmented_select.h"
#include "icp/solve.h"
#include "icp/ransac.h"
#include "icp/fused_close.h"
#include "icp/fused_pass.h"
#include "icp/steady_pass.h"

namespace {

// ------------------------------------------------------------------ host side

struct TargetPrep {
    double c[3];
    float Tn, T2;
    double lo[3], hi[3];
    double bc[3];  // centre of the box (lo, hi): the motion bound of the fused pass and its close measure from it
};

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

struct IcpWorkspace {
    IcpState *st;
    double *P, *d2, *partials, *packet, *trace;
    float4 *B, *blk_sph;
    pedp_cloud_t source, target;                      // the pair of clouds it works on (bind_clouds), and its view of them:
    const float4 *tgt4, *tile_sph;
    const int32_t *src_perm, *tgt_perm;
    float *eps, *S;
    int32_t *idx, *fb, *list;
    unsigned long long *mask;                         // [blocks_cap][n_words] surviving-tile bits
    int32_t *blk_cnt, *blk_segstart;                  // [blocks_cap], [blocks_cap + 1]
    int32_t *seg_blk, *seg_rank0, *seg_n;             // [max_segs]
    float *tr_b1, *tr_b2;
    int32_t *tr_t1;
    int64_t Ns_pad, Nt_pad, blocks_cap;
    int n_words, max_segs;
    int qt;  // MFMA tiles per target unit for this call (1: culled registration, 4: dense sweep)
    // fused pass (qt == 1 inside a registration)
    double *Pk, *hist, *cpart, *Tprev;
    double *follow;  // the records of a steady launch's closers, [2][follow_cap] slots of FOLLOW_STRIDE doubles (steady_pass.h)
    int follow_cap;
    float *cert;   // certificates, two copies by pass parity (see PassArgs)
    unsigned *ticket;
    unsigned long long *live;
    int32_t *live_list;
    int4 *visit;   // visit plan and chunk durations (single registration; see PassArgs)
    int2 *dur;
    int visit_cap;
    int n_lw, n_chunks;
    const float4 *word_sph;
    const double *tgt_s;
    size_t pose_stride;  // bytes between the per-pose blocks of a batch (all pointers above are pose 0's)
};

// trace and update history are sized for a capacity class of max_iter, not for max_iter itself: the
// per-pose block layout a captured batch graph bakes in then changes only with the class
inline int iter_capacity(int max_iter) { return (max_iter + 2 + 63) / 64 * 64; }

int carve_workspace(pedp_ctx_t c, int64_t Ns, int64_t Nt, int max_iter, int qt, IcpWorkspace &w, bool fused = false,
                    int poses = 1) {
    w = IcpWorkspace{};  // (what a path does not use stays null)
    w.qt = qt;
    w.Ns_pad = (int64_t)align_up((size_t)(Ns > 0 ? Ns : 1), NN_PTS_PER_WG);
    w.Nt_pad = (int64_t)align_up((size_t)(Nt > 0 ? Nt : 1), 16 * NN_TU);
    w.blocks_cap = w.Ns_pad / (NN_SB * 16) + 1;
    const int64_t n_tiles = w.Nt_pad / (16 * qt);  // target units
    w.n_words = (int)((n_tiles + 63) / 64);
    // segment table: enough pieces that even the dense case (every tile survives for every
    // block) keeps a piece within the LDS list of one wave
    const int64_t list_units = NN_LIST_TILES / qt;
    int64_t ms = (w.blocks_cap * n_tiles + list_units - 1) / list_units + w.blocks_cap;
    // room for shortest-length (SEG_MIN) pieces up to 8192 of them: the table bounds the sweep's
    // grid, so a small scene (a few blocks) gets a small grid instead of thousands of idle workgroups
    const int64_t seg_min_units = SEG_MIN_TILES / qt;
    int64_t fine = (w.blocks_cap * n_tiles + seg_min_units - 1) / seg_min_units + w.blocks_cap;
    if (fine > 8192) fine = 8192;
    if (ms < fine) ms = fine;
    if (fused) ms = 1;  // the fused pass keeps its triples in LDS: no segment table
    PEDP_REQUIRE(ms < (int64_t)1 << 22, "pedp_icp: problem too large for the segment table (%lld x %lld points)",
                 (long long)Ns, (long long)Nt);
    w.max_segs = (int)ms;
    w.n_chunks = (int)((Ns + CH - 1) / CH);
    w.n_lw = (w.n_chunks + 63) / 64;
    if (w.n_lw < 1) w.n_lw = 1;
    // Every buffer is named once: take() lays it behind the ones before it, 256-byte aligned, and notes where its
    // pointer lives in w; the pointers are set once the executor's scratch buffer is known to be large enough.
    size_t off = 0;
    constexpr int MAX_SLOTS = 32;  // (32 buffers below)
    struct { size_t member, off; } slot[MAX_SLOTS];  // byte offset of the pointer inside w, of the buffer inside the block
    int n_slots = 0;
    auto take = [&](auto *&p, size_t bytes) {
        if (n_slots < MAX_SLOTS) {
            slot[n_slots].member = (size_t)((char *)&p - (char *)&w);
            slot[n_slots].off = off;
        }
        ++n_slots;
        off = align_up(off + bytes, 256);
    };
    // what only the segmented (dense / large-radius) path uses shrinks to nothing in the fused pass,
    // which keeps a chunk's slots, masks and triples in LDS
    const size_t seg_only = fused ? 0 : 1;
    take(w.st, 2 * sizeof(IcpState));  // two slots by pass parity (head close); every other path keeps to the first
    take(w.P, sizeof(double) * 3 * (size_t)w.Ns_pad * seg_only);
    take(w.d2, sizeof(double) * (size_t)w.Ns_pad * seg_only);
    take(w.partials, sizeof(double) * ACC_BLOCKS * PACKET);
    take(w.packet, sizeof(double) * 32);
    take(w.trace, sizeof(double) * 18 * (size_t)iter_capacity(max_iter));
    take(w.B, sizeof(float4) * (size_t)w.Ns_pad);
    take(w.eps, sizeof(float) * (size_t)w.Ns_pad);
    take(w.S, sizeof(float) * (size_t)w.Ns_pad);
    take(w.idx, sizeof(int32_t) * (size_t)w.Ns_pad);
    take(w.fb, sizeof(int32_t) * (size_t)w.Ns_pad);
    take(w.list, sizeof(int32_t) * (size_t)w.Ns_pad);
    take(w.blk_sph, sizeof(float4) * NN_SB * (size_t)w.blocks_cap);
    take(w.mask, sizeof(unsigned long long) * (size_t)w.blocks_cap * (size_t)w.n_words);
    take(w.blk_cnt, sizeof(int32_t) * (size_t)w.blocks_cap);
    take(w.blk_segstart, sizeof(int32_t) * (size_t)(w.blocks_cap + 1));
    take(w.seg_blk, sizeof(int32_t) * (size_t)w.max_segs);
    take(w.seg_rank0, sizeof(int32_t) * (size_t)w.max_segs);
    take(w.seg_n, sizeof(int32_t) * (size_t)w.max_segs);
    const size_t tr = (size_t)w.max_segs * 4 * (NN_SB * 16);
    take(w.tr_b1, sizeof(float) * tr);
    take(w.tr_t1, sizeof(int32_t) * tr);
    take(w.tr_b2, sizeof(float) * tr);
    if (fused) {
        take(w.Pk, sizeof(double) * 3 * (size_t)w.Ns_pad * 2);     // read from [pass & 1], written to the other: no wave
        take(w.Tprev, sizeof(double) * 3 * (size_t)w.Ns_pad * 2);  // ever reads what a faster wave of the same pass has rewritten
        take(w.cert, sizeof(float) * (size_t)w.Ns_pad * (poses <= 1 ? 2 : 0));  // likewise (a batch keeps none)
        take(w.hist, sizeof(double) * 16 * (size_t)iter_capacity(max_iter));
        take(w.cpart, sizeof(double) * PSTRIDE * (size_t)w.blocks_cap * 2);  // two copies by pass parity (head close; else the first)
        // a steady launch's ranks are live chunks and workgroups of its grid, at most two per CU: a slot for each, both parities
        w.follow_cap = poses <= 1 ? (int)(w.blocks_cap < 2 * c->num_cus ? w.blocks_cap : 2 * c->num_cus) : 0;
        take(w.follow, sizeof(double) * FOLLOW_STRIDE * 2 * (size_t)w.follow_cap);
        // the ticket and the sixteen sign-off counters, a line each, and the live masks right behind them: one span
        // that starts every registration at zero (zeroed_span_bytes) -- nothing may come between these two
        take(w.ticket, 17 * 128);
        take(w.live, sizeof(unsigned long long) * 2 * (size_t)w.n_lw);  // live mask + the mask before the last rebuild
        take(w.live_list, sizeof(int32_t) * (size_t)w.blocks_cap);
        if (poses <= 1) {  // a batch fills every CU several times over anyway
            w.visit_cap = (int)(w.blocks_cap < 2 * c->num_cus ? w.blocks_cap : 2 * c->num_cus);
            // both parities of the visit plan, the durations (w.dur) right behind them: one span (plan_span_bytes)
            take(w.visit, (sizeof(int4) + sizeof(int2)) * 2 * (size_t)w.visit_cap);
        }
    }
    PEDP_REQUIRE(n_slots <= MAX_SLOTS, "pedp_icp: carve_workspace lays out %d buffers, its table holds %d", n_slots, MAX_SLOTS);
    off = align_up(off, 4096);
    w.pose_stride = off;  // a batch lays `poses` such blocks one behind the other
    int st = c->icp_ws.reserve(off * (size_t)(poses > 0 ? poses : 1));
    if (st) return st;
    for (int k = 0; k < n_slots; ++k) {
        char *buf = (char *)c->icp_ws.ptr + slot[k].off;
        memcpy((char *)&w + slot[k].member, &buf, sizeof(buf));  // (every member taken above is a plain object pointer)
    }
    if (w.visit) w.dur = (int2 *)(w.visit + 2 * (size_t)w.visit_cap);
    // the per-block survivor counters start at zero (the segment kernel re-zeroes them per pass)
    if (!fused) PEDP_HIP_CHECK(hipMemsetAsync(w.blk_cnt, 0, sizeof(int32_t) * (size_t)w.blocks_cap, c->stream));
    return PEDP_OK;
}

// Two spans of a fused workspace are cleared as a whole when a registration starts, from the first byte of their
// first buffer to the last byte of their last one.  carve_workspace takes their buffers one right behind the other.
//
// The ticket with the sign-off counters, then both live masks:
inline size_t zeroed_span_bytes(const IcpWorkspace &w) {
    if (!w.ticket) return 0;  // (segmented path)
    const unsigned long long *end = w.live + 2 * (size_t)w.n_lw;
    return (size_t)((const char *)end - (const char *)w.ticket);
}
// Both parities of the visit plan, then their durations (nothing where there is no plan):
inline size_t plan_span_bytes(const IcpWorkspace &w) {
    if (!w.visit) return 0;
    const int2 *end = w.dur + 2 * (size_t)w.visit_cap;
    return (size_t)((const char *)end - (const char *)w.visit);
}

// A workspace's view of the pair of clouds it works on: the target's sorted operand with the spheres of its units
// (qt tiles each) and of its mask words, its sorted rows, and both spatial orders.
void bind_clouds(IcpWorkspace &w, pedp_cloud_t source, pedp_cloud_t target, int qt) {
    w.source = source;
    w.target = target;
    w.tgt4 = (const float4 *)target->tgt4;
    w.word_sph = (const float4 *)target->tile_sphw;
    w.tgt_s = (const double *)target->tgt_s;
    w.tile_sph = (const float4 *)(qt == 4 ? target->tile_sph4 : target->tile_sph);
    w.tgt_perm = (const int32_t *)target->tile_perm;
    w.src_perm = (const int32_t *)source->perm;
}

// What the kernels derive from the correspondence radius r.  r_cull is the radius of the box test and of the sphere
// culling: r itself, or "infinite" in an exhaustive sweep (the selection still applies r).
struct IcpRadii {
    float r1;        // distance scale of the candidates the fp32 bound must hold for (anything farther is not an
                     // inlier anyway); huge radii fall back to the cloud scale inside the kernel
    float r_search;  // culling radius, rounded up
    float r2f;       // r^2 of the fp32 selection window, rounded up
    double r2cut;    // rounding-safe r^2 of the box test
};
inline IcpRadii icp_radii(double r, double r_cull) {
    IcpRadii k;
    k.r1 = (float)(r * 1.01);
    k.r_search = (float)(r_cull * (1.0 + 1e-6)) + 1e-6f;
    k.r2f = (float)(r * r) * 1.00001f;
    k.r2cut = r_cull * r_cull * (1.0 + 1e-12);
    return k;
}

// Every environment switch this file reads (include/pedp.h: pedp_icp_switches), asked once per process.  Each restores
// an earlier behaviour so that tests and A/B runs can compare the two sides bit for bit.
using IcpSwitches = pedp_icp_switches;
inline const IcpSwitches &icp_switches() {
    static const IcpSwitches sw = [] {
        auto flag = [](const char *name, int unset) { const char *v = getenv(name); return v ? atoi(v) != 0 : unset; };
        auto num = [](const char *name, int unset) { const char *v = getenv(name); return v && *v ? atoi(v) : unset; };
        const char *order = getenv("PEDP_ICP_TARGET_ORDER");
        IcpSwitches s;
        s.nn_f32 = flag("PEDP_NN_F32", 0); s.unfused_finish = flag("PEDP_ICP_UNFUSED_FINISH", 0);
        s.no_visit_plan = flag("PEDP_ICP_NO_VISIT_PLAN", 0); s.serial_close = flag("PEDP_ICP_SERIAL_CLOSE", 0);
        s.copy_bracket = flag("PEDP_ICP_COPY_BRACKET", 0); s.head_close = flag("PEDP_ICP_HEAD_CLOSE", 1);
        s.cert = flag("PEDP_ICP_CERT", 1); s.steady = flag("PEDP_ICP_STEADY", 1);
        s.steady_from = num("PEDP_ICP_STEADY_FROM", 5); s.steady_grid = num("PEDP_ICP_STEADY_GRID", 0);
        s.steady_closers = num("PEDP_ICP_STEADY_CLOSERS", 0); s.steady_groups = num("PEDP_ICP_STEADY_GROUPS", 0);
        s.lane_solve = num("PEDP_ICP_LANE_SOLVE", 1); s.pass_grid = num("PEDP_ICP_PASS_GRID", 0);
        s.target_order = order && !strcmp(order, "hilbert") ? PEDP_TARGET_ORDER_HILBERT
                         : order && !strcmp(order, "compact") ? PEDP_TARGET_ORDER_COMPACT : PEDP_TARGET_ORDER_AUTO;
        return s;
    }();
    return sw;
}

// What is decided for a registration (or a group of a fused batch) before anything is enqueued (include/pedp.h): everything
// the host code and the kernels' arguments branch on follows from these fields; no switch is read anywhere else.
using IcpPath = pedp_icp_path;
using IcpPathInputs = pedp_icp_path_inputs;
// the fused pass lists a target's mask words in LDS: up to BK_WCAP words of 1024 rows
inline bool fused_eligible(int qt, bool exhaustive, double r, int64_t Ns, int64_t Nt) {
    return qt == 1 && !exhaustive && r > 0.0 && Ns > 0 && Nt > 0 && (Nt + 1023) / 1024 <= BK_WCAP;
}
// Pure: no HIP call, no global.
inline IcpPath icp_decide_path(const IcpSwitches &sw, const IcpPathInputs &in) {
    IcpPath p{};
    p.fused = fused_eligible(in.unit_size, in.exhaustive, in.radius, in.n_source, in.n_target);
    p.copy_bracket = sw.copy_bracket; p.exchange = in.exchange;  // (the segmented path has both, too)
    p.steady_from = sw.steady_from < 1 ? 1 : sw.steady_from;
    if (!p.fused) return p;
    const bool single = in.poses <= 1;
    const bool closes_itself = !in.exchange && !sw.unfused_finish;  // the workgroup that finishes last closes the pass
    p.serial_close = sw.serial_close; p.unfused_finish = sw.unfused_finish;
    p.lane_solve = !sw.serial_close && sw.lane_solve > 0;  // (the wide close's solve; the one-lane close keeps its own)
    p.plan = single && !sw.no_visit_plan;  // (a batch fills every CU several times over anyway)
    p.certify = single && closes_itself && sw.cert;
    p.dev_result = single && !in.batch && closes_itself && !sw.copy_bracket;
    p.head = p.dev_result && !sw.serial_close && sw.head_close;
    // (a pass timed on its own, or every fourth one, is a launch of its own; -3 times the whole registration)
    p.steady = p.head && p.certify && sw.steady && !in.no_steady && !in.early_exit && (in.timed_pass == -1 || in.timed_pass == -3) &&
               in.resident;
    return p;
}

// The shape of a steady launch: wave groups per workgroup (the kernel's GROUPS) and workgroups, all of which must be resident at
// once -- so the grid is what the runtime says fits, hipOccupancyMaxActiveBlocksPerMultiprocessor x CUs, at most two workgroups
// per CU with one group (512 threads) and one with two (1,024 threads at 128 registers fill a CU).
// Two groups where a second workgroup per CU would have a rank: the scene has more chunks than the device has CUs (n_chunks
// bounds the live chunks from above); smaller scenes keep one group, the kernel they always ran.  PEDP_ICP_STEADY_GROUPS=1|2 forces
// the choice; PEDP_ICP_STEADY_GRID=n caps the workgroups (tests: several chunks per workgroup at a few hundred points) and implies
// one group where the other switch is unset.  An instantiation that cannot be resident falls back to one group; grid 0: that one
// cannot be either -- the registration keeps to generic launches.
struct SteadyShape { int groups, grid; };
inline int steady_per_cu(pedp_ctx_t c, int groups) {
    static std::atomic<int> per_cu[2][64];  // by instantiation and device; 0: not asked yet, -1: asked and refused
    const int dev = c->device >= 0 && c->device < 64 ? c->device : 0;
    int n = per_cu[groups - 1][dev].load(std::memory_order_relaxed);
    if (n == 0) {
        int nb = 0;
        // (a steady launch closes wide: its instantiation follows the process's PEDP_ICP_LANE_SOLVE alone)
        const bool lanes = icp_switches().lane_solve > 0;
        const hipError_t e = groups == 2 ? (lanes ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, icp_steady_kernel<2, true>, 2 * BK_W * 64, 0)
                                                  : hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, icp_steady_kernel<2, false>, 2 * BK_W * 64, 0))
                                         : (lanes ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, icp_steady_kernel<1, true>, BK_W * 64, 0)
                                                  : hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, icp_steady_kernel<1, false>, BK_W * 64, 0));
        if (e != hipSuccess || nb < 1) { (void)hipGetLastError(); nb = -1; }
        per_cu[groups - 1][dev].store(n = nb, std::memory_order_relaxed);
    }
    const int most = groups == 2 ? 1 : 2;
    return n < 1 ? 0 : (n < most ? n : most);
}
inline SteadyShape steady_shape(pedp_ctx_t c, int64_t n_chunks) {
    const IcpSwitches &sw = icp_switches();
    int groups = sw.steady_groups == 1 || sw.steady_groups == 2 ? sw.steady_groups : (sw.steady_grid <= 0 && n_chunks > c->num_cus ? 2 : 1);
    if (groups == 2 && steady_per_cu(c, 2) < 1) groups = 1;
    int64_t g = (int64_t)steady_per_cu(c, groups) * c->num_cus;
    if (sw.steady_grid > 0 && g > sw.steady_grid) g = sw.steady_grid;
    return {groups, (int)g};
}
// One steady launch at a time per device and process: two resident grids whose ranks together exceed what the device holds
// could each wait for workgroups the other keeps out (the bounded wait would turn that into PEDP_ERR_HIP).  A registration
// that finds the device taken keeps to generic launches.  (Other PROCESSES on the device are not seen from here.)
inline std::atomic<int> &steady_busy(int device) {
    static std::atomic<int> busy[64];
    return busy[device >= 0 && device < 64 ? device : 0];
}
inline bool steady_acquire(int device) {
    int free_ = 0;
    return steady_busy(device).compare_exchange_strong(free_, 1, std::memory_order_acq_rel);
}
inline void steady_release(int device) { steady_busy(device).store(0, std::memory_order_release); }

// Enqueue one correspondence pass (transform, sweep, fallback) between the workspace's clouds.  mode as in
// icp_transform_pack_kernel.
int enqueue_nn_pass(pedp_ctx_t c, const IcpWorkspace &w, int mode, const TargetPrep &tp, double r, hipEvent_t ev0, hipEvent_t ev1,
                    bool exhaustive) {
    const pedp_cloud_t src = w.source, tgt = w.target;
    const int64_t Ns = src->N, Nt = target_rows(tgt);
    // exhaustive: the box test and the sphere culling use an infinite radius (every point is a
    // candidate, every mask bit is set); the selection still applies r, so results do not change
    const IcpRadii rad = icp_radii(r, exhaustive ? 1e18 : r);
    const float r_search = rad.r_search, r2f = rad.r2f;
    const int n_tiles = (int)(w.Nt_pad / (16 * w.qt));  // target units
    // the dense sweep (units of four tiles) runs on the bf16 matrix pipe (PEDP_NN_F32=1: the f32-input MFMA of rounds 1-3)
    const bool bf16_sweep = w.qt == 4 && !icp_switches().nn_f32 && tgt->tgt_bf != nullptr;
    {
        int64_t grid = (Ns + 511) / 512;  // 128 points per wave, 4 waves per workgroup
        hipLaunchKernelGGL(icp_transform_pack_kernel, dim3((unsigned)grid), dim3(256), 0, c->stream, w.st, mode,
                           src->pts, w.P, w.src_perm, Ns, w.B, w.eps, w.S, w.list, w.blk_sph, w.idx, w.d2, tp.Tn, tp.T2,
                           rad.r1, rad.r2cut, tp.lo[0], tp.lo[1], tp.lo[2], tp.hi[0], tp.hi[1], tp.hi[2], bf16_sweep ? 34.0f : 5.0f);
    }
    const unsigned sel_grid = (unsigned)((4 * w.Ns_pad + 255) / 256);
    const unsigned sweep_grid = (unsigned)((w.max_segs + NN_WAVES - 1) / NN_WAVES);
    // ambiguous slots are a small fraction of the scene: one workgroup per 8 slots at most, two per CU at most
    int64_t fbg = w.Ns_pad / 8;
    if (fbg > 2 * c->num_cus) fbg = 2 * c->num_cus;
    if (fbg < 1) fbg = 1;
    const unsigned fb_grid = (unsigned)fbg;
    {
        const int64_t groups = (w.n_words + CULL_WORDS - 1) / CULL_WORDS;
        const int64_t waves = w.blocks_cap * groups;
        hipLaunchKernelGGL(nn_cull_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, c->stream, w.st, w.tile_sph,
                           n_tiles, w.n_words, w.blk_sph, r_search, w.mask, w.blk_cnt);
        hipLaunchKernelGGL(nn_segment_kernel, dim3(1), dim3(1024), 0, c->stream, w.st, w.blk_cnt, w.blk_segstart,
                           w.seg_blk, w.seg_rank0, w.seg_n, w.max_segs, SEG_MIN_TILES / w.qt, NN_LIST_TILES / w.qt);
    }
#define PEDP_NN_STAGE(QTV, SWEEP, TGT_OPERAND, B_OPERAND)                                                               \
    do {                                                                                                              \
        if (ev0) PEDP_HIP_CHECK(hipEventRecord(ev0, c->stream));                                                      \
        hipLaunchKernelGGL(SWEEP, dim3(sweep_grid), dim3(NN_WAVES * 64), 0, c->stream, w.st, TGT_OPERAND, n_tiles,     \
                           w.n_words, w.mask, w.seg_blk, w.seg_rank0, w.seg_n, B_OPERAND, w.tr_b1, w.tr_t1, w.tr_b2);  \
        if (ev1) { PEDP_HIP_CHECK(hipEventRecord(ev1, c->stream)); c->nn_timed = true; }                               \
        hipLaunchKernelGGL(nn_select_kernel<QTV>, dim3(sel_grid), dim3(256), 0, c->stream, w.st, w.blk_segstart,       \
                           w.tr_b1, w.tr_t1, w.tr_b2, tgt->pts, w.tgt_perm, Nt, w.P, w.eps, w.S, w.list, r2f, w.idx,   \
                           w.d2, w.fb);                                                                               \
        hipLaunchKernelGGL(nn_fallback_kernel<QTV>, dim3(fb_grid), dim3(FB_WAVES * 64), 0, c->stream, w.st, w.fb, w.list,     \
                           w.mask, w.n_words, w.tile_sph, r_search, tgt->pts, w.tgt_perm, Nt, w.P, w.idx, w.d2);       \
    } while (0)
    if (bf16_sweep) PEDP_NN_STAGE(4, (nn_sweep_bf16_kernel<4, 2>), (const uint4 *)tgt->tgt_bf, (const float4 *)w.B);
    else if (w.qt == 4) PEDP_NN_STAGE(4, (nn_sweep_kernel<4, 2>), (const float *)w.tgt4, (const float *)w.B);
    else PEDP_NN_STAGE(1, (nn_sweep_kernel<1, 4>), (const float *)w.tgt4, (const float *)w.B);
#undef PEDP_NN_STAGE
    PEDP_HIP_CHECK(hipGetLastError());
    return PEDP_OK;
}

// Margin of the live set beyond the correspondence radius (see the fused-pass comment).
inline double fused_margin(double r) { return 2.0 * r; }   // (1 r ... 4 r measured on the bench registration: 0.702-0.720 ms, no trend; any margin > 0 is exact)

// One registration = enqueue (all passes, on the executor's stream and workspace) + collect
// (one synchronisation, results to the host).  The executor is the clouds' own context for
// pedp_icp and one of its sub-contexts (own stream + workspace) for pedp_icp_batched, where
// several registrations are in flight at once.  A group of a fused batch is a job, too.
struct IcpJob {
    IcpWorkspace w;
    int max_iter = 0;
    IcpPathInputs in{};  // the registration's shape ...
    IcpPath path{};      // ... and what is decided from it, once, when the job is staged
    // holds the device's steady launch until collected: the passes from path.steady_from on run in icp_steady_kernel
    bool steady_held = false;
    TargetPrep tp{};
    int estimator = 0;
    bool want_trace = false;
    PassArgs pa{};  // fused path: what a pass kernel's arguments have in common over the job's launches (stage_pass_args)
};
constexpr size_t RESULT_OFF = pedp_pinned::ICP_RESULT.off;
static_assert(sizeof(IcpState) <= pedp_pinned::ICP_STATE.bytes && sizeof(IcpState) <= pedp_pinned::ICP_RESULT.bytes && sizeof(IcpState) % 8 == 0, "start and final state share the block's first 4 KB, as 8-byte words");

// The arguments of the job's pass kernels, from its workspace, clouds and path: filled once, copied per launch.
void stage_pass_args(pedp_ctx_t x, IcpJob &job) {
    const IcpWorkspace &w = job.w;
    const IcpPath &path = job.path;
    PassArgs &pa = job.pa;
    pa.src = w.source->pts; pa.perm = w.src_perm; pa.N = w.source->N; pa.n_chunks = w.n_chunks;
    pa.hist = w.hist; pa.Pk = w.Pk; pa.Tprev = w.Tprev; pa.live = w.live; pa.live_list = w.live_list;
    pa.chunk_sph = (const double *)w.source->chunk_sph;
    pa.pp_stride = 3 * (size_t)w.Ns_pad;
    pa.tgtf = (const float *)w.tgt4; pa.n_tiles = (int)(w.Nt_pad / 16); pa.n_words = w.n_words;
    pa.tile_sph = w.tile_sph; pa.word_sph = w.word_sph; pa.tgt_s = w.tgt_s; pa.tperm = w.tgt_perm; pa.Nt = target_rows(w.target);
    pa.tgt = w.target->pts; pa.nrm = w.target->normals;
    pa.Tn = job.tp.Tn; pa.T2 = job.tp.T2;
    for (int k = 0; k < 3; ++k) { pa.lo[k] = job.tp.lo[k]; pa.hi[k] = job.tp.hi[k]; pa.bc[k] = job.tp.bc[k]; }
    pa.estimator = job.estimator; pa.idx_out = w.idx; pa.partials = w.cpart;
    pa.pose_stride = job.in.poses > 1 ? w.pose_stride : 0;
    // the workgroup that finishes last closes the pass (sum, solve, update); otherwise icp_finish_kernel launches follow
    pa.fuse = !path.exchange && !path.unfused_finish ? 1 : 0;
    pa.n_lw = w.n_lw; pa.packet = w.packet; pa.trace = job.want_trace ? w.trace : nullptr; pa.ticket = w.ticket;
    pa.down = path.dev_result ? (unsigned long long *)((char *)x->pinned + RESULT_OFF) : nullptr;
    pa.serial_close = path.serial_close; pa.lane_solve = path.lane_solve; pa.head = path.head; pa.launch = 0;  // (the launch index is the launch's own)
    pa.part_stride = (size_t)PSTRIDE * (size_t)w.blocks_cap;
    pa.cert = path.certify ? w.cert : nullptr; pa.cert_stride = (size_t)w.Ns_pad;
    pa.visit = path.plan ? w.visit : nullptr; pa.dur = path.plan ? w.dur : nullptr; pa.visit_cap = w.visit_cap; pa.n_cu = x->num_cus;
}

// What one launch of a fused pass has of its own.
struct PassLaunch {
    int pass = 0;                // head close: the index of this launch = the pass it runs
    bool steady_launch = false;  // `pass` and every pass behind it that is fully certified, in one resident launch (steady_pass.h)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;  // around the launch (null: not timed)
};

// Enqueue the kernel of a fused pass of the job.
int enqueue_fused_pass(pedp_ctx_t c, const IcpJob &job, const PassLaunch &l) {
    PassArgs pa = job.pa;
    pa.launch = pa.head ? l.pass : 0;
    // grid-stride loop over the live chunks: any grid is correct; two workgroups per CU are resident
    int64_t g = job.w.n_chunks;
    if (g > 2 * c->num_cus) g = 2 * c->num_cus;
    // PEDP_ICP_PASS_GRID=n caps the generic pass kernels' workgroups with chunks (tests: many chunks per workgroup at a few hundred points)
    if (!l.steady_launch && icp_switches().pass_grid > 0 && g > icp_switches().pass_grid) g = icp_switches().pass_grid;
    if (g < 1) g = 1;
    if (pa.head) g += 1;  // head close: one workgroup more than the chunks can fill (the service workgroup)
    if (l.ev0) PEDP_HIP_CHECK(hipEventRecord(l.ev0, c->stream));
    if (l.steady_launch) {
        // workgroups below `closers` close a pass, the others follow one of them: one closer per CU unless the switch says otherwise
        const int asked = icp_switches().steady_closers;
        const SteadyShape sh = steady_shape(c, job.w.n_chunks);
        double *const follow = job.w.follow_cap > 0 ? job.w.follow : nullptr;
        const int n_closers = asked > 0 ? asked : c->num_cus;
        auto steady = [&](auto kernel, int groups) {
            hipLaunchKernelGGL(kernel, dim3((unsigned)sh.grid), dim3(groups * BK_W * 64), 0, c->stream, job.w.st, pa, follow, job.w.follow_cap, n_closers);
        };
        if (sh.groups == 2) { if (pa.lane_solve) steady(icp_steady_kernel<2, true>, 2); else steady(icp_steady_kernel<2, false>, 2); }
        else { if (pa.lane_solve) steady(icp_steady_kernel<1, true>, 1); else steady(icp_steady_kernel<1, false>, 1); }
    } else {
        // the instantiation: a batch's or a single registration's, with the close's solve a row per lane or on one lane
        const bool batch = job.in.poses > 1;
        auto pass = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3((unsigned)g, batch ? (unsigned)job.in.poses : 1u), dim3(BK_W * 64), 0, c->stream, job.w.st, pa);
        };
        if (batch) { if (pa.lane_solve) pass(icp_pass_kernel<BK_W, true, true>); else pass(icp_pass_kernel<BK_W, true, false>); }
        else { if (pa.lane_solve) pass(icp_pass_kernel<BK_W, false, true>); else pass(icp_pass_kernel<BK_W, false, false>); }
    }
    if (l.ev1) { PEDP_HIP_CHECK(hipEventRecord(l.ev1, c->stream)); c->nn_timed = true; }
    PEDP_HIP_CHECK(hipGetLastError());
    return PEDP_OK;
}

// The close of a fused pass as a launch of its own (icp_finish_kernel): one workgroup per pose of the job, their blocks
// pose_stride bytes apart.  stage 0: sum, solve, update; 1: sum only (the packet then goes through the exchange step);
// 2: solve from the summed packet.
void launch_finish(pedp_ctx_t x, const IcpJob &job, int stage) {
    const IcpWorkspace &w = job.w;
    hipLaunchKernelGGL(icp_finish_kernel, dim3((unsigned)job.in.poses), dim3(FIN_THREADS), 0, x->stream, w.st, w.live, w.live_list, w.n_lw,
                       w.cpart, w.packet, stage, job.estimator, job.pa.trace, w.hist, job.tp.bc[0], job.tp.bc[1], job.tp.bc[2],
                       job.pa.pose_stride, job.pa.serial_close, job.pa.lane_solve);
}

// Spatial order of a cloud, cached in the handle: a function of the cloud alone (cells over its own
// bounding box), built once, stream-ordered in pooled scratch (no allocation besides the order
// itself, no synchronisation).
int ensure_spatial_perm(pedp_ctx_t c, pedp_cloud_t cl) {
    if (cl->N == 0 || cl->perm) return PEDP_OK;
    const int64_t n_chunks = (cl->N + 127) / 128;
    size_t perm_cap = 0, sph_cap = 0;
    void *perm = c->cloud_pool.take(sizeof(int32_t) * (size_t)cl->N, &perm_cap);
    void *sph = c->cloud_pool.take(sizeof(double) * 32 * (size_t)n_chunks, &sph_cap);
    auto fail = [&](int rc, const char *what) {
        (void)hipStreamSynchronize(c->stream);
        c->cloud_pool.give(perm, perm_cap);
        c->cloud_pool.give(sph, sph_cap);
        if (what) pedp_set_error("pedp_icp: spatial order: %s", what);
        return rc;
    };
    if (!perm || !sph) return fail(PEDP_ERR_ALLOC, "allocation failed");
    unsigned long long *keys = nullptr;
    int rcs = pedp_sort_keys64_begin(c, cl->N, SORT_KEY_BITS, &keys);
    if (rcs) return fail(rcs, nullptr);
    const unsigned grid = (unsigned)((cl->N + 255) / 256);
    hipLaunchKernelGGL(cell_key_kernel, dim3(grid), dim3(256), 0, c->stream, cl->pts, cl->N, (const double *)cl->d_box, keys);
    rcs = pedp_sort_keys64_run(c, cl->N, SORT_KEY_BITS, (int32_t *)perm);
    if (rcs) return fail(rcs, nullptr);
    hipLaunchKernelGGL(chunk_sphere_kernel, dim3((unsigned)n_chunks), dim3(64), 0, c->stream, cl->pts, (const int32_t *)perm, cl->N,
                       (double *)sph);
    if (hipGetLastError() != hipSuccess) return fail(PEDP_ERR_HIP, "launch failed");
    cl->perm = perm; cl->perm_cap = perm_cap;
    cl->chunk_sph = sph; cl->sph_cap = sph_cap;
    return PEDP_OK;
}

// The pack's kernels over the target's tile order (tgt->tile_perm), into the pack's buffers where they are: the first
// build and every change of order.  A bf16 operand that exists follows.
int write_target_pack(pedp_ctx_t c, pedp_cloud_t tgt, const TargetPrep &tp) {
    const int64_t nt = target_rows(tgt), pad = tgt->tgt4_pad;
    const int64_t n_wsph = (pad / 16 + 63) / 64;  // one sphere per mask word of 16-row tiles (1024 rows)
    const int32_t *order = (const int32_t *)tgt->tile_perm;
    int64_t grid = (pad + 255) / 256;
    hipLaunchKernelGGL(pack_target_kernel, dim3((unsigned)grid), dim3(256), 0, c->stream, tgt->pts, order, nt, pad, tp.c[0], tp.c[1],
                       tp.c[2], (float4 *)tgt->tgt4);
    hipLaunchKernelGGL(tile_sphere_kernel, dim3((unsigned)((pad / 16 + 255) / 256)), dim3(256), 0, c->stream,
                       (const float4 *)tgt->tgt4, nt, pad / 16, 16, (float4 *)tgt->tile_sph);
    hipLaunchKernelGGL(tile_sphere_kernel, dim3((unsigned)((pad / 64 + 255) / 256)), dim3(256), 0, c->stream,
                       (const float4 *)tgt->tgt4, nt, pad / 64, 64, (float4 *)tgt->tile_sph4);
    hipLaunchKernelGGL(tile_sphere_kernel, dim3((unsigned)((n_wsph + 63) / 64)), dim3(64), 0, c->stream,
                       (const float4 *)tgt->tgt4, nt, n_wsph, 1024, (float4 *)tgt->tile_sphw);
    hipLaunchKernelGGL(sort_rows_kernel, dim3((unsigned)grid), dim3(256), 0, c->stream, tgt->pts, tgt->normals, order, nt, pad,
                       (double *)tgt->tgt_s);
    if (tgt->tgt_bf) {
        const int64_t n = pad * 4;
        hipLaunchKernelGGL(pack_target_bf16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream,
                           (const float4 *)tgt->tgt4, pad, (uint4 *)tgt->tgt_bf);
    }
    PEDP_HIP_CHECK(hipGetLastError());
    return PEDP_OK;
}

// The compact tile order (icp/target_order.h) into tgt->tile_perm, from the Hilbert pack that tgt->tgt4 holds.
int build_compact_order(pedp_ctx_t c, pedp_cloud_t tgt) {
    const int64_t nt64 = target_rows(tgt);
    if (nt64 <= 16) return PEDP_OK;  // one tile: the Hilbert order is the compact one
    const int nt = (int)nt64;
    const int n_blocks = (nt + TORD_BLOCK - 1) / TORD_BLOCK, levels = tord_top_levels(nt);
    const size_t rows = align_up(sizeof(int32_t) * (size_t)nt, 256);
    const size_t off_box = 3 * rows, off_seg = off_box + align_up(sizeof(float) * 6 * (size_t)n_blocks, 256);
    size_t cap = 0;
    char *ws = (char *)c->cloud_pool.take(off_seg + sizeof(int2) * (size_t)n_blocks, &cap);
    if (!ws) { pedp_set_error("pedp_icp: target order: allocation failed"); return PEDP_ERR_ALLOC; }
    int32_t *cur[2] = {(int32_t *)ws, (int32_t *)(ws + rows)}, *sigma = (int32_t *)(ws + 2 * rows);
    float *blk_box = (float *)(ws + off_box);
    int2 *blk_seg = (int2 *)(ws + off_seg);
    const float4 *t4 = (const float4 *)tgt->tgt4;
    int rc = PEDP_OK, side = 0;
    bool sorted = false;
    if (levels > 0) {
        int key_bits = 32;
        while (((int64_t)1 << (key_bits - 32)) < n_blocks) ++key_bits;
        unsigned long long *keys = nullptr;
        rc = pedp_sort_keys64_exact_begin(c, nt, key_bits, &keys);
        if (!rc) hipLaunchKernelGGL(tord_init_kernel, dim3((unsigned)((n_blocks + 255) / 256)), dim3(256), 0, c->stream, blk_seg, n_blocks, nt);
        for (int l = 0; l < levels && !rc; ++l) {
            hipLaunchKernelGGL(tord_block_box_kernel, dim3((unsigned)n_blocks), dim3(256), 0, c->stream, t4, (const int32_t *)cur[side],
                               sorted ? (const int32_t *)sigma : nullptr, cur[side ^ 1], nt, blk_box);
            side ^= 1;
            hipLaunchKernelGGL(tord_key_kernel, dim3((unsigned)n_blocks), dim3(256), 0, c->stream, t4, (const int32_t *)cur[side], nt,
                               (const float *)blk_box, blk_seg, keys);
            rc = pedp_sort_keys64_exact_run(c, nt, key_bits, sigma);
            sorted = true;
        }
    }
    if (!rc) {
        hipLaunchKernelGGL(tord_leaf_kernel, dim3((unsigned)n_blocks), dim3(256), 0, c->stream, t4, (const int32_t *)cur[side],
                           sorted ? (const int32_t *)sigma : nullptr, (const int32_t *)tgt->perm, nt, (int32_t *)tgt->tile_perm);
        if (hipGetLastError() != hipSuccess) { pedp_set_error("pedp_icp: target order: launch failed"); rc = PEDP_ERR_HIP; }
    }
    if (rc) (void)hipStreamSynchronize(c->stream);
    c->cloud_pool.give(ws, cap);  // (reuse is ordered by the stream)
    return rc;
}

// Which order a target's pack should have now.  Automatic mode: the Hilbert runs that the first registration gets for
// the price of five launches, the compact order from the second registration on against targets large enough that the
// shorter tile lists pay the build back, unless PEDP_ICP_TARGET_ORDER decides for every cloud in
// automatic mode.
constexpr int64_t TORD_AUTO_MIN_ROWS = 16384;
constexpr int TORD_AUTO_REGISTRATION = 2;
// a registration against tgt has been enqueued whole (counted up to the one that upgrades the order)
inline void count_registration(pedp_cloud_t tgt) {
    if (tgt->registrations < TORD_AUTO_REGISTRATION) ++tgt->registrations;
}
// upcoming: the call is a registration (it becomes number registrations + 1 once its passes are enqueued)
inline int target_order_wanted(pedp_cloud_t tgt, bool upcoming) {
    if (tgt->order_mode != PEDP_TARGET_ORDER_AUTO) return tgt->order_mode;
    if (icp_switches().target_order != PEDP_TARGET_ORDER_AUTO) return icp_switches().target_order;
    return tgt->registrations + (upcoming ? 1 : 0) >= TORD_AUTO_REGISTRATION && target_rows(tgt) >= TORD_AUTO_MIN_ROWS ? PEDP_TARGET_ORDER_COMPACT
                                                                                                 : PEDP_TARGET_ORDER_HILBERT;
}

// Target-side operand of the sweep, built once per cloud and kept in the handle (the
// reference re-runs ICP ~50x per frame against the same model, pose_estimation.py:577-613).
// Its rows follow the target's tile order: the cloud's Hilbert order at first, the compact order once that is
// wanted (target_order_wanted).  A change of order rewrites the pack where it is -- no buffer moves, so captured
// graphs and sub-contexts stay valid -- in front of the caller's passes on the owner's stream.
int ensure_target_pack(pedp_ctx_t c, pedp_cloud_t tgt, TargetPrep &tp, bool registration = false) {
    { const int rs = pedp_cloud_host_stats(c, tgt); if (rs) return rs; }
    for (int k = 0; k < 3; ++k) tp.c[k] = tgt->centroid[k];
    tp.Tn = tgt->Tn;
    tp.T2 = tgt->T2;
    for (int k = 0; k < 3; ++k) { tp.lo[k] = tgt->lo[k]; tp.hi[k] = tgt->hi[k]; tp.bc[k] = 0.5 * (tp.lo[k] + tp.hi[k]); }
    const int want = target_order_wanted(tgt, registration);
    if (tgt->tgt4 && tgt->order_in_force == want) return PEDP_OK;
    int rc = ensure_spatial_perm(c, tgt);
    if (rc) return rc;
    if (!tgt->tgt4) {
        // real tiles rounded to NN_TU, plus readable pad tiles the pipelined sweep may prefetch
        int64_t pad = (int64_t)align_up((size_t)(tgt->N > 0 ? tgt->N : 1), 16 * NN_TU) + 16 * NN_TILE_PAD;
        // all or none: a half-built pack must not look finished to the next call
        const int64_t n_wsph = (pad / 16 + 63) / 64;
        void *buf[6] = {};  // the operand, the spheres of 16 / 64 / 1024 rows, the sorted rows, the tile order
        const size_t bytes[6] = {sizeof(float4) * (size_t)pad, sizeof(float4) * (size_t)(pad / 16), sizeof(float4) * (size_t)(pad / 64),
                                 sizeof(float4) * (size_t)n_wsph, sizeof(double) * 6 * (size_t)pad, sizeof(int32_t) * (size_t)(tgt->N > 0 ? tgt->N : 1)};
        hipError_t e = hipSuccess;
        for (int k = 0; k < 6 && e == hipSuccess; ++k) e = hipMalloc(&buf[k], bytes[k]);
        if (e != hipSuccess) {
            for (void *b : buf)
                if (b) (void)hipFree(b);
            pedp_set_error("pedp_icp: target pack allocation failed: %s", hipGetErrorString(e));
            return PEDP_ERR_ALLOC;
        }
        tgt->tgt4 = buf[0]; tgt->tile_sph = buf[1]; tgt->tile_sph4 = buf[2]; tgt->tile_sphw = buf[3]; tgt->tgt_s = buf[4]; tgt->tile_perm = buf[5];
        tgt->tgt4_pad = pad;
        tgt->order_in_force = PEDP_TARGET_ORDER_AUTO;  // (none yet)
    }
    if (tgt->order_in_force != PEDP_TARGET_ORDER_HILBERT) {  // the Hilbert pack: what is wanted, or what the split starts from
        tgt->order_in_force = PEDP_TARGET_ORDER_AUTO;  // (no order holds while the pack is rewritten: a failure leaves "none")
        if (tgt->N > 0)
            PEDP_HIP_CHECK(hipMemcpyAsync(tgt->tile_perm, tgt->perm, sizeof(int32_t) * (size_t)tgt->N, hipMemcpyDeviceToDevice, c->stream));
        rc = write_target_pack(c, tgt, tp);
        if (rc) return rc;
        tgt->order_in_force = PEDP_TARGET_ORDER_HILBERT;
    }
    if (want == PEDP_TARGET_ORDER_COMPACT) {
        tgt->order_in_force = PEDP_TARGET_ORDER_AUTO;
        rc = build_compact_order(c, tgt);
        if (!rc) rc = write_target_pack(c, tgt, tp);
        if (rc) return rc;  // (rebuilt from the Hilbert order next time)
        tgt->order_in_force = PEDP_TARGET_ORDER_COMPACT;
    }
    return PEDP_OK;
}

// The bf16 pieces of the sorted operand, for the dense sweep: built when a call first takes that path
int ensure_target_bf16(pedp_ctx_t c, pedp_cloud_t tgt) {
    if (tgt->tgt_bf || !tgt->tgt4 || icp_switches().nn_f32) return PEDP_OK;
    void *p = nullptr;
    if (hipMalloc(&p, sizeof(uint4) * 4 * (size_t)tgt->tgt4_pad) != hipSuccess) {
        pedp_set_error("pedp_icp: target pack allocation failed (bf16 operand)");
        return PEDP_ERR_ALLOC;
    }
    tgt->tgt_bf = p;
    const int64_t n = tgt->tgt4_pad * 4;
    hipLaunchKernelGGL(pack_target_bf16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, (const float4 *)tgt->tgt4,
                       tgt->tgt4_pad, (uint4 *)tgt->tgt_bf);
    PEDP_HIP_CHECK(hipGetLastError());
    return PEDP_OK;
}

int icp_check_args(pedp_ctx_t c, pedp_cloud_t source, pedp_cloud_t target, const pedp_icp_params *prm) {
    PEDP_REQUIRE(source->ctx == c && target->ctx == c, "pedp_icp: cloud belongs to another context");
    PEDP_REQUIRE(prm->estimator == PEDP_POINT_TO_PLANE || prm->estimator == PEDP_POINT_TO_POINT,
                 "pedp_icp: unknown estimator %d", prm->estimator);
    PEDP_REQUIRE(prm->max_iteration >= 0 && prm->max_iteration <= 100000, "pedp_icp: max_iteration out of range");
    PEDP_REQUIRE(!prm->use_comm || c->comm, "pedp_icp: use_comm is set but the context has no communicator (pedp_comm_create)");
    PEDP_REQUIRE(!(prm->use_comm && prm->allreduce), "pedp_icp: use_comm and an all-reduce hook are exclusive");
    if (prm->estimator == PEDP_POINT_TO_PLANE && !target->has_normals) {
        pedp_set_error("pedp_icp: TransformationEstimationPointToPlane requires target normals");
        return PEDP_ERR_NO_NORMALS;
    }
    return PEDP_OK;
}

// unit size: fine units while the radius is small against the model (culling decides the
// cost), 64-row units when the sweep is dense anyway (cheaper epilogue)
int icp_unit_size(pedp_cloud_t target, double r) {
    double diag2 = 0.0;
    for (int k = 0; k < 3; ++k) diag2 += (target->hi[k] - target->lo[k]) * (target->hi[k] - target->lo[k]);
    return (r * r < diag2 / 16.0) ? 1 : 4;
}

// Cached per-cloud preparation on the owner's stream: sorted target operand + unit spheres, spatial
// order of the scene.
int icp_prepare(pedp_ctx_t c, pedp_cloud_t source, pedp_cloud_t target, const pedp_icp_params *prm, TargetPrep &tp) {
    int rc = icp_check_args(c, source, target, prm);
    if (rc) return rc;
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    rc = ensure_target_pack(c, target, tp, true);
    if (rc) return rc;
    rc = ensure_target_bf16(c, target);   // (with the pack, on the owner's stream: sub-contexts start after it is complete)
    if (rc) return rc;
    return ensure_spatial_perm(c, source);
}

// What a caller asks of one registration.
enum { ICP_TRACE = 1, ICP_EARLY_STOP = 2 /* pedp_icp: look at `done` behind every 8th launch */, ICP_NO_STEADY = 4 /* generic launches only */ };
struct IcpCall {
    pedp_cloud_t source, target;
    const TargetPrep *tp;
    const pedp_icp_params *prm;
    const double *init;
    unsigned how;  // ICP_* bits
};

// start state of a registration in the executor's pinned block (uploaded by the first node of
// icp_enqueue; the same block receives the final state)
void icp_fill_state(IcpState *dst, const TargetPrep &tp, const double init[16], const pedp_icp_params *prm, int64_t Ns) {
    IcpState h{};
    static std::atomic<int> registration_counter{0};
    h.nonce = ((registration_counter.fetch_add(1, std::memory_order_relaxed) & 0x3FFF) + 1) << 16;
    for (int k = 0; k < 16; ++k) { h.T[k] = init[k]; h.upd[k] = init[k]; h.T_init[k] = init[k]; }
    for (int k = 0; k < 3; ++k) h.centroid[k] = tp.c[k];
    h.rebuild = 1;  // fused pass: pass 0 builds the live chunk set from the whole scene
    const double r = prm->max_correspondence_distance, margin = fused_margin(r);
    double rho2 = 0.0;
    for (int k = 0; k < 3; ++k) rho2 += 0.25 * (tp.hi[k] - tp.lo[k]) * (tp.hi[k] - tp.lo[k]);
    h.r2 = r * r;
    const IcpRadii rad = icp_radii(r, r);
    h.r2cut = rad.r2cut;
    h.r2live = (r + margin) * (r + margin) * (1.0 + 1e-12);
    h.reachE = r + margin + std::sqrt(rho2);
    h.margin = margin;
    h.rel_fitness = prm->relative_fitness;
    h.rel_rmse = prm->relative_rmse;
    const double ng = prm->n_source_global > 0 ? (double)prm->n_source_global : (double)Ns;
    h.n_source = ng > 0 ? ng : 1.0;
    h.r1 = rad.r1;
    h.r_search = rad.r_search;
    h.wide_radius = (float)r;
    h.r2f = rad.r2f;
    h.max_iter = prm->max_iteration;
    *dst = h;
}

// The closing workgroup that ends the registration writes its final state RESULT_OFF bytes into the page-locked
// block; until then the slot says "not done" (called in front of every enqueue or replay, with the stream's earlier
// registration collected).
void icp_arm_result(pedp_ctx_t x) { ((IcpState *)((char *)x->pinned + RESULT_OFF))->done = 0; }

// Timing events of a pass, as pedp_icp_configure's timed_pass asks: that one pass (the pair nn_ev0/1); -2: every
// fourth pass from pass 1 on, up to eight pairs, whose mean pedp_nn_last_sweep_ms reports; -3: ONE pair around all
// the passes' launches, the mean launch-to-launch span.  Null events: the pass is not timed.
int pass_timing_events(pedp_ctx_t x, int timed_pass, int pass, int max_iter, hipEvent_t &ev0, hipEvent_t &ev1) {
    ev0 = ev1 = nullptr;
    if (pass == timed_pass) { ev0 = x->nn_ev0; ev1 = x->nn_ev1; }
    if (timed_pass == -3) {
        if (pass == 0) { ev0 = x->nn_ev0; x->nn_span_launches = max_iter + 1; }
        if (pass == max_iter) ev1 = x->nn_ev1;
    }
    if (timed_pass == -2 && (pass & 3) == 1 && x->nn_pairs < 8) {
        for (int k = 0; k < 2; ++k)
            if (!x->nn_evs[2 * x->nn_pairs + k]) PEDP_HIP_CHECK(hipEventCreate(&x->nn_evs[2 * x->nn_pairs + k]));
        ev0 = x->nn_evs[2 * x->nn_pairs];
        ev1 = x->nn_evs[2 * x->nn_pairs + 1];
        ++x->nn_pairs;
    }
    return PEDP_OK;
}

// The exchange step of a sharded registration: the packet summed over the ranks, on x's stream -- by the library's own
// RCCL all-reduce (use_comm) or by the caller's hook.  On failure the stream is drained before the error is returned.
int exchange_packet(pedp_ctx_t x, const pedp_icp_params *prm, double *packet, int pass) {
    if (prm->use_comm) {
        const int rc = pedp_comm_allreduce_sum_f64(x, packet, PACKET);
        if (rc) (void)hipStreamSynchronize(x->stream);
        return rc;
    }
    if (prm->allreduce && prm->allreduce(prm->allreduce_user, packet, PACKET, (void *)x->stream) != 0) {
        pedp_set_error("pedp_icp: all-reduce hook failed in pass %d", pass);
        (void)hipStreamSynchronize(x->stream);
        return PEDP_ERR_COLLECTIVE;
    }
    return PEDP_OK;
}

// every pass of one registration on x's stream; nothing here allocates or synchronises unless
// early_stop is set, so the sequence can be captured into a graph
int icp_enqueue(pedp_ctx_t x, const pedp_icp_params *prm, bool early_stop, const IcpJob &job) {
    const IcpWorkspace &w = job.w;
    const IcpPath &path = job.path;
    const int64_t Ns = job.in.n_source, Nt = job.in.n_target;
    const int max_iter = prm->max_iteration;
    const double r = prm->max_correspondence_distance;
    const double n_global = prm->n_source_global > 0 ? (double)prm->n_source_global : (double)Ns;
    int rc;
    // Open3D: max_correspondence_distance <= 0 or an empty cloud gives an empty result (never on the fused path)
    const bool degenerate = (r <= 0.0 || Ns == 0 || Nt == 0);
    IcpState *hp = pedp_pinned_at<IcpState>(x, pedp_pinned::ICP_STATE);
    const double r2 = r * r;
    const double ng = n_global > 0 ? n_global : 1.0;
    const bool fused = path.fused, head = path.head;
    int launches = 0;
    double *trace = job.want_trace ? w.trace : nullptr;
    // Fused: tickets, sign-off counters and both live masks start at zero (they lie one behind the other); the start
    // transformation -- slot 0 of the history -- arrives inside the state; pass 0 itself writes "no correspondence" for
    // every chunk it does not visit.
    if (path.copy_bracket) {
        PEDP_HIP_CHECK(hipMemcpyAsync(w.st, hp, sizeof(IcpState), hipMemcpyHostToDevice, x->stream));
        if (fused) PEDP_HIP_CHECK(hipMemsetAsync(w.ticket, 0, zeroed_span_bytes(w), x->stream));
    } else  // state, zeroes and an empty visit plan in one launch (the plan and the durations lie one behind the other)
        hipLaunchKernelGGL(icp_state_start_kernel, dim3(1), dim3(256), 0, x->stream, (const unsigned long long *)hp, (unsigned long long *)w.st,
                           (int)(sizeof(IcpState) / 8), (unsigned long long *)w.ticket, (int)(zeroed_span_bytes(w) / 8),
                           (unsigned long long *)w.visit, (int)(plan_span_bytes(w) / 8), head ? 2 : 1);  // (null spans off the fused path)
    PEDP_HIP_CHECK(hipGetLastError());
    if (job.in.timed_pass != -1) { x->nn_pairs = 0; x->nn_span_launches = 1; }
    for (int pass = 0; pass <= max_iter; ++pass) {
        PassLaunch l{pass};
        if (job.steady_held && pass == path.steady_from) {
            // this pass and all behind it in one launch; what it hands back icp_collect continues (the second event of
            // timed_pass = -3 stands behind the launch that ends the registration: this one, unless it hands back)
            rc = pass_timing_events(x, job.in.timed_pass, max_iter, max_iter, l.ev0, l.ev1);
            if (rc) return rc;
            l.ev0 = nullptr;
            l.steady_launch = true;
            rc = enqueue_fused_pass(x, job, l);
            if (rc) return rc;
            x->icp_last_launches = max_iter + 1;  // (the passes this enqueue covers)
            break;
        }
        rc = pass_timing_events(x, job.in.timed_pass, pass, max_iter, l.ev0, l.ev1);
        if (rc) return rc;
        x->icp_last_launches = ++launches;  // passes enqueued (statistics: the early exit stops enqueuing)
        if (fused) {
            rc = enqueue_fused_pass(x, job, l);
            if (rc) return rc;
            if (path.exchange) {  // sum -> all-reduce over the ranks -> solve
                launch_finish(x, job, 1);
                rc = exchange_packet(x, prm, w.packet, pass);
                if (rc) return rc;
                launch_finish(x, job, 2);
            } else if (path.unfused_finish)
                launch_finish(x, job, 0);
            PEDP_HIP_CHECK(hipGetLastError());
        } else {
            if (!degenerate) {
                rc = enqueue_nn_pass(x, w, pass == 0 ? 0 : 1, job.tp, r, l.ev0, l.ev1, job.in.exhaustive);
                if (rc) return rc;
                hipLaunchKernelGGL(icp_accumulate_kernel, dim3(ACC_BLOCKS), dim3(ACC_THREADS), 0, x->stream, w.st,
                                   prm->estimator, w.P, Ns, w.target->pts, w.target->normals, w.idx, w.d2, r2, w.partials);
                if (path.exchange) hipLaunchKernelGGL(icp_reduce_kernel, dim3(1), dim3(64), 0, x->stream, w.st, w.partials, w.packet);
            } else {
                PEDP_HIP_CHECK(hipMemsetAsync(w.packet, 0, sizeof(double) * 32, x->stream));
                if (pass == 0 && Ns > 0) PEDP_HIP_CHECK(hipMemsetAsync(w.idx, 0xFF, sizeof(int32_t) * (size_t)Ns, x->stream));
            }
            rc = exchange_packet(x, prm, w.packet, pass);  // (nothing without an exchange)
            if (rc) return rc;
            // A fused accumulate + solve (last workgroup done runs the solve) was measured slower:
            // the device-scope release every workgroup needs writes the whole L2 back (43 us vs 12 + 16).
            const double *fold = (!degenerate && !path.exchange) ? w.partials : nullptr;
            hipLaunchKernelGGL(icp_solve_kernel, dim3(1), dim3(256), 0, x->stream, w.st, w.packet, fold, pass, max_iter,
                               prm->estimator, ng, prm->relative_fitness, prm->relative_rmse, trace);
            PEDP_HIP_CHECK(hipGetLastError());
        }
        // Passes after convergence are no-ops on the device but still cost launches; with the
        // early exit enabled, look at the flag every 8th pass (one 4-byte read-back, identical
        // on every rank of a sharded run) and stop enqueuing once it is set.
        if (early_stop && prm->relative_fitness >= 0.0 && (pass & 7) == 7 && pass < max_iter) {
            int *flag = pedp_pinned_at<int>(x, pedp_pinned::ICP_DONE);
            // (head close: whoever ends the registration writes `done` into the slot of the pass behind the one it closed,
            // either parity; the other slot's `done` stays 0 -- both are read)
            flag[1] = 0;
            PEDP_HIP_CHECK(hipMemcpyAsync(flag, &w.st->done, sizeof(int), hipMemcpyDeviceToHost, x->stream));
            if (head) PEDP_HIP_CHECK(hipMemcpyAsync(flag + 1, &(w.st + 1)->done, sizeof(int), hipMemcpyDeviceToHost, x->stream));
            PEDP_HIP_CHECK(hipStreamSynchronize(x->stream));
            if (flag[0] || flag[1]) break;
        }
    }
    if (!path.dev_result) PEDP_HIP_CHECK(hipMemcpyAsync(hp, w.st, sizeof(IcpState), hipMemcpyDeviceToHost, x->stream));
    return PEDP_OK;
}

// A registration made ready on executor x: its path, workspace (may grow the executor's scratch buffer) and pass arguments,
// its start state in x's pinned block, the result slot armed.  (All that a replay of a captured graph needs.)
int icp_stage(pedp_ctx_t x, const IcpCall &call, IcpJob &job) {
    PEDP_HIP_CHECK(hipSetDevice(x->device));
    const pedp_icp_params *prm = call.prm;
    job.max_iter = prm->max_iteration;
    job.tp = *call.tp; job.estimator = prm->estimator; job.want_trace = call.how & ICP_TRACE;
    IcpPathInputs &in = job.in;
    in.n_source = call.source->N; in.n_target = target_rows(call.target); in.radius = prm->max_correspondence_distance;
    in.exhaustive = x->icp_exhaustive; in.unit_size = in.exhaustive ? 4 : icp_unit_size(call.target, in.radius);
    in.exchange = prm->allreduce || prm->use_comm; in.poses = 1; in.timed_pass = x->icp_timed_pass;
    // (pedp_icp's look at `done` behind every 8th launch needs launches to look behind)
    in.early_exit = (call.how & ICP_EARLY_STOP) && prm->relative_fitness >= 0.0;
    in.no_steady = (call.how & ICP_NO_STEADY) != 0;
    in.resident = 1;  // (asked of the runtime only where everything else allows the steady launch)
    job.path = icp_decide_path(icp_switches(), in);
    if (job.path.steady && steady_shape(x, (in.n_source + CH - 1) / CH).grid <= 0) { in.resident = 0; job.path = icp_decide_path(icp_switches(), in); }
    int rc = carve_workspace(x, job.in.n_source, job.in.n_target, job.max_iter, job.in.unit_size, job.w, job.path.fused);
    if (rc) return rc;
    bind_clouds(job.w, call.source, call.target, job.in.unit_size);
    if (job.path.fused) stage_pass_args(x, job);
    icp_fill_state(pedp_pinned_at<IcpState>(x, pedp_pinned::ICP_STATE), *call.tp, call.init, prm, call.source->N);
    icp_arm_result(x);
    return PEDP_OK;
}
// ... and started: every pass enqueued on x's stream
int icp_start(pedp_ctx_t x, const IcpCall &call, IcpJob &job) {
    int rc = icp_stage(x, call, job);
    if (rc) return rc;
    if (job.path.steady && call.prm->max_iteration >= job.path.steady_from) job.steady_held = steady_acquire(x->device);
    rc = icp_enqueue(x, call.prm, call.how & ICP_EARLY_STOP, job);
    if (rc && job.steady_held) { steady_release(x->device); job.steady_held = false; }
    return rc;
}

int icp_collect(pedp_ctx_t x, const IcpJob &job, double T_out[16], double *fitness, double *inlier_rmse,
                int32_t *n_iter_done, int32_t *corr, double *trace) {
    PEDP_HIP_CHECK(hipSetDevice(x->device));
    const IcpWorkspace &w = job.w;
    long long handbacks = 0;
    struct SteadyHold {  // (released on every way out of here, once the stream has been waited for)
        int device; bool held;
        ~SteadyHold() { if (held) steady_release(device); }
    } hold{x->device, job.steady_held};
    if (job.steady_held) {
        // A steady launch either ends the registration or hands it back with the state of the pass that is to run next
        // (in its slot, and a marked copy in the page-locked block): two generic launches from that pass, the steady
        // launch again, until the registration is over.  Each round runs at least one pass.
        PEDP_HIP_CHECK(hipStreamSynchronize(x->stream));
        IcpState *res = (IcpState *)((char *)x->pinned + RESULT_OFF);
        while (res->done == STEADY_HANDBACK) {
            ++handbacks;
            const int from = res->pass;
            res->done = 0;
            for (int pass = from; pass <= job.max_iter && pass <= from + 2; ++pass) {
                const int rc = enqueue_fused_pass(x, job, PassLaunch{pass, pass == from + 2});
                if (rc) return rc;
            }
            if (job.in.timed_pass == -3) { PEDP_HIP_CHECK(hipEventRecord(x->nn_ev1, x->stream)); }
            PEDP_HIP_CHECK(hipStreamSynchronize(x->stream));
        }
    }
    bool copies = false;
    if (corr && job.in.n_source > 0)
        { int dn_ = pedp_download(x, corr, w.idx, sizeof(int32_t) * (size_t)job.in.n_source); if (dn_) return dn_; copies = true; }
    if (trace) {
        PEDP_HIP_CHECK(hipMemcpyAsync(trace, w.trace, sizeof(double) * 18 * (size_t)(job.max_iter + 1), hipMemcpyDeviceToHost, x->stream));
        copies = true;
    }
    if (copies || !job.steady_held) PEDP_HIP_CHECK(hipStreamSynchronize(x->stream));
    const IcpState *hp = (const IcpState *)((const char *)x->pinned + (job.path.dev_result ? RESULT_OFF : pedp_pinned::ICP_STATE.off));
    if (job.path.dev_result && hp->done == 0) {  // (armed by icp_arm_result; the workgroup that sets `done` writes the state)
        pedp_set_error("pedp_icp: the registration's final state did not arrive");
        return PEDP_ERR_HIP;
    }
    if (hp->done < 0) {
        pedp_set_error("pedp_icp: a pass could not be closed (workgroups of its launch did not sign off in time)");
        return PEDP_ERR_HIP;
    }
    for (int k = 0; k < 16; ++k) T_out[k] = hp->T[k];
    // (scene slot, target point) pairs the MFMAs evaluated: fused pass counts 16 x 16 wave-tiles, the segmented path units x 128 slots
    x->icp_last_cand = job.path.fused ? hp->sum_tiles * 256 : hp->sum_tiles * (16 * job.in.unit_size) * (NN_SB * 16);
    x->icp_last_fb = hp->sum_fb;
    x->icp_last_passes = hp->iters + 1;
    x->icp_last_planned = hp->n_planned;
    x->icp_last_wide = hp->n_wide;
    x->icp_last_lane = hp->n_lane;
    x->icp_last_head = hp->n_head;
    x->icp_last_cert = hp->sum_cert;
    x->icp_last_searched = hp->sum_searched;
    x->icp_last_steady = hp->n_steady;
    x->icp_last_handbacks = handbacks;
    x->icp_last_followed = hp->n_followed;
    x->icp_last_rebuilds = hp->n_rebuilds;
    x->icp_last_bracket = (job.path.copy_bracket ? 0 : 1) + (job.path.dev_result ? 2 : 0);
    x->icp_last_nt = job.in.n_target;
    if (fitness) *fitness = hp->fitness;
    if (inlier_rmse) *inlier_rmse = hp->rmse;
    if (n_iter_done) *n_iter_done = hp->iters;
    return PEDP_OK;
}

// Batched registrations on the SEGMENTED path (dense sweeps, large radii) are bound by the launch
// rate of their short kernels, so a sub-context captures the whole pass sequence of a registration
// once into a hipGraph and replays it per start pose: the graph's nodes read the start state from
// the executor's pinned block and everything else from device memory.  Anything the captured
// launches depend on is in the key.
bool graph_key_equal(const pedp_icp_graph_key &a, const pedp_icp_graph_key &b) {
    return a.src_gen == b.src_gen && a.tgt_gen == b.tgt_gen && a.ws == b.ws && a.Ns == b.Ns && a.Nt == b.Nt &&
           a.max_iter == b.max_iter && a.qt == b.qt && a.estimator == b.estimator && a.r == b.r &&
           a.rel_fitness == b.rel_fitness && a.rel_rmse == b.rel_rmse && a.seg == b.seg && a.poses == b.poses;
}

// What `enqueue` puts on x's stream, captured into a graph and instantiated into `exec` (whose earlier graph goes).
// Returns enqueue's error.  `exec` stays null where capture or instantiation failed; `e` says why.
template <typename Enqueue>
int capture_graph(pedp_ctx_t x, hipGraphExec_t &exec, hipError_t &e, Enqueue enqueue) {
    if (exec) { (void)hipGraphExecDestroy(exec); exec = nullptr; }
    e = hipStreamBeginCapture(x->stream, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) return PEDP_OK;
    hipGraph_t graph = nullptr;
    const int rc = enqueue();
    e = hipStreamEndCapture(x->stream, &graph);
    if (!rc && e == hipSuccess && graph) {
        e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        if (e == hipSuccess) ++x->icp_graph_captures;
        else exec = nullptr;
    }
    if (graph) (void)hipGraphDestroy(graph);
    return rc;
}

int icp_launch_replayed(pedp_ctx_t x, const IcpCall &call, IcpJob &job) {
    int rc = icp_stage(x, call, job);  // (ICP_NO_STEADY: a captured graph holds generic launches only)
    if (rc) return rc;
    const pedp_icp_params *prm = call.prm;
    pedp_icp_graph_key key;
    key.src_gen = call.source->gen; key.tgt_gen = call.target->gen; key.ws = x->icp_ws.ptr;
    key.Ns = job.in.n_source; key.Nt = job.in.n_target; key.max_iter = job.max_iter; key.qt = job.in.unit_size; key.estimator = prm->estimator;
    key.r = prm->max_correspondence_distance; key.rel_fitness = prm->relative_fitness; key.rel_rmse = prm->relative_rmse;
    key.seg = job.path.fused ? -1 : 0;
    const bool same = x->icp_graph && graph_key_equal(x->icp_graph_key, key);
    if (!same) {
        hipError_t e;
        rc = capture_graph(x, x->icp_graph, e, [&] { return icp_enqueue(x, prm, false, job); });
        if (rc) return rc;
        (void)hipGetLastError();
        if (!x->icp_graph)  // capture unavailable: plain launches, same work
            return icp_enqueue(x, prm, false, job);
        x->icp_graph_key = key;
    }
    PEDP_HIP_CHECK(hipGraphLaunch(x->icp_graph, x->stream));
    return PEDP_OK;
}

// Batched registrations on the FUSED path share their launches: pose b of a group is blockIdx.y
// of the chunk kernel and blockIdx.x of the finish kernel, and owns one of `G` equal blocks of the
// workspace.  One captured graph holds `seg` passes (two launches each, no copies) for the whole
// group; the start states are uploaded in front of the first replay, the states are read back
// behind every replay, and the graph is replayed until every pose reports done.  Radius, criteria,
// pass counter and iteration limit live in the device state, so the same graph serves any start
// poses -- and a group that converges after 7 iterations costs 10 passes of launches, not 31.
constexpr int BATCH_GROUP_MAX = 32;

// `n` passes of a group, each closed by a launch of icp_finish_kernel where the pass does not close itself
int enqueue_batch_stretch(pedp_ctx_t c, const IcpJob &job, int n) {
    for (int p = 0; p < n; ++p) {
        const int rc = enqueue_fused_pass(c, job, PassLaunch{});
        if (rc) return rc;
        if (job.path.unfused_finish) launch_finish(c, job, 0);
    }
    return PEDP_OK;
}

// Per-pose results of a batch (any but T may be null).
struct BatchOut {
    double *T, *fitness, *inlier_rmse;
    int32_t *n_iter_done;
};

int icp_batch_fused(pedp_ctx_t c, pedp_cloud_t source, pedp_cloud_t target, const TargetPrep &tp,
                    const pedp_icp_params *prms, const double *inits, int B, const BatchOut &out) {
    bool no_exit = true;
    for (int b = 0; b < B; ++b) no_exit = no_exit && (prms[b].relative_fitness < 0.0 || prms[b].relative_rmse < 0.0);
    int G = 1;  // group size: the power of two that holds the batch, at most BATCH_GROUP_MAX (one cached graph per size)
    int slot = 0;
    while (G < B && G < BATCH_GROUP_MAX) { G <<= 1; ++slot; }
    static_assert(sizeof(IcpState) * BATCH_GROUP_MAX <= pedp_pinned::ICP_BATCH_UP.bytes && pedp_pinned::ICP_BATCH_DOWN.bytes == pedp_pinned::ICP_BATCH_UP.bytes,
                  "two pinned halves hold a group's states");
    IcpJob job;
    job.max_iter = prms[0].max_iteration;
    job.tp = tp; job.estimator = prms[0].estimator;
    IcpPathInputs &in = job.in;  // (every pose is fused-eligible, whatever its radius: pedp_icp_batched_ex has looked)
    in.n_source = source->N; in.n_target = target_rows(target); in.radius = prms[0].max_correspondence_distance; in.unit_size = 1;
    in.poses = G; in.batch = 1; in.timed_pass = -1; in.no_steady = 1;
    job.path = icp_decide_path(icp_switches(), in);
    IcpWorkspace &w = job.w;
    int rc = carve_workspace(c, job.in.n_source, job.in.n_target, job.max_iter, 1, w, true, G);
    if (rc) return rc;
    bind_clouds(w, source, target, 1);
    stage_pass_args(c, job);
    const int all = job.max_iter + 1;
    pedp_icp_graph_key key;
    key.src_gen = source->gen; key.tgt_gen = target->gen; key.ws = c->icp_ws.ptr;
    key.Ns = job.in.n_source; key.Nt = job.in.n_target; key.qt = 1; key.estimator = prms[0].estimator;
    key.max_iter = iter_capacity(job.max_iter);  // the limit itself is in the device state; the workspace layout (trace, history) depends on its capacity class
    // passes per replay: everything when no pose can stop early, else a stretch that covers the usual
    // convergence (Open3D's default criteria stop problems of this kind after 6-9 iterations)
    key.seg = no_exit ? all : (all < 10 ? all : 10);
    key.poses = G; key.r = -1.0;
    slot = 3 * slot + (key.seg == 1 ? 0 : (key.seg == 2 ? 1 : 2));  // a graph per group size and kind of stretch
    // One or two passes per stretch (a z-search probe is a one-iteration registration) are launched as they are: a graph
    // of two kernels saves nothing, and with a new scene handle every frame its capture and instantiation (35-50 us) came
    // back for every frame's first batch
    const bool direct = key.seg <= 2;
    if (!direct && !(c->icp_bgraph[slot] && graph_key_equal(c->icp_bgraph_key[slot], key))) {
        hipError_t e;
        rc = capture_graph(c, c->icp_bgraph[slot], e, [&] { return enqueue_batch_stretch(c, job, key.seg); });
        if (rc) return rc;
        if (!c->icp_bgraph[slot]) {
            pedp_set_error("pedp_icp_batched: graph capture failed: %s", hipGetErrorString(e));
            return PEDP_ERR_HIP;
        }
        c->icp_bgraph_key[slot] = key;
    }
    IcpState *up = pedp_pinned_at<IcpState>(c, pedp_pinned::ICP_BATCH_UP), *down = pedp_pinned_at<IcpState>(c, pedp_pinned::ICP_BATCH_DOWN);
    c->icp_last_cand = c->icp_last_fb = c->icp_last_passes = c->icp_last_lane = 0;  // statistics: totals over the batch
    c->icp_last_nt = target->N;
    for (int b0 = 0; b0 < B; b0 += G) {
        const int n = B - b0 < G ? B - b0 : G;
        for (int k = 0; k < G; ++k) {
            if (k < n) {
                icp_fill_state(&up[k], tp, inits + 16 * (b0 + k), &prms[b0 + k], source->N);
            } else {
                up[k] = IcpState{};
                up[k].done = 1;  // an empty seat of the group: every kernel returns at once
            }
        }
        // start states (each carries its start transformation: slot 0 of the history); tickets and live masks at zero
        static_assert(sizeof(IcpState) % 8 == 0, "states move as 8-byte words");
        hipLaunchKernelGGL(batch_state_scatter_kernel, dim3((unsigned)G), dim3(256), 0, c->stream, (const unsigned long long *)up, (char *)w.st,
                           w.pose_stride, (int)(sizeof(IcpState) / 8), (char *)w.ticket, (int)(zeroed_span_bytes(w) / 8));
        bool finished = false;
        for (int guard = 0; guard < (1 << 20) && !finished; ++guard) {
            if (direct) {
                rc = enqueue_batch_stretch(c, job, key.seg);
                if (rc) return rc;
            } else
                PEDP_HIP_CHECK(hipGraphLaunch(c->icp_bgraph[slot], c->stream));
            hipLaunchKernelGGL(batch_state_gather_kernel, dim3((unsigned)G), dim3(256), 0, c->stream, (const char *)w.st, w.pose_stride,
                               (int)(sizeof(IcpState) / 8), (unsigned long long *)down);
            PEDP_HIP_CHECK(hipGetLastError());
            PEDP_HIP_CHECK(hipStreamSynchronize(c->stream));
            finished = true;
            for (int k = 0; k < n; ++k) finished = finished && down[k].done;
        }
        PEDP_REQUIRE(finished, "pedp_icp_batched: a registration did not finish");
        for (int k = 0; k < n; ++k)
            if (down[k].done < 0) {
                pedp_set_error("pedp_icp_batched: a pass of registration %d could not be closed (workgroups of its launch did not sign off in time)", b0 + k);
                return PEDP_ERR_HIP;
            }
        for (int k = 0; k < n; ++k) {
            const IcpState &h = down[k];
            for (int q = 0; q < 16; ++q) out.T[16 * (b0 + k) + q] = h.T[q];
            if (out.fitness) out.fitness[b0 + k] = h.fitness;
            if (out.inlier_rmse) out.inlier_rmse[b0 + k] = h.rmse;
            if (out.n_iter_done) out.n_iter_done[b0 + k] = h.iters;
            c->icp_last_cand += h.sum_tiles * 256;
            c->icp_last_fb += h.sum_fb;
            c->icp_last_passes += h.iters + 1;
            c->icp_last_lane += h.n_lane;
        }
    }
    return PEDP_OK;
}

}  // namespace

void pedp_icp_drop_pending(pedp_ctx_t c) {
    if (c && c->icp_pending) {
        if (((IcpJob *)c->icp_pending)->steady_held) steady_release(c->device);
        delete (IcpJob *)c->icp_pending;
        c->icp_pending = nullptr;
    }
}

extern "C" {

int pedp_icp(pedp_ctx_t c, pedp_cloud_t source, pedp_cloud_t target, const pedp_icp_params *prm,
             const double init[16], double T_out[16], double *fitness, double *inlier_rmse,
             int32_t *n_iter_done, int32_t *corr, double *trace) {
    PEDP_REQUIRE(c && source && target && prm && init && T_out, "pedp_icp: null argument");
    PEDP_REQUIRE(!c->icp_pending, "pedp_icp: a registration is pending on this context (pedp_icp_end first)");
    TargetPrep tp;
    int rc = icp_prepare(c, source, target, prm, tp);
    if (rc) return rc;
    IcpJob job;
    rc = icp_start(c, IcpCall{source, target, &tp, prm, init, ICP_EARLY_STOP | (trace ? ICP_TRACE : 0u)}, job);
    if (rc) return rc;
    count_registration(target);
    return icp_collect(c, job, T_out, fitness, inlier_rmse, n_iter_done, corr, trace);
}

int pedp_icp_begin(pedp_ctx_t c, pedp_cloud_t source, pedp_cloud_t target, const pedp_icp_params *prm, const double init[16],
                   int want_trace) {
    PEDP_REQUIRE(c && source && target && prm && init, "pedp_icp_begin: null argument");
    PEDP_REQUIRE(!c->icp_pending, "pedp_icp_begin: a registration is pending on this context (pedp_icp_end first)");
    TargetPrep tp;
    int rc = icp_prepare(c, source, target, prm, tp);
    if (rc) return rc;
    IcpJob *job = new (std::nothrow) IcpJob;
    PEDP_REQUIRE(job, "pedp_icp_begin: out of memory");
    rc = icp_start(c, IcpCall{source, target, &tp, prm, init, want_trace ? ICP_TRACE : 0u}, *job);
    if (rc) { delete job; return rc; }
    count_registration(target);
    c->icp_pending = job;
    return PEDP_OK;
}

int pedp_icp_end(pedp_ctx_t c, double T_out[16], double *fitness, double *inlier_rmse, int32_t *n_iter_done, int32_t *corr,
                 double *trace) {
    PEDP_REQUIRE(c && T_out, "pedp_icp_end: null argument");
    PEDP_REQUIRE(c->icp_pending, "pedp_icp_end: no registration is pending on this context");
    IcpJob *job = (IcpJob *)c->icp_pending;
    c->icp_pending = nullptr;
    const int rc = icp_collect(c, *job, T_out, fitness, inlier_rmse, n_iter_done, corr, trace);
    delete job;
    return rc;
}

// Hypotheses are independent: up to PEDP_MAX_SUB registrations are in flight at once, each on
// its own stream and workspace (sub-contexts of c), sharing the clouds' cached preparation.
int pedp_icp_batched_ex(pedp_ctx_t c, pedp_cloud_t source, pedp_cloud_t target, const pedp_icp_params *prms,
                        const double *inits, int B, double *T_out, double *fitness, double *inlier_rmse, int32_t *n_iter_done) {
    PEDP_REQUIRE(c && source && target && prms && inits && T_out, "pedp_icp_batched: null argument");
    PEDP_REQUIRE(!c->icp_pending, "pedp_icp_batched: a registration is pending on this context (pedp_icp_end first)");
    PEDP_REQUIRE(B >= 0, "pedp_icp_batched: negative batch");
    if (B == 0) return PEDP_OK;
    bool uniform = true;
    double r_max = prms[0].max_correspondence_distance;
    for (int b = 0; b < B; ++b) {
        const pedp_icp_params &q = prms[b];
        PEDP_REQUIRE(!q.allreduce && !q.use_comm, "pedp_icp_batched: hypotheses shard across ranks, not within one registration");
        PEDP_REQUIRE(q.estimator == prms[0].estimator && q.max_iteration == prms[0].max_iteration,
                     "pedp_icp_batched: estimator and max_iteration must be the same for the whole batch");
        uniform = uniform && q.max_correspondence_distance == prms[0].max_correspondence_distance &&
                  q.relative_fitness == prms[0].relative_fitness && q.relative_rmse == prms[0].relative_rmse;
        if (q.max_correspondence_distance > r_max) r_max = q.max_correspondence_distance;
    }
    TargetPrep tp;
    int rc = icp_prepare(c, source, target, &prms[0], tp);
    if (rc) return rc;
    // The fused path takes a whole group of poses per launch, whatever their radii and criteria (they
    // live in the device state).  The segmented path replays one graph per pose on sub-contexts and
    // needs one radius and one set of criteria for that; a mixed batch that is not fused-eligible
    // runs one by one on the owner's stream -- same results.
    bool all_fused = true;
    for (int b = 0; b < B && all_fused; ++b) {
        const double r = prms[b].max_correspondence_distance;
        all_fused = fused_eligible(icp_unit_size(target, r), c->icp_exhaustive, r, source->N, target_rows(target));
    }
    if (all_fused) {
        rc = icp_batch_fused(c, source, target, tp, prms, inits, B, BatchOut{T_out, fitness, inlier_rmse, n_iter_done});
        if (!rc) count_registration(target);
        return rc;
    }
    if (!uniform) {
        for (int b = 0; b < B; ++b) {
            IcpJob job;
            rc = icp_start(c, IcpCall{source, target, &tp, &prms[b], inits + 16 * b, ICP_EARLY_STOP | ICP_NO_STEADY}, job);
            if (rc) return rc;
            rc = icp_collect(c, job, T_out + 16 * b, fitness ? fitness + b : nullptr, inlier_rmse ? inlier_rmse + b : nullptr,
                             n_iter_done ? n_iter_done + b : nullptr, nullptr, nullptr);
            if (rc) return rc;
        }
        count_registration(target);
        return PEDP_OK;
    }
    PEDP_HIP_CHECK(hipStreamSynchronize(c->stream));  // preparation is visible to the sub-streams
    const int K = B < PEDP_MAX_SUB ? B : PEDP_MAX_SUB;
    for (int k = 0; k < K; ++k) {
        if (!c->sub[k]) {
            rc = pedp_ctx_create(c->device, nullptr, &c->sub[k]);
            if (rc) return rc;
        }
        c->sub[k]->icp_exhaustive = c->icp_exhaustive;
    }
    IcpJob jobs[PEDP_MAX_SUB];
    c->icp_last_cand = c->icp_last_fb = c->icp_last_passes = 0;  // statistics: totals over the batch
    c->icp_last_nt = target->N;
    // on an error return no sub-stream may still be running on the clouds' buffers (the caller
    // is free to destroy them): drain them all first
    auto drain = [&](int rc_) {
        for (int k = 0; k < K; ++k)
            if (c->sub[k]) (void)hipStreamSynchronize(c->sub[k]->stream);
        return rc_;
    };
    for (int b0 = 0; b0 < B; b0 += K) {
        const int n = (B - b0 < K) ? B - b0 : K;
        for (int k = 0; k < n; ++k) {
            rc = icp_launch_replayed(c->sub[k], IcpCall{source, target, &tp, &prms[b0 + k], inits + 16 * (b0 + k), ICP_NO_STEADY}, jobs[k]);
            if (rc) return drain(rc);
        }
        for (int k = 0; k < n; ++k) {
            rc = icp_collect(c->sub[k], jobs[k], T_out + 16 * (b0 + k), fitness ? fitness + b0 + k : nullptr,
                             inlier_rmse ? inlier_rmse + b0 + k : nullptr, n_iter_done ? n_iter_done + b0 + k : nullptr,
                             nullptr, nullptr);
            if (rc) return drain(rc);
            c->icp_last_cand += c->sub[k]->icp_last_cand;
            c->icp_last_fb += c->sub[k]->icp_last_fb;
            c->icp_last_passes += c->sub[k]->icp_last_passes;
        }
    }
    count_registration(target);
    return PEDP_OK;
}

int pedp_icp_batched(pedp_ctx_t c, pedp_cloud_t source, pedp_cloud_t target, const pedp_icp_params *prm,
                     const double *inits, int B, double *T_out, double *fitness, double *inlier_rmse) {
    PEDP_REQUIRE(prm, "pedp_icp_batched: null argument");
    PEDP_REQUIRE(B >= 0 && B <= (1 << 20), "pedp_icp_batched: batch size out of range");
    pedp_icp_params *all = (pedp_icp_params *)malloc(sizeof(pedp_icp_params) * (size_t)(B > 0 ? B : 1));
    if (!all) { pedp_set_error("pedp_icp_batched: out of host memory"); return PEDP_ERR_ALLOC; }
    for (int b = 0; b < B; ++b) {
        all[b] = *prm;
        all[b].relative_fitness = -1.0;  // no early exit across the batch
        all[b].relative_rmse = -1.0;
    }
    const int rc = pedp_icp_batched_ex(c, source, target, all, inits, B, T_out, fitness, inlier_rmse, nullptr);
    free(all);
    return rc;
}

int pedp_nn(pedp_ctx_t c, pedp_cloud_t source, pedp_cloud_t target, const double T[16], int32_t *idx, double *d2) {
    PEDP_REQUIRE(c && source && target && T && idx && d2, "pedp_nn: null argument");
    PEDP_REQUIRE(source->ctx == c && target->ctx == c, "pedp_nn: cloud belongs to another context");
    PEDP_REQUIRE(target->N > 0, "pedp_nn: empty target");
    PEDP_REQUIRE(!c->icp_pending, "pedp_nn: a registration is pending on this context (pedp_icp_end first)");
    if (source->N == 0) return PEDP_OK;
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    TargetPrep tp;
    int rc = ensure_target_pack(c, target, tp);
    if (!rc) rc = ensure_target_bf16(c, target);
    if (rc) return rc;
    if (target_rows(target) == 0) {  // no finite target row: no neighbour anywhere
        for (int64_t i = 0; i < source->N; ++i) { idx[i] = -1; d2[i] = HUGE_VAL; }
        return PEDP_OK;
    }
    IcpWorkspace w;
    rc = carve_workspace(c, source->N, target_rows(target), 0, 4, w);  // no radius: dense sweep, 64-row units
    if (rc) return rc;
    rc = ensure_spatial_perm(c, source);
    if (rc) return rc;
    bind_clouds(w, source, target, 4);
    IcpState *hp = pedp_pinned_at<IcpState>(c, pedp_pinned::ICP_STATE);
    IcpState h{};
    for (int k = 0; k < 16; ++k) { h.T[k] = T[k]; h.upd[k] = T[k]; }
    for (int k = 0; k < 3; ++k) h.centroid[k] = tp.c[k];
    *hp = h;
    PEDP_HIP_CHECK(hipMemcpyAsync(w.st, hp, sizeof(IcpState), hipMemcpyHostToDevice, c->stream));
    // every point is a candidate: radius = "infinite" (cloud scale bound)
    c->nn_pairs = 0;
    rc = enqueue_nn_pass(c, w, 0, tp, 1e18, c->nn_ev0, c->nn_ev1, false);
    if (rc) return rc;
    { int dn_ = pedp_download(c, idx, w.idx, sizeof(int32_t) * (size_t)source->N); if (dn_) return dn_; }
    { int dn_ = pedp_download(c, d2, w.d2, sizeof(double) * (size_t)source->N); if (dn_) return dn_; }
    PEDP_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PEDP_OK;
}

int pedp_ransac_hypotheses(pedp_ctx_t c, pedp_cloud_t src, pedp_cloud_t tgt, const int32_t *corr, uint64_t seed, int64_t itr0,
                           int count, double edge_similarity, double max_distance, double normal_angle, uint8_t *accepted,
                           double *T) {
    PEDP_REQUIRE(c && src && tgt, "pedp_ransac_hypotheses: null context / cloud");
    PEDP_REQUIRE(src->ctx == c && tgt->ctx == c, "pedp_ransac_hypotheses: clouds belong to another context");
    PEDP_REQUIRE(!c->icp_pending, "pedp_ransac_hypotheses: a registration is pending on this context (pedp_icp_end first)");
    PEDP_REQUIRE(count >= 0 && count <= (1 << 22) && itr0 >= 0, "pedp_ransac_hypotheses: count must be in 0..2^22");
    if (count == 0) return PEDP_OK;
    PEDP_REQUIRE(corr && accepted && T, "pedp_ransac_hypotheses: null arrays");
    PEDP_REQUIRE(src->N > 0 && tgt->N > 0, "pedp_ransac_hypotheses: empty cloud");
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    const size_t sz_corr = align_up(sizeof(int32_t) * (size_t)src->N, 256), sz_flag = align_up((size_t)count, 256);
    int st = c->ops.reserve(sz_corr + sz_flag + sizeof(double) * 16 * (size_t)count + 256);
    if (st) return st;
    int32_t *d_corr = (int32_t *)c->ops.ptr;
    unsigned char *d_flag = (unsigned char *)c->ops.ptr + sz_corr;
    double *d_T = (double *)((char *)c->ops.ptr + sz_corr + sz_flag);
    // correspondences must point inside the target (checked on the host: they index device memory)
    for (int64_t i = 0; i < src->N; ++i)
        PEDP_REQUIRE(corr[i] >= 0 && corr[i] < tgt->N, "pedp_ransac_hypotheses: correspondence %lld -> %d outside the target",
                     (long long)i, (int)corr[i]);
    { int up_ = pedp_upload(c, d_corr, corr, sizeof(int32_t) * (size_t)src->N); if (up_) return up_; }
    hipLaunchKernelGGL(ransac_hypothesis_kernel, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, c->stream,
                       (unsigned long long)seed, (long long)itr0, count, (const double *)src->pts, (const double *)src->normals,
                       (long long)src->N, (const double *)tgt->pts, (const double *)tgt->normals, (const int32_t *)d_corr,
                       edge_similarity, max_distance, cos(normal_angle), d_flag, d_T);
    PEDP_HIP_CHECK(hipGetLastError());
    { int dn_ = pedp_download(c, accepted, d_flag, (size_t)count); if (dn_) return dn_; }
    { int dn_ = pedp_download(c, T, d_T, sizeof(double) * 16 * (size_t)count); if (dn_) return dn_; }
    PEDP_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PEDP_OK;
}

int pedp_icp_configure(pedp_ctx_t c, int exhaustive, int timed_pass) {
    PEDP_REQUIRE(c, "pedp_icp_configure: null context");
    PEDP_REQUIRE(!c->icp_pending, "pedp_icp_configure: a registration is pending on this context (pedp_icp_end first)");
    c->icp_exhaustive = exhaustive != 0;
    c->icp_timed_pass = timed_pass;
    for (int k = 0; k < PEDP_MAX_SUB; ++k)  // captured graphs bake the mode in
        if (c->sub[k] && c->sub[k]->icp_graph) { (void)hipGraphExecDestroy(c->sub[k]->icp_graph); c->sub[k]->icp_graph = nullptr; }
    for (hipGraphExec_t &g : c->icp_bgraph)
        if (g) { (void)hipGraphExecDestroy(g); g = nullptr; }
    return PEDP_OK;
}

int pedp_cloud_set_target_order(pedp_cloud_t cl, int mode) {
    PEDP_REQUIRE(cl, "pedp_cloud_set_target_order: null cloud");
    PEDP_REQUIRE(mode == PEDP_TARGET_ORDER_AUTO || mode == PEDP_TARGET_ORDER_HILBERT || mode == PEDP_TARGET_ORDER_COMPACT,
                 "pedp_cloud_set_target_order: unknown mode %d", mode);
    PEDP_REQUIRE(!pedp_ctx_is_live(cl->ctx) || !cl->ctx->icp_pending,
                 "pedp_cloud_set_target_order: a registration is pending on the cloud's context (pedp_icp_end first)");
    cl->order_mode = mode;  // a pack in the other order is rewritten by the next call that uses the cloud as a target
    return PEDP_OK;
}

int pedp_cloud_target_order(pedp_cloud_t cl, int *in_force) {
    PEDP_REQUIRE(cl && in_force, "pedp_cloud_target_order: null argument");
    *in_force = cl->tgt4 ? cl->order_in_force : PEDP_TARGET_ORDER_AUTO;
    return PEDP_OK;
}

int pedp_debug_target_pack(pedp_ctx_t c, pedp_cloud_t cl, int64_t *rows, int64_t *pad_rows, int32_t *tile_perm, float *tgt4,
                           float *sph16, float *sph64, float *sph1024) {
    PEDP_REQUIRE(c && cl && cl->ctx == c, "pedp_debug_target_pack: null context / cloud of another context");
    PEDP_REQUIRE(cl->tgt4, "pedp_debug_target_pack: the cloud has not been a target yet");
    PEDP_REQUIRE(!c->icp_pending, "pedp_debug_target_pack: a registration is pending on this context (pedp_icp_end first)");
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    const int64_t pad = cl->tgt4_pad;
    if (rows) *rows = target_rows(cl);
    if (pad_rows) *pad_rows = pad;
    struct { void *dst; const void *src; size_t bytes; } part[5] = {
        {tile_perm, cl->tile_perm, sizeof(int32_t) * (size_t)cl->N},
        {tgt4, cl->tgt4, sizeof(float4) * (size_t)pad},
        {sph16, cl->tile_sph, sizeof(float4) * (size_t)(pad / 16)},
        {sph64, cl->tile_sph4, sizeof(float4) * (size_t)(pad / 64)},
        {sph1024, cl->tile_sphw, sizeof(float4) * (size_t)((pad / 16 + 63) / 64)}};
    for (const auto &p : part)
        if (p.dst && p.bytes) { int dn_ = pedp_download(c, p.dst, p.src, p.bytes); if (dn_) return dn_; }
    return PEDP_OK;
}

int pedp_icp_last_stats(pedp_ctx_t c, int64_t *passes, int64_t *pairs_swept, int64_t *fallback_points) {
    PEDP_REQUIRE(c, "pedp_icp_last_stats: null context");
    if (passes) *passes = c->icp_last_passes;
    if (pairs_swept) *pairs_swept = c->icp_last_cand;
    if (fallback_points) *fallback_points = c->icp_last_fb;
    return PEDP_OK;
}

int pedp_debug_nn_bf16(pedp_ctx_t c, const float *src4, int64_t n_src, const float *tgt4, int64_t n_tgt, float *g) {
    PEDP_REQUIRE(c && src4 && tgt4 && g && n_src > 0 && n_tgt > 0 && n_src % 16 == 0 && n_tgt % 16 == 0 && n_src * n_tgt <= ((int64_t)1 << 26),
                 "pedp_debug_nn_bf16: counts must be positive multiples of 16, at most 2^26 pairs");
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    float4 *d_s = nullptr, *d_t = nullptr;
    uint4 *d_b = nullptr;
    float *d_g = nullptr;
    hipError_t e = hipMalloc((void **)&d_s, sizeof(float4) * (size_t)n_src);
    if (e == hipSuccess) e = hipMalloc((void **)&d_t, sizeof(float4) * (size_t)n_tgt);
    if (e == hipSuccess) e = hipMalloc((void **)&d_b, sizeof(uint4) * 4 * (size_t)n_tgt);
    if (e == hipSuccess) e = hipMalloc((void **)&d_g, sizeof(float) * (size_t)(n_src * n_tgt));
    if (e == hipSuccess) e = hipMemcpyAsync(d_s, src4, sizeof(float4) * (size_t)n_src, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_t, tgt4, sizeof(float4) * (size_t)n_tgt, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(pack_target_bf16_kernel, dim3((unsigned)((n_tgt * 4 + 255) / 256)), dim3(256), 0, c->stream, (const float4 *)d_t, n_tgt, d_b);
        hipLaunchKernelGGL(nn_bf16_debug_kernel, dim3((unsigned)((n_src / 16) * (n_tgt / 16))), dim3(64), 0, c->stream, (const uint4 *)d_b,
                           (const float4 *)d_s, (int)(n_src / 16), (int)n_tgt, d_g);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(g, d_g, sizeof(float) * (size_t)(n_src * n_tgt), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d_s); (void)hipFree(d_t); (void)hipFree(d_b); (void)hipFree(d_g);
    PEDP_HIP_CHECK(e);
    return PEDP_OK;
}

int pedp_debug_solve6(pedp_ctx_t c, int64_t n, const double *A, const double *b, double *x_lanes, int32_t *ok_lanes, double *x_one, int32_t *ok_one) {
    PEDP_REQUIRE(c && A && b && x_lanes && ok_lanes && x_one && ok_one && n > 0 && n <= ((int64_t)1 << 20),
                 "pedp_debug_solve6: null argument, or a count outside 1 .. 2^20");
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    double *d_A = nullptr, *d_b = nullptr, *d_x = nullptr;
    int32_t *d_ok = nullptr;
    hipError_t e = hipMalloc((void **)&d_A, sizeof(double) * 36 * (size_t)n);
    if (e == hipSuccess) e = hipMalloc((void **)&d_b, sizeof(double) * 6 * (size_t)n);
    if (e == hipSuccess) e = hipMalloc((void **)&d_x, sizeof(double) * 12 * (size_t)n);
    if (e == hipSuccess) e = hipMalloc((void **)&d_ok, sizeof(int32_t) * 2 * (size_t)n);
    if (e == hipSuccess) e = hipMemcpyAsync(d_A, A, sizeof(double) * 36 * (size_t)n, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_b, b, sizeof(double) * 6 * (size_t)n, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        // the lane form: a wave per system, four to a workgroup; the one-lane form: a thread per system, the only one of its wave
        hipLaunchKernelGGL(solve6_lanes_debug_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, c->stream, (const double *)d_A, (const double *)d_b, n, d_x, d_ok);
        hipLaunchKernelGGL(solve6_one_debug_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, c->stream, (const double *)d_A, (const double *)d_b, n,
                           d_x + 6 * (size_t)n, d_ok + (size_t)n);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(x_lanes, d_x, sizeof(double) * 6 * (size_t)n, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(x_one, d_x + 6 * (size_t)n, sizeof(double) * 6 * (size_t)n, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(ok_lanes, d_ok, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(ok_one, d_ok + (size_t)n, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d_A); (void)hipFree(d_b); (void)hipFree(d_x); (void)hipFree(d_ok);
    PEDP_HIP_CHECK(e);
    return PEDP_OK;
}

int pedp_debug_live_list(pedp_ctx_t c, const unsigned long long *mask_words, int n_lw, int threads, int32_t *list_out, int32_t *n_live_out) {
    PEDP_REQUIRE(c && mask_words && list_out && n_live_out && n_lw > 0 && n_lw <= (1 << 20) && (threads == BK_W * 64 || threads == FIN_THREADS),
                 "pedp_debug_live_list: null argument, a word count outside 1 .. 2^20, or a thread count other than 512 and 1024");
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    unsigned long long *d_m = nullptr;
    int32_t *d_l = nullptr;  // the list (64 n_lw entries), behind it the count
    const size_t cap = 64 * (size_t)n_lw;
    hipError_t e = hipMalloc((void **)&d_m, sizeof(unsigned long long) * (size_t)n_lw);
    if (e == hipSuccess) e = hipMalloc((void **)&d_l, sizeof(int32_t) * (cap + 1));
    if (e == hipSuccess) e = hipMemcpyAsync(d_m, mask_words, sizeof(unsigned long long) * (size_t)n_lw, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_l, list_out, sizeof(int32_t) * cap, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        if (threads == BK_W * 64) hipLaunchKernelGGL((live_list_debug_kernel<BK_W * 64, 2048, true>), dim3(1), dim3(BK_W * 64), 0, c->stream, d_m, n_lw, d_l, d_l + cap);
        else hipLaunchKernelGGL((live_list_debug_kernel<FIN_THREADS, LIVE_CAP, false>), dim3(1), dim3(FIN_THREADS), 0, c->stream, d_m, n_lw, d_l, d_l + cap);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(list_out, d_l, sizeof(int32_t) * cap, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(n_live_out, d_l + cap, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d_m); (void)hipFree(d_l);
    PEDP_HIP_CHECK(e);
    return PEDP_OK;
}

int pedp_debug_icp_path(const pedp_icp_switches *switches, const pedp_icp_path_inputs *inputs, pedp_icp_path *path) {
    PEDP_REQUIRE(inputs && path, "pedp_debug_icp_path: null argument");
    *path = icp_decide_path(switches ? *switches : icp_switches(), *inputs);
    return PEDP_OK;
}

int pedp_icp_graph_captures(pedp_ctx_t c, int64_t *captures) {
    PEDP_REQUIRE(c && captures, "pedp_icp_graph_captures: null argument");
    long long n = c->icp_graph_captures;
    for (int k = 0; k < PEDP_MAX_SUB; ++k)
        if (c->sub[k]) n += c->sub[k]->icp_graph_captures;
    *captures = n;
    return PEDP_OK;
}

int pedp_icp_last_planned_passes(pedp_ctx_t c, int64_t *planned) {
    PEDP_REQUIRE(c && planned, "pedp_icp_last_planned_passes: null argument");
    *planned = c->icp_last_planned;
    return PEDP_OK;
}

int pedp_icp_last_serial_path(pedp_ctx_t c, int64_t *wide_closes, int64_t *bracket) {
    PEDP_REQUIRE(c && wide_closes && bracket, "pedp_icp_last_serial_path: null argument");
    *wide_closes = c->icp_last_wide;
    *bracket = c->icp_last_bracket;
    return PEDP_OK;
}

int pedp_icp_last_lane_solves(pedp_ctx_t c, int64_t *lane_solves) {
    PEDP_REQUIRE(c && lane_solves, "pedp_icp_last_lane_solves: null argument");
    *lane_solves = c->icp_last_lane;
    return PEDP_OK;
}

int pedp_icp_last_certified(pedp_ctx_t c, int64_t *slots, int64_t *searched_slots) {
    PEDP_REQUIRE(c && slots, "pedp_icp_last_certified: null argument");
    *slots = c->icp_last_cert;
    if (searched_slots) *searched_slots = c->icp_last_searched;
    return PEDP_OK;
}

int pedp_icp_last_steady(pedp_ctx_t c, int64_t *passes, int64_t *handbacks) {
    PEDP_REQUIRE(c && passes, "pedp_icp_last_steady: null argument");
    *passes = c->icp_last_steady;
    if (handbacks) *handbacks = c->icp_last_handbacks;
    return PEDP_OK;
}

int pedp_icp_last_steady_followers(pedp_ctx_t c, int64_t *followers) {
    PEDP_REQUIRE(c && followers, "pedp_icp_last_steady_followers: null argument");
    *followers = c->icp_last_followed;
    return PEDP_OK;
}

int pedp_icp_last_head_closed(pedp_ctx_t c, int64_t *head_closed, int64_t *rebuilds, int64_t *launches) {
    PEDP_REQUIRE(c && head_closed, "pedp_icp_last_head_closed: null argument");
    *head_closed = c->icp_last_head;
    if (rebuilds) *rebuilds = c->icp_last_rebuilds;
    if (launches) *launches = c->icp_last_launches;
    return PEDP_OK;
}

int pedp_nn_last_sweep_ms(pedp_ctx_t c, float *ms) {
    PEDP_REQUIRE(c && ms, "pedp_nn_last_sweep_ms: null argument");
    PEDP_REQUIRE(c->nn_timed, "pedp_nn_last_sweep_ms: no timed sweep has run on this context");
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    if (c->nn_pairs > 0) {  // sampled passes: the mean
        float sum = 0.f;
        for (int k = 0; k < c->nn_pairs; ++k) {
            float one = 0.f;
            PEDP_HIP_CHECK(hipEventSynchronize(c->nn_evs[2 * k + 1]));
            PEDP_HIP_CHECK(hipEventElapsedTime(&one, c->nn_evs[2 * k], c->nn_evs[2 * k + 1]));
            sum += one;
        }
        *ms = sum / (float)c->nn_pairs;
        return PEDP_OK;
    }
    PEDP_HIP_CHECK(hipEventSynchronize(c->nn_ev1));
    PEDP_HIP_CHECK(hipEventElapsedTime(ms, c->nn_ev0, c->nn_ev1));
    if (c->nn_span_launches > 1) *ms /= (float)c->nn_span_launches;
    return PEDP_OK;
}

}  // extern "C"
