// Internal declarations shared by the translation units of libpedp_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <vector>
#include "../../include/pedp.h"

void pedp_set_error(const char *fmt, ...);
uint64_t pedp_next_generation();
// Host -> device copy of a caller's (pageable) array on the context's stream.  Large copies go
// through a pinned staging buffer of the context: a fresh pageable buffer -- a new numpy array per
// frame -- otherwise pays for pinning its pages on every call (measured 25-30 ms for 8.8 MB against
// ~1.5 ms staged).  The source may be reused as soon as the call returns.
struct pedp_ctx_s;
int pedp_upload(pedp_ctx_s *c, void *dst, const void *src, size_t bytes);
// The way back: device -> caller's (pageable) array through the same staging buffers.  Returns
// after the data are in `dst` (the stream has been drained up to and including the copy).
int pedp_download(pedp_ctx_s *c, void *dst, const void *src, size_t bytes);
// `bytes` of device memory into the context's page-locked download buffer (valid until the next download through it);
// returns when the copy is complete: host code that only READS a result needs neither an array of its own nor a staged copy
int pedp_download_view(pedp_ctx_s *c, const void *src, size_t bytes, const void **view);
int pedp_download_parts(pedp_ctx_s *c, const void *src, size_t span, int n, const size_t *off, void *const *dst, const size_t *bytes);
struct pedp_ctx_s;
int pedp_sort_keys64_begin(pedp_ctx_s *c, int64_t N, int bits, unsigned long long **d_keys);
int pedp_sort_keys64_run(pedp_ctx_s *c, int64_t N, int bits, int32_t *d_perm);
// the same pooled sort on all `bits` low bits of the keys (the Hilbert sort above looks only at the leading levels)
int pedp_sort_keys64_exact_begin(pedp_ctx_s *c, int64_t N, int bits, unsigned long long **d_keys);
int pedp_sort_keys64_exact_run(pedp_ctx_s *c, int64_t N, int bits, int32_t *d_perm);

// Row i of an N x 3 float64 array has no NaN / infinite coordinate.  Tested on the exponent bits, so that no
// compiler assumption about NaNs (-fno-honor-nans) can fold it away.
__host__ __device__ inline bool pedp_row_finite(const double *pts, int64_t i) {
    uint64_t b[3];
    memcpy(b, pts + 3 * i, sizeof(b));
    const uint64_t e = 0x7FF0000000000000ull;
    return (b[0] & e) != e && (b[1] & e) != e && (b[2] & e) != e;
}

#define PEDP_HIP_CHECK(expr)                                                              \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess) {                                                           \
            pedp_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(e_)); \
            return PEDP_ERR_HIP;                                                          \
        }                                                                                 \
    } while (0)

#define PEDP_REQUIRE(cond, ...)             \
    do {                                    \
        if (!(cond)) {                      \
            pedp_set_error(__VA_ARGS__);    \
            return PEDP_ERR_BAD_ARG;        \
        }                                   \
    } while (0)

// call, return its status if it is not PEDP_OK
#define PEDP_TRY(expr)           \
    do {                         \
        int st_ = (expr);        \
        if (st_) return st_;     \
    } while (0)

// A growable device scratch buffer owned by the context (no hipMalloc on the hot path
// once sizes have settled).
struct pedp_scratch {
    void *ptr = nullptr;
    size_t cap = 0;
    int reserve(size_t bytes);
    void release();
};

// Device buffers of cloud handles that have been destroyed, kept for the next cloud of about that size: a scene
// cloud per camera frame would otherwise pay hipMalloc and a device-synchronising hipFree for each of its
// buffers.  Reuse is ordered by the context's stream (every use of a cloud's buffers is enqueued there).
struct pedp_pool {
    struct entry { void *p; size_t cap; };
    std::vector<entry> free_;
    std::mutex mu;  // a handle may be destroyed on another thread (Python drops the last reference wherever it likes)
    void *take(size_t bytes, size_t *cap);   // a pooled buffer of cap >= bytes (not wastefully larger), or a new one
    void give(void *p, size_t cap);
    void clear();
};

#define PEDP_MAX_SUB 8

// What a captured registration graph depends on besides device-memory contents: if any of it
// changes, the graph is captured again.
struct pedp_icp_graph_key {
    // clouds are identified by their generation id, not by the handle address: a destroyed
    // cloud's address can be handed out again by the next pedp_cloud_create
    uint64_t src_gen = 0, tgt_gen = 0;
    const void *ws = nullptr;
    int64_t Ns = 0, Nt = 0;
    int max_iter = 0, qt = 0, estimator = 0;
    int seg = 0, poses = 0;  // fused-path group graphs: passes per replay, poses per launch
    double r = 0.0, rel_fitness = 0.0, rel_rmse = 0.0;
};

struct pedp_comm_s;  // pedp_comm.hip: RCCL communicator of this rank
int pedp_comm_allreduce_sum_f64(pedp_ctx_t c, double *buf, int64_t n);
struct pedp_cloud_s;
int pedp_cloud_host_stats(pedp_ctx_t c, pedp_cloud_s *cl);  // makes centroid / lo / hi / Tn / T2 valid on the host
bool pedp_ctx_is_live(pedp_ctx_t c);

struct pedp_ctx_s {
    int device = 0;
    pedp_comm_s *comm = nullptr;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int num_cus = 256;
    // ray casting
    pedp_scratch ray_keys;   // N x u64 packed (t_bits << 32 | prim_id)
    pedp_scratch ray_in;     // staging for host-memory calls
    pedp_scratch ray_out;
    pedp_scratch ray_aux;    // shared-origin flag + per-call shared-origin pair records
    pedp_scratch ray_order;  // direction order of the last frame's rays (kept between calls) + the samples it is checked by
    int64_t ray_order_n = -1;
    pedp_scratch ray_rast;   // variant 4: header, chain heads, nodes, item table
    void *rast_hdr_ready = nullptr;  // the buffer whose header holds its start values
    int *rast_status = nullptr;      // pinned, written by the last kernel of a variant-4 cast: [0] why the grid failed (0: it did not), [1] ray count
    unsigned rast_seq = 0;           // casts enqueued: picks one of the two headers
    int rast_avoid_n = -2;           // ray count for which the grid is known not to work: variant 3 instead
    int ray_last_variant = 0;        // variant the last cast on this context ran
    int ray_tri_chunks = 0;  // 0 = auto
    int ray_variant = 0;     // 0 = auto; written by pedp_raycast_configure only
    // all-hits queries (pedp_count_intersections, pedp_test_occlusions, pedp_list_intersections)
    pedp_scratch hits_ws;    // per ray: counts, cursors, splits; the scan's scratch
    pedp_scratch hits_keys;  // a list's keys as they arrive and sorted; the sort's scratch
    pedp_scratch hits_io;    // outputs of host-memory calls
    int *hits_status = nullptr;  // pinned, the queries' own words (the casts' rast_status stays theirs): [0] why the grid gave up (0: it did not), [1] ray count
    const int *hits_last_status = nullptr;  // the words the last query's grid pass reports to (the context's or a ray set's)
    int hits_avoid_n = -2;   // ray count whose last per-call query the grid gave up on: the exhaustive path instead (auto only)
    int hits_last_path = 0;  // 4: the grid, 1: every ray against every triangle; 0: no query yet
    hipEvent_t ev0 = nullptr, ev1 = nullptr;  // sweep timing
    hipEvent_t ev_copy = nullptr;             // pedp_cloud_create_device: behind its copies (the host waits on it)
    bool ray_timed = false;
    bool nn_timed = false;
    hipEvent_t nn_ev0 = nullptr, nn_ev1 = nullptr;
    // sampled timing of a registration's sweep kernels (pedp_icp_configure timed_pass = -2): event
    // pairs around the sweep kernel of every fourth pass, created on first use
    hipEvent_t nn_evs[16] = {};
    int nn_pairs = 0;  // pairs recorded by the last timed registration (0: the single pair above)
    int nn_span_launches = 1;  // timed_pass = -3: launches between the single pair's two events
    // ICP
    pedp_scratch icp_ws;
    pedp_scratch ops;        // point-cloud operations (voxel grid, DBSCAN, kNN, plane RANSAC)
    pedp_scratch sort_ws;    // spatial order of a cloud: keys + radix-sort buffers (pooled, stream-ordered)
    pedp_pool cloud_pool;    // buffers of destroyed cloud handles
    pedp_scratch ops_small;  // partial bounds and counters of the point-cloud operations
    pedp_scratch chain;      // pedp_preprocess_source: the clouds between its stages
    void *avg_host = nullptr;  // pinned: preprocess_source's voxel means of the normals, written by the kernel itself (zero copy)
    size_t avg_host_cap = 0;
    pedp_scratch ops_in;     // a large cloud's points, uploaded ahead of the workspace sizing (its box comes from the device copy)
    pedp_scratch proj, proj_out;  // fused heat-map projection: selection, rays, hit records / compacted outputs
    pedp_scratch render_ws;  // renderer: pose records, per-pixel depth keys of one pose chunk, big-triangle list
    pedp_scratch render_io;  // renderer: inputs and outputs of host-memory calls
    pedp_scratch crop_ws;    // crop batches: per-pose float64 maps
    pedp_scratch crop_io;    // crop batches: inputs and outputs of host-memory calls
    pedp_scratch pose_ws;    // pose arithmetic: the pair maximum's key and flag (and its host-memory points)
    pedp_scratch pose_io;    // pose update: inputs and outputs of host-memory calls
    pedp_scratch stats_ws;   // mask/depth statistics: counters, the three passes' histograms, the record
    pedp_scratch stats_io;   // mask/depth statistics: the frame and the mask of host-memory calls
    int render_chunk = 0;    // pedp_render_configure: poses per chunk (0 = by a key budget)
    bool icp_exhaustive = false;  // pedp_icp_configure: no culling (all-pairs sweep every pass)
    int icp_timed_pass = -1;      // pedp_icp_configure: HIP events around the sweep kernel of this pass
    long long icp_last_cand = 0, icp_last_fb = 0, icp_last_passes = 0, icp_last_nt = 0, icp_last_planned = 0, icp_last_wide = 0, icp_last_lane = 0, icp_last_bracket = 0, icp_last_head = 0, icp_last_rebuilds = 0, icp_last_launches = 0, icp_last_cert = 0, icp_last_searched = 0, icp_last_steady = 0, icp_last_handbacks = 0, icp_last_followed = 0;
    void *icp_pending = nullptr;   // pedp_icp_begin's job until pedp_icp_end collects it (an IcpJob of pedp_icp.hip)  // last pedp_icp
    pedp_ctx_s *sub[PEDP_MAX_SUB] = {};  // sub-contexts (own stream + workspace) for batched registrations
    hipGraphExec_t icp_graph = nullptr;  // sub-contexts: one whole registration, replayed per start pose
    pedp_icp_graph_key icp_graph_key;
    // fused path: one graph per group size 1, 2, 4, ... 32 (poses share launches) and per stretch of passes
    // [0] one pass (evaluation), [1] two (single-iteration probes), [2] the rest -- a frame alternates between them
    hipGraphExec_t icp_bgraph[18] = {};
    pedp_icp_graph_key icp_bgraph_key[18];
    long long icp_graph_captures = 0;  // graphs captured and instantiated on this executor so far (pedp_icp_graph_captures)
    void *pinned = nullptr;  // small pinned host block for result read-back
    size_t pinned_cap = 0;
    void *stage[2] = {nullptr, nullptr};  // pinned staging buffers of pedp_upload [0] / pedp_download [1], grown on demand
    size_t stage_cap[2] = {0, 0};
    bool stage_busy = false;              // an upload's DMA may still be reading stage[0]
    pedp_scratch metrics_ws; // pose errors: the partial sums of one slab of poses (pedp_metrics.hip)
    pedp_scratch metrics_io; // pose errors: inputs and outputs of host-memory calls
    pedp_scratch closest_ws; // closest points: the counter of tested point-triangle pairs (pedp_closest.hip)
    pedp_scratch closest_io; // closest points: inputs and outputs of host-memory calls
    pedp_scratch fit_ws;     // surface fit: the state, the search's outputs, the blocks' partial sums, the trace (pedp_surface_fit.hip)
    pedp_scratch fit_io;     // surface fit: the points of a host-memory call
    pedp_scratch sample_ws;  // thinning to a spacing: the grid index, the states, the scans' and the sort's scratch (pedp_sample.hip)
    pedp_scratch sample_io;  // thinning a given cloud: its points, keys and the kept indices of a host-memory call
    int closest_mode = 0;    // pedp_closest_configure: 0 culled (the kernel by N), 1 exhaustive, 2 / 3 one culled kernel
};

// The layout of the context's page-locked block (pedp_ctx_s::pinned, PEDP_PINNED_CAP bytes): small results on their way
// to the host and small inputs on their way up.  A context's calls are serial and every user below waits for its copy
// before it reads, rewrites or returns -- that is what lets slots be shared -- with two exceptions, which have slots of
// their own: preprocess_source's average normal and refit plane are collected after a LATER wait of the same call, and a
// registration begun by pedp_icp_begin keeps ICP_STATE / ICP_RESULT until pedp_icp_end (pedp.h: the context must not be
// used in between).
struct pedp_pinned_slot { size_t off, bytes; };
namespace pedp_pinned {
constexpr pedp_pinned_slot ICP_STATE{0, 2048};        // pedp_icp.hip: a registration's start state up, its final state down
constexpr pedp_pinned_slot ICP_RESULT{2048, 2048};    // pedp_icp.hip: the final state the closing workgroup writes itself
constexpr pedp_pinned_slot ICP_DONE{4096, 4096};      // pedp_icp.hip: the two `done` words the early exit reads every 8th pass
// Counters read back behind a wait of the same function -- pedp_cloudops.hip: voxel runs, kept points, the best plane's
// 10 doubles; pedp_depth.hip: scene points; pedp_project.hip: selected rays and hits.  One name on purpose: each reader
// synchronises the stream and takes its value before anything else of the context can be enqueued.
constexpr pedp_pinned_slot COUNTERS{8192, 4096};
// A few words on their way UP -- pedp_ctx.hip: a new cloud's box; pedp_depth.hip: the camera matrix.  Shared: both
// write the words, enqueue the copy and wait for the stream before they return.
constexpr pedp_pinned_slot SMALL_UPLOAD{12288, 4096};
constexpr pedp_pinned_slot BOUNDS{16384, 12288};      // pedp_cloudops.hip: 256 workgroups' partial boxes, folded by the host
// A batched registration's group (pedp_icp.hip, icp_batch_fused) lays its start states over the whole lower half and
// reads the final ones from the upper: the slots above are overlaid, none of them is live during a batch.
constexpr pedp_pinned_slot ICP_BATCH_UP{0, 32768};
constexpr pedp_pinned_slot ICP_BATCH_DOWN{32768, 32768};
constexpr pedp_pinned_slot AVERAGE_NORMAL{65536, 1024};  // pedp_cloudops.hip: rows, overflow flag of the voxel means (5 doubles)
constexpr pedp_pinned_slot REFIT{66560, 3072};           // pedp_cloudops.hip: the refit plane and its inlier count (8 doubles)
constexpr pedp_pinned_slot JET{69632, 6144};             // pedp_project.hip: the 768-double colour table on its way up
constexpr size_t CAP = 1 << 17;
constexpr bool before(pedp_pinned_slot a, pedp_pinned_slot b) { return a.off + a.bytes <= b.off; }
static_assert(before(ICP_STATE, ICP_RESULT) && before(ICP_RESULT, ICP_DONE) && before(ICP_DONE, COUNTERS) &&
                  before(COUNTERS, SMALL_UPLOAD) && before(SMALL_UPLOAD, BOUNDS) && before(BOUNDS, ICP_BATCH_DOWN),
              "the lower half's slots follow each other");
static_assert(before(ICP_BATCH_UP, ICP_BATCH_DOWN) && before(ICP_BATCH_DOWN, AVERAGE_NORMAL) && before(AVERAGE_NORMAL, REFIT) &&
                  before(REFIT, JET) && JET.off + JET.bytes <= CAP,
              "the halves and the slots above them follow each other inside the block");
}  // namespace pedp_pinned
template <class T>
inline T *pedp_pinned_at(pedp_ctx_s *c, pedp_pinned_slot s) { return (T *)((char *)c->pinned + s.off); }

// Triangle record: 12 floats (48 B, 16-B aligned so a wave fetches it with scalar
// dwordx4/x8 loads): v0.xyz, e1.xyz, e2.xyz, 3 pad.
#define PEDP_TRI_STRIDE 12

struct pedp_mesh_s {
    pedp_ctx_t ctx = nullptr;
    int device = 0;  // copied at creation: destroy must not dereference a context that may be gone
    uint64_t gen = 0;  // process-wide creation counter (never reused): names the handle where its address could be reused
    int64_t V = 0, F = 0;
    float *tri = nullptr;  // F_padded x PEDP_TRI_STRIDE floats on the device
    float *tri2 = nullptr; // F_padded/2 pair-interleaved general-origin records (24 floats each)
    void *spheres = nullptr;  // n_clusters x float4 bounding spheres of 16-triangle clusters
    int64_t n_clusters = 0;
    void *super_spheres = nullptr;  // bounding sphere of every 64 clusters (one cull-mask word)
    int64_t n_super = 0;
    int64_t F_padded = 0;  // multiple of 8; pad records can never be hit (all zero => det == 0)
    // posable meshes keep the model-frame float64 vertices, the float32 posed vertices and the
    // index buffer resident so that a new pose rebuilds the records on the device
    double *verts64 = nullptr;
    float *verts32 = nullptr;
    uint32_t *idx = nullptr;
};

struct pedp_cloud_s {
    pedp_ctx_t ctx = nullptr;
    int device = 0;     // copied at creation: destroy must not dereference a context that may be gone
    uint64_t gen = 0;   // process-wide creation counter (never reused), keys cached graphs
    int64_t N = 0;
    bool has_normals = false;
    double *pts = nullptr;      // N x 3 f64 (device)
    double *normals = nullptr;  // N x 3 f64 (device) or null
    size_t pts_cap = 0, normals_cap = 0, perm_cap = 0, sph_cap = 0, box_cap = 0;  // capacities (the buffers may come from the pool)
    double *d_box = nullptr;    // device: lo xyz, hi xyz of the points (what the spatial order is laid over)
    // centroid, box and the filter's magnitudes ON THE HOST: at creation for clouds made from host arrays, on first
    // use as a registration TARGET for clouds made from device memory (a scene cloud never needs them: no read-back
    // and no synchronisation between the camera frame and its registration)
    bool host_stats = false;
    // Set at creation (host pass over the points): centroid and the two magnitudes of the
    // centred cloud that the NN filter's error bound needs when this cloud is the target.
    double centroid[3] = {0, 0, 0};
    float Tn = 0.f;  // max |t'|_1
    float T2 = 0.f;  // max |t'|_2^2
    double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};  // axis-aligned bounding box of the points (finite rows)
    int64_t n_finite = -1;  // rows without a NaN / infinite coordinate, valid with host_stats (-1: not counted, all N)
    // Built on first use in ICP: spatial order of the points (device int32[N]); as a target
    // additionally the sorted float4 operand (x', y', z', |t'|^2), padded, and one bounding
    // sphere per 16-row tile.
    void *perm = nullptr;       // built from the cloud alone (its own bounding box): never rebuilt
    void *chunk_sph = nullptr;  // with it: bounding sphere (float64 x 4) of every 128 consecutive points of that order
    void *tgt4 = nullptr;
    void *tile_sph = nullptr;   // one sphere per 16 sorted rows
    void *tile_sph4 = nullptr;  // one sphere per 64 sorted rows
    void *tile_sphw = nullptr;  // one sphere per 1024 sorted rows (one cull-mask word of 16-row tiles)
    void *tgt_s = nullptr;      // sorted rows as float64 x 3 (exact re-scoring)
    void *tgt_bf = nullptr;     // the sorted operand as bf16 pieces for the dense sweep's v_mfma_f32_16x16x32_bf16 (1 KB per 16-row tile; built on first use)
    int64_t tgt4_pad = 0;
    // the order of the pack's rows (device int32[N], allocated with the pack): a copy of perm, or the compact order of
    // icp/target_order.h; perm itself stays what defines the source role and every sum
    void *tile_perm = nullptr;
    int order_mode = 0;      // pedp_cloud_set_target_order (PEDP_TARGET_ORDER_*)
    int order_in_force = 0;  // what the pack holds (0: none)
    int registrations = 0;   // registrations against this handle whose passes were all enqueued, counted up to the one that upgrades the order
};

// pedp_closest.hip: the search of pedp_closest_points on device memory, enqueued on the context's stream.  region
// (nullable): the rule 1 ... 7 of pedp.h's table that decided the chosen triangle's closest point, 0 where there is none
int pedp_closest_launch(pedp_ctx_t c, pedp_mesh_t mesh, const double *pts, int64_t N, double *closest, double *dist, uint32_t *prim_id,
                        double *uv, int8_t *side, uint8_t *region);

// the same search for pedp_fit_to_surface: the finite rows go through T (device, row-major 4 x 4) as they are loaded, the launch
// exits at once when *done (device) is set, and `pairs` (device, zeroed by the caller) counts the pairs tested
int pedp_closest_launch_posed(pedp_ctx_t c, pedp_mesh_t mesh, const double *pts, int64_t N, const double *T, const int *done,
                              unsigned long long *pairs, double *closest, double *dist, uint32_t *prim_id);

// pedp_icp.hip: frees the job of a pedp_icp_begin that was never ended (called by pedp_ctx_destroy)
void pedp_icp_drop_pending(pedp_ctx_t c);
