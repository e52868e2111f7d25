// Next-best-view planning over the coverage map: what each of V candidate views would add to the map,
// their gains against a working copy of the map's per-face state, and the greedy choice.
//   * OBSERVE: one lane per pixel of a candidate's cast, the per-pixel rule and the in-wave combine of
//     coverage_add_kernel (coverage/shared.h, defectmap/shared.h), integer atomics onto the candidate's row.
//   * SCORE: one wave per (candidate, block of 4096 faces) over the whole V x ceil(F / 4096) grid; a lane reads the pixel
//     count coalesced and goes to the two 64-bit columns and the state only where it is not 0.  A second kernel adds the
//     block sums per candidate.  s4.17's block-and-butterfly order, no atomics.
//   * the greedy rounds: the choice, the stop and the merge are made on the device; the host waits once.
// The coverage map is only ever read.
#include "coverage/shared.h"

namespace {

using namespace coverage;

constexpr int64_t MAX_CAPACITY = (int64_t)1 << 20;
constexpr int64_t MAX_WAVES = (int64_t)1 << 26;  // waves of a score launch: its threads stay below 2^32

// the candidates' rows: row v of a column starts at v F
struct Columns {
    uint32_t *pix;
    unsigned long long *key, *fp;
};
// the working state, writable
struct Work {
    unsigned long long *pixels, *best, *minfp;
    int32_t *views;
    State state() const { return State{pixels, nullptr, best, minfp, views}; }
};
// what a selection keeps on the device between its rounds
struct Sel {
    int32_t cur;      // the candidate the last round chose
    int32_t stopped;  // a round found no gain above min_gain: every later round is a no-op
    int32_t n;        // rounds recorded
    int32_t pad;
};

struct ObserveArgs : View {
    Columns row;  // of this candidate
};

// One candidate, a lane per pixel: the SEEN pixels of a run of equal faces in neighbouring lanes send one count, one
// maximum and one minimum through the run's first lane.
__global__ __launch_bounds__(DT) void view_plan_observe_kernel(ObserveArgs a) {
    const int64_t i = (int64_t)blockIdx.x * DT + threadIdx.x;
    const int lane = threadIdx.x & 63;
    uint32_t f = NONE;
    unsigned long long key = 0, fp = NEVER;
    const bool seen = i < a.n && classify(a, i, f, key, fp) == SEEN;
    unsigned n_seen = seen;
    const LaneRun run = lane_run(seen ? f : NONE, lane);
    if (run.wide) {
        key = run_max(key, lane, run.end);
        fp = run_min(fp, lane, run.end);
        n_seen = (unsigned)(run.end - lane + 1);  // every lane of a run is SEEN
    }
    if (run.head) {  // f < F: classify gives SEEN to no other id
        atomicAdd(&a.row.pix[f], n_seen);
        atomicMax(&a.row.key[f], key);
        if (fp != NEVER) atomicMin(&a.row.fp[f], fp);
    }
}

__global__ __launch_bounds__(DT) void view_plan_candidate_kernel(Columns row, int64_t F, int64_t *__restrict__ pixels,
                                                                double *__restrict__ best_cos, double *__restrict__ min_footprint) {
    const int64_t f = (int64_t)blockIdx.x * DT + threadIdx.x;
    if (f >= F) return;
    if (pixels) pixels[f] = (int64_t)row.pix[f];
    if (best_cos) best_cos[f] = cos_of_key(row.key[f]);
    if (min_footprint) min_footprint[f] = footprint_of_bits(row.fp[f]);
}

__global__ __launch_bounds__(DT) void view_plan_reset_kernel(State s, Work w, int64_t F) {
    const int64_t f = (int64_t)blockIdx.x * DT + threadIdx.x;
    if (f >= F) return;
    w.pixels[f] = s.pixels[f];
    w.views[f] = s.views[f];
    w.best[f] = s.best[f];
    w.minfp[f] = s.minfp[f];
}

// w merged with candidate v, or with the candidate the last round chose (sel: unless the selection has stopped)
__global__ __launch_bounds__(DT) void view_plan_commit_kernel(Columns col, Work w, int64_t F, int64_t v, const Sel *__restrict__ sel) {
    if (sel) {
        if (sel->stopped) return;
        v = sel->cur;
    }
    const int64_t f = (int64_t)blockIdx.x * DT + threadIdx.x;
    if (f >= F) return;
    const size_t at = (size_t)v * (size_t)F + (size_t)f;
    const uint32_t cp = col.pix[at];
    if (!cp) return;
    const unsigned long long key = col.key[at], fp = col.fp[at];
    w.pixels[f] += cp;
    w.views[f] += 1;
    if (key > w.best[f]) w.best[f] = key;
    if (fp < w.minfp[f]) w.minfp[f] = fp;
}

// the progress of a face (pedp.h): 0 ... m, m exactly when it is covered
__device__ __forceinline__ int progress(const pedp_coverage_criteria &c, unsigned long long pixels, int32_t views, unsigned long long key,
                                        unsigned long long fp) {
    const bool q = (int64_t)pixels >= c.min_pixels && cos_of_key(key) >= c.min_cos && footprint_of_bits(fp) <= c.max_footprint;
    if (!q) return 0;
    return c.min_views <= 0 ? 1 : (views < c.min_views ? views : c.min_views);
}

struct ScoreArgs {
    Columns col;
    State w;
    pedp_coverage_criteria c;
    const double *area;
    int64_t F, n_blocks, V;
    const uint8_t *chosen;  // nullable: a chosen candidate is not scored
    const Sel *sel;         // nullable: nothing is scored once the selection has stopped
    double *part_area;      // V x n_blocks
    int64_t *part_faces;
};

// One wave per (candidate v, block b of SUM_BLOCK consecutive faces): lane l adds the terms of faces l, l + 64, ... of
// the block one after the other, the butterfly adds the lanes.  A term of +0 changes no bit of a sum of non-negative
// terms, so a face the candidate does not see costs the one coalesced load of its pixel count.
__global__ __launch_bounds__(DT) void view_plan_score_kernel(ScoreArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * SUM_WPB + (threadIdx.x >> 6);
    if (wave >= a.V * a.n_blocks) return;  // wave-uniform, as are the next two
    if (a.sel && a.sel->stopped) return;
    const int64_t v = wave / a.n_blocks, b = wave - v * a.n_blocks;
    if (a.chosen && a.chosen[v]) return;
    const int64_t f0 = b * SUM_BLOCK, f1 = f0 + SUM_BLOCK < a.F ? f0 + SUM_BLOCK : a.F;
    const size_t row = (size_t)v * (size_t)a.F;
    const int m = a.c.min_views > 1 ? a.c.min_views : 1;
    const double dm = (double)m;
    double gain = 0.0;
    int64_t faces = 0;
    for (int64_t f = f0 + lane; f < f1; f += 64) {
        const uint32_t cp = a.col.pix[row + f];
        if (!cp) continue;
        const unsigned long long ckey = a.col.key[row + f], cfp = a.col.fp[row + f];
        const unsigned long long px = a.w.pixels[f], key = a.w.best[f], fp = a.w.minfp[f];
        const int32_t views = a.w.views[f];
        const int before = progress(a.c, px, views, key, fp);
        const int after = progress(a.c, px + cp, views + 1, ckey > key ? ckey : key, cfp < fp ? cfp : fp);
        const int delta = after - before;
        if (delta > 0) {
            gain = gain + (a.area[f] * (double)delta) / dm;
            if (after == m) faces += 1;  // before < after == m
        }
    }
    gain = butterfly_sum(gain);
    faces = butterfly_sum(faces);
    if (lane == 0) {
        a.part_area[wave] = gain;
        a.part_faces[wave] = faces;
    }
}

// One wave per candidate adds its block sums l, l + 64, ... the same way.
__global__ __launch_bounds__(DT) void view_plan_total_kernel(const double *__restrict__ part_area, const int64_t *__restrict__ part_faces,
                                                            int64_t n_blocks, int64_t V, const uint8_t *__restrict__ chosen,
                                                            const Sel *__restrict__ sel, double *__restrict__ gain_area,
                                                            int64_t *__restrict__ gain_faces) {
    const int lane = threadIdx.x & 63;
    const int64_t v = (int64_t)blockIdx.x * SUM_WPB + (threadIdx.x >> 6);
    if (v >= V) return;
    if (sel && sel->stopped) return;
    if (chosen && chosen[v]) return;
    double gain = 0.0;
    int64_t faces = 0;
    for (int64_t b = lane; b < n_blocks; b += 64) {
        gain = gain + part_area[v * n_blocks + b];
        faces += part_faces[v * n_blocks + b];
    }
    gain = butterfly_sum(gain);
    faces = butterfly_sum(faces);
    if (lane == 0) {
        if (gain_area) gain_area[v] = gain;
        if (gain_faces) gain_faces[v] = faces;
    }
}

// One round's choice, one wave: among the candidates not yet chosen whose gain is > min_gain the largest gain, the
// lowest index among equals.  Lane l looks at candidates l, l + 64, ... in rising order, then the butterfly compares the
// lanes' (gain, index) pairs; an index of -1 (read as the largest unsigned) stands for "none" and carries min_gain, which
// no candidate ties.  A NaN passes no `>`.
__global__ __launch_bounds__(64) void view_plan_choose_kernel(const double *__restrict__ gain_area, const int64_t *__restrict__ gain_faces,
                                                             int64_t V, double min_gain, uint8_t *__restrict__ chosen, Sel *__restrict__ sel,
                                                             int32_t *__restrict__ order, double *__restrict__ sel_area,
                                                             int64_t *__restrict__ sel_faces) {
    if (sel->stopped) return;
    const int lane = threadIdx.x;
    double best = min_gain;
    uint32_t at = 0xFFFFFFFFu;
    for (int64_t v = lane; v < V; v += 64) {
        if (chosen[v]) continue;
        const double g = gain_area[v];
        if (g > best) {
            best = g;
            at = (uint32_t)v;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double g = double_of(shfl_xor_u64(bits_of(best), off));
        const uint32_t i = __shfl_xor(at, off, 64);
        if (g > best || (g == best && i < at)) {
            best = g;
            at = i;
        }
    }
    if (lane != 0) return;
    if (at == 0xFFFFFFFFu) {
        sel->stopped = 1;
        return;
    }
    const int32_t n = sel->n;
    order[n] = (int32_t)at;
    sel_area[n] = best;
    sel_faces[n] = gain_faces[at];
    chosen[at] = 1;
    sel->cur = (int32_t)at;
    sel->n = n + 1;
}

}  // namespace

struct pedp_view_plan_s {
    pedp_coverage_s *cov = nullptr;  // borrowed: it must outlive this handle
    pedp_ctx_t ctx = nullptr;
    int device = 0;
    int64_t F = 0, capacity = 0, n = 0, n_blocks = 0;
    char *store = nullptr;  // one allocation: everything below
    Columns col;
    Work w;
    size_t w_zero_off = 0, w_zero_bytes = 0, w_ones_off = 0, w_ones_bytes = 0;
    double *part_area = nullptr, *gain_area = nullptr;
    int64_t *part_faces = nullptr, *gain_faces = nullptr;
    Sums *sum_part = nullptr;
    uint8_t *chosen = nullptr;
    // a selection's result, one stretch of memory: the rounds' state, the totals of w, then capacity entries each
    char *result = nullptr;
    size_t result_bytes = 0, o_order = 0, o_area = 0, o_faces = 0;
    Sel *sel = nullptr;
    Sums *total = nullptr;
    pedp_scratch io;  // staging of host-memory calls
};

namespace {

// rows [v0, v1) as a view that sees nothing
int clear_rows(pedp_view_plan_s *p, int64_t v0, int64_t v1) {
    const size_t a = (size_t)v0 * (size_t)p->F, n = (size_t)(v1 - v0) * (size_t)p->F;
    if (!n) return PEDP_OK;
    PEDP_HIP_CHECK(hipMemsetAsync(p->col.pix + a, 0, 4 * n, p->ctx->stream));
    PEDP_HIP_CHECK(hipMemsetAsync(p->col.key + a, 0, 8 * n, p->ctx->stream));
    PEDP_HIP_CHECK(hipMemsetAsync(p->col.fp + a, 0xFF, 8 * n, p->ctx->stream));
    return PEDP_OK;
}

// the gains of candidates [0, n) against w into gain_area / gain_faces (device, either nullable); inside a selection
// (sel) the chosen candidates are left out and nothing runs once it has stopped
int launch_score(pedp_view_plan_s *p, const pedp_coverage_criteria &k, bool selecting, double *gain_area, int64_t *gain_faces) {
    hipStream_t stream = p->ctx->stream;
    const int64_t waves = p->n * p->n_blocks;
    const uint8_t *chosen = selecting ? p->chosen : nullptr;
    const Sel *sel = selecting ? p->sel : nullptr;
    if (waves) {
        ScoreArgs a;
        a.col = p->col; a.w = p->w.state(); a.c = k; a.area = p->cov->map->area;
        a.F = p->F; a.n_blocks = p->n_blocks; a.V = p->n;
        a.chosen = chosen; a.sel = sel;
        a.part_area = p->part_area; a.part_faces = p->part_faces;
        hipLaunchKernelGGL(view_plan_score_kernel, dim3((unsigned)((waves + SUM_WPB - 1) / SUM_WPB)), dim3(DT), 0, stream, a);
    }
    hipLaunchKernelGGL(view_plan_total_kernel, dim3((unsigned)((p->n + SUM_WPB - 1) / SUM_WPB)), dim3(DT), 0, stream, p->part_area,
                       p->part_faces, p->n_blocks, p->n, chosen, sel, gain_area, gain_faces);
    PEDP_HIP_CHECK(hipGetLastError());
    return PEDP_OK;
}

}  // namespace

extern "C" {

int pedp_view_plan_create(pedp_coverage_t cov, int64_t capacity, pedp_view_plan_t *out) {
    const char *who = "pedp_view_plan_create";
    PEDP_REQUIRE(cov && out, "%s: null coverage map/out", who);
    pedp_ctx_t c = cov->ctx;
    PEDP_REQUIRE(capacity >= 1 && capacity <= MAX_CAPACITY, "%s: capacity = %lld, 1 ... %lld", who, (long long)capacity,
                 (long long)MAX_CAPACITY);
    const int64_t n_blocks = (cov->F + SUM_BLOCK - 1) / SUM_BLOCK;
    PEDP_REQUIRE(capacity * (n_blocks > 0 ? n_blocks : 1) < MAX_WAVES, "%s: %lld candidates x %lld blocks of faces are more than one launch",
                 who, (long long)capacity, (long long)n_blocks);
    PEDP_REQUIRE(!c->icp_pending, "%s: a registration is pending on this context (the call allocates device memory)", who);
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    pedp_view_plan_s *p = new pedp_view_plan_s;
    p->cov = cov;
    p->ctx = c;
    p->device = c->device;
    p->F = cov->F;
    p->capacity = capacity;
    p->n_blocks = n_blocks;
    const size_t f = (size_t)p->F, cap = (size_t)capacity, rows = cap * f;
    size_t off = 0;
    auto place = [&](size_t bytes) { const size_t o = off; off += a256(bytes); return o; };
    const size_t o_pix = place(4 * rows), o_key = place(8 * rows), o_fp = place(8 * rows);
    p->w_zero_off = off;
    const size_t o_wpix = place(8 * f), o_wbest = place(8 * f), o_wviews = place(4 * f);
    p->w_zero_bytes = off - p->w_zero_off;
    p->w_ones_off = place(8 * f);
    p->w_ones_bytes = off - p->w_ones_off;
    const size_t o_parta = place(8 * cap * (size_t)n_blocks), o_partf = place(8 * cap * (size_t)n_blocks), o_ga = place(8 * cap),
                 o_gf = place(8 * cap), o_sum = place(sizeof(Sums) * (size_t)n_blocks), o_chosen = place(cap);
    const size_t o_result = off;
    const size_t o_sel = place(sizeof(Sel)), o_total = place(sizeof(Sums));
    p->o_order = place(4 * cap) - o_result;
    p->o_area = place(8 * cap) - o_result;
    p->o_faces = place(8 * cap) - o_result;
    p->result_bytes = off - o_result;
    hipError_t e = hipMalloc((void **)&p->store, off);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        pedp_set_error("%s: hipMalloc(%zu) for %lld candidates x %lld faces -> %s", who, off, (long long)capacity, (long long)p->F,
                       hipGetErrorString(e));
        delete p;
        return PEDP_ERR_HIP;
    }
    char *s = p->store;
    p->col = Columns{(uint32_t *)(s + o_pix), (unsigned long long *)(s + o_key), (unsigned long long *)(s + o_fp)};
    p->w = Work{(unsigned long long *)(s + o_wpix), (unsigned long long *)(s + o_wbest), (unsigned long long *)(s + p->w_ones_off),
                (int32_t *)(s + o_wviews)};
    p->part_area = (double *)(s + o_parta); p->part_faces = (int64_t *)(s + o_partf);
    p->gain_area = (double *)(s + o_ga); p->gain_faces = (int64_t *)(s + o_gf);
    p->sum_part = (Sums *)(s + o_sum); p->chosen = (uint8_t *)(s + o_chosen);
    p->result = s + o_result; p->sel = (Sel *)(s + o_sel); p->total = (Sums *)(s + o_total);
    // enqueued: every later use is behind it on the context's stream
    int rc = clear_rows(p, 0, capacity);
    if (!rc && f && hipMemsetAsync(s + p->w_zero_off, 0, p->w_zero_bytes, c->stream) != hipSuccess) rc = PEDP_ERR_HIP;
    if (!rc && f && hipMemsetAsync(s + p->w_ones_off, 0xFF, p->w_ones_bytes, c->stream) != hipSuccess) rc = PEDP_ERR_HIP;
    if (!rc && hipMemsetAsync(s + o_parta, 0, off - o_parta, c->stream) != hipSuccess) rc = PEDP_ERR_HIP;
    if (rc) {
        if (rc == PEDP_ERR_HIP) pedp_set_error("%s: clearing the plan failed", who);
        pedp_view_plan_destroy(p);
        return rc;
    }
    *out = p;
    return PEDP_OK;
}

int pedp_view_plan_destroy(pedp_view_plan_t p) {
    if (!p) return PEDP_OK;
    if (hipSetDevice(p->device) == hipSuccess) {
        if (p->store) (void)hipFree(p->store);  // waits for the device: nothing enqueued still uses it
        p->io.release();
    }
    delete p;
    return PEDP_OK;
}

int pedp_view_plan_clear(pedp_view_plan_t p) {
    PEDP_REQUIRE(p, "pedp_view_plan_clear: null handle");
    PEDP_HIP_CHECK(hipSetDevice(p->device));
    const int64_t n = p->n;
    p->n = 0;
    return clear_rows(p, 0, n);  // the rows beyond were never written
}

int pedp_view_plan_observe(pedp_view_plan_t p, pedp_mesh_t mesh, const pedp_pinhole *cam, const float *t_hit, const uint32_t *prim_id,
                           double min_cos, int mem, int64_t *index) {
    const char *who = "pedp_view_plan_observe";
    PEDP_REQUIRE(p && mesh && cam, "%s: null handle/mesh/camera", who);
    pedp_ctx_t c = p->ctx;
    PEDP_REQUIRE(mem == PEDP_HOST || mem == PEDP_DEVICE, "%s: bad mem flag %d", who, mem);
    PEDP_REQUIRE(mesh->ctx == c, "%s: the mesh belongs to another context than the coverage map", who);
    PEDP_REQUIRE(mesh->F == p->F, "%s: the mesh has %lld faces, the map %lld", who, (long long)mesh->F, (long long)p->F);
    PEDP_REQUIRE(cam->width > 0 && cam->height > 0 && (int64_t)cam->width * cam->height < MAX_PIXELS, "%s: a %d x %d frame", who,
                 cam->width, cam->height);
    PEDP_REQUIRE(cam->fx > 0.0 && cam->fy > 0.0 && std::isfinite(cam->fx) && std::isfinite(cam->fy) && std::isfinite(cam->cx) &&
                     std::isfinite(cam->cy),
                 "%s: focal lengths must be positive and the intrinsics finite", who);
    PEDP_REQUIRE(t_hit && prim_id, "%s: null t_hit/prim_id", who);
    PEDP_REQUIRE(min_cos >= 0.0 && min_cos <= 1.0, "%s: min_cos = %g, 0 ... 1", who, min_cos);
    PEDP_REQUIRE(p->n < p->capacity, "%s: the plan is full (%lld candidates)", who, (long long)p->capacity);
    PEDP_REQUIRE(mem == PEDP_DEVICE || !c->icp_pending, "%s: a registration is pending on this context (host-memory call)", who);
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    const int64_t n = (int64_t)cam->width * cam->height;
    ObserveArgs a;
    a.t = t_hit; a.id = prim_id; a.depth = nullptr; a.mask = nullptr;
    if (mem == PEDP_HOST) {
        const size_t b4 = a256(4 * (size_t)n);
        int rc = p->io.reserve(2 * b4);
        if (rc) return rc;
        char *io = (char *)p->io.ptr;
        rc = pedp_upload(c, io, t_hit, 4 * (size_t)n);
        if (!rc) rc = pedp_upload(c, io + b4, prim_id, 4 * (size_t)n);
        if (rc) return rc;
        a.t = (const float *)io; a.id = (const uint32_t *)(io + b4);
    }
    a.tri = mesh->tri;
    a.n = n; a.F = p->F;
    a.cam = camera::Cam{cam->fx, cam->fy, cam->cx, cam->cy, cam->width};
    a.fxfy = cam->fx * cam->fy;
    a.depth_scale = 1.0; a.depth_tol = 0.0; a.min_cos = min_cos; a.z_min = 0.001f;
    const size_t at = (size_t)p->n * (size_t)p->F;
    a.row = Columns{p->col.pix + at, p->col.key + at, p->col.fp + at};
    hipLaunchKernelGGL(view_plan_observe_kernel, dim3(blocks_for(n)), dim3(DT), 0, c->stream, a);
    PEDP_HIP_CHECK(hipGetLastError());
    if (index) *index = p->n;
    p->n += 1;  // behind the launch's check: a candidate that was not enqueued is not counted
    if (mem == PEDP_HOST) PEDP_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PEDP_OK;
}

int pedp_view_plan_candidate(pedp_view_plan_t p, int64_t v, int mem, int64_t *pixels, double *best_cos, double *min_footprint) {
    const char *who = "pedp_view_plan_candidate";
    PEDP_REQUIRE(p, "%s: null handle", who);
    pedp_ctx_t c = p->ctx;
    PEDP_REQUIRE(mem == PEDP_HOST || mem == PEDP_DEVICE, "%s: bad mem flag %d", who, mem);
    PEDP_REQUIRE(v >= 0 && v < p->n, "%s: candidate %lld of %lld", who, (long long)v, (long long)p->n);
    PEDP_REQUIRE(mem == PEDP_DEVICE || !c->icp_pending, "%s: a registration is pending on this context (host-memory call)", who);
    if (p->F == 0 || (!pixels && !best_cos && !min_footprint)) return PEDP_OK;
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    const size_t f = (size_t)p->F, b8 = a256(8 * f);
    int64_t *d_pix = pixels;
    double *d_cos = best_cos, *d_fp = min_footprint;
    if (mem == PEDP_HOST) {
        const int rc = p->io.reserve(3 * b8);
        if (rc) return rc;
        char *io = (char *)p->io.ptr;
        d_pix = pixels ? (int64_t *)io : nullptr;
        d_cos = best_cos ? (double *)(io + b8) : nullptr;
        d_fp = min_footprint ? (double *)(io + 2 * b8) : nullptr;
    }
    const size_t at = (size_t)v * f;
    hipLaunchKernelGGL(view_plan_candidate_kernel, dim3(blocks_for(p->F)), dim3(DT), 0, c->stream,
                       Columns{p->col.pix + at, p->col.key + at, p->col.fp + at}, p->F, d_pix, d_cos, d_fp);
    PEDP_HIP_CHECK(hipGetLastError());
    int rc = PEDP_OK;
    if (mem == PEDP_HOST) {
        if (pixels) rc = pedp_download(c, pixels, d_pix, 8 * f);
        if (!rc && best_cos) rc = pedp_download(c, best_cos, d_cos, 8 * f);
        if (!rc && min_footprint) rc = pedp_download(c, min_footprint, d_fp, 8 * f);
    }
    return rc;
}

int pedp_view_plan_reset(pedp_view_plan_t p) {
    PEDP_REQUIRE(p, "pedp_view_plan_reset: null handle");
    if (p->F == 0) return PEDP_OK;
    PEDP_HIP_CHECK(hipSetDevice(p->device));
    hipLaunchKernelGGL(view_plan_reset_kernel, dim3(blocks_for(p->F)), dim3(DT), 0, p->ctx->stream, p->cov->state(), p->w, p->F);
    PEDP_HIP_CHECK(hipGetLastError());
    return PEDP_OK;
}

int pedp_view_plan_commit(pedp_view_plan_t p, int64_t v) {
    const char *who = "pedp_view_plan_commit";
    PEDP_REQUIRE(p, "%s: null handle", who);
    PEDP_REQUIRE(v >= 0 && v < p->n, "%s: candidate %lld of %lld", who, (long long)v, (long long)p->n);
    if (p->F == 0) return PEDP_OK;
    PEDP_HIP_CHECK(hipSetDevice(p->device));
    hipLaunchKernelGGL(view_plan_commit_kernel, dim3(blocks_for(p->F)), dim3(DT), 0, p->ctx->stream, p->col, p->w, p->F, v, (const Sel *)nullptr);
    PEDP_HIP_CHECK(hipGetLastError());
    return PEDP_OK;
}

int pedp_view_plan_score(pedp_view_plan_t p, const pedp_coverage_criteria *crit, int mem, double *gain_area, int64_t *gain_faces) {
    const char *who = "pedp_view_plan_score";
    PEDP_REQUIRE(p, "%s: null handle", who);
    pedp_ctx_t c = p->ctx;
    PEDP_REQUIRE(mem == PEDP_HOST || mem == PEDP_DEVICE, "%s: bad mem flag %d", who, mem);
    PEDP_REQUIRE(mem == PEDP_DEVICE || !c->icp_pending, "%s: a registration is pending on this context (host-memory call)", who);
    if (p->n == 0 || (!gain_area && !gain_faces)) return PEDP_OK;
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    const pedp_coverage_criteria k = crit ? *crit : DEFAULT_CRITERIA;
    const bool host = mem == PEDP_HOST;
    int rc = launch_score(p, k, false, host ? p->gain_area : gain_area, host ? p->gain_faces : gain_faces);
    if (!rc && host && gain_area) rc = pedp_download(c, gain_area, p->gain_area, 8 * (size_t)p->n);
    if (!rc && host && gain_faces) rc = pedp_download(c, gain_faces, p->gain_faces, 8 * (size_t)p->n);
    return rc;
}

int pedp_view_plan_select(pedp_view_plan_t p, const pedp_coverage_criteria *crit, int64_t k, double min_gain, int32_t *order,
                          double *gain_area, int64_t *gain_faces, int64_t *n_selected, pedp_coverage_totals *totals) {
    const char *who = "pedp_view_plan_select";
    PEDP_REQUIRE(p && n_selected, "%s: null handle/n_selected", who);
    pedp_ctx_t c = p->ctx;
    *n_selected = 0;
    PEDP_REQUIRE(k >= 0, "%s: k = %lld", who, (long long)k);
    PEDP_REQUIRE(!c->icp_pending, "%s: a registration is pending on this context (the call waits for the stream)", who);
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    const pedp_coverage_criteria crt = crit ? *crit : DEFAULT_CRITERIA;
    int rc = pedp_view_plan_reset(p);
    if (rc) return rc;
    PEDP_HIP_CHECK(hipMemsetAsync(p->chosen, 0, (size_t)p->capacity, c->stream));
    PEDP_HIP_CHECK(hipMemsetAsync(p->result, 0, (size_t)((char *)(p->total + 1) - p->result), c->stream));  // the rounds' state and the totals
    const int64_t rounds = k < p->n ? k : p->n;  // a round after the last candidate could only stop
    for (int64_t r = 0; r < rounds; ++r) {
        rc = launch_score(p, crt, true, p->gain_area, p->gain_faces);
        if (rc) return rc;
        hipLaunchKernelGGL(view_plan_choose_kernel, dim3(1), dim3(64), 0, c->stream, p->gain_area, p->gain_faces, p->n, min_gain, p->chosen,
                           p->sel, (int32_t *)(p->result + p->o_order), (double *)(p->result + p->o_area),
                           (int64_t *)(p->result + p->o_faces));
        if (p->F)
            hipLaunchKernelGGL(view_plan_commit_kernel, dim3(blocks_for(p->F)), dim3(DT), 0, c->stream, p->col, p->w, p->F, (int64_t)0,
                               (const Sel *)p->sel);
        PEDP_HIP_CHECK(hipGetLastError());
    }
    if (p->F) {
        launch_summary(c->stream, p->w.state(), crt, p->cov->map->area, p->F, p->sum_part, p->total);
        PEDP_HIP_CHECK(hipGetLastError());
    }
    const void *view = nullptr;
    rc = pedp_download_view(c, p->result, p->result_bytes, &view);  // the one wait
    if (rc) return rc;
    const char *h = (const char *)view;
    Sel sel;
    Sums sums;
    memcpy(&sel, h + ((char *)p->sel - p->result), sizeof(sel));
    memcpy(&sums, h + ((char *)p->total - p->result), sizeof(sums));
    const size_t n = (size_t)sel.n;
    if (order) memcpy(order, h + p->o_order, 4 * n);
    if (gain_area) memcpy(gain_area, h + p->o_area, 8 * n);
    if (gain_faces) memcpy(gain_faces, h + p->o_faces, 8 * n);
    *n_selected = sel.n;
    if (totals) {
        totals->faces = p->F;
        totals->covered_faces = sums.covered;
        totals->covered_area = sums.covered_area;
        totals->total_area = sums.total_area;
    }
    return PEDP_OK;
}

}  // extern "C"
