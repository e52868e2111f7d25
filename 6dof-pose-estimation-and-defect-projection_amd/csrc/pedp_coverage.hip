// The inspection coverage map: which faces of the CAD model the camera has seen, and how well.
//   * per VIEW (one camera frame, the model posed as the frame sees it): every pixel of the cast gets one class --
//     masked, miss, no depth, occluded, behind, grazing, seen -- from the cast's hit, the measured depth and the angle
//     between the ray and the face.
//   * per FACE, laid over the faces of a defect map: the seen pixels, the views that saw it, the best cosine, the
//     smallest footprint of a pixel on it, and the pixels where something stood in front of it.
// Integer atomics only, as in pedp_defectmap.hip: the cosine's maximum through the order-preserving key, the footprint's
// minimum on the bits of a non-negative double, counts and the view stamp.  The areas, centroids, boxes, the welded
// adjacency and the regions' body are the defect map's (defectmap/shared.h): one weld and one adjacency per model.  The
// per-pixel rule, the state's criteria, the summary's sums and the handle are in coverage/shared.h, which the view
// planner (pedp_viewplan.hip) includes too.
#include "coverage/shared.h"

#ifndef PEDP_COVERAGE_COMBINE
#define PEDP_COVERAGE_COMBINE 1  // 0: every pixel goes to the atomics itself (the A/B of profiles/coverage_time.json)
#endif

namespace {

using namespace coverage;

constexpr int COUNTER_SLOTS = 64;  // copies of the seven class counters: a block adds to copy blockIdx % 64

struct AddArgs : View {
    uint8_t *status;  // nullable
    uint32_t view;    // this view's stamp, 1 ...
    unsigned long long *pixels, *blocked, *best, *minfp, *counters;
    int32_t *views;
    uint32_t *stamp;
};

// One view, a lane per pixel.  A coarse CAD face covers thousands of neighbouring pixels, so a run of equal faces in
// neighbouring lanes (defectmap/shared.h) sends one maximum, one minimum, its SEEN count, its OCCLUDED count and one
// stamp through its first lane.
__global__ __launch_bounds__(DT) void coverage_add_kernel(AddArgs a) {
    __shared__ unsigned block_count[N_CLASSES];
    const int64_t i = (int64_t)blockIdx.x * DT + threadIdx.x;
    const int lane = threadIdx.x & 63;
    if (threadIdx.x < N_CLASSES) block_count[threadIdx.x] = 0;
    __syncthreads();
    int cls = -1;  // beyond the frame
    uint32_t f = NONE;
    unsigned long long key = 0, fp = NEVER;  // an OCCLUDED lane's values change neither the maximum nor the minimum
    if (i < a.n) {
        cls = classify(a, i, f, key, fp);
        if (a.status) a.status[i] = (uint8_t)cls;
    }
    const bool seen = cls == SEEN, occluded = cls == OCCLUDED;
    unsigned long long n_seen = seen, n_occluded = occluded;
#if PEDP_COVERAGE_COMBINE
    const LaneRun run = lane_run(seen || occluded ? f : NONE, lane);
    if (run.wide) {
        key = run_max(key, lane, run.end);
        fp = run_min(fp, lane, run.end);
        const unsigned long long mine = run.lanes(lane);
        n_seen = (unsigned long long)__builtin_popcountll(__builtin_amdgcn_ballot_w64(seen) & mine);
        n_occluded = (unsigned long long)__builtin_popcountll(__builtin_amdgcn_ballot_w64(occluded) & mine);
    }
    const bool head = run.head;
#else
    const bool head = seen || occluded;
#endif
    if (head) {
        if (n_seen) {
            atomicMax(&a.best[f], key);
            if (fp != NEVER) atomicMin(&a.minfp[f], fp);
            atomicAdd(&a.pixels[f], n_seen);
            if (atomicMax(&a.stamp[f], a.view) < a.view) atomicAdd(&a.views[f], 1);
        }
        if (n_occluded) atomicAdd(&a.blocked[f], n_occluded);
    }
    // The class counters: a wave's counts meet in LDS and the block adds each class once, to one of COUNTER_SLOTS copies.
    // Every wave of a frame would otherwise add to the same seven addresses, which serialises them.
#pragma unroll
    for (int k = 0; k < N_CLASSES; ++k) {
        const int cnt = __builtin_popcountll(__builtin_amdgcn_ballot_w64(cls == k));
        if (lane == 0 && cnt) atomicAdd(&block_count[k], (unsigned)cnt);
    }
    __syncthreads();
    if (threadIdx.x < N_CLASSES && block_count[threadIdx.x])
        atomicAdd(&a.counters[(blockIdx.x % COUNTER_SLOTS) * N_CLASSES + threadIdx.x], (unsigned long long)block_count[threadIdx.x]);
}

__global__ __launch_bounds__(DT) void coverage_faces_kernel(State s, int64_t F, int64_t *__restrict__ pixels, int32_t *__restrict__ views,
                                                           double *__restrict__ best_cos, double *__restrict__ min_footprint,
                                                           int64_t *__restrict__ blocked) {
    const int64_t f = (int64_t)blockIdx.x * DT + threadIdx.x;
    if (f >= F) return;
    if (pixels) pixels[f] = (int64_t)s.pixels[f];
    if (views) views[f] = s.views[f];
    if (best_cos) best_cos[f] = best_cos_of(s, f);
    if (min_footprint) min_footprint[f] = min_footprint_of(s, f);
    if (blocked) blocked[f] = (int64_t)s.blocked[f];
}

// the marking of a regions call: the covered faces (want = 1) or the uncovered ones (want = 0)
__global__ __launch_bounds__(DT) void coverage_seed_kernel(State s, pedp_coverage_criteria c, int want, int64_t F, uint8_t *__restrict__ seed,
                                                          uint8_t *__restrict__ mark) {
    const int64_t f = (int64_t)blockIdx.x * DT + threadIdx.x;
    if (f >= F) return;
    const uint8_t m = (is_covered(s, c, f) ? 1 : 0) == want;
    seed[f] = m;
    mark[f] = m;
}

}  // namespace

namespace {
int clear_state(pedp_coverage_s *v) {
    PEDP_HIP_CHECK(hipMemsetAsync(v->store, 0, v->zero_bytes, v->ctx->stream));
    if (v->ones_bytes) PEDP_HIP_CHECK(hipMemsetAsync(v->store + v->ones_off, 0xFF, v->ones_bytes, v->ctx->stream));
    return PEDP_OK;
}
}  // namespace

extern "C" {

int pedp_coverage_create(pedp_defect_map_t map, pedp_coverage_t *out) {
    const char *who = "pedp_coverage_create";
    PEDP_REQUIRE(map && out, "%s: null map/out", who);
    pedp_ctx_t c = map->ctx;
    PEDP_REQUIRE(!c->icp_pending, "%s: a registration is pending on this context (the call allocates device memory)", who);
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    pedp_coverage_s *v = new pedp_coverage_s;
    v->map = map;
    v->ctx = c;
    v->device = c->device;
    v->F = map->F;
    const size_t f = (size_t)v->F;
    size_t off = 0;
    auto place = [&](size_t bytes) { const size_t o = off; off += a256(bytes); return o; };
    const size_t o_pix = place(8 * f), o_blk = place(8 * f), o_best = place(8 * f), o_views = place(4 * f), o_stamp = place(4 * f),
                 o_cnt = place(8 * N_CLASSES * COUNTER_SLOTS);
    v->zero_bytes = off;
    v->ones_off = place(8 * f);
    v->ones_bytes = off - v->ones_off;
    hipError_t e = hipMalloc((void **)&v->store, off);
    if (e != hipSuccess) {
        pedp_set_error("%s: hipMalloc(%zu) -> %s", who, off, hipGetErrorString(e));
        delete v;
        return PEDP_ERR_HIP;
    }
    v->pixels = (unsigned long long *)(v->store + o_pix); v->blocked = (unsigned long long *)(v->store + o_blk);
    v->best = (unsigned long long *)(v->store + o_best); v->views = (int32_t *)(v->store + o_views);
    v->stamp = (uint32_t *)(v->store + o_stamp); v->counters = (unsigned long long *)(v->store + o_cnt);
    v->minfp = (unsigned long long *)(v->store + v->ones_off);
    const int rc = clear_state(v);  // enqueued: every later use is behind it on the context's stream
    if (rc) {
        pedp_coverage_destroy(v);
        return rc;
    }
    *out = v;
    return PEDP_OK;
}

int pedp_coverage_destroy(pedp_coverage_t v) {
    if (!v) return PEDP_OK;
    if (hipSetDevice(v->device) == hipSuccess) {
        if (v->store) (void)hipFree(v->store);  // waits for the device: nothing enqueued still uses it
        v->io.release();
    }
    delete v;
    return PEDP_OK;
}

int pedp_coverage_add(pedp_coverage_t v, pedp_mesh_t mesh, const pedp_pinhole *cam, const float *t_hit, const uint32_t *prim_id,
                      const float *depth, const uint8_t *mask, const pedp_coverage_view *prm, int mem, uint8_t *status) {
    const char *who = "pedp_coverage_add";
    PEDP_REQUIRE(v && mesh && cam, "%s: null handle/mesh/camera", who);
    pedp_ctx_t c = v->ctx;
    PEDP_REQUIRE(mem == PEDP_HOST || mem == PEDP_DEVICE, "%s: bad mem flag %d", who, mem);
    PEDP_REQUIRE(mesh->ctx == c, "%s: the mesh belongs to another context than the coverage map", who);
    PEDP_REQUIRE(mesh->F == v->F, "%s: the mesh has %lld faces, the map %lld", who, (long long)mesh->F, (long long)v->F);
    PEDP_REQUIRE(cam->width > 0 && cam->height > 0 && (int64_t)cam->width * cam->height < MAX_PIXELS, "%s: a %d x %d frame", who,
                 cam->width, cam->height);
    PEDP_REQUIRE(cam->fx > 0.0 && cam->fy > 0.0 && std::isfinite(cam->fx) && std::isfinite(cam->fy) && std::isfinite(cam->cx) &&
                     std::isfinite(cam->cy),
                 "%s: focal lengths must be positive and the intrinsics finite", who);
    PEDP_REQUIRE(t_hit && prim_id, "%s: null t_hit/prim_id", who);
    PEDP_REQUIRE(prm || !depth, "%s: depth needs parameters (depth_tol has no default)", who);
    const pedp_coverage_view p = prm ? *prm : pedp_coverage_view{1.0, 0.0, 0.0, 0.001f};
    PEDP_REQUIRE(!depth || p.depth_tol >= 0.0, "%s: depth_tol = %g with a depth image (it must be >= 0)", who, p.depth_tol);
    PEDP_REQUIRE(p.min_cos >= 0.0 && p.min_cos <= 1.0, "%s: min_cos = %g, 0 ... 1", who, p.min_cos);
    PEDP_REQUIRE(mem == PEDP_DEVICE || !c->icp_pending, "%s: a registration is pending on this context (host-memory call)", who);
    PEDP_REQUIRE(v->n_views < 0xFFFFFFFEll, "%s: 2^32 - 2 views since the last clear", who);
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    const int64_t n = (int64_t)cam->width * cam->height;
    AddArgs a;
    a.t = t_hit; a.id = prim_id; a.depth = depth; a.mask = mask; a.status = status;
    if (mem == PEDP_HOST) {
        const size_t b4 = a256(4 * (size_t)n), b1 = a256((size_t)n);
        int rc = v->io.reserve(3 * b4 + 2 * b1);
        if (rc) return rc;
        char *io = (char *)v->io.ptr;
        rc = pedp_upload(c, io, t_hit, 4 * (size_t)n);
        if (!rc) rc = pedp_upload(c, io + b4, prim_id, 4 * (size_t)n);
        if (!rc && depth) rc = pedp_upload(c, io + 2 * b4, depth, 4 * (size_t)n);
        if (!rc && mask) rc = pedp_upload(c, io + 3 * b4, mask, (size_t)n);
        if (rc) return rc;
        a.t = (const float *)io; a.id = (const uint32_t *)(io + b4);
        a.depth = depth ? (const float *)(io + 2 * b4) : nullptr;
        a.mask = mask ? (const uint8_t *)(io + 3 * b4) : nullptr;
        a.status = status ? (uint8_t *)(io + 3 * b4 + b1) : nullptr;
    }
    a.tri = mesh->tri;
    a.n = n; a.F = v->F;
    a.cam = camera::Cam{cam->fx, cam->fy, cam->cx, cam->cy, cam->width};
    a.fxfy = cam->fx * cam->fy;
    a.depth_scale = p.depth_scale; a.depth_tol = p.depth_tol; a.min_cos = p.min_cos; a.z_min = p.z_min;
    a.view = (uint32_t)(v->n_views + 1);
    a.pixels = v->pixels; a.blocked = v->blocked; a.best = v->best; a.minfp = v->minfp; a.counters = v->counters;
    a.views = v->views; a.stamp = v->stamp;
    hipLaunchKernelGGL(coverage_add_kernel, dim3(blocks_for(n)), dim3(DT), 0, c->stream, a);
    PEDP_HIP_CHECK(hipGetLastError());
    v->n_views += 1;  // behind the launch's check: a view that was not enqueued is not counted
    if (mem == PEDP_HOST) {
        if (status) return pedp_download(c, status, a.status, (size_t)n);
        PEDP_HIP_CHECK(hipStreamSynchronize(c->stream));
    }
    return PEDP_OK;
}

int pedp_coverage_clear(pedp_coverage_t v) {
    PEDP_REQUIRE(v, "pedp_coverage_clear: null handle");
    v->n_views = 0;
    PEDP_HIP_CHECK(hipSetDevice(v->device));
    return clear_state(v);
}

int pedp_coverage_faces(pedp_coverage_t v, int mem, int64_t *pixels, int32_t *views, double *best_cos, double *min_footprint,
                        int64_t *blocked) {
    const char *who = "pedp_coverage_faces";
    PEDP_REQUIRE(v, "%s: null handle", who);
    pedp_ctx_t c = v->ctx;
    PEDP_REQUIRE(mem == PEDP_HOST || mem == PEDP_DEVICE, "%s: bad mem flag %d", who, mem);
    PEDP_REQUIRE(mem == PEDP_DEVICE || !c->icp_pending, "%s: a registration is pending on this context (host-memory call)", who);
    if (v->F == 0 || (!pixels && !views && !best_cos && !min_footprint && !blocked)) return PEDP_OK;
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    const size_t f = (size_t)v->F, b8 = a256(8 * f);
    int64_t *d_pix = pixels, *d_blk = blocked;
    int32_t *d_views = views;
    double *d_cos = best_cos, *d_fp = min_footprint;
    if (mem == PEDP_HOST) {
        const int rc = v->io.reserve(4 * b8 + a256(4 * f));
        if (rc) return rc;
        char *io = (char *)v->io.ptr;
        d_pix = pixels ? (int64_t *)io : nullptr;
        d_blk = blocked ? (int64_t *)(io + b8) : nullptr;
        d_cos = best_cos ? (double *)(io + 2 * b8) : nullptr;
        d_fp = min_footprint ? (double *)(io + 3 * b8) : nullptr;
        d_views = views ? (int32_t *)(io + 4 * b8) : nullptr;
    }
    hipLaunchKernelGGL(coverage_faces_kernel, dim3(blocks_for(v->F)), dim3(DT), 0, c->stream, v->state(), v->F, d_pix, d_views, d_cos, d_fp,
                       d_blk);
    PEDP_HIP_CHECK(hipGetLastError());
    int rc = PEDP_OK;
    if (mem == PEDP_HOST) {
        if (pixels) rc = pedp_download(c, pixels, d_pix, 8 * f);
        if (!rc && views) rc = pedp_download(c, views, d_views, 4 * f);
        if (!rc && best_cos) rc = pedp_download(c, best_cos, d_cos, 8 * f);
        if (!rc && min_footprint) rc = pedp_download(c, min_footprint, d_fp, 8 * f);
        if (!rc && blocked) rc = pedp_download(c, blocked, d_blk, 8 * f);
    }
    return rc;
}

int pedp_coverage_stats(pedp_coverage_t v, int64_t *views, int64_t classes[7]) {
    const char *who = "pedp_coverage_stats";
    PEDP_REQUIRE(v, "%s: null handle", who);
    pedp_ctx_t c = v->ctx;
    if (views) *views = v->n_views;
    if (!classes) return PEDP_OK;
    PEDP_REQUIRE(!c->icp_pending, "%s: a registration is pending on this context (the call waits for the stream)", who);
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    unsigned long long cnt[COUNTER_SLOTS * N_CLASSES];
    const int rc = pedp_download(c, cnt, v->counters, sizeof(cnt));
    if (rc) return rc;
    for (int k = 0; k < N_CLASSES; ++k) {
        classes[k] = 0;
        for (int slot = 0; slot < COUNTER_SLOTS; ++slot) classes[k] += (int64_t)cnt[slot * N_CLASSES + k];
    }
    return PEDP_OK;
}

int pedp_coverage_summary(pedp_coverage_t v, const pedp_coverage_criteria *crit, pedp_coverage_totals *out) {
    const char *who = "pedp_coverage_summary";
    PEDP_REQUIRE(v && out, "%s: null handle/out", who);
    pedp_ctx_t c = v->ctx;
    PEDP_REQUIRE(!c->icp_pending, "%s: a registration is pending on this context (the call waits for the stream)", who);
    out->faces = v->F;
    out->covered_faces = 0;
    out->covered_area = 0.0;
    out->total_area = 0.0;
    if (v->F == 0) return PEDP_OK;
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    const int64_t n_blocks = (v->F + SUM_BLOCK - 1) / SUM_BLOCK;
    int rc = v->io.reserve(a256(sizeof(Sums) * (size_t)(n_blocks + 1)));
    if (rc) return rc;
    Sums *part = (Sums *)v->io.ptr, *total = part + n_blocks;
    const pedp_coverage_criteria k = crit ? *crit : DEFAULT_CRITERIA;
    launch_summary(c->stream, v->state(), k, v->map->area, v->F, part, total);
    PEDP_HIP_CHECK(hipGetLastError());
    Sums s;
    rc = pedp_download(c, &s, total, sizeof(s));
    if (rc) return rc;
    out->covered_faces = s.covered;
    out->covered_area = s.covered_area;
    out->total_area = s.total_area;
    return PEDP_OK;
}

int pedp_coverage_regions(pedp_coverage_t v, const pedp_coverage_criteria *crit, int covered, int32_t grow, int mem, int32_t *labels,
                          int64_t capacity, pedp_defect_region *table, int64_t *n_regions) {
    const char *who = "pedp_coverage_regions";
    PEDP_REQUIRE(v, "%s: null handle", who);
    pedp_defect_map_s *m = v->map;
    pedp_region_ws w;
    const int rc = pedp_defect_regions_begin(m, who, grow, mem, capacity, table, n_regions, w);
    if (rc || !w.seed) return rc;
    const pedp_coverage_criteria k = crit ? *crit : DEFAULT_CRITERIA;
    hipLaunchKernelGGL(coverage_seed_kernel, dim3(blocks_for(v->F)), dim3(DT), 0, v->ctx->stream, v->state(), k, covered ? 1 : 0, v->F, w.seed,
                       w.mark[0]);
    const pedp_region_columns col{v->best, v->pixels, v->views};
    return pedp_defect_regions_finish(m, who, w, col, grow, mem, labels, capacity, table, n_regions);
}

}  // extern "C"
