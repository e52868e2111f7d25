// Ray / triangle closest-hit sweep for gfx950 (MI355X): the host side.  The kernels live in csrc/ray/*.h.
//
// Replaces RaycastingScene.add_triangles + cast_rays as called by
// src/defect_projection.py:245-256 (one camera ray per heat-map pixel against every
// triangle of the posed mesh).  Arithmetic contract: oracle/ray.c -- Moeller-Trumbore in
// scalar-triple-product form, division deferred to accepted hits, every operation one fp32
// rounding in a fixed order.  Results are bit-identical to it: t_hit, primitive ids, (u, v).
//
//   per triangle:  e1 = v1 - v0, e2 = v2 - v0, m = e2 x e1
//   per test:      det = d . m ; s = o - v0 ; un = d . (e2 x s) ; vn = d . (s x e1) ; tn = -(s . m)
//
// Whatever a variant does, the pairs it accepts go through the same mt_eval / mt_accept / mt_key (ray/mt.h) and
// meet in one packed 64-bit atomicMin per ray: key = (bits(t) << 32) | triangle id orders by t (t >= 0: IEEE bits
// are monotone), then by triangle index -- the oracle's tie rule, independent of execution order.
// ray_finalize_kernel (ray/finalize.h) turns the keys into t_hit / prim_id / (u, v).
//
//   variant (pedp_raycast_configure)                                              kernels
//   1  every ray x every triangle, one origin: bf16 MFMA filter + exact test      ray/sweep_matrix.h
//   2  triangle per lane, wavefront-wide min-t reduction (auto below 16,384 rays) ray/sweep_tri_lane.h
//   3  ray per lane with conservative cluster culling, one origin                 ray/sweep_culled.h
//   4  triangle-driven over a grid of ray directions, one origin (auto from       ray/grid.h
//      16,384 rays; what a resident ray set keeps built)
//   5  every ray x every triangle, packed fp32 on the vector pipe                 ray/sweep_packed.h
// Variants 1, 3 and 5 hand rays of differing origins to the general-origin sweep of ray/sweep_packed.h on the
// device; variant 4 completes what its grid cannot answer in ray_finalize_kernel.  ray/mesh_records.h builds what
// a mesh handle holds.
//
// The all-hits queries (count / occlusion / list of intersections, at the end of this file) hand the same accepted
// pairs to other sinks than the atomicMin: ray/all_hits.h, over the grid's traversal or an exhaustive sweep.
#include "pedp_internal.h"
#include <algorithm>
#include <cstdlib>
#include <new>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>
#include "ray/mt.h"
#include "ray/mesh_records.h"
#include "ray/sweep_packed.h"
#include "ray/sweep_matrix.h"
#include "ray/sweep_culled.h"
#include "ray/grid.h"
#include "ray/sweep_tri_lane.h"
#include "ray/finalize.h"
#include "ray/all_hits.h"

namespace {

// kernel k on the context's stream: `grid` workgroups of `block` threads
template <class K, class... A> void launch(pedp_ctx_t c, K k, int64_t grid, int block, A... a) {
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(block), 0, c->stream, a...);
}

// Hands out consecutive pieces of one buffer, each a multiple of 256 bytes.  A layout below holds one in front of
// its pointers, which take their pieces as they are initialised, so the order of declaration IS the layout.
// base == nullptr only measures: every piece is then a null pointer and `at` ends as the size the layout needs.
struct Carver {
    char *base;
    size_t at = 0;
    template <class T> T *take(size_t count) {
        T *p = base ? (T *)(base + at) : nullptr;
        at += (sizeof(T) * count + 255) / 256 * 256;
        return p;
    }
};

// ---------------------------------------------------------------- where a cast writes its results (uv: nullable)
struct RayOut { float *t; uint32_t *id; float *uv; };

// PEDP_DEVICE: the caller's arrays.  PEDP_HOST: slices of c->ray_out, delivered by ray_out_deliver after the cast;
// host rays (rays != nullptr; a ray set's are resident) go into c->ray_in and *rays becomes their device address.
int ray_stage(pedp_ctx_t c, int mem, int64_t N, const float **rays, float *t_hit, uint32_t *prim_id, float *uv, RayOut *o) {
    *o = RayOut{t_hit, prim_id, uv};
    if (mem != PEDP_HOST) return PEDP_OK;
    int st = c->ray_out.reserve(sizeof(float) * 4 * (size_t)N);
    if (!st && rays) st = c->ray_in.reserve(sizeof(float) * 6 * (size_t)N);
    if (!st && rays) st = pedp_upload(c, c->ray_in.ptr, *rays, sizeof(float) * 6 * (size_t)N);
    if (st) return st;
    if (rays) *rays = (const float *)c->ray_in.ptr;
    o->t = (float *)c->ray_out.ptr;
    o->id = (uint32_t *)(o->t + N);
    o->uv = uv ? (float *)(o->id + N) : nullptr;
    return PEDP_OK;
}

int ray_out_deliver(pedp_ctx_t c, int mem, int64_t N, const RayOut &o, float *t_hit, uint32_t *prim_id, float *uv) {
    if (mem != PEDP_HOST) return PEDP_OK;
    int rc = pedp_download(c, t_hit, o.t, sizeof(float) * (size_t)N);
    if (!rc) rc = pedp_download(c, prim_id, o.id, sizeof(uint32_t) * (size_t)N);
    if (!rc && uv) rc = pedp_download(c, uv, o.uv, sizeof(float) * 2 * (size_t)N);
    if (rc) return rc;
    PEDP_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PEDP_OK;
}

// ---------------------------------------------------------------- variant 4: the grid's scratch, its build, its cast
// What the grid kernels work in, for N rays: the context's ray_rast buffer per call, part of a ray set's allocation.
// (The order of the members, the two headers' take<> calls included, is the buffer's layout: see Carver.)
struct GridScratch {
    Carver cv; int64_t N;
    // two headers, used in turn: the last kernel of a cast puts the OTHER one back to its start values
    // (it still reads its own), so no kernel ever resets a word that workgroups of the same launch test
    RastHdr *hdr[2] = {cv.take<RastHdr>(1), cv.take<RastHdr>(1)};
    uint4 *part = cv.take<uint4>(RAST_BBLOCKS);               // partial bounds of rast_bounds_kernel's workgroups
    unsigned *head = cv.take<unsigned>((size_t)N);            // chain head per cell
    float4 *nodes = cv.take<float4>((size_t)N);               // direction + next index per ray
    RastItem *items = cv.take<RastItem>(RAST_ITEM_CAP);       // tiles of the larger rectangles
    unsigned *full_list = cv.take<unsigned>(RAST_FULL_CAP);   // triangles without a bounded image
    GridScratch(char *base = nullptr, int64_t N = 0) : cv{base}, N(N) { static_assert(sizeof(RastHdr) <= 256, "header slot"); }
    static size_t bytes(int64_t N) { return GridScratch(nullptr, N).cv.at; }
};

// a header's start values (static: the copy that takes them is asynchronous)
const RastHdr RAST_HDR_START = {1};

// The frame, the bounds and the chains of N rays under header h; the bounds kernel also sets every key to "miss"
// and every head to "none".
void grid_enqueue_build(pedp_ctx_t c, const float *d_rays, int64_t N, const GridScratch &g, RastHdr *h, unsigned long long *keys) {
    launch(c, rast_bounds_kernel, RAST_BBLOCKS, 256, d_rays, N, h, keys, g.head, g.part);
    launch(c, rast_insert_kernel, (N + 255) / 256, 256, d_rays, N, h, g.head, g.nodes, g.part);
}

// The triangles against the grid built under header h: every accepted pair goes to `sink` (HitMin: a cast).
template <class Sink>
void grid_enqueue_walk(pedp_ctx_t c, pedp_mesh_t mesh, const float *d_rays, int64_t N, const GridScratch &g, RastHdr *h, Sink sink) {
    if (mesh->F > 0)
        launch(c, rast_tri_kernel<Sink>, (mesh->F + 255) / 256, 256, mesh->tri, mesh->F, h, g.head, g.nodes, g.items, sink, g.full_list);
    launch(c, rast_item_kernel<Sink>, RAST_ITEM_WAVES / 4, 256, mesh->tri, h, g.head, g.nodes, g.items, sink);
    launch(c, rast_full_kernel<Sink>, (N + 255) / 256, 256, mesh->tri, d_rays, N, h, g.full_list, sink);
}

// The triangles against the built grid, the end of the timed stretch, the results.  seq picks the header; status:
// the pinned status words, which the last kernel writes through the device's address of them.
int grid_enqueue_cast(pedp_ctx_t c, pedp_mesh_t mesh, const float *d_rays, int64_t N, const GridScratch &g, unsigned seq,
                      unsigned long long *keys, int *status, const RayOut &o, int reset_keys) {
    int *d_status = nullptr;
    PEDP_HIP_CHECK(hipHostGetDevicePointer((void **)&d_status, status, 0));
    RastHdr *h = g.hdr[seq & 1], *h_next = g.hdr[(seq + 1) & 1];
    grid_enqueue_walk(c, mesh, d_rays, N, g, h, HitMin{keys});
    PEDP_HIP_CHECK(hipGetLastError());
    PEDP_HIP_CHECK(hipEventRecord(c->ev1, c->stream));
    c->ray_timed = true;
    launch(c, ray_finalize_kernel, (N + 255) / 256, 256, mesh->tri, d_rays, N, keys, o.t, o.id, o.uv, h, h_next, d_status,
           (const f2 *)mesh->tri2, (int)(mesh->F_padded / (2 * RPL_PAIRS)), reset_keys);
    PEDP_HIP_CHECK(hipGetLastError());
    return PEDP_OK;
}

// per call: grid and chains rebuilt from the rays in the context's scratch
int cast_grid(pedp_ctx_t c, pedp_mesh_t mesh, const float *d_rays, int64_t N, unsigned long long *keys, const RayOut &o) {
    PEDP_REQUIRE(N < (int64_t)0x7FFFFFF0 && mesh->F < (int64_t)0x7FFFFFF0, "pedp_raycast: variant 4 takes fewer than 2^31 rays / triangles");
    if (!c->rast_status) {
        PEDP_HIP_CHECK(hipHostMalloc((void **)&c->rast_status, 64, hipHostMallocMapped));
        c->rast_status[0] = 0; c->rast_status[1] = -1;
    }
    int st = c->ray_rast.reserve(GridScratch::bytes(N));
    if (st) return st;
    char *base = (char *)c->ray_rast.ptr;
    const GridScratch g(base, N);
    RastHdr *h = g.hdr[c->rast_seq & 1];
    if (c->rast_hdr_ready != (void *)base) {  // new buffer, or a cast that did not reach its last kernel
        PEDP_HIP_CHECK(hipMemcpyAsync(h, &RAST_HDR_START, sizeof(RastHdr), hipMemcpyHostToDevice, c->stream));
        PEDP_HIP_CHECK(hipStreamSynchronize(c->stream));
    }
    c->rast_hdr_ready = nullptr;
    PEDP_HIP_CHECK(hipEventRecord(c->ev0, c->stream));
    grid_enqueue_build(c, d_rays, N, g, h, keys);
    st = grid_enqueue_cast(c, mesh, d_rays, N, g, c->rast_seq, keys, c->rast_status, o, 0);
    if (st) return st;
    c->rast_hdr_ready = (void *)base;
    c->rast_seq += 1;
    return PEDP_OK;
}

// Triangle chunks per ray block (chunk c is served by XCD c % 8): the configured count, or enough workgroups for
// >= 4 rounds over the chip with no chunk below min_units.
int tri_chunks(pedp_ctx_t c, int64_t ray_blocks, int64_t units, int64_t min_units) {
    int n = c->ray_tri_chunks;
    if (n == 0)
        for (n = 8; ray_blocks * n < 4 * 8 * (int64_t)c->num_cus && units / (n * 2) >= min_units;) n *= 2;
    return n;
}

// ---------------------------------------------------------------- variants 1, 3, 5: sweeps that know a shared origin
// What these variants' kernels work in, and the counts that size it: the context's ray_aux buffer (cv) and, kept
// between calls, variant 3's direction order in ray_order (order).  Member order is layout, as in GridScratch.
struct SweepAux {
    Carver cv, order; const pedp_mesh_s *mesh; int64_t N; bool matrix;   // (matrix: variant 1)
    int64_t n_packets = (N + 63) / 64;
    int n_cwords = (int)((mesh->n_clusters + 63) / 64);
    int64_t max_segs = std::max<int64_t>(16384, (n_packets * mesh->n_clusters + RLIST - 1) / RLIST + n_packets);
    int *flag = cv.take<int>(1);             // origin_check_kernel: non-zero while every origin equals ray 0's
    unsigned *bounds = cv.take<unsigned>(4);  // variant 3: bounds of the rays' octahedral coordinates
    int *seg_info = cv.take<int>(2);          // variant 3: number of segments, segment length
    float *tri3 = cv.take<float>(PAIR_SH * (size_t)(mesh->F_padded / 2));                // shared-origin pair records
    float4 *cones = cv.take<float4>(2 * (size_t)(mesh->n_clusters + mesh->n_super));     // clusters, then super-clusters
    unsigned *hist = cv.take<unsigned>(BIN_CELLS);                                       // direction cells
    unsigned long long *pmask = cv.take<unsigned long long>((size_t)n_packets * (size_t)n_cwords);  // per packet: a bit per cluster
    int *pk_cnt = cv.take<int>((size_t)n_packets);
    int *seg_pk = cv.take<int>((size_t)max_segs);
    int *seg_rank0 = cv.take<int>((size_t)max_segs);
    int *seg_n = cv.take<int>((size_t)max_segs);
    unsigned short *mf_rec = cv.take<unsigned short>(matrix ? 96 * (size_t)mesh->F_padded : 0);  // 3 x 32 bf16 per triangle, in fragment order
    int *stale = order.take<int>(1);          // the order is rebuilt when the ray count or the buffer changes
    float *samples = order.take<float>(3 * RAY_SAMPLES);
    unsigned *perm = order.take<unsigned>((size_t)N);
    SweepAux(char *aux, char *ord, const pedp_mesh_s *m, int64_t n, bool mx) : cv{aux}, order{ord}, mesh(m), N(n), matrix(mx) {}
};

// The origin check, the shared-origin records, the variant's own sweep and, behind it, the general-origin sweep:
// the device flag lets exactly one of the two work.
int cast_shared_origin(pedp_ctx_t c, pedp_mesh_t mesh, const float *d_rays, int64_t N, int variant, unsigned long long *keys) {
    SweepAux a(nullptr, nullptr, mesh, N, variant == 1);   // (counts and sizes; the pointers follow the reserves)
    PEDP_REQUIRE(a.max_segs < (int64_t)1 << 26, "pedp_raycast: problem too large for the segment table");
    PEDP_REQUIRE(mesh->F_padded % 16 == 0, "pedp_raycast: padded triangle count is not a multiple of 16");
    const void *order_before = c->ray_order.ptr;
    int st = c->ray_aux.reserve(a.cv.at);
    if (!st) st = c->ray_order.reserve(a.order.at);
    if (st) return st;
    a = SweepAux((char *)c->ray_aux.ptr, (char *)c->ray_order.ptr, mesh, N, variant == 1);
    const bool order_kept = c->ray_order.ptr == order_before && c->ray_order_n == N;
    PEDP_HIP_CHECK(hipMemsetAsync(a.flag, 0xFF, sizeof(int), c->stream));
    launch(c, origin_check_kernel, 2 * c->num_cus, 256, d_rays, N, a.flag);
    launch(c, pair_shared_kernel, (mesh->F_padded + 255) / 256, 256, mesh->tri, mesh->F_padded, d_rays, a.flag, a.tri3);
    const int64_t ray_blocks = (N + RPL_BLOCK - 1) / RPL_BLOCK;
    const int groups_total = (int)(mesh->F_padded / (2 * RPL_PAIRS));
    const int n_chunks = tri_chunks(c, ray_blocks, groups_total, 512);  // (triangle chunks not below 2k)
    const int gpc = (groups_total + n_chunks - 1) / n_chunks;
    const int64_t grid = ray_blocks * n_chunks;
    PEDP_REQUIRE(grid < (int64_t)0x7FFFFFFF, "pedp_raycast: grid too large");
    PEDP_HIP_CHECK(hipEventRecord(c->ev0, c->stream));
    if (variant == 3) {
        // shared origin: cluster cones, direction binning, culled sweep
        // 0 = "keep the order unless the sampled directions differ", 1 = rebuild (other ray count or buffer)
        PEDP_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)a.stale, order_kept ? 0 : 1, 1, c->stream));
        c->ray_order_n = N;
        launch(c, ray_order_check_kernel, RAY_SAMPLES / 256, 256, d_rays, N, a.samples, a.stale, a.bounds);
        float4 *scones = a.cones + 2 * mesh->n_clusters;
        launch(c, cluster_cone_kernel, (mesh->n_clusters + 255) / 256, 256, (const float4 *)mesh->spheres, mesh->n_clusters, d_rays,
               a.flag, a.cones);
        launch(c, cluster_cone_kernel, (mesh->n_super + 255) / 256, 256, (const float4 *)mesh->super_spheres, mesh->n_super, d_rays,
               a.flag, scones);
        launch(c, ray_bounds_kernel, c->num_cus, 256, d_rays, N, a.stale, a.bounds, a.hist);
        launch(c, ray_count_kernel, (N + 255) / 256, 256, d_rays, N, a.stale, a.bounds, a.hist);
        launch(c, bin_scan_kernel, 1, 1024, a.stale, a.hist);
        launch(c, ray_scatter_kernel, (N + 255) / 256, 256, d_rays, N, a.stale, a.bounds, a.hist, a.perm);
        launch(c, ray_cull_mask_kernel, (a.n_packets + 3) / 4, 256, a.cones, scones, (int)mesh->n_clusters, a.n_cwords, d_rays,
               a.perm, N, a.pmask, a.pk_cnt, a.flag);
        launch(c, ray_segment_kernel, 1, 1024, a.pk_cnt, (int)a.n_packets, a.seg_pk, a.seg_rank0, a.seg_n, (int)a.max_segs,
               a.seg_info, a.flag);
        launch(c, ray_sweep_seg_kernel, (a.max_segs + 3) / 4, RPL_BLOCK, (const f2 *)a.tri3, mesh->tri, a.n_cwords, a.pmask,
               a.seg_pk, a.seg_rank0, a.seg_n, a.seg_info, d_rays, a.perm, N, keys);
    } else if (variant == 5) {   // the packed fp32 loop on the vector pipe
        launch(c, ray_sweep_rpl_kernel<true>, grid, RPL_BLOCK, (const f2 *)a.tri3, mesh->tri, groups_total, gpc, n_chunks, d_rays, N,
               keys, a.flag);
    } else {                     // exhaustive on the matrix pipe: bf16 filter, exact test on the rare branch
        launch(c, mfma_rec_kernel, (mesh->F_padded + 255) / 256, 256, mesh->tri, mesh->F_padded, d_rays, a.flag, a.mf_rec);
        const int tg_total = (int)(mesh->F_padded / 16);
        int mf_chunks = n_chunks;   // (its own count: the general-origin kernel behind keeps n_chunks / gpc / grid)
        if (c->ray_tri_chunks == 0 && mf_chunks < 32 && tg_total / 32 >= 64) mf_chunks = 32;   // (measured: 4.35 ms against 4.54 with 8)
        const int tgpc = (tg_total + mf_chunks - 1) / mf_chunks;
        static const int mf_rg = getenv("PEDP_MF_RG") ? atoi(getenv("PEDP_MF_RG")) : 8;   // (experiments: 8 or 16 ray groups per wave)
        const int64_t mf_rays = 16 * (mf_rg == 16 ? 16 : 8) * MF_WAVES;
        const int64_t mf_grid = ((N + mf_rays - 1) / mf_rays) * mf_chunks;
        PEDP_REQUIRE(mf_grid < (int64_t)0x7FFFFFFF, "pedp_raycast: grid too large");
        launch(c, mf_rg == 16 ? ray_sweep_mfma_kernel<16> : ray_sweep_mfma_kernel<8>, mf_grid, 64 * MF_WAVES, (const uint4 *)a.mf_rec,
               mesh->tri, tg_total, tgpc, mf_chunks, d_rays, N, keys, a.flag);
    }
    launch(c, ray_sweep_rpl_kernel<false>, grid, RPL_BLOCK, (const f2 *)mesh->tri2, mesh->tri, groups_total, gpc, n_chunks, d_rays, N,
           keys, a.flag);
    return PEDP_OK;
}

// ---------------------------------------------------------------- variant 2
int cast_tri_lane(pedp_ctx_t c, pedp_mesh_t mesh, const float *d_rays, int64_t N, unsigned long long *keys) {
    const int64_t rays_per_block = (TPL_BLOCK / 64) * TPL_RAYS;
    const int64_t ray_blocks = (N + rays_per_block - 1) / rays_per_block;
    const int n_chunks = tri_chunks(c, ray_blocks, mesh->F_padded, 1024);
    int tpc = (int)((mesh->F_padded + n_chunks - 1) / n_chunks);
    tpc = ((tpc + 63) / 64) * 64;
    const int64_t grid = ray_blocks * n_chunks;
    PEDP_REQUIRE(grid < (int64_t)0x7FFFFFFF, "pedp_raycast: grid too large");
    PEDP_HIP_CHECK(hipEventRecord(c->ev0, c->stream));
    launch(c, ray_sweep_tpl_kernel, grid, TPL_BLOCK, (const float4 *)mesh->tri, mesh->F_padded, tpc, n_chunks, d_rays, N, keys);
    return PEDP_OK;
}

// ---------------------------------------------------------------- a cast of device rays by a given variant (1 ... 5)
// Leaves c->ray_variant and c->rast_avoid_n alone: the caller has made the choice.
int raycast_device(pedp_ctx_t c, pedp_mesh_t mesh, const float *d_rays, int64_t N, int variant, const RayOut &o) {
    int st = c->ray_keys.reserve(sizeof(unsigned long long) * (size_t)N);
    if (st) return st;
    unsigned long long *keys = (unsigned long long *)c->ray_keys.ptr;
    c->ray_last_variant = variant;
    if (variant == 4) return cast_grid(c, mesh, d_rays, N, keys, o);  // (its first kernel sets the keys)
    PEDP_HIP_CHECK(hipMemsetAsync(keys, 0xFF, sizeof(unsigned long long) * (size_t)N, c->stream));
    st = variant == 2 ? cast_tri_lane(c, mesh, d_rays, N, keys) : cast_shared_origin(c, mesh, d_rays, N, variant, keys);
    if (st) return st;
    PEDP_HIP_CHECK(hipGetLastError());
    PEDP_HIP_CHECK(hipEventRecord(c->ev1, c->stream));
    c->ray_timed = true;
    launch(c, ray_finalize_kernel, (N + 255) / 256, 256, mesh->tri, d_rays, N, keys, o.t, o.id, o.uv, (const RastHdr *)nullptr,
           (RastHdr *)nullptr, (int *)nullptr, (const f2 *)nullptr, 0, 0);
    PEDP_HIP_CHECK(hipGetLastError());
    return PEDP_OK;
}

// a device buffer of a diagnostic entry point, freed on every return path
template <class T> struct DebugBuffer {
    T *p = nullptr;
    hipError_t alloc(size_t count) { return hipMalloc((void **)&p, sizeof(T) * count); }
    ~DebugBuffer() { (void)hipFree(p); }
};

}  // namespace

extern "C" {

// Everything derived from the posed float32 vertices: triangle records, pair records,
// cluster and super-cluster spheres.  Enqueued on the context's stream.
static hipError_t mesh_build_records(pedp_ctx_t c, pedp_mesh_s *m, const float *d_verts, const uint32_t *d_tris) {
    launch(c, tri_setup_kernel, (m->F_padded + 255) / 256, 256, d_verts, d_tris, m->F, m->F_padded, m->tri);
    launch(c, pair_general_kernel, (m->F_padded + 255) / 256, 256, m->tri, m->F_padded, m->tri2);
    launch(c, cluster_sphere_kernel, (m->n_clusters + 255) / 256, 256, m->tri, m->F, m->n_clusters, (float4 *)m->spheres);
    launch(c, supercluster_sphere_kernel, (m->n_super + 3) / 4, 256, (const float4 *)m->spheres, m->n_clusters, m->n_super,
           (float4 *)m->super_spheres);
    return hipGetLastError();
}

// a creation that failed in HIP: the error under the entry point's name, the handle freed
static int mesh_fail(pedp_mesh_s *m, const char *who, hipError_t e) {
    pedp_set_error("%s: %s", who, hipGetErrorString(e));
    pedp_mesh_destroy(m);
    return PEDP_ERR_HIP;
}

// What both creators share: the argument checks, the handle and its device arrays, the indices on their way.
static int mesh_alloc(pedp_ctx_t c, const void *verts, int64_t V, const uint32_t *tris, int64_t F, const char *who,
                      pedp_mesh_t *out, pedp_mesh_s **made) {
    PEDP_REQUIRE(c && out, "%s: null context/output", who);
    *out = nullptr;
    PEDP_REQUIRE((verts || V == 0) && (tris || F == 0), "%s: null arrays", who);
    PEDP_REQUIRE(V >= 0 && F >= 0 && F < (int64_t)0x7FFFFF00, "%s: sizes out of range", who);
    for (int64_t i = 0; i < 3 * F; ++i)
        PEDP_REQUIRE((int64_t)tris[i] < V, "%s: triangle %lld references vertex %u >= V=%lld", who,
                     (long long)(i / 3), tris[i], (long long)V);
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    pedp_mesh_s *m = new (std::nothrow) pedp_mesh_s();
    if (!m) { pedp_set_error("%s: out of host memory", who); return PEDP_ERR_ALLOC; }
    m->ctx = c;
    m->device = c->device;
    m->gen = pedp_next_generation();
    m->V = V;
    m->F = F;
    m->F_padded = ((F + 63) / 64) * 64;
    if (m->F_padded == 0) m->F_padded = 64;
    m->n_clusters = m->F_padded / CL_TRIS;
    m->n_super = (m->n_clusters + 63) / 64;
    hipError_t e = hipMalloc((void **)&m->tri, sizeof(float) * PEDP_TRI_STRIDE * (size_t)m->F_padded);
    if (e == hipSuccess) e = hipMalloc((void **)&m->tri2, sizeof(float) * PAIR_GEN * (size_t)(m->F_padded / 2));
    if (e == hipSuccess) e = hipMalloc((void **)&m->spheres, sizeof(float4) * (size_t)m->n_clusters);
    if (e == hipSuccess) e = hipMalloc((void **)&m->super_spheres, sizeof(float4) * (size_t)m->n_super);
    if (e == hipSuccess) e = hipMalloc((void **)&m->verts32, sizeof(float) * 3 * (size_t)(V ? V : 1));
    if (e == hipSuccess) e = hipMalloc((void **)&m->idx, sizeof(uint32_t) * 3 * (size_t)(F ? F : 1));
    if (e == hipSuccess && F) e = hipMemcpyAsync(m->idx, tris, sizeof(uint32_t) * 3 * (size_t)F, hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) return mesh_fail(m, who, e);
    *made = m;
    return PEDP_OK;
}

int pedp_mesh_create(pedp_ctx_t c, const float *verts, int64_t V, const uint32_t *tris, int64_t F, pedp_mesh_t *out) {
    pedp_mesh_s *m = nullptr;
    int rc = mesh_alloc(c, verts, V, tris, F, "pedp_mesh_create", out, &m);
    if (rc) return rc;
    hipError_t e = hipSuccess;
    if (V) e = hipMemcpyAsync(m->verts32, verts, sizeof(float) * 3 * (size_t)V, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = mesh_build_records(c, m, m->verts32, m->idx);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    // a fixed mesh needs neither the vertices nor the indices again
    (void)hipFree(m->verts32);
    (void)hipFree(m->idx);
    m->verts32 = nullptr;
    m->idx = nullptr;
    if (e != hipSuccess) return mesh_fail(m, "pedp_mesh_create", e);
    *out = m;
    return PEDP_OK;
}

int pedp_mesh_create_posable(pedp_ctx_t c, const double *verts, int64_t V, const uint32_t *tris, int64_t F, pedp_mesh_t *out) {
    pedp_mesh_s *m = nullptr;
    int rc = mesh_alloc(c, verts, V, tris, F, "pedp_mesh_create_posable", out, &m);
    if (rc) return rc;
    hipError_t e = hipMalloc((void **)&m->verts64, sizeof(double) * 3 * (size_t)(V ? V : 1));
    if (e == hipSuccess && V) e = hipMemcpyAsync(m->verts64, verts, sizeof(double) * 3 * (size_t)V, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);  // the caller's arrays are free again
    if (e != hipSuccess) return mesh_fail(m, "pedp_mesh_create_posable", e);
    *out = m;
    return pedp_mesh_set_pose(m, nullptr);
}

int pedp_mesh_set_pose(pedp_mesh_t m, const double T[16]) {
    PEDP_REQUIRE(m, "pedp_mesh_set_pose: null mesh");
    PEDP_REQUIRE(m->verts64, "pedp_mesh_set_pose: mesh was not created with pedp_mesh_create_posable");
    pedp_ctx_t c = m->ctx;
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    Pose16 P;
    for (int k = 0; k < 16; ++k) P.m[k] = T ? T[k] : ((k % 5) == 0 ? 1.0 : 0.0);
    if (m->V) launch(c, pose_verts_kernel, (m->V + 255) / 256, 256, m->verts64, m->V, P, T ? 0 : 1, m->verts32);
    PEDP_HIP_CHECK(hipGetLastError());
    PEDP_HIP_CHECK(mesh_build_records(c, m, m->verts32, m->idx));
    return PEDP_OK;
}

int pedp_mesh_posed_vertices(pedp_mesh_t m, const double T[16], int mem, double *out) {
    PEDP_REQUIRE(m && T && out, "pedp_mesh_posed_vertices: null argument");
    PEDP_REQUIRE(m->verts64, "pedp_mesh_posed_vertices: mesh was not created with pedp_mesh_create_posable");
    PEDP_REQUIRE(mem == PEDP_HOST || mem == PEDP_DEVICE, "pedp_mesh_posed_vertices: bad mem flag %d", mem);
    if (m->V == 0) return PEDP_OK;
    pedp_ctx_t c = m->ctx;
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    Pose16 P;
    for (int k = 0; k < 16; ++k) P.m[k] = T[k];
    double *d_out = out;
    if (mem == PEDP_HOST) {
        int st = c->ray_out.reserve(sizeof(double) * 3 * (size_t)m->V);
        if (st) return st;
        d_out = (double *)c->ray_out.ptr;
    }
    launch(c, pose_verts64_kernel, (m->V + 255) / 256, 256, m->verts64, m->V, P, d_out);
    PEDP_HIP_CHECK(hipGetLastError());
    return mem == PEDP_HOST ? pedp_download(c, out, d_out, sizeof(double) * 3 * (size_t)m->V) : PEDP_OK;
}

void pedp_mesh_destroy(pedp_mesh_t m) {
    if (!m) return;
    // the context may already be gone (Python collects handles in any order): use the ordinal
    // stored at creation; hipFree itself waits for the device's outstanding work
    (void)hipSetDevice(m->device);
    if (m->tri) (void)hipFree(m->tri);
    if (m->tri2) (void)hipFree(m->tri2);
    if (m->spheres) (void)hipFree(m->spheres);
    if (m->super_spheres) (void)hipFree(m->super_spheres);
    if (m->verts64) (void)hipFree(m->verts64);
    if (m->verts32) (void)hipFree(m->verts32);
    if (m->idx) (void)hipFree(m->idx);
    delete m;
}

int pedp_mesh_size(pedp_mesh_t m, int64_t *V, int64_t *F) {
    PEDP_REQUIRE(m, "pedp_mesh_size: null mesh");
    if (V) *V = m->V;
    if (F) *F = m->F;
    return PEDP_OK;
}

int pedp_raycast_configure(pedp_ctx_t c, int tri_chunks, int variant) {
    PEDP_REQUIRE(c, "pedp_raycast_configure: null context");
    PEDP_REQUIRE(tri_chunks >= 0 && tri_chunks % 8 == 0, "pedp_raycast_configure: tri_chunks must be a multiple of 8");
    PEDP_REQUIRE(variant >= 0 && variant <= 5, "pedp_raycast_configure: variant must be 0..5");
    c->ray_tri_chunks = tri_chunks;
    c->ray_variant = variant;
    return PEDP_OK;
}

int pedp_raycast(pedp_ctx_t c, pedp_mesh_t mesh, const float *rays6, int64_t N, int mem,
                 float *t_hit, uint32_t *prim_id, float *uv) {
    PEDP_REQUIRE(c && mesh, "pedp_raycast: null context/mesh");
    PEDP_REQUIRE(mesh->ctx == c, "pedp_raycast: mesh belongs to another context");
    PEDP_REQUIRE(N >= 0 && N < (int64_t)1 << 40, "pedp_raycast: N out of range");
    PEDP_REQUIRE(mem == PEDP_HOST || mem == PEDP_DEVICE, "pedp_raycast: bad mem flag %d", mem);
    if (N == 0) return PEDP_OK;
    PEDP_REQUIRE(rays6 && t_hit && prim_id, "pedp_raycast: null arrays");
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    int variant = c->ray_variant;
    if (variant == 0 && N < 16384) variant = 2;
    if (variant == 0) {
        // the grid of variant 4 unless an earlier cast of this many rays reported that it could not
        // answer them (origins that differ, rays behind the frame's plane, crowded cells, a full item
        // table): such rays would pay the grid's four kernels AND the exhaustive completion in every
        // call, where variant 3's chunked general-origin sweep is several times faster
        volatile int *status = c->rast_status;
        if (status && (status[0] & (1 | 2 | 4 | 8))) c->rast_avoid_n = status[1];
        variant = c->rast_avoid_n == (int)(N & 0x7FFFFFFF) ? 3 : 4;
    }
    const float *d_rays = rays6;
    RayOut o;
    int st = ray_stage(c, mem, N, &d_rays, t_hit, prim_id, uv, &o);
    if (!st) st = raycast_device(c, mesh, d_rays, N, variant, o);
    if (!st) st = ray_out_deliver(c, mem, N, o, t_hit, prim_id, uv);
    return st;
}

// ---------------------------------------------------------------- resident ray sets (include/pedp.h)
struct pedp_rayset_s {
    pedp_ctx_t ctx = nullptr;
    int device = 0;
    int64_t N = 0;
    char *buf = nullptr;        // one allocation: rays, keys, the grid's scratch
    float *rays = nullptr;
    unsigned long long *keys = nullptr;
    GridScratch grid;
    int *status = nullptr;      // pinned: [0] why the grid failed in the last cast (0: it did not), [1] ray count
    unsigned seq = 0;           // casts enqueued: picks one of the two headers
    bool grid_ok = false;       // the build found the rays servable; cleared for good by a cast that was not answered by the grid
    int last_variant = 0, last_status = 0;
    uint64_t id = 0;            // process-wide, never reused: names the set in the all-hits queries' status words
    bool hits_avoid = false;    // an all-hits query's grid pass gave up on these rays: the exhaustive path from now on (auto only)
};

// the set's one allocation; base == nullptr: its size only
static size_t rayset_carve(pedp_rayset_s *r, char *base) {
    Carver cv{base};
    r->rays = cv.take<float>(6 * (size_t)r->N);
    r->keys = cv.take<unsigned long long>((size_t)r->N);
    r->grid = GridScratch(base ? base + cv.at : nullptr, r->N);
    return cv.at + r->grid.cv.at;
}

int pedp_rayset_create(pedp_ctx_t c, const float *rays6, int64_t N, int mem, pedp_rayset_t *out) {
    PEDP_REQUIRE(c && out, "pedp_rayset_create: null context/output");
    *out = nullptr;
    PEDP_REQUIRE(N > 0 && N < (int64_t)0x7FFFFFF0, "pedp_rayset_create: N out of range");
    PEDP_REQUIRE(rays6, "pedp_rayset_create: null rays");
    PEDP_REQUIRE(mem == PEDP_HOST || mem == PEDP_DEVICE, "pedp_rayset_create: bad mem flag %d", mem);
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    pedp_rayset_s *r = new (std::nothrow) pedp_rayset_s();
    if (!r) { pedp_set_error("pedp_rayset_create: out of host memory"); return PEDP_ERR_ALLOC; }
    r->ctx = c; r->device = c->device; r->N = N; r->id = pedp_next_generation();
    hipError_t e = hipMalloc((void **)&r->buf, rayset_carve(r, nullptr));
    if (e == hipSuccess) e = hipHostMalloc((void **)&r->status, 64, hipHostMallocMapped);
    if (e != hipSuccess) { pedp_set_error("pedp_rayset_create: %s", hipGetErrorString(e)); pedp_rayset_destroy(r); return PEDP_ERR_ALLOC; }
    r->status[0] = 0; r->status[1] = -1;
    rayset_carve(r, r->buf);
    RastHdr *h0 = r->grid.hdr[0];
    int rc = PEDP_OK;
    if (mem == PEDP_HOST) rc = pedp_upload(c, r->rays, rays6, sizeof(float) * 6 * (size_t)N);
    else e = hipMemcpyAsync(r->rays, rays6, sizeof(float) * 6 * (size_t)N, hipMemcpyDeviceToDevice, c->stream);
    if (rc == PEDP_OK && e == hipSuccess) e = hipMemcpyAsync(h0, &RAST_HDR_START, sizeof(RastHdr), hipMemcpyHostToDevice, c->stream);
    if (rc == PEDP_OK && e == hipSuccess) {
        grid_enqueue_build(c, r->rays, N, r->grid, h0, r->keys);  // what pedp_raycast's variant 4 builds per call
        e = hipGetLastError();
    }
    RastHdr hb;
    if (rc == PEDP_OK && e == hipSuccess) e = hipMemcpyAsync(&hb, h0, sizeof(hb), hipMemcpyDeviceToHost, c->stream);
    if (rc == PEDP_OK && e == hipSuccess) e = hipStreamSynchronize(c->stream);   // (also: the caller's array is free again)
    if (rc != PEDP_OK || e != hipSuccess) {
        if (rc == PEDP_OK) pedp_set_error("pedp_rayset_create: %s", hipGetErrorString(e));
        pedp_rayset_destroy(r);
        return rc != PEDP_OK ? rc : PEDP_ERR_HIP;
    }
    r->grid_ok = hb.ok != 0;
    r->last_status = hb.ok ? 0 : hb.reason;
    if (r->grid_ok) {  // the second header: the same frame and grid, its counters at their start values
        e = hipMemcpyAsync(r->grid.hdr[1], h0, sizeof(RastHdr), hipMemcpyDeviceToDevice, c->stream);
        if (e != hipSuccess) { pedp_set_error("pedp_rayset_create: %s", hipGetErrorString(e)); pedp_rayset_destroy(r); return PEDP_ERR_HIP; }
    }
    *out = r;
    return PEDP_OK;
}

void pedp_rayset_destroy(pedp_rayset_t r) {
    if (!r) return;
    (void)hipSetDevice(r->device);
    if (r->buf) (void)hipFree(r->buf);
    if (r->status) (void)hipHostFree(r->status);
    delete r;
}

int pedp_raycast_rayset(pedp_ctx_t c, pedp_mesh_t mesh, pedp_rayset_t r, int mem, float *t_hit, uint32_t *prim_id, float *uv) {
    PEDP_REQUIRE(c && mesh && r, "pedp_raycast_rayset: null argument");
    PEDP_REQUIRE(mesh->ctx == c && r->ctx == c, "pedp_raycast_rayset: mesh or ray set belongs to another context");
    PEDP_REQUIRE(mem == PEDP_HOST || mem == PEDP_DEVICE, "pedp_raycast_rayset: bad mem flag %d", mem);
    PEDP_REQUIRE(t_hit && prim_id, "pedp_raycast_rayset: null arrays");
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    const int64_t N = r->N;
    // a cast the grid did not answer (its last kernel completed it exhaustively, correctly but slowly): from now on the
    // other variants, from the resident copy
    if (r->grid_ok && ((volatile int *)r->status)[1] == (int)(N & 0x7FFFFFFF) && ((volatile int *)r->status)[0] != 0) {
        r->grid_ok = false;
        r->last_status = ((volatile int *)r->status)[0];
    }
    RayOut o;
    int st = ray_stage(c, mem, N, nullptr, t_hit, prim_id, uv, &o);
    if (st) return st;
    if (!r->grid_ok || mesh->F >= (int64_t)0x7FFFFFF0) {
        // (differing origins: variant 3 takes the general sweep on the device)
        const int configured = c->ray_variant;
        st = raycast_device(c, mesh, r->rays, N, (configured == 0 || configured == 4) ? 3 : configured, o);
        r->last_variant = c->ray_last_variant;
    } else {
        PEDP_HIP_CHECK(hipEventRecord(c->ev0, c->stream));
        // reset_keys: a ray set's keys start the next cast clean (nothing else clears them)
        st = grid_enqueue_cast(c, mesh, r->rays, N, r->grid, r->seq, r->keys, r->status, o, 1);
        if (st) return st;
        r->seq += 1;
        r->last_variant = 4;
        c->ray_last_variant = 4;
    }
    if (!st) st = ray_out_deliver(c, mem, N, o, t_hit, prim_id, uv);
    return st;
}

int pedp_rayset_last_variant(pedp_rayset_t r, int *variant, int *grid_status) {
    PEDP_REQUIRE(r && variant && grid_status, "pedp_rayset_last_variant: null argument");
    PEDP_HIP_CHECK(hipSetDevice(r->device));
    PEDP_HIP_CHECK(hipStreamSynchronize(r->ctx->stream));
    *variant = r->last_variant;
    *grid_status = r->last_variant == 4 ? ((volatile int *)r->status)[0] : r->last_status;
    return PEDP_OK;
}

int pedp_raycast_last_variant(pedp_ctx_t c, int *variant, int *grid_status) {
    PEDP_REQUIRE(c && variant && grid_status, "pedp_raycast_last_variant: null argument");
    PEDP_REQUIRE(c->ray_last_variant > 0, "pedp_raycast_last_variant: no cast has run on this context");
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    PEDP_HIP_CHECK(hipStreamSynchronize(c->stream));
    *variant = c->ray_last_variant;
    *grid_status = (c->ray_last_variant == 4 && c->rast_status) ? ((volatile int *)c->rast_status)[0] : 0;
    return PEDP_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- all-hits queries (ray/all_hits.h, DESIGN s4.24)
namespace {

constexpr int HITS_PATH_GRID = 4, HITS_PATH_EXHAUSTIVE = 1;   // pedp_intersections_last_path

// The rays of a query, checked: device rows (a call's own, uploaded in host mode, or a ray set's resident copy).
struct HitsRays { const float *d; int64_t N; pedp_rayset_s *set; };
int hits_rays(pedp_ctx_t c, pedp_mesh_t mesh, const float *rays6, int64_t N, pedp_rayset_t set, bool by_set, int mem, const char *who,
              HitsRays *out) {
    PEDP_REQUIRE(c && mesh && (!by_set || set), "%s: null context / mesh / ray set", who);
    PEDP_REQUIRE(mesh->ctx == c && (!by_set || set->ctx == c), "%s: mesh or ray set belongs to another context", who);
    PEDP_REQUIRE(mem == PEDP_HOST || mem == PEDP_DEVICE, "%s: bad mem flag %d", who, mem);
    if (by_set) N = set->N;
    PEDP_REQUIRE(N >= 0 && N < (int64_t)0x7FFFFFF0, "%s: N out of range", who);
    PEDP_REQUIRE(mesh->F > 0 && mesh->F < (int64_t)0x7FFFFFF0, "%s: the mesh has no triangles (or 2^31 and more)", who);
    PEDP_REQUIRE(by_set || rays6 || N == 0, "%s: null rays", who);
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    *out = HitsRays{by_set ? set->rays : rays6, N, by_set ? set : nullptr};
    if (!by_set && mem == PEDP_HOST && N > 0) {
        PEDP_TRY(c->ray_in.reserve(sizeof(float) * 6 * (size_t)N));
        PEDP_TRY(pedp_upload(c, c->ray_in.ptr, rays6, sizeof(float) * 6 * (size_t)N));
        out->d = (const float *)c->ray_in.ptr;
    }
    return PEDP_OK;
}

// Path choice: pedp_raycast_configure's variant.  0: the grid from 16,384 rays on and for a ray set, unless an earlier
// query's grid pass gave up on these rays (read from the status words without waiting: at worst the news comes a call
// late); 4: the grid; others: every ray against every triangle.  A ray set whose grid cannot serve it has no grid to use.
bool hits_use_grid(pedp_ctx_t c, const HitsRays &r) {
    const int variant = c->ray_variant;
    volatile int *st = c->hits_status;
    if (st && st[0] != 0) {
        const uint64_t owner = (uint64_t)(unsigned)st[2] | ((uint64_t)(unsigned)st[3] << 32);
        if (owner == 0) c->hits_avoid_n = st[1];
        else if (r.set && r.set->id == owner) r.set->hits_avoid = true;
    }
    if (r.set) {
        volatile int *cs = r.set->status;   // (a cast the grid did not answer: pedp_raycast_rayset retires the grid at its next call)
        const bool cast_gave_up = cs[1] == (int)(r.N & 0x7FFFFFFF) && cs[0] != 0;
        if (!r.set->grid_ok || cast_gave_up) return false;
        return variant == 4 || (variant == 0 && !r.set->hits_avoid);
    }
    return variant == 4 || (variant == 0 && r.N >= 16384 && c->hits_avoid_n != (int)(r.N & 0x7FFFFFFF));
}

// One pass over the rays: every pair that mt_accept accepts reaches `sink` exactly once.  The sink's words are zero
// before it.  With the grid: the casts' three kernels, then ah_close_kernel (status; the next header; where the grid
// gave up, the words back to zero), then ah_sweep_kernel, which returns at once unless the grid gave up -- the
// decision stays on the device.  Without: ah_sweep_kernel alone.  The grid's scratch is the context's (built here, as
// cast_grid does, the casts' header protocol kept) or the ray set's (built at creation; its keys are not touched).
template <class Sink>
int hits_pass(pedp_ctx_t c, pedp_mesh_t mesh, const HitsRays &r, bool use_grid, Sink sink) {
    const int64_t N = r.N;
    const RastHdr *h_walked = nullptr;
    if (use_grid) {
        if (!c->hits_status) {
            PEDP_HIP_CHECK(hipHostMalloc((void **)&c->hits_status, 64, hipHostMallocMapped));
            memset(c->hits_status, 0, 64);
            c->hits_status[1] = -1;
        }
        int *d_status = nullptr;
        PEDP_HIP_CHECK(hipHostGetDevicePointer((void **)&d_status, c->hits_status, 0));
        GridScratch g;
        unsigned seq;
        if (r.set) {
            g = r.set->grid;
            seq = r.set->seq;
        } else {
            PEDP_TRY(c->ray_keys.reserve(sizeof(unsigned long long) * (size_t)N));
            PEDP_TRY(c->ray_rast.reserve(GridScratch::bytes(N)));
            char *base = (char *)c->ray_rast.ptr;
            g = GridScratch(base, N);
            seq = c->rast_seq;
            if (c->rast_hdr_ready != (void *)base) {  // new buffer, or a pass that did not reach its last kernel
                PEDP_HIP_CHECK(hipMemcpyAsync(g.hdr[seq & 1], &RAST_HDR_START, sizeof(RastHdr), hipMemcpyHostToDevice, c->stream));
                PEDP_HIP_CHECK(hipStreamSynchronize(c->stream));
            }
            c->rast_hdr_ready = nullptr;
            grid_enqueue_build(c, r.d, N, g, g.hdr[seq & 1], (unsigned long long *)c->ray_keys.ptr);
        }
        RastHdr *h = g.hdr[seq & 1], *h_next = g.hdr[(seq + 1) & 1];
        grid_enqueue_walk(c, mesh, r.d, N, g, h, sink);
        launch(c, ah_close_kernel<Sink>, (N + 255) / 256, 256, N, (const RastHdr *)h, h_next, d_status,
               (unsigned long long)(r.set ? r.set->id : 0), sink);
        PEDP_HIP_CHECK(hipGetLastError());
        if (r.set) r.set->seq += 1;
        else { c->rast_hdr_ready = c->ray_rast.ptr; c->rast_seq += 1; }
        h_walked = h;
    }
    // triangle chunks: enough workgroups for four rounds over the chip, no chunk below 256 triangles
    const int64_t ray_blocks = (N + 255) / 256;
    int64_t n_chunks = 1;
    while (ray_blocks * n_chunks < 4 * (int64_t)c->num_cus && mesh->F / (n_chunks * 2) >= 256 && n_chunks < 32768) n_chunks *= 2;
    const int64_t per_chunk = (mesh->F + n_chunks - 1) / n_chunks;
    hipLaunchKernelGGL(ah_sweep_kernel<Sink>, dim3((unsigned)ray_blocks, (unsigned)n_chunks), dim3(256), 0, c->stream, (const float *)mesh->tri,
                       mesh->F, per_chunk, r.d, N, h_walked, sink);
    PEDP_HIP_CHECK(hipGetLastError());
    return PEDP_OK;
}

// count_intersections / test_occlusions: one word per ray, zeroed, one pass, delivered.  T: int32_t with HitCount,
// uint8_t with HitInRange (make: the sink over the device words).
template <class T, class Make>
int hits_per_ray(pedp_ctx_t c, pedp_mesh_t mesh, const HitsRays &r, int mem, T *out, const char *who, Make make) {
    if (r.N == 0) return PEDP_OK;
    PEDP_REQUIRE(out, "%s: null output", who);
    T *d_out = out;
    if (mem == PEDP_HOST) {
        PEDP_TRY(c->hits_io.reserve(sizeof(T) * (size_t)r.N));
        d_out = (T *)c->hits_io.ptr;
    }
    PEDP_HIP_CHECK(hipMemsetAsync(d_out, 0, sizeof(T) * (size_t)r.N, c->stream));
    const bool use_grid = hits_use_grid(c, r);
    c->hits_last_path = use_grid ? HITS_PATH_GRID : HITS_PATH_EXHAUSTIVE;
    PEDP_TRY(hits_pass(c, mesh, r, use_grid, make(d_out)));
    return mem == PEDP_HOST ? pedp_download(c, out, d_out, sizeof(T) * (size_t)r.N) : PEDP_OK;
}

// What a list works in besides its keys (member order is layout, as in GridScratch).
struct HitsListScratch {
    Carver cv; int64_t N; size_t scan_bytes;
    int *counts = cv.take<int>((size_t)N + 1);            // (the last one stays zero: the scan runs over N + 1)
    int *cursor = cv.take<int>((size_t)N);
    long long *splits = cv.take<long long>((size_t)N + 1);
    char *scan_tmp = cv.take<char>(scan_bytes);
    HitsListScratch(char *base, int64_t N, size_t scan_bytes) : cv{base}, N(N), scan_bytes(scan_bytes) {}
};
struct HitsKeys {   // a list's M keys as the fill pass leaves them and sorted, and the sort's scratch
    Carver cv; int64_t M; size_t sort_bytes;
    unsigned long long *arrived = cv.take<unsigned long long>((size_t)M);
    unsigned long long *sorted = cv.take<unsigned long long>((size_t)M);
    char *sort_tmp = cv.take<char>(sort_bytes);
    HitsKeys(char *base, int64_t M, size_t sort_bytes) : cv{base}, M(M), sort_bytes(sort_bytes) {}
};
struct HitsOut {    // a host-memory list's outputs on the device
    Carver cv; int64_t M;
    long long *ray_ids = cv.take<long long>((size_t)M);
    float *t = cv.take<float>((size_t)M);
    uint32_t *prim = cv.take<uint32_t>((size_t)M);
    float *uv = cv.take<float>(2 * (size_t)M);
    HitsOut(char *base, int64_t M) : cv{base}, M(M) {}
};

// list_intersections: count pass, exclusive scan (ray_splits and M), fill pass, a segmented radix sort of the keys
// over ray_splits (rocPRIM: linear in a segment's length), the outputs from the sorted keys.  One host wait, which M
// needs; the count pass's grid status comes with it and picks the fill pass's path.  Both passes hand the sink the
// pairs mt_accept accepts, each once, whatever the path: the same set (DESIGN s4.24).
int hits_list(pedp_ctx_t c, pedp_mesh_t mesh, const HitsRays &r, int mem, int64_t capacity, int64_t *ray_splits, int64_t *ray_ids,
              float *t_hit, uint32_t *prim_id, float *uv, int64_t *total, const char *who) {
    PEDP_REQUIRE(total && ray_splits && capacity >= 0, "%s: null ray_splits / total, or a negative capacity", who);
    PEDP_REQUIRE(capacity == 0 || (ray_ids && t_hit && prim_id && uv), "%s: null output arrays", who);
    const int64_t N = r.N;
    *total = 0;
    size_t scan_bytes = 0;
    PEDP_HIP_CHECK(rocprim::exclusive_scan(nullptr, scan_bytes, (int *)nullptr, (long long *)nullptr, 0ll, (size_t)N + 1,
                                           rocprim::plus<long long>(), c->stream));
    PEDP_TRY(c->hits_ws.reserve(HitsListScratch(nullptr, N, scan_bytes).cv.at));
    const HitsListScratch w((char *)c->hits_ws.ptr, N, scan_bytes);
    long long *splits = mem == PEDP_DEVICE ? (long long *)ray_splits : w.splits;
    PEDP_HIP_CHECK(hipMemsetAsync(w.counts, 0, sizeof(int) * ((size_t)N + 1), c->stream));
    if (N > 0) PEDP_HIP_CHECK(hipMemsetAsync(w.cursor, 0, sizeof(int) * (size_t)N, c->stream));
    bool use_grid = N > 0 && hits_use_grid(c, r);
    if (N > 0) {
        c->hits_last_path = use_grid ? HITS_PATH_GRID : HITS_PATH_EXHAUSTIVE;
        PEDP_TRY(hits_pass(c, mesh, r, use_grid, HitCount{w.counts}));
    }
    size_t tmp = scan_bytes;   // rocprim takes it by reference
    PEDP_HIP_CHECK(rocprim::exclusive_scan(w.scan_tmp, tmp, w.counts, splits, 0ll, (size_t)N + 1, rocprim::plus<long long>(), c->stream));
    long long *h_total = pedp_pinned_at<long long>(c, pedp_pinned::COUNTERS);
    PEDP_HIP_CHECK(hipMemcpyAsync(h_total, splits + N, sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    PEDP_HIP_CHECK(hipStreamSynchronize(c->stream));
    const int64_t M = *h_total;
    if (use_grid && ((volatile int *)c->hits_status)[0] != 0) use_grid = false;   // the grid gave up: the fill pass need not ask it again
    *total = M;
    if (mem == PEDP_HOST) PEDP_TRY(pedp_download(c, ray_splits, splits, sizeof(long long) * ((size_t)N + 1)));
    PEDP_REQUIRE(M <= capacity, "%s: %lld intersections, room for %lld", who, (long long)M, (long long)capacity);
    if (M == 0) return PEDP_OK;
    PEDP_REQUIRE(M < (int64_t)0x7FFFFFF0, "%s: 2^31 intersections and more", who);
    size_t sort_bytes = 0;
    PEDP_HIP_CHECK(rocprim::segmented_radix_sort_keys(nullptr, sort_bytes, (unsigned long long *)nullptr, (unsigned long long *)nullptr,
                                                      (unsigned)M, (unsigned)N, (const long long *)nullptr, (const long long *)nullptr, 0, 64,
                                                      c->stream));
    PEDP_TRY(c->hits_keys.reserve(HitsKeys(nullptr, M, sort_bytes).cv.at));
    const HitsKeys k((char *)c->hits_keys.ptr, M, sort_bytes);
    PEDP_TRY(hits_pass(c, mesh, r, use_grid, HitFill{splits, w.cursor, k.arrived}));
    PEDP_HIP_CHECK(rocprim::segmented_radix_sort_keys(k.sort_tmp, sort_bytes, k.arrived, k.sorted, (unsigned)M, (unsigned)N,
                                                      (const long long *)splits, (const long long *)splits + 1, 0, 64, c->stream));
    HitsOut o(nullptr, M);
    if (mem == PEDP_HOST) {
        PEDP_TRY(c->hits_io.reserve(o.cv.at));
        o = HitsOut((char *)c->hits_io.ptr, M);
    } else {
        o.ray_ids = (long long *)ray_ids; o.t = t_hit; o.prim = prim_id; o.uv = uv;
    }
    launch(c, ah_emit_kernel, (M + 255) / 256, 256, (const float *)mesh->tri, mesh->F, r.d, N, (const long long *)splits,
           (const unsigned long long *)k.sorted, M, o.ray_ids, o.t, o.prim, o.uv);
    PEDP_HIP_CHECK(hipGetLastError());
    if (mem == PEDP_HOST) {
        PEDP_TRY(pedp_download(c, ray_ids, o.ray_ids, sizeof(long long) * (size_t)M));
        PEDP_TRY(pedp_download(c, t_hit, o.t, sizeof(float) * (size_t)M));
        PEDP_TRY(pedp_download(c, prim_id, o.prim, sizeof(uint32_t) * (size_t)M));
        PEDP_TRY(pedp_download(c, uv, o.uv, sizeof(float) * 2 * (size_t)M));
    }
    return PEDP_OK;
}

}  // namespace

extern "C" {

int pedp_count_intersections(pedp_ctx_t c, pedp_mesh_t mesh, const float *rays6, int64_t N, int mem, int32_t *counts) {
    HitsRays r;
    PEDP_TRY(hits_rays(c, mesh, rays6, N, nullptr, false, mem, "pedp_count_intersections", &r));
    return hits_per_ray(c, mesh, r, mem, counts, "pedp_count_intersections", [](int32_t *d) { return HitCount{d}; });
}

int pedp_count_intersections_rayset(pedp_ctx_t c, pedp_mesh_t mesh, pedp_rayset_t rays, int mem, int32_t *counts) {
    HitsRays r;
    PEDP_TRY(hits_rays(c, mesh, nullptr, 0, rays, true, mem, "pedp_count_intersections_rayset", &r));
    return hits_per_ray(c, mesh, r, mem, counts, "pedp_count_intersections_rayset", [](int32_t *d) { return HitCount{d}; });
}

int pedp_test_occlusions(pedp_ctx_t c, pedp_mesh_t mesh, const float *rays6, int64_t N, int mem, float tnear, float tfar, uint8_t *occluded) {
    HitsRays r;
    PEDP_TRY(hits_rays(c, mesh, rays6, N, nullptr, false, mem, "pedp_test_occlusions", &r));
    return hits_per_ray(c, mesh, r, mem, occluded, "pedp_test_occlusions", [=](uint8_t *d) { return HitInRange{d, tnear, tfar}; });
}

int pedp_test_occlusions_rayset(pedp_ctx_t c, pedp_mesh_t mesh, pedp_rayset_t rays, int mem, float tnear, float tfar, uint8_t *occluded) {
    HitsRays r;
    PEDP_TRY(hits_rays(c, mesh, nullptr, 0, rays, true, mem, "pedp_test_occlusions_rayset", &r));
    return hits_per_ray(c, mesh, r, mem, occluded, "pedp_test_occlusions_rayset", [=](uint8_t *d) { return HitInRange{d, tnear, tfar}; });
}

int pedp_list_intersections(pedp_ctx_t c, pedp_mesh_t mesh, const float *rays6, int64_t N, int mem, int64_t capacity, int64_t *ray_splits,
                            int64_t *ray_ids, float *t_hit, uint32_t *prim_ids, float *uvs, int64_t *total) {
    HitsRays r;
    PEDP_TRY(hits_rays(c, mesh, rays6, N, nullptr, false, mem, "pedp_list_intersections", &r));
    return hits_list(c, mesh, r, mem, capacity, ray_splits, ray_ids, t_hit, prim_ids, uvs, total, "pedp_list_intersections");
}

int pedp_list_intersections_rayset(pedp_ctx_t c, pedp_mesh_t mesh, pedp_rayset_t rays, int mem, int64_t capacity, int64_t *ray_splits,
                                   int64_t *ray_ids, float *t_hit, uint32_t *prim_ids, float *uvs, int64_t *total) {
    HitsRays r;
    PEDP_TRY(hits_rays(c, mesh, nullptr, 0, rays, true, mem, "pedp_list_intersections_rayset", &r));
    return hits_list(c, mesh, r, mem, capacity, ray_splits, ray_ids, t_hit, prim_ids, uvs, total, "pedp_list_intersections_rayset");
}

int pedp_intersections_last_path(pedp_ctx_t c, int *path, int *grid_status) {
    PEDP_REQUIRE(c && path && grid_status, "pedp_intersections_last_path: null argument");
    PEDP_REQUIRE(c->hits_last_path > 0, "pedp_intersections_last_path: no all-hits query has run on this context");
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    PEDP_HIP_CHECK(hipStreamSynchronize(c->stream));
    *path = c->hits_last_path;
    *grid_status = (c->hits_last_path == HITS_PATH_GRID && c->hits_status) ? ((volatile int *)c->hits_status)[0] : 0;
    return PEDP_OK;
}

/* Diagnostics of the triangle-driven ray stage (tests/test_ray_gpu.py::test_grid_margin_*): run a variant-4 cast
 * of the N host rays and return, for every triangle, [live, every-cell, fx0, fx1, fy0, fy1 (the bounding rectangle of
 * its mapped corners in cell units, before widening), mx, my (the margins), x0, x1, y0, y1 (the cells visited)] and,
 * for every ray, [kind (1: mapped), cell coordinate x, y (continuous)]; grid[0..1] = GX, GY, grid[2] = status.
 * The cast is the device part of a host-memory pedp_raycast: its results stay in c->ray_out, neither downloaded nor
 * waited for, and the diagnostic kernels follow it on the stream. */
int pedp_debug_rast_rects(pedp_ctx_t c, pedp_mesh_t mesh, const float *rays6, int64_t N, float *tri_out, float *ray_out, int *grid) {
    PEDP_REQUIRE(c && mesh && rays6 && tri_out && ray_out && grid && N > 0, "pedp_debug_rast_rects: bad argument");
    PEDP_REQUIRE(mesh->ctx == c, "pedp_debug_rast_rects: mesh belongs to another context");
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    const float *d_rays = rays6;
    RayOut o;
    int st = ray_stage(c, PEDP_HOST, N, &d_rays, nullptr, nullptr, nullptr, &o);
    if (!st) st = raycast_device(c, mesh, d_rays, N, 4, o);
    if (st) return st;
    // the header the cast used (the finalize kernel reset the OTHER one) and the rays it uploaded are still in place
    const RastHdr *h = GridScratch((char *)c->ray_rast.ptr, N).hdr[(c->rast_seq + 1) & 1];
    DebugBuffer<float> d_tri, d_ray;
    PEDP_HIP_CHECK(d_tri.alloc(12 * (size_t)(mesh->F > 0 ? mesh->F : 1)));
    PEDP_HIP_CHECK(d_ray.alloc(3 * (size_t)N));
    if (mesh->F > 0) launch(c, rast_debug_tri_kernel, (mesh->F + 255) / 256, 256, mesh->tri, mesh->F, h, d_tri.p);
    launch(c, rast_debug_ray_kernel, (N + 255) / 256, 256, d_rays, N, h, d_ray.p);
    RastHdr hh;
    PEDP_HIP_CHECK(hipMemcpyAsync(tri_out, d_tri.p, sizeof(float) * 12 * (size_t)mesh->F, hipMemcpyDeviceToHost, c->stream));
    PEDP_HIP_CHECK(hipMemcpyAsync(ray_out, d_ray.p, sizeof(float) * 3 * (size_t)N, hipMemcpyDeviceToHost, c->stream));
    PEDP_HIP_CHECK(hipMemcpyAsync(&hh, h, sizeof(hh), hipMemcpyDeviceToHost, c->stream));
    PEDP_HIP_CHECK(hipStreamSynchronize(c->stream));
    grid[0] = hh.GX; grid[1] = hh.GY; grid[2] = c->rast_status ? c->rast_status[0] : -1;
    return PEDP_OK;
}

/* Diagnostics of the matrix-pipe filter of the exhaustive sweep: for N host rays of ONE origin the filter's score of every
 * (ray, triangle) pair (>= 0: the pair goes to the exact test) and the slack inside it, N x F float32 each, row-major. */
int pedp_debug_mfma_scores(pedp_ctx_t c, pedp_mesh_t mesh, const float *rays6, int64_t N, float *score, float *slack) {
    PEDP_REQUIRE(c && mesh && rays6 && score && slack && N > 0 && mesh->F > 0, "pedp_debug_mfma_scores: bad argument");
    PEDP_REQUIRE(mesh->ctx == c && N * mesh->F <= ((int64_t)1 << 27), "pedp_debug_mfma_scores: foreign mesh, or more than 2^27 pairs");
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    DebugBuffer<float> d_rays, d_sc, d_sl;
    DebugBuffer<unsigned short> d_rec;
    DebugBuffer<int> d_flag;
    const size_t pairs = (size_t)N * (size_t)mesh->F;
    PEDP_HIP_CHECK(d_rays.alloc(6 * (size_t)N));
    PEDP_HIP_CHECK(d_sc.alloc(pairs));
    PEDP_HIP_CHECK(d_sl.alloc(pairs));
    PEDP_HIP_CHECK(d_rec.alloc(96 * (size_t)mesh->F_padded));
    PEDP_HIP_CHECK(d_flag.alloc(1));
    PEDP_HIP_CHECK(hipMemcpyAsync(d_rays.p, rays6, sizeof(float) * 6 * (size_t)N, hipMemcpyHostToDevice, c->stream));
    PEDP_HIP_CHECK(hipMemsetAsync(d_flag.p, 0xFF, sizeof(int), c->stream));
    launch(c, mfma_rec_kernel, (mesh->F_padded + 255) / 256, 256, mesh->tri, mesh->F_padded, d_rays.p, d_flag.p, d_rec.p);
    launch(c, mfma_debug_kernel, (N + 15) / 16, 64, (const uint4 *)d_rec.p, (int)(mesh->F_padded / 16), d_rays.p, N, mesh->F,
           d_sc.p, d_sl.p);
    PEDP_HIP_CHECK(hipGetLastError());
    PEDP_HIP_CHECK(hipMemcpyAsync(score, d_sc.p, sizeof(float) * pairs, hipMemcpyDeviceToHost, c->stream));
    PEDP_HIP_CHECK(hipMemcpyAsync(slack, d_sl.p, sizeof(float) * pairs, hipMemcpyDeviceToHost, c->stream));
    PEDP_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PEDP_OK;
}

int pedp_raycast_last_sweep_ms(pedp_ctx_t c, float *ms) {
    PEDP_REQUIRE(c && ms, "pedp_raycast_last_sweep_ms: null argument");
    PEDP_REQUIRE(c->ray_timed, "pedp_raycast_last_sweep_ms: no sweep has run on this context");
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    PEDP_HIP_CHECK(hipEventSynchronize(c->ev1));
    PEDP_HIP_CHECK(hipEventElapsedTime(ms, c->ev0, c->ev1));
    return PEDP_OK;
}

}  // extern "C"
