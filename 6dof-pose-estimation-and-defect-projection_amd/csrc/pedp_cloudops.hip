// Point-cloud operations for gfx950: the Open3D calls the reference chains in src/pose_estimation.py:186-378, restated
// from the published open3d==0.18.0 algorithms (oracle/cloudops.c and oracle/features.c are the CPU statements the tests
// compare with).  This file is the host side -- box and grid set-up, the device-to-device cores, the C entry points and
// preprocess_source's chain; the kernels are in cloud/*.h, one stage per header, all in this one translation unit.
//
//   entry point                                Open3D / reference                         kernels
//   pedp_voxel_down_sample[_device_in]         voxel_down_sample                          cloud/voxel.h
//   pedp_cluster_dbscan                        cluster_dbscan                             cloud/grid.h, cloud/dbscan.h
//   pedp_knn_mean_distance                     per-point part of remove_statistical_outlier   cloud/knn.h
//   pedp_estimate_normals                      estimate_normals (hybrid search)           cloud/normals.h
//   pedp_fpfh, pedp_feature_match              compute_fpfh_feature, feature kNN          cloud/fpfh.h
//   pedp_segment_plane                         segment_plane                              cloud/plane.h
//   pedp_preprocess_source[_ex]                the whole chain on the device, with        cloud/average_normal.h,
//                                              compute_average_normal and the cuts        cloud/select.h, cloud/bounds.h
//   pedp_sort_keys64_[exact_]{begin,run}       the stable 64-bit key sort other sources use (cloud/common.h: RadixPasses)
//
// Everything with an order-dependent result is made order-free or given the oracle's order, and each is settled where
// its kernel is:
//   * voxel averages (voxel.h): points are sorted by voxel key with a STABLE sort (sort_pairs_u64 below), so a voxel's
//     members are summed in point order like Open3D's sequential accumulation;
//   * the uniform grid (grid.h): built by counting, the order inside a cell is the hardware's -- every reader is
//     indifferent to it (counts, minima, sets, lists in explicit (distance, index) order);
//   * DBSCAN (dbscan.h): clusters are the connected components of the core points (lock-free union-find, smaller index
//     wins); cluster ids rank the representatives -- Open3D's discovery order -- and a border point takes the smallest
//     id among its core neighbours;
//   * k nearest neighbours (knn.h): the k smallest squared distances are summed as roots in ascending order;
//   * normals and FPFH (normals.h, fpfh.h, grid.h: hybrid_collect): neighbours in (d^2, index) order;
//   * plane RANSAC (plane.h): integer inlier counts per iteration, the best iteration -- most inliers, the earliest on
//     ties -- chosen on the device, the refit summed in fixed blocks of 256 points on the device (preprocess_source)
//     and, in the same order, on the host (pedp_segment_plane: plane_from_points);
//   * the average normal (average_normal.h): a voxel's members added in ascending point index, the voxels' means added
//     row by row on the host (mean_of_rows below) after the stream's next wait;
//   * selections (select.h): flags -> exclusive scan -> scatter, index order.
#include "pedp_internal.h"
#include <cmath>
#include <cstddef>
#include <cstring>
#include <type_traits>
#include <vector>
#include "cloud/common.h"
#include "cloud/grid.h"
#include "cloud/voxel.h"
#include "cloud/dbscan.h"
#include "cloud/knn.h"
#include "cloud/normals.h"
#include "cloud/fpfh.h"
#include "cloud/plane.h"
#include "cloud/average_normal.h"
#include "cloud/bounds.h"
#include "cloud/select.h"

namespace {

int check_cloud(pedp_ctx_t c, const double *pts, int64_t N, const char *who) {
    PEDP_REQUIRE(c, "%s: null context", who);
    PEDP_REQUIRE(N >= 0 && N < (int64_t)1 << 31, "%s: N out of range", who);
    PEDP_REQUIRE(pts || N == 0, "%s: null points", who);
    return PEDP_OK;
}

// The small device block of the context (ops_small, never inside `ops`, which the cores re-carve): the partial bounds
// and the few values preprocess_source keeps on the device between its stages.  The members are the layout.
struct SmallBlock {
    double part[6 * BND_BLOCKS];  // bounds_kernel: a box per workgroup (avgn_origin_kernel reads them too)
    double best[16];              // ransac_best_kernel: the best iteration, its three points, its plane (14 used)
    double origin[4];             // avgn_origin_kernel: the origin of the average normal's grid
    double avg_res[8];            // avgn_rows_kernel: [3] the number of voxel means, [4] the overflow flag
    int avg_overflow, pad0_;      // avgn_mean_kernel: a voxel with more members than its LDS share
    double pad1_[19];
    double refit[8];              // refit_fold_kernel: centroid, plane, inlier count
    double spare_[456];           // (the reservation stays what it was: the partial bounds and 4096 bytes)
};
static_assert(offsetof(SmallBlock, best) == sizeof(double) * (6 * BND_BLOCKS) && offsetof(SmallBlock, origin) == sizeof(double) * (6 * BND_BLOCKS + 16) &&
                  offsetof(SmallBlock, avg_res) == sizeof(double) * (6 * BND_BLOCKS + 20) &&
                  offsetof(SmallBlock, avg_overflow) == sizeof(double) * (6 * BND_BLOCKS + 28) &&
                  offsetof(SmallBlock, refit) == sizeof(double) * (6 * BND_BLOCKS + 48),
              "the block's members keep their places");
static_assert(sizeof(SmallBlock) == ((sizeof(double) * 6 * BND_BLOCKS + 255) & ~(size_t)255) + 4096, "and its size");
int small_block(pedp_ctx_t c, SmallBlock **sb) {
    PEDP_TRY(c->ops_small.reserve(sizeof(SmallBlock)));
    *sb = (SmallBlock *)c->ops_small.ptr;
    return PEDP_OK;
}

int bounds_device(pedp_ctx_t c, const double *d_pts, int64_t N, double *d_part /* 6 * BND_BLOCKS */, double lo[3], double hi[3]) {
    hipLaunchKernelGGL(bounds_kernel, dim3(BND_BLOCKS), dim3(256), 0, c->stream, d_pts, N, d_part);
    PEDP_HIP_CHECK(hipGetLastError());
    static_assert(sizeof(double) * 6 * BND_BLOCKS <= pedp_pinned::BOUNDS.bytes, "the partial boxes fit their slot");
    double *h = pedp_pinned_at<double>(c, pedp_pinned::BOUNDS);
    PEDP_HIP_CHECK(hipMemcpyAsync(h, d_part, sizeof(double) * 6 * BND_BLOCKS, hipMemcpyDeviceToHost, c->stream));
    PEDP_HIP_CHECK(hipStreamSynchronize(c->stream));
    bool bad = h[0] != h[0];
    for (int k = 0; k < 3; ++k) { lo[k] = h[k]; hi[k] = h[3 + k]; }
    for (int b = 1; b < BND_BLOCKS; ++b) {
        bad |= h[6 * b] != h[6 * b];  // a poisoned partial
        for (int k = 0; k < 3; ++k) {
            if (h[6 * b + k] < lo[k]) lo[k] = h[6 * b + k];
            if (h[6 * b + 3 + k] > hi[k]) hi[k] = h[6 * b + 3 + k];
        }
    }
    if (bad) lo[0] = std::nan("");
    return PEDP_OK;
}

// the host pass: the box, and whether every coordinate is finite (the comparisons alone pass over a NaN)
bool bounds(const double *pts, int64_t N, double lo[3], double hi[3]) {
    bool bad = false;
    for (int k = 0; k < 3; ++k) { lo[k] = hi[k] = pts[k]; bad |= !std::isfinite(pts[k]); }
    for (int64_t i = 1; i < N; ++i)
        for (int k = 0; k < 3; ++k) {
            const double v = pts[3 * i + k];
            if (v < lo[k]) lo[k] = v;
            if (v > hi[k]) hi[k] = v;
            bad |= !std::isfinite(v);
        }
    return !bad;
}

// The box of a caller's cloud: a large one's from its device copy (d_pts, with d_part for the partial boxes) -- no host
// pass over the caller's array -- a small one's by the host pass.
constexpr int64_t BND_DEVICE_MIN = 32768;
int box_of(pedp_ctx_t c, const double *pts, const double *d_pts, int64_t N, double *d_part, double lo[3], double hi[3]) {
    if (N >= BND_DEVICE_MIN) return bounds_device(c, d_pts, N, d_part, lo, hi);
    if (!bounds(pts, N, lo, hi)) lo[0] = std::nan("");  // (make_grid refuses, like the device pass's poisoned box)
    return PEDP_OK;
}
// The same for a caller that sizes its workspace by the grid: a large cloud's points go up first, into their own
// scratch.  Returns the device copy or nullptr.
int bounds_of(pedp_ctx_t c, const double *pts, int64_t N, double lo[3], double hi[3], double **d_in) {
    double *d = nullptr, *d_part = nullptr;
    if (N >= BND_DEVICE_MIN) {
        PEDP_HIP_CHECK(hipSetDevice(c->device));
        PEDP_TRY(c->ops_in.reserve(a256(sizeof(double) * 3 * (size_t)N) + a256(sizeof(double) * 6 * BND_BLOCKS)));
        d = (double *)c->ops_in.ptr;
        d_part = (double *)((char *)c->ops_in.ptr + a256(sizeof(double) * 3 * (size_t)N));
        PEDP_TRY(pedp_upload(c, d, pts, sizeof(double) * 3 * (size_t)N));
    }
    *d_in = d;
    return box_of(c, pts, d, N, d_part, lo, hi);
}

// grid over the bounding box with the given cell size, coarsened until it has at most 2^24 cells
int make_grid(const double lo[3], const double hi[3], double cell, Grid &g, int64_t &n_cells, const char *who) {
    g.cell = cell;
    while (true) {
        double cells = 1.0;
        for (int k = 0; k < 3; ++k) {
            PEDP_REQUIRE(std::isfinite(lo[k]) && std::isfinite(hi[k]), "%s: non-finite coordinates", who);
            g.lo[k] = lo[k];
            const double d = std::floor((hi[k] - lo[k]) / g.cell) + 1.0;
            g.dim[k] = d < 1.0 ? 1 : (d > 1e9 ? 1000000000 : (int)d);
            cells *= (double)g.dim[k];
        }
        if (cells <= 16777216.0) break;
        g.cell *= 2.0;  // a coarser grid is still a valid (slower) neighbourhood index
    }
    n_cells = (int64_t)g.dim[0] * g.dim[1] * g.dim[2];
    return PEDP_OK;
}

// ------------------------------------------------------------------ rocPRIM, said once
// Stable sort of (64-bit key, int) pairs on bits [begin_bit, end_bit).  rocPRIM's default sorts up to a million items by
// merging (about twenty launches whatever the key's width); `passes` takes the radix passes instead, whose number
// follows the bits asked for (cloud/common.h: RadixPasses).  From SORT_RADIX_MIN items on the passes are the shorter
// way: below, the merge sort's launches are (a radix pass takes 20 us whatever the size).  tmp == nullptr asks for the
// scratch size, as rocPRIM does.
constexpr int64_t SORT_RADIX_MIN = 131072;
int sort_pairs_u64(void *tmp, size_t &tmp_bytes, unsigned long long *keys, unsigned long long *keys_s, int *val, int *val_s, unsigned n,
                   int begin_bit, int end_bit, bool passes, hipStream_t stream) {
    if (passes) PEDP_ROCPRIM(rocprim::radix_sort_pairs<RadixPasses>(tmp, tmp_bytes, keys, keys_s, val, val_s, n, begin_bit, end_bit, stream));
    else PEDP_ROCPRIM(rocprim::radix_sort_pairs(tmp, tmp_bytes, keys, keys_s, val, val_s, n, begin_bit, end_bit, stream));
    return PEDP_OK;
}
// scratch of rocprim::exclusive_scan over n unsigned counts or flags (Out: what the sums are written as, In: what is read)
template <class Out = unsigned, class In = unsigned *>
int scan_tmp_bytes(size_t n, hipStream_t stream, size_t &bytes, In in = nullptr) {
    PEDP_ROCPRIM(rocprim::exclusive_scan(nullptr, bytes, in, (Out *)nullptr, 0u, n, rocprim::plus<unsigned>(), stream));
    return PEDP_OK;
}

// ------------------------------------------------------------------ the 64-bit key sort
// Stable sort of point indices by a small integer key (pedp_icp.hip: spatial order of a cloud by the Hilbert index of
// its grid cell; the defect map, the solid queries and the mesh topology sort with it too).  Stable = equal keys keep
// ascending point index, so the order is a function of the data alone -- the ICP sums that follow it are run-to-run
// bit-stable.  keys: N 64-bit keys below 2^bits on the device (overwritten); d_perm: N int32 out.
// Two calls: _begin reserves the context's scratch for N 64-bit keys plus the sort's buffers and returns the key
// array for the caller's key kernel; _run sorts.  Everything is stream-ordered in the context's pooled scratch:
// no allocation once sizes have settled, no synchronisation.
struct Sort64Layout {
    unsigned long long *keys, *keys_s;
    int *val;
    void *tmp;
    size_t tmp_bytes;
};
// The keys are Hilbert indices, most significant level first: their top 3 b bits are the index at b bits per axis.
// Only as many levels are sorted on as tell the points apart -- b = ceil(log2(N) / 3) + 1 bits per axis, a few
// points per cell; inside a cell the stable sort keeps the point order -- because the radix passes' number follows
// the bits (a 368 k-point frame: 24 bits, three passes, instead of six for all 48).
struct SortPlan { int begin_bit, end_bit; bool passes; };
SortPlan sort_plan(int64_t N, int bits) {
    int lg = 0;
    while (lg < 62 && ((int64_t)1 << lg) < N) ++lg;
    int per_axis = (lg + 2) / 3 + 1;
    per_axis = per_axis < 5 ? 5 : per_axis;
    const int used = 3 * per_axis < bits ? 3 * per_axis : bits;
    return {bits - used, bits, N >= SORT_RADIX_MIN};
}
// every bit of the key counts (the target's tile order: segment id over a coordinate's bits)
SortPlan sort_plan_exact(int64_t N, int bits) { return {0, bits, N >= SORT_RADIX_MIN}; }
int sort64_layout(pedp_ctx_t c, int64_t N, const SortPlan &sp, Sort64Layout &L) {
    size_t tmp_sort = 0;
    PEDP_TRY(sort_pairs_u64(nullptr, tmp_sort, nullptr, nullptr, nullptr, nullptr, (unsigned)N, sp.begin_bit, sp.end_bit, sp.passes, c->stream));
    const size_t need = 2 * a256(sizeof(unsigned long long) * N) + a256(sizeof(int) * N) + a256(tmp_sort) + 1024;
    PEDP_TRY(c->sort_ws.reserve(need));
    Carver cv{(char *)c->sort_ws.ptr};
    L.keys = cv.take<unsigned long long>(N);
    L.keys_s = cv.take<unsigned long long>(N);
    L.val = cv.take<int>(N);
    L.tmp = cv.take<char>(tmp_sort);
    L.tmp_bytes = tmp_sort;
    return PEDP_OK;
}
int sort64_begin(pedp_ctx_t c, int64_t N, const SortPlan &sp, unsigned long long **d_keys) {
    Sort64Layout L;
    PEDP_TRY(sort64_layout(c, N, sp, L));
    *d_keys = L.keys;
    return PEDP_OK;
}
int sort64_run(pedp_ctx_t c, int64_t N, const SortPlan &sp, int32_t *d_perm) {
    if (N <= 0) return PEDP_OK;
    Sort64Layout L;
    PEDP_TRY(sort64_layout(c, N, sp, L));  // same sizes as _begin: the scratch does not move
    hipLaunchKernelGGL(iota_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, c->stream, L.val, N);
    PEDP_TRY(sort_pairs_u64(L.tmp, L.tmp_bytes, L.keys, L.keys_s, L.val, (int *)d_perm, (unsigned)N, sp.begin_bit, sp.end_bit, sp.passes, c->stream));
    PEDP_HIP_CHECK(hipGetLastError());
    return PEDP_OK;
}

// ------------------------------------------------------------------ device-to-device cores
// Every operation below takes its points where they already are -- in device memory -- and leaves its result
// there (inside the context's `ops` scratch, valid until the next operation).  The C entry points with host
// arrays are thin wrappers (upload, core, download); pedp_preprocess_source chains the cores without the
// points ever visiting the host.

int voxel_core(pedp_ctx_t c, const double *d_pts, const double *d_nrm, int64_t N, double voxel_size, double **out_pts,
               double **out_nrm, int64_t *n_out, double *box_lo = nullptr, double *box_hi = nullptr,
               const char *who = "pedp_voxel_down_sample") {
    double lo[3], hi[3];
    SmallBlock *sb = nullptr;
    PEDP_TRY(small_block(c, &sb));
    PEDP_TRY(bounds_device(c, d_pts, N, sb->part, lo, hi));
    for (int k = 0; k < 3 && box_lo && box_hi; ++k) { box_lo[k] = lo[k]; box_hi[k] = hi[k]; }  // the averages lie inside it
    for (int k = 0; k < 3; ++k)  // before any key is formed (bounds_device hands a NaN box for a NaN / infinite row)
        PEDP_REQUIRE(std::isfinite(lo[k]) && std::isfinite(hi[k]), "%s: non-finite coordinates", who);
    int bits[3];
    for (int k = 0; k < 3; ++k) {
        lo[k] = lo[k] - voxel_size * 0.5;
        PEDP_REQUIRE((hi[k] - lo[k]) / voxel_size < 2097151.0, "pedp_voxel_down_sample: voxel_size is too small");
        // the largest cell index of the axis, one to spare for the division's rounding
        const unsigned long long top = (unsigned long long)std::floor((hi[k] - lo[k]) / voxel_size) + 1ull;
        bits[k] = 1;
        while (bits[k] < 21 && (top >> bits[k])) ++bits[k];
    }
    const int key_bits = bits[0] + bits[1] + bits[2];
    const unsigned n = (unsigned)N;
    size_t tmp_sort = 0, tmp_rle = 0, tmp_scan = 0;
    const bool passes = N >= SORT_RADIX_MIN;
    PEDP_TRY(sort_pairs_u64(nullptr, tmp_sort, nullptr, nullptr, nullptr, nullptr, n, 0, key_bits, passes, c->stream));
    PEDP_ROCPRIM(rocprim::run_length_encode(nullptr, tmp_rle, (unsigned long long *)nullptr, n, (unsigned long long *)nullptr,
                                            (unsigned *)nullptr, (unsigned *)nullptr, c->stream));
    PEDP_TRY(scan_tmp_bytes(n, c->stream, tmp_scan));
    size_t tmp = tmp_sort > tmp_rle ? tmp_sort : tmp_rle;
    if (tmp_scan > tmp) tmp = tmp_scan;
    const size_t need = a256(sizeof(double) * 3 * N) * 2 + a256(sizeof(unsigned long long) * N) * 3 + a256(sizeof(int) * N) * 2 +
                        a256(sizeof(unsigned) * N) * 2 + 256 + a256(tmp) + 4096;
    PEDP_TRY(c->ops.reserve(need));
    Carver cv{(char *)c->ops.ptr};
    double *d_out = cv.take<double>(3 * (size_t)N), *d_outn = cv.take<double>(3 * (size_t)N);
    unsigned long long *key = cv.take<unsigned long long>(N), *key_s = cv.take<unsigned long long>(N),
                       *uniq = cv.take<unsigned long long>(N);
    int *val = cv.take<int>(N), *val_s = cv.take<int>(N);
    unsigned *counts = cv.take<unsigned>(N), *offsets = cv.take<unsigned>(N), *n_runs = cv.take<unsigned>(1);
    void *d_tmp = cv.take<char>(tmp);
    const unsigned grid = (unsigned)((N + 255) / 256);
    hipLaunchKernelGGL(voxel_key_kernel, dim3(grid), dim3(256), 0, c->stream, d_pts, N, lo[0], lo[1], lo[2], voxel_size, bits[1], bits[2],
                       key, val);
    PEDP_TRY(sort_pairs_u64(d_tmp, tmp_sort, key, key_s, val, val_s, n, 0, key_bits, passes, c->stream));
    PEDP_ROCPRIM(rocprim::run_length_encode(d_tmp, tmp_rle, key_s, n, uniq, counts, n_runs, c->stream));
    PEDP_ROCPRIM(rocprim::exclusive_scan(d_tmp, tmp_scan, counts, offsets, 0u, n, rocprim::plus<unsigned>(), c->stream));
    hipLaunchKernelGGL(voxel_average_kernel, dim3(grid), dim3(256), 0, c->stream, d_pts, d_nrm, val_s, counts, offsets, n_runs,
                       d_out, d_outn);
    PEDP_HIP_CHECK(hipGetLastError());
    unsigned *h_runs = pedp_pinned_at<unsigned>(c, pedp_pinned::COUNTERS);
    PEDP_HIP_CHECK(hipMemcpyAsync(h_runs, n_runs, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    PEDP_HIP_CHECK(hipStreamSynchronize(c->stream));
    *n_out = *h_runs;
    *out_pts = d_out;
    *out_nrm = d_nrm ? d_outn : nullptr;
    return PEDP_OK;
}

// the uniform grid of a cloud on the device: cells, sorted order, ranges, points gathered in that order
struct GridIndex {
    Grid g;
    double *sp;
    int *val_s, *cell_start, *cell_end;  // cell_end = cell_start + 1: one monotone array of n_cells + 1 run starts
    unsigned *cell_s;                    // cell of every sorted position
    void *tmp;  // the scan's scratch, free once the index stands
    size_t tmp_bytes;
};
// reserves `ops` for the index and `extra` bytes behind it, carves the index out of cv -- the caller takes its own
// arrays from cv afterwards -- and builds it
int grid_index(pedp_ctx_t c, const double *d_pts, int64_t N, const Grid &g, int64_t n_cells, size_t extra, Carver &cv, GridIndex &ix) {
    size_t tmp_scan = 0;
    PEDP_TRY(scan_tmp_bytes<int>((size_t)n_cells + 1, c->stream, tmp_scan));
    const size_t ix_bytes = a256(sizeof(double) * 3 * N) + a256(sizeof(unsigned) * N) * 2 + a256(sizeof(int) * N) * 2 +
                            a256(sizeof(int) * (n_cells + 1)) * 2 + a256(tmp_scan < 256 ? 256 : tmp_scan);
    PEDP_TRY(c->ops.reserve(ix_bytes + extra));
    cv = Carver{(char *)c->ops.ptr};
    ix.g = g;
    ix.sp = cv.take<double>(3 * (size_t)N);
    unsigned *cell = cv.take<unsigned>(N);
    ix.cell_s = cv.take<unsigned>(N);
    int *slot = cv.take<int>(N);
    ix.val_s = cv.take<int>(N);
    unsigned *count = cv.take<unsigned>(n_cells + 1);
    ix.cell_start = cv.take<int>(n_cells + 1);
    ix.cell_end = ix.cell_start + 1;
    ix.tmp = cv.take<char>(tmp_scan < 256 ? 256 : tmp_scan);
    ix.tmp_bytes = tmp_scan;
    const unsigned grid = (unsigned)((N + 255) / 256);
    PEDP_HIP_CHECK(hipMemsetAsync(count, 0, sizeof(unsigned) * ((size_t)n_cells + 1), c->stream));
    hipLaunchKernelGGL(grid_count_kernel, dim3(grid), dim3(256), 0, c->stream, d_pts, N, g, cell, slot, count);
    PEDP_ROCPRIM(rocprim::exclusive_scan(ix.tmp, tmp_scan, count, ix.cell_start, 0u, (size_t)n_cells + 1, rocprim::plus<unsigned>(), c->stream));
    hipLaunchKernelGGL(grid_place_kernel, dim3(grid), dim3(256), 0, c->stream, d_pts, N, (const unsigned *)cell, (const int *)slot,
                       (const int *)ix.cell_start, ix.sp, ix.val_s, ix.cell_s);
    PEDP_HIP_CHECK(hipGetLastError());
    return PEDP_OK;
}

int dbscan_core(pedp_ctx_t c, const double *d_pts, int64_t N, double eps, int min_points, const double lo[3], const double hi[3],
                int32_t **out_labels) {
    Grid g;
    int64_t n_cells = 0;
    // cell = eps / sqrt(3) less a hair: a cell's diameter is below eps and neighbours within eps are never three cells apart
    PEDP_TRY(make_grid(lo, hi, eps * 0.57735026918962576 * (1.0 - 1e-9), g, n_cells, "pedp_cluster_dbscan"));
    const bool clique = g.cell * 1.7320508075688772 < eps;
    // beyond the cell budget: cells of eps (or its next doubling that fits), neighbours one cell apart
    if (!clique) PEDP_TRY(make_grid(lo, hi, eps * (1.0 + 1e-9), g, n_cells, "pedp_cluster_dbscan"));
    const unsigned n = (unsigned)N;
    size_t tmp_scan = 0;
    PEDP_TRY(scan_tmp_bytes(n, c->stream, tmp_scan));
    Carver cv{};
    GridIndex ix;
    PEDP_TRY(grid_index(c, d_pts, N, g, n_cells,
                        a256(sizeof(unsigned) * N) * 2 + a256(sizeof(int) * N) * 4 + a256(sizeof(int) * n_cells) + a256(tmp_scan) + 4096, cv, ix));
    unsigned *is_rep = cv.take<unsigned>(N), *rank = cv.take<unsigned>(N);
    int *core = cv.take<int>(N), *parent = cv.take<int>(N), *root = cv.take<int>(N), *rep = cv.take<int>(n_cells);
    int32_t *d_labels = cv.take<int32_t>(N);
    void *d_tmp = cv.take<char>(tmp_scan);
    const unsigned grid = (unsigned)((N + 255) / 256);
    const double e2 = eps * eps;
    const unsigned grid_w = (unsigned)((N + DB_WPB - 1) / DB_WPB);
    auto launches = [&](auto with_cliques) -> int {  // std::true_type / std::false_type: the kernels' CLIQUE
        constexpr bool CLIQUE = decltype(with_cliques)::value;
        hipLaunchKernelGGL(dbscan_core_kernel<CLIQUE>, dim3(grid_w), dim3(DB_WPB * 64), 0, c->stream, g, ix.sp, N, ix.cell_start, ix.cell_end, e2,
                           min_points, ix.val_s, core, parent);
        if (CLIQUE)
            hipLaunchKernelGGL(dbscan_cell_kernel, dim3((unsigned)((n_cells + 255) / 256)), dim3(256), 0, c->stream, n_cells, ix.cell_start,
                               ix.cell_end, ix.val_s, core, rep, parent);
        hipLaunchKernelGGL(dbscan_union_kernel<CLIQUE>, dim3(grid_w), dim3(DB_WPB * 64), 0, c->stream, g, ix.sp, N, ix.cell_start, ix.cell_end,
                           ix.cell_s, e2, ix.val_s, core, rep, parent);
        hipLaunchKernelGGL(dbscan_root_kernel, dim3(grid), dim3(256), 0, c->stream, N, core, parent, root, is_rep);
        PEDP_ROCPRIM(rocprim::exclusive_scan(d_tmp, tmp_scan, is_rep, rank, 0u, n, rocprim::plus<unsigned>(), c->stream));
        hipLaunchKernelGGL(dbscan_label_kernel<CLIQUE>, dim3(grid_w), dim3(DB_WPB * 64), 0, c->stream, g, ix.sp, N, ix.cell_start, ix.cell_end, e2,
                           ix.val_s, root, rank, d_labels);
        PEDP_HIP_CHECK(hipGetLastError());
        return PEDP_OK;
    };
    PEDP_TRY(clique ? launches(std::true_type{}) : launches(std::false_type{}));
    *out_labels = d_labels;
    return PEDP_OK;
}

int knn_core(pedp_ctx_t c, const double *d_pts, int64_t N, int k, const double lo[3], const double hi[3], double **out_avg) {
    if (N <= KNN_SMALL_MAX) {  // a wave per query, all distances in LDS
        PEDP_TRY(c->ops.reserve(a256(sizeof(double) * N) + 512));
        double *d_avg0 = (double *)c->ops.ptr;
        PEDP_HIP_CHECK(hipFuncSetAttribute((const void *)knn_mean_small_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)(sizeof(double) * KNN_SMALL_MAX)));
        hipLaunchKernelGGL(knn_mean_small_kernel, dim3((unsigned)N), dim3(64), sizeof(double) * (size_t)N, c->stream, d_pts, (int)N, k,
                           d_avg0);
        PEDP_HIP_CHECK(hipGetLastError());
        *out_avg = d_avg0;
        return PEDP_OK;
    }
    // cell ~ the radius that holds k points if the cloud were spread over a sheet of the box's
    // largest extent (scanned surfaces are sheets); any cell size gives the same result
    double ext = 0.0;
    for (int d = 0; d < 3; ++d) ext = std::fmax(ext, hi[d] - lo[d]);
    double cell = ext * std::sqrt((double)k / (3.14159265358979 * (double)N));
    if (!(cell > 0.0) || !std::isfinite(cell)) cell = 1.0;
    Grid g;
    int64_t n_cells = 0;
    PEDP_TRY(make_grid(lo, hi, cell, g, n_cells, "pedp_knn_mean_distance"));
    Carver cv{};
    GridIndex ix;
    PEDP_TRY(grid_index(c, d_pts, N, g, n_cells, a256(sizeof(double) * N) + 4096, cv, ix));
    double *d_avg = cv.take<double>(N);
    // a wave per query; a cloud too dense for the LDS share of some query falls back to a thread per query: that kernel
    // is launched behind the first one and leaves at once unless the overflow flag is up (no trip to the host to ask)
    int *d_over = (int *)ix.tmp;  // the scan is done: its scratch is free
    PEDP_HIP_CHECK(hipMemsetAsync(d_over, 0, sizeof(int), c->stream));
    hipLaunchKernelGGL(knn_mean_wave_kernel, dim3((unsigned)((N + KNN_WPB - 1) / KNN_WPB)), dim3(KNN_WPB * 64), 0, c->stream, g, ix.sp, N,
                       ix.cell_start, ix.cell_end, ix.val_s, k, d_avg, d_over);
    const size_t lds = sizeof(double) * (size_t)k * KNN_THREADS;
    PEDP_HIP_CHECK(hipFuncSetAttribute((const void *)knn_mean_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(knn_mean_kernel, dim3((unsigned)((N + KNN_THREADS - 1) / KNN_THREADS)), dim3(KNN_THREADS), lds, c->stream, g, ix.sp,
                       N, ix.cell_start, ix.cell_end, ix.val_s, k, d_avg, (const int *)d_over);
    PEDP_HIP_CHECK(hipGetLastError());
    *out_avg = d_avg;
    return PEDP_OK;
}

int normals_core(pedp_ctx_t c, const double *d_pts, int64_t N, double radius, int max_nn, const double *d_prior, const double lo[3],
                 const double hi[3], double **out_normals) {
    Grid g;
    int64_t n_cells = 0;
    PEDP_TRY(make_grid(lo, hi, radius * (1.0 + 1e-9), g, n_cells, "pedp_estimate_normals"));
    Carver cv{};
    GridIndex ix;
    PEDP_TRY(grid_index(c, d_pts, N, g, n_cells, a256(sizeof(double) * 3 * N) + 4096, cv, ix));
    double *d_out = cv.take<double>(3 * (size_t)N);
    const size_t lds = (sizeof(double) + sizeof(int)) * (size_t)max_nn * NRM_THREADS;
    PEDP_HIP_CHECK(hipFuncSetAttribute((const void *)normals_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(normals_kernel, dim3((unsigned)((N + NRM_THREADS - 1) / NRM_THREADS)), dim3(NRM_THREADS), lds, c->stream, g,
                       ix.sp, N, ix.cell_start, ix.cell_end, ix.val_s, radius * radius, max_nn, d_pts, d_prior, d_out);
    PEDP_HIP_CHECK(hipGetLastError());
    *out_normals = d_out;
    return PEDP_OK;
}

// compute_average_normal's voxel means on the device (cloud/average_normal.h), nothing read back here: the means go to the context's
// pinned block as the kernel writes them, their number and the overflow flag (h_res[3], [4]) are on their way to `h_res`
// (pinned) when the call returns; all valid after the stream's next synchronisation.  *enqueued = false: the dense grid does not fit (the caller takes the sort-based grid).
int average_normal_core(pedp_ctx_t c, const double *d_pts, const double *d_nrm, int64_t N, double voxel, const double box_lo[3],
                        const double box_hi[3], SmallBlock *sb, double *h_res, bool *enqueued) {
    *enqueued = false;
    AvgGrid g;
    g.voxel = voxel;
    double cells = 1.0;
    for (int k = 0; k < 3; ++k) {
        const double d = std::floor((box_hi[k] - box_lo[k]) / voxel) + 3.0;  // origin >= box_lo - voxel / 2, points <= box_hi
        if (!(d >= 1.0) || d > 4194304.0) return PEDP_OK;
        g.dim[k] = (int)d;
        cells *= d;
    }
    if (cells > 4194304.0) return PEDP_OK;
    const int64_t n_cells = (int64_t)g.dim[0] * g.dim[1] * g.dim[2];
    size_t tmp_a = 0, tmp_b = 0;
    PEDP_TRY(scan_tmp_bytes((size_t)n_cells + 1, c->stream, tmp_a));
    PEDP_TRY(scan_tmp_bytes((size_t)n_cells, c->stream, tmp_b, rocprim::make_transform_iterator((const unsigned *)nullptr, NonEmpty())));
    const size_t tmp = tmp_a > tmp_b ? tmp_a : tmp_b;
    const int64_t max_rows = n_cells < N ? n_cells : N;
    if (sizeof(double) * 3 * (size_t)max_rows > c->avg_host_cap) {
        if (c->avg_host) { PEDP_HIP_CHECK(hipStreamSynchronize(c->stream)); (void)hipHostFree(c->avg_host); }
        c->avg_host = nullptr;
        c->avg_host_cap = 0;
        const size_t want = sizeof(double) * 3 * (size_t)max_rows + sizeof(double) * 3 * (size_t)max_rows / 4 + 4096;
        PEDP_HIP_CHECK(hipHostMalloc(&c->avg_host, want, hipHostMallocDefault));
        c->avg_host_cap = want;
    }
    PEDP_TRY(c->ops.reserve(a256(sizeof(unsigned) * ((size_t)n_cells + 1)) * 3 + a256(sizeof(unsigned) * N) + a256(sizeof(int) * N) * 2 +
                            a256(tmp) + 4096));
    Carver cv{(char *)c->ops.ptr};
    unsigned *count = cv.take<unsigned>((size_t)n_cells + 1), *begin = cv.take<unsigned>((size_t)n_cells + 1),
             *rank = cv.take<unsigned>((size_t)n_cells + 1), *cell = cv.take<unsigned>(N);
    int *slot = cv.take<int>(N), *member = cv.take<int>(N);
    double *means = (double *)c->avg_host;  // (pinned host memory, written by the device)
    void *d_tmp = cv.take<char>(tmp);
    double *d_part = sb->part, *d_org = sb->origin, *d_res = sb->avg_res;
    int *d_over = &sb->avg_overflow;
    const unsigned grid = (unsigned)((N + 255) / 256);
    hipLaunchKernelGGL(bounds_kernel, dim3(BND_BLOCKS), dim3(256), 0, c->stream, d_pts, N, d_part);
    hipLaunchKernelGGL(avgn_origin_kernel, dim3(1), dim3(256), 0, c->stream, (const double *)d_part, BND_BLOCKS, voxel, d_org);
    PEDP_HIP_CHECK(hipMemsetAsync(count, 0, sizeof(unsigned) * ((size_t)n_cells + 1), c->stream));
    PEDP_HIP_CHECK(hipMemsetAsync(d_over, 0, sizeof(int), c->stream));
    hipLaunchKernelGGL(avgn_count_kernel, dim3(grid), dim3(256), 0, c->stream, d_pts, N, (const double *)d_org, g, cell, slot, count);
    PEDP_ROCPRIM(rocprim::exclusive_scan(d_tmp, tmp_a, count, begin, 0u, (size_t)n_cells + 1, rocprim::plus<unsigned>(), c->stream));
    hipLaunchKernelGGL(avgn_place_kernel, dim3(grid), dim3(256), 0, c->stream, N, (const unsigned *)cell, (const int *)slot,
                       (const unsigned *)begin, member);
    auto flags = rocprim::make_transform_iterator((const unsigned *)count, NonEmpty());
    PEDP_ROCPRIM(rocprim::exclusive_scan(d_tmp, tmp_b, flags, rank, 0u, (size_t)n_cells, rocprim::plus<unsigned>(), c->stream));
    hipLaunchKernelGGL(avgn_mean_kernel, dim3((unsigned)((n_cells + 64 * AVGN_WPB - 1) / (64 * AVGN_WPB))), dim3(64 * AVGN_WPB), 0, c->stream, n_cells, (const unsigned *)begin,
                       (const unsigned *)rank, (const int *)member, d_nrm, means, d_over);
    hipLaunchKernelGGL(avgn_rows_kernel, dim3(1), dim3(1), 0, c->stream, n_cells, (const unsigned *)rank, (const unsigned *)count,
                       (const int *)d_over, d_res);
    PEDP_HIP_CHECK(hipGetLastError());
    PEDP_HIP_CHECK(hipMemcpyAsync(h_res, d_res, sizeof(double) * 5, hipMemcpyDeviceToHost, c->stream));
    *enqueued = true;
    return PEDP_OK;
}

// plane RANSAC: inlier counts of every iteration -> the best iteration (most inliers, earliest on ties) and its plane
int plane_best_core(pedp_ctx_t c, const double *d_pts, int64_t N, double distance_threshold, int num_iterations, uint64_t seed,
                    int *best_t, double best[4], double *d_keep = nullptr /* 14 doubles on the device: the result stays there */) {
    PEDP_TRY(c->ops.reserve(a256(sizeof(int) * (size_t)num_iterations) + a256(sizeof(double) * (4 * (size_t)num_iterations + 32)) + 512));
    int *d_cnt = (int *)c->ops.ptr;
    double *d_planes = (double *)((char *)c->ops.ptr + a256(sizeof(int) * (size_t)num_iterations));
    hipLaunchKernelGGL(ransac_plane_kernel, dim3((unsigned)((num_iterations + 63) / 64)), dim3(64), 0, c->stream, d_pts, (long long)N,
                       (unsigned long long)seed, num_iterations, d_planes, d_cnt);
    hipLaunchKernelGGL(ransac_count_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)((num_iterations + RS_PLANES - 1) / RS_PLANES)),
                       dim3(256), 0, c->stream, d_pts, (long long)N, distance_threshold, num_iterations, (const double *)d_planes, d_cnt);
    PEDP_HIP_CHECK(hipGetLastError());
    double *d_best = d_keep ? d_keep : d_planes + 4 * (size_t)num_iterations, *h_best = pedp_pinned_at<double>(c, pedp_pinned::COUNTERS);
    hipLaunchKernelGGL(ransac_best_kernel, dim3(1), dim3(256), 0, c->stream, (const int *)d_cnt, num_iterations, d_pts, (long long)N,
                       (unsigned long long)seed, (const double *)d_planes, d_best);
    PEDP_HIP_CHECK(hipGetLastError());
    if (d_keep) return PEDP_OK;
    PEDP_HIP_CHECK(hipMemcpyAsync(h_best, d_best, sizeof(double) * 10, hipMemcpyDeviceToHost, c->stream));
    PEDP_HIP_CHECK(hipStreamSynchronize(c->stream));
    const int bt = (int)h_best[0];
    *best_t = bt;
    if (bt < 0) return PEDP_OK;
    const double *p3 = h_best + 1;  // the three sampled points
    triangle_plane(p3, p3 + 3, p3 + 6, best);
    return PEDP_OK;
}

// d_flag (N unsigned, in the chain's own buffers) -> kept points (and normals) in index order at out_*; one 4-byte read-back
int select_core(pedp_ctx_t c, const double *d_pts, const double *d_nrm, int64_t N, const unsigned *d_flag, double *out_pts,
                double *out_nrm, int64_t *n_out) {
    *n_out = 0;
    if (N == 0) return PEDP_OK;
    size_t tmp_scan = 0;
    PEDP_TRY(scan_tmp_bytes((unsigned)N, c->stream, tmp_scan));
    PEDP_TRY(c->ops.reserve(a256(sizeof(unsigned) * N) + a256(tmp_scan) + 512));
    Carver cv{(char *)c->ops.ptr};
    unsigned *pos = cv.take<unsigned>(N), *count = cv.take<unsigned>(1);
    void *d_tmp = cv.take<char>(tmp_scan);
    PEDP_ROCPRIM(rocprim::exclusive_scan(d_tmp, tmp_scan, d_flag, pos, 0u, (unsigned)N, rocprim::plus<unsigned>(), c->stream));
    hipLaunchKernelGGL(scatter_kept_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, c->stream, d_pts, d_nrm, N, d_flag, pos,
                       out_pts, out_nrm, count);
    PEDP_HIP_CHECK(hipGetLastError());
    unsigned *h = pedp_pinned_at<unsigned>(c, pedp_pinned::COUNTERS);
    PEDP_HIP_CHECK(hipMemcpyAsync(h, count, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    PEDP_HIP_CHECK(hipStreamSynchronize(c->stream));
    *n_out = *h;
    return PEDP_OK;
}

// The plane segment_plane returns -- the best plane refit over its inliers (plane_from_points' blocked sums) -- on the
// device, nothing read back here: res[3..6] the plane, res[7] the inlier count are on their way to `h_res` (pinned, 8
// doubles) when the call returns and valid after the stream's next synchronisation.
int refit_core(pedp_ctx_t c, const double *d_pts, int64_t N, const double *d_best, double thr, double *d_res, double *h_res) {
    const size_t n_blocks = (size_t)((N + 255) / 256);
    PEDP_TRY(c->ops.reserve(a256(sizeof(double) * 6 * n_blocks) + 1024));
    double *part = (double *)c->ops.ptr;
    const unsigned grid = (unsigned)n_blocks;
    hipLaunchKernelGGL(refit_block_kernel<3>, dim3(grid), dim3(256), 0, c->stream, d_pts, N, d_best, thr, (const double *)d_res, part);
    hipLaunchKernelGGL(refit_fold_kernel<3>, dim3(1), dim3(256), 0, c->stream, (const double *)part, (int64_t)n_blocks, d_res);
    hipLaunchKernelGGL(refit_block_kernel<6>, dim3(grid), dim3(256), 0, c->stream, d_pts, N, d_best, thr, (const double *)d_res, part);
    hipLaunchKernelGGL(refit_fold_kernel<6>, dim3(1), dim3(256), 0, c->stream, (const double *)part, (int64_t)n_blocks, d_res);
    PEDP_HIP_CHECK(hipGetLastError());
    PEDP_HIP_CHECK(hipMemcpyAsync(h_res, d_res, sizeof(double) * 8, hipMemcpyDeviceToHost, c->stream));
    return PEDP_OK;
}

// upload of a wrapper's host array into the context's input scratch (its own allocation: the cores re-carve `ops`)
int upload_in(pedp_ctx_t c, const double *pts, const double *second, int64_t N, double **d_a, double **d_b) {
    const size_t bytes = a256(sizeof(double) * 3 * (size_t)N);
    PEDP_TRY(c->ops_in.reserve(bytes * (second ? 2 : 1) + 256));
    *d_a = (double *)c->ops_in.ptr;
    PEDP_TRY(pedp_upload(c, *d_a, pts, sizeof(double) * 3 * (size_t)N));
    if (second) {
        *d_b = (double *)((char *)c->ops_in.ptr + bytes);
        PEDP_TRY(pedp_upload(c, *d_b, second, sizeof(double) * 3 * (size_t)N));
    } else if (d_b) {
        *d_b = nullptr;
    }
    return PEDP_OK;
}

// ------------------------------------------------------------------ the stages of pedp_preprocess_source
// What the chain carries: the clouds between its stages -- three (points, normals) pairs and a flag array in the
// context's `chain` scratch, sized by the down-sampled cloud -- and the two results that are enqueued early and collected
// after the stream's next wait, the refit plane and the average normal.
struct Chain {
    double *A_pts, *A_nrm, *B_pts, *B_nrm, *C_pts, *C_nrm;
    unsigned *flag;
    int *d_members;               // members per label, then the largest cluster's label
    double box_lo[3], box_hi[3];  // of the input cloud: every later stage's points lie inside, so it can shape their grids
    SmallBlock *sb;
    double *report;               // pedp_preprocess_source_ex's, or null
    bool refit_pending = false, avg_pending = false, plane_found = false;
    double refit[4] = {0, 0, 0, 0};
    double avg[3] = {1.0, 1.0, 1.0};  // tracking frames: the reference's np.array([1, 1, 1]) (:217)
};
int chain_reserve(pedp_ctx_t c, int64_t m1, Chain &ch) {
    const size_t one = a256(sizeof(double) * 3 * (size_t)m1);
    PEDP_TRY(c->chain.reserve(6 * one + a256(sizeof(unsigned) * (size_t)m1) + a256(sizeof(int) * ((size_t)m1 + 1)) + 256));
    PEDP_TRY(small_block(c, &ch.sb));
    char *cb = (char *)c->chain.ptr;
    ch.A_pts = (double *)cb; ch.A_nrm = (double *)(cb + one); ch.B_pts = (double *)(cb + 2 * one); ch.B_nrm = (double *)(cb + 3 * one);
    ch.C_pts = (double *)(cb + 4 * one); ch.C_nrm = (double *)(cb + 5 * one);
    ch.flag = (unsigned *)(cb + 6 * one);
    ch.d_members = (int *)(cb + 6 * one + a256(sizeof(unsigned) * (size_t)m1));
    return PEDP_OK;
}

// numpy's mean over axis 0 of the voxel means: the rows added one after the other
void mean_of_rows(const double *rows, int64_t n, double mean[3]) {
    double sum[3] = {0.0, 0.0, 0.0};
    for (int64_t i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) sum[k] += rows[3 * (size_t)i + k];
    for (int k = 0; k < 3; ++k) mean[k] = sum[k] / (double)n;
}
// the average normal by the sort-based grid (a grid too large for dense cells, or a crowded voxel); A is still the
// down-sampled cloud
int average_by_sort(pedp_ctx_t c, Chain &ch, int64_t m1, double avg_voxel) {
    double *g_pts = nullptr, *g_nrm = nullptr;
    int64_t m10 = 0;
    PEDP_TRY(voxel_core(c, ch.A_pts, ch.A_nrm, m1, avg_voxel, &g_pts, &g_nrm, &m10));
    std::vector<double> vn(3 * (size_t)m10);
    PEDP_TRY(pedp_download(c, vn.data(), g_nrm, sizeof(double) * 3 * (size_t)m10));
    mean_of_rows(vn.data(), m10, ch.avg);
    if (ch.report) ch.report[9] = (double)m10;
    return PEDP_OK;
}
// after a wait on the stream: what average_normal_core left in the pinned block (sum xyz, voxels, overflow) and avg_host
int average_collect(pedp_ctx_t c, Chain &ch, int64_t m1, double avg_voxel) {
    if (!ch.avg_pending) return PEDP_OK;
    ch.avg_pending = false;
    const double *h_avg = pedp_pinned_at<double>(c, pedp_pinned::AVERAGE_NORMAL);
    if (h_avg[4] != 0.0) return average_by_sort(c, ch, m1, avg_voxel);
    mean_of_rows((const double *)c->avg_host, (int64_t)h_avg[3], ch.avg);  // the voxel means, written by avgn_mean_kernel
    if (ch.report) ch.report[9] = h_avg[3];
    return PEDP_OK;
}
// after a wait on the stream: what refit_core left in the pinned block
void refit_collect(pedp_ctx_t c, Chain &ch) {
    if (!ch.refit_pending) return;
    ch.refit_pending = false;
    const double *h_refit = pedp_pinned_at<double>(c, pedp_pinned::REFIT);
    ch.plane_found = h_refit[7] > 0.0;
    for (int k = 0; k < 4; ++k) ch.refit[k] = h_refit[3 + k];
    if (ch.report) { for (int k = 0; k < 4; ++k) ch.report[k] = ch.refit[k]; ch.report[8] = h_refit[7]; }
}

// flip_plane_normal_if_needed (:342-359) + remove_points_below_plane (:366-378) on A, from the collected refit plane
// and average normal.  Only the SIGN of dot(plane normal, average normal) is used; a dot product within rounding of
// zero is left to the step-by-step path (status AMBIGUOUS), whose numpy arithmetic is then the reference's to the letter.
int halfspace_flags(pedp_ctx_t c, Chain &ch, int64_t m1, bool nrm, int *status) {
    const double *refit = ch.refit, *avg = ch.avg;
    if (!ch.plane_found) { *status = PEDP_PREPROCESS_NO_CLUSTER; return PEDP_OK; }
    const double pn = std::sqrt((refit[0] * refit[0] + refit[1] * refit[1]) + refit[2] * refit[2]);
    const double an = nrm ? std::sqrt((avg[0] * avg[0] + avg[1] * avg[1]) + avg[2] * avg[2]) : 1.0;
    const double dot = ((refit[0] * avg[0] + refit[1] * avg[1]) + refit[2] * avg[2]) / (pn * an);
    if (!(std::fabs(dot) > 1e-9)) { *status = PEDP_PREPROCESS_AMBIGUOUS; return PEDP_OK; }
    const int flipped = dot < 0.0 ? 1 : 0;
    if (ch.report) ch.report[7] = (double)flipped;
    hipLaunchKernelGGL(halfspace_keep_kernel, dim3((unsigned)((m1 + 255) / 256)), dim3(256), 0, c->stream, ch.A_pts, m1, refit[0], refit[1],
                       refit[2], refit[3], flipped, ch.flag);
    return PEDP_OK;
}

// DBSCAN on B and the flags of its largest cluster (np.unique + argmax: the lowest label among the largest); the grid
// over the input's box: no trip to the host for this cloud's own
int largest_cluster_flags(pedp_ctx_t c, Chain &ch, int64_t m2, const pedp_preprocess_params *prm) {
    int32_t *d_labels = nullptr;
    PEDP_TRY(dbscan_core(c, ch.B_pts, m2, prm->cluster_eps, prm->cluster_min_points, ch.box_lo, ch.box_hi, &d_labels));
    int *d_members = ch.d_members;
    PEDP_HIP_CHECK(hipMemsetAsync(d_members, 0, sizeof(int) * (size_t)(m2 + 1), c->stream));
    hipLaunchKernelGGL(label_count_kernel, dim3((unsigned)((m2 + 255) / 256)), dim3(256), 0, c->stream, (const int32_t *)d_labels, m2,
                       d_members);
    hipLaunchKernelGGL(label_largest_kernel, dim3(1), dim3(256), 0, c->stream, (const int *)d_members, m2, d_members + m2);
    hipLaunchKernelGGL(label_keep_kernel, dim3((unsigned)((m2 + 255) / 256)), dim3(256), 0, c->stream, (const int32_t *)d_labels, m2,
                       (const int *)(d_members + m2), ch.flag);
    return PEDP_OK;
}

// Open3D's global step of remove_statistical_outlier over the mean neighbour distances, in index order
// (cloud_ops.statistical_outlier_indices: sequential sums): the limit mean + ratio * std.  false: no valid distance.
bool outlier_limit(const double *dist, int64_t n, double std_ratio, double *limit) {
    int64_t valid = 0;
    double sum = 0.0;  // (the count is exact in any order)
    for (int64_t i = 0; i < n; ++i) {
        valid += dist[i] >= 0.0 ? 1 : 0;
        sum += dist[i] > 0.0 ? dist[i] : 0.0;
    }
    if (valid <= 0) return false;
    const double mean = sum / (double)valid;
    double sq = 0.0;
    for (int64_t i = 0; i < n; ++i) sq += dist[i] > 0.0 ? (dist[i] - mean) * (dist[i] - mean) : 0.0;
    const double sd = valid > 1 ? std::sqrt(sq / (double)(valid - 1)) : std::nan("");
    *limit = mean + std_ratio * sd;
    return true;
}
// the statistical outlier filter on C: mean distance to the k nearest on the device, the limit on the host, the flags
// again on the device (*any = false: no flags, nothing is kept)
int outlier_flags(pedp_ctx_t c, Chain &ch, int64_t m3, const pedp_preprocess_params *prm, bool *any) {
    double lo[3], hi[3], *d_avg = nullptr, limit = 0.0;
    if (m3 > KNN_SMALL_MAX) PEDP_TRY(bounds_device(c, ch.C_pts, m3, ch.sb->part, lo, hi));  // (below, knn_core takes no grid)
    PEDP_TRY(knn_core(c, ch.C_pts, m3, prm->outlier_neighbors, lo, hi, &d_avg));
    // (read where the copy lands, in the context's page-locked buffer: a std::vector of its own cost an allocation, its
    // page faults and a staged copy -- 0.13 ms of host time in a frame's trace for 12 k doubles)
    const void *dist = nullptr;
    PEDP_TRY(pedp_download_view(c, d_avg, sizeof(double) * (size_t)m3, &dist));
    *any = outlier_limit((const double *)dist, m3, prm->outlier_std_ratio, &limit);
    if (*any)
        hipLaunchKernelGGL(range_keep_kernel, dim3((unsigned)((m3 + 255) / 256)), dim3(256), 0, c->stream, (const double *)d_avg, m3, limit,
                           ch.flag);
    return PEDP_OK;
}

}  // namespace

extern "C" {

static int voxel_down_sample_impl(pedp_ctx_t c, const double *pts, const double *normals, int64_t N, double voxel_size,
                                  double *out_pts, double *out_normals, int64_t capacity, int64_t *n_out, bool pts_on_device) {
    PEDP_TRY(check_cloud(c, pts, N, "pedp_voxel_down_sample"));
    PEDP_REQUIRE(n_out, "pedp_voxel_down_sample: null count");
    *n_out = 0;
    PEDP_REQUIRE(voxel_size > 0.0, "pedp_voxel_down_sample: voxel_size <= 0");  // Open3D raises too
    if (N == 0) return PEDP_OK;
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    double *d_pts = const_cast<double *>(pts), *d_nrm = nullptr;
    if (!pts_on_device) PEDP_TRY(upload_in(c, pts, normals, N, &d_pts, &d_nrm));
    double *d_out = nullptr, *d_outn = nullptr;
    int64_t m = 0;
    PEDP_TRY(voxel_core(c, d_pts, d_nrm, N, voxel_size, &d_out, &d_outn, &m));
    *n_out = m;
    PEDP_REQUIRE(m <= capacity, "pedp_voxel_down_sample: %lld voxels exceed the output capacity %lld", (long long)m,
                 (long long)capacity);
    PEDP_REQUIRE(out_pts && (out_normals || !normals), "pedp_voxel_down_sample: null output arrays");
    PEDP_TRY(pedp_download(c, out_pts, d_out, sizeof(double) * 3 * (size_t)m));
    if (normals) PEDP_TRY(pedp_download(c, out_normals, d_outn, sizeof(double) * 3 * (size_t)m));
    PEDP_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PEDP_OK;
}

int pedp_voxel_down_sample(pedp_ctx_t c, const double *pts, const double *normals, int64_t N, double voxel_size,
                           double *out_pts, double *out_normals, int64_t capacity, int64_t *n_out) {
    return voxel_down_sample_impl(c, pts, normals, N, voxel_size, out_pts, out_normals, capacity, n_out, false);
}

int pedp_voxel_down_sample_device_in(pedp_ctx_t c, const double *d_pts, int64_t N, double voxel_size, double *out_pts,
                                     int64_t capacity, int64_t *n_out) {
    return voxel_down_sample_impl(c, d_pts, nullptr, N, voxel_size, out_pts, nullptr, capacity, n_out, true);
}

int pedp_cluster_dbscan(pedp_ctx_t c, const double *pts, int64_t N, double eps, int min_points, int32_t *labels) {
    PEDP_TRY(check_cloud(c, pts, N, "pedp_cluster_dbscan"));
    PEDP_REQUIRE(eps > 0.0 && std::isfinite(eps), "pedp_cluster_dbscan: eps must be positive and finite");
    if (N == 0) return PEDP_OK;
    PEDP_REQUIRE(labels, "pedp_cluster_dbscan: null labels");
    double lo[3], hi[3];
    PEDP_REQUIRE(bounds(pts, N, lo, hi), "pedp_cluster_dbscan: non-finite coordinates");
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    double *d_pts = nullptr;
    PEDP_TRY(upload_in(c, pts, nullptr, N, &d_pts, nullptr));
    int32_t *d_labels = nullptr;
    PEDP_TRY(dbscan_core(c, d_pts, N, eps, min_points, lo, hi, &d_labels));
    PEDP_TRY(pedp_download(c, labels, d_labels, sizeof(int32_t) * (size_t)N));
    PEDP_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PEDP_OK;
}

int pedp_knn_mean_distance(pedp_ctx_t c, const double *pts, int64_t N, int k, double *avg) {
    PEDP_TRY(check_cloud(c, pts, N, "pedp_knn_mean_distance"));
    PEDP_REQUIRE(k >= 1 && k <= 300, "pedp_knn_mean_distance: k must be in 1..300");  // k x 64 doubles of LDS per workgroup
    if (N == 0) return PEDP_OK;
    PEDP_REQUIRE(avg, "pedp_knn_mean_distance: null output");
    double lo[3], hi[3];
    PEDP_REQUIRE(bounds(pts, N, lo, hi), "pedp_knn_mean_distance: non-finite coordinates");  // (N <= KNN_SMALL_MAX takes no grid)
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    double *d_pts = nullptr;
    PEDP_TRY(upload_in(c, pts, nullptr, N, &d_pts, nullptr));
    double *d_avg = nullptr;
    PEDP_TRY(knn_core(c, d_pts, N, k, lo, hi, &d_avg));
    PEDP_TRY(pedp_download(c, avg, d_avg, sizeof(double) * (size_t)N));
    PEDP_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PEDP_OK;
}

int pedp_estimate_normals(pedp_ctx_t c, const double *pts, int64_t N, double radius, int max_nn, const double *prior,
                          double *normals) {
    PEDP_TRY(check_cloud(c, pts, N, "pedp_estimate_normals"));
    PEDP_REQUIRE(radius > 0.0 && std::isfinite(radius), "pedp_estimate_normals: radius must be positive and finite");
    PEDP_REQUIRE(max_nn >= 1 && max_nn <= 128, "pedp_estimate_normals: max_nn must be in 1..128");
    if (N == 0) return PEDP_OK;
    PEDP_REQUIRE(normals, "pedp_estimate_normals: null output");
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    double lo[3], hi[3], *d_pts = nullptr, *d_prior = nullptr;
    SmallBlock *sb = nullptr;
    PEDP_TRY(upload_in(c, pts, prior, N, &d_pts, &d_prior));
    if (N >= BND_DEVICE_MIN) PEDP_TRY(small_block(c, &sb));
    PEDP_TRY(box_of(c, pts, d_pts, N, sb ? sb->part : nullptr, lo, hi));  // (a NaN box: normals_core's grid refuses)
    double *d_out = nullptr;
    PEDP_TRY(normals_core(c, d_pts, N, radius, max_nn, d_prior, lo, hi, &d_out));
    PEDP_TRY(pedp_download(c, normals, d_out, sizeof(double) * 3 * (size_t)N));
    PEDP_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PEDP_OK;
}

int pedp_fpfh(pedp_ctx_t c, const double *pts, const double *normals, int64_t N, double radius, int max_nn, double *out) {
    PEDP_TRY(check_cloud(c, pts, N, "pedp_fpfh"));
    PEDP_REQUIRE(radius > 0.0 && std::isfinite(radius), "pedp_fpfh: radius must be positive and finite");
    PEDP_REQUIRE(max_nn >= 1 && max_nn <= 128, "pedp_fpfh: max_nn must be in 1..128");
    if (N == 0) return PEDP_OK;
    PEDP_REQUIRE(normals && out, "pedp_fpfh: null normals / output (FPFH needs the cloud's normals)");
    PEDP_REQUIRE(N * (int64_t)max_nn < (int64_t)1 << 31, "pedp_fpfh: neighbour table too large");
    double lo[3], hi[3], *d_in = nullptr;
    PEDP_TRY(bounds_of(c, pts, N, lo, hi, &d_in));
    Grid g;
    int64_t n_cells = 0;
    PEDP_TRY(make_grid(lo, hi, radius * (1.0 + 1e-9), g, n_cells, "pedp_fpfh"));
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    const unsigned n = (unsigned)N;
    size_t tmp_sort = 0;
    PEDP_ROCPRIM(rocprim::radix_sort_pairs(nullptr, tmp_sort, (unsigned *)nullptr, (unsigned *)nullptr, (int *)nullptr,
                                           (int *)nullptr, n, 0, 32, c->stream));
    const size_t need = a256(sizeof(double) * 3 * N) * 3 + a256(sizeof(unsigned) * N) * 2 + a256(sizeof(int) * N) * 3 +
                        a256(sizeof(int) * n_cells) * 2 + a256(tmp_sort) + a256(sizeof(int) * (size_t)N * max_nn) +
                        a256(sizeof(double) * (size_t)N * max_nn) + a256(sizeof(double) * 33 * N) * 2 + 8192;
    PEDP_TRY(c->ops.reserve(need));
    Carver cv{(char *)c->ops.ptr};
    double *d_pts = cv.take<double>(3 * (size_t)N), *sp = cv.take<double>(3 * (size_t)N), *d_nrm = cv.take<double>(3 * (size_t)N);
    unsigned *cell_id = cv.take<unsigned>(N), *cell_s = cv.take<unsigned>(N);
    int *val = cv.take<int>(N), *val_s = cv.take<int>(N), *nbr_n = cv.take<int>(N);
    int *cell_start = cv.take<int>(2 * (size_t)n_cells), *cell_end = cell_start + n_cells;
    void *d_tmp = cv.take<char>(tmp_sort);
    int *nbr_j = cv.take<int>((size_t)N * max_nn);
    double *nbr_d = cv.take<double>((size_t)N * max_nn);
    double *spfh = cv.take<double>(33 * (size_t)N), *d_out = cv.take<double>(33 * (size_t)N);
    if (d_in) d_pts = d_in;  // already up (bounds_of)
    else PEDP_TRY(pedp_upload(c, d_pts, pts, sizeof(double) * 3 * (size_t)N));
    PEDP_TRY(pedp_upload(c, d_nrm, normals, sizeof(double) * 3 * (size_t)N));
    PEDP_HIP_CHECK(hipMemsetAsync(cell_start, 0, sizeof(int) * 2 * (size_t)n_cells, c->stream));
    const unsigned grid = (unsigned)((N + 255) / 256), grid64 = (unsigned)((N + NRM_THREADS - 1) / NRM_THREADS);
    hipLaunchKernelGGL(grid_cell_kernel, dim3(grid), dim3(256), 0, c->stream, d_pts, N, g, cell_id, val);
    PEDP_ROCPRIM(rocprim::radix_sort_pairs(d_tmp, tmp_sort, cell_id, cell_s, val, val_s, n, 0, 32, c->stream));
    hipLaunchKernelGGL(grid_ranges_kernel, dim3(grid), dim3(256), 0, c->stream, cell_s, val_s, d_pts, N, cell_start, cell_end, sp);
    // a wave per query, 1,024 candidates each; a denser neighbourhood somewhere sends the cloud to the 4,096-candidate
    // instantiation and, past that, to the thread-per-query kernel
    int *d_over = cv.take<int>(64), h_over = 0;
    for (int attempt = 0; attempt < 3; ++attempt) {
        PEDP_HIP_CHECK(hipMemsetAsync(d_over, 0, sizeof(int), c->stream));
        if (attempt == 0)
            hipLaunchKernelGGL((hybrid_list_wave_kernel<1024, 4>), dim3((unsigned)((N + 3) / 4)), dim3(256), 0, c->stream, g, sp, N,
                               cell_start, cell_end, val_s, radius * radius, max_nn, nbr_j, nbr_d, nbr_n, d_over);
        else if (attempt == 1)
            hipLaunchKernelGGL((hybrid_list_wave_kernel<4096, 2>), dim3((unsigned)((N + 1) / 2)), dim3(128), 0, c->stream, g, sp, N,
                               cell_start, cell_end, val_s, radius * radius, max_nn, nbr_j, nbr_d, nbr_n, d_over);
        else {
            const size_t lds = (sizeof(double) + sizeof(int)) * (size_t)max_nn * NRM_THREADS;
            PEDP_HIP_CHECK(hipFuncSetAttribute((const void *)hybrid_list_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(hybrid_list_kernel, dim3(grid64), dim3(NRM_THREADS), lds, c->stream, g, sp, N, cell_start, cell_end,
                               val_s, radius * radius, max_nn, nbr_j, nbr_d, nbr_n);
        }
        PEDP_HIP_CHECK(hipGetLastError());
        PEDP_HIP_CHECK(hipMemcpyAsync(&h_over, d_over, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        PEDP_HIP_CHECK(hipStreamSynchronize(c->stream));
        if (!h_over) break;
    }
    hipLaunchKernelGGL(spfh_kernel, dim3(grid64), dim3(NRM_THREADS), 0, c->stream, d_pts, d_nrm, N, nbr_j, nbr_n, spfh);
    hipLaunchKernelGGL(fpfh_kernel, dim3(grid64), dim3(NRM_THREADS), 0, c->stream, N, nbr_j, nbr_d, nbr_n, spfh, d_out);
    PEDP_HIP_CHECK(hipGetLastError());
    PEDP_TRY(pedp_download(c, out, d_out, sizeof(double) * 33 * (size_t)N));
    PEDP_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PEDP_OK;
}

int pedp_feature_match(pedp_ctx_t c, const double *fs, int64_t Ns, const double *ft, int64_t Nt, int32_t *idx) {
    PEDP_REQUIRE(c, "pedp_feature_match: null context");
    PEDP_REQUIRE(Ns >= 0 && Nt >= 0 && Ns < (int64_t)1 << 31 && Nt < (int64_t)1 << 31, "pedp_feature_match: sizes out of range");
    if (Ns == 0) return PEDP_OK;
    PEDP_REQUIRE(fs && idx && (ft || Nt == 0), "pedp_feature_match: null arrays");
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    const int n_chunks = (int)((Nt + FM_CHUNK - 1) / FM_CHUNK > 0 ? (Nt + FM_CHUNK - 1) / FM_CHUNK : 1);
    PEDP_REQUIRE(n_chunks <= 65535, "pedp_feature_match: more than 67 M target features");
    PEDP_TRY(c->ops.reserve(a256(sizeof(double) * 33 * Ns) + a256(sizeof(double) * 33 * (Nt > 0 ? Nt : 1)) + a256(sizeof(int32_t) * Ns) +
                            a256(sizeof(double) * (size_t)n_chunks * Ns) + a256(sizeof(int32_t) * (size_t)n_chunks * Ns) + 1024));
    Carver cv{(char *)c->ops.ptr};
    double *d_fs = cv.take<double>(33 * (size_t)Ns), *d_ft = cv.take<double>(33 * (size_t)(Nt > 0 ? Nt : 1));
    int32_t *d_idx = cv.take<int32_t>(Ns);
    double *part_d = cv.take<double>((size_t)n_chunks * Ns);
    int32_t *part_j = cv.take<int32_t>((size_t)n_chunks * Ns);
    PEDP_TRY(pedp_upload(c, d_fs, fs, sizeof(double) * 33 * (size_t)Ns));
    if (Nt > 0) PEDP_TRY(pedp_upload(c, d_ft, ft, sizeof(double) * 33 * (size_t)Nt));
    hipLaunchKernelGGL(feature_match_kernel, dim3((unsigned)((Ns + 63) / 64), (unsigned)n_chunks), dim3(64), 0, c->stream, d_fs, Ns,
                       d_ft, Nt, part_d, part_j);
    hipLaunchKernelGGL(feature_match_fold_kernel, dim3((unsigned)((Ns + 255) / 256)), dim3(256), 0, c->stream, Ns, n_chunks,
                       (const double *)part_d, (const int32_t *)part_j, d_idx);
    PEDP_HIP_CHECK(hipGetLastError());
    PEDP_TRY(pedp_download(c, idx, d_idx, sizeof(int32_t) * (size_t)Ns));
    PEDP_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PEDP_OK;
}

int pedp_segment_plane(pedp_ctx_t c, const double *pts, int64_t N, double distance_threshold, int num_iterations,
                       uint64_t seed, double plane[4], int32_t *inliers, int64_t *n_inliers) {
    PEDP_TRY(check_cloud(c, pts, N, "pedp_segment_plane"));
    PEDP_REQUIRE(plane && n_inliers, "pedp_segment_plane: null outputs");
    PEDP_REQUIRE(num_iterations >= 0 && num_iterations <= RS_MAX_ITERATIONS, "pedp_segment_plane: num_iterations out of range (0..%d)",
                 RS_MAX_ITERATIONS);
    plane[0] = plane[1] = plane[2] = plane[3] = 0.0;
    *n_inliers = 0;
    if (N > 0) {  // no box is taken here: the same host pass, for its flag alone
        double lo[3], hi[3];
        PEDP_REQUIRE(bounds(pts, N, lo, hi), "pedp_segment_plane: non-finite coordinates");
    }
    if (N < 3 || num_iterations == 0) return PEDP_OK;
    PEDP_REQUIRE(inliers, "pedp_segment_plane: null inlier array");
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    double *d_pts = nullptr;
    PEDP_TRY(upload_in(c, pts, nullptr, N, &d_pts, nullptr));
    int best_t = -1;
    double best[4];
    PEDP_TRY(plane_best_core(c, d_pts, N, distance_threshold, num_iterations, seed, &best_t, best));
    if (best_t < 0) return PEDP_OK;
    int64_t n = 0;
    for (int64_t i = 0; i < N; ++i)
        if (plane_dist(best, pts + 3 * i) < distance_threshold) inliers[n++] = (int32_t)i;
    plane_from_points(pts, inliers, n, plane);
    *n_inliers = n;
    return PEDP_OK;
}

// ------------------------------------------------------------------ preprocess_source, device resident
// The reference's scene preprocessing (src/pose_estimation.py:186-268, the branch without param['box'] /
// param['mesh'] / background): voxel grid -> table plane by RANSAC -> [normals of the down-sampled cloud] ->
// plane removed -> DBSCAN, largest cluster -> statistical outlier filter -> [normals, oriented like the first
// ones].  The same kernels as the single operations above, chained on the device: what crosses PCIe is the
// input cloud (if it is not on the device already), the counters of the voxel grid and the selections, partial
// bounds, the mean neighbour distances of the largest cluster (the host sets the outlier limit), the refit plane and
// the voxel means of the normals where someone reads them, and the processed cloud; the best plane and the cluster
// labels stay on the device.  The stages are the functions above.  Results are bit for bit those of the step-by-step
// calls.
int pedp_preprocess_source(pedp_ctx_t c, const double *pts, int64_t N, int pts_on_device, const pedp_preprocess_params *prm,
                           double *out_pts, double *out_normals, int64_t capacity, int64_t *n_out, int64_t stage_counts[4],
                           int *status) {
    return pedp_preprocess_source_ex(c, pts, N, pts_on_device, prm, out_pts, out_normals, capacity, n_out, stage_counts, status, nullptr);
}

int pedp_preprocess_source_ex(pedp_ctx_t c, const double *pts, int64_t N, int pts_on_device, const pedp_preprocess_params *prm,
                              double *out_pts, double *out_normals, int64_t capacity, int64_t *n_out, int64_t stage_counts[4],
                              int *status, double report[PEDP_PREPROCESS_REPORT_DOUBLES]) {
    PEDP_TRY(check_cloud(c, pts, N, "pedp_preprocess_source"));
    PEDP_REQUIRE(prm && n_out && status && out_pts, "pedp_preprocess_source: null argument");
    PEDP_REQUIRE(prm->voxel_size > 0.0, "pedp_preprocess_source: voxel_size <= 0");
    PEDP_REQUIRE(prm->plane_iterations >= 1 && prm->plane_iterations <= RS_MAX_ITERATIONS,
                 "pedp_preprocess_source: plane_iterations out of range (1..%d)", RS_MAX_ITERATIONS);
    PEDP_REQUIRE(prm->cluster_eps > 0.0 && std::isfinite(prm->cluster_eps), "pedp_preprocess_source: cluster_eps must be positive");
    PEDP_REQUIRE(prm->outlier_neighbors >= 1 && prm->outlier_neighbors <= 300, "pedp_preprocess_source: outlier_neighbors must be in 1..300");
    PEDP_REQUIRE(!prm->first_frame || (prm->normal_radius > 0.0 && prm->normal_max_nn >= 1 && prm->normal_max_nn <= 128 && out_normals),
                 "pedp_preprocess_source: normals (first frame) need a radius, max_nn in 1..128 and an output array");
    *n_out = 0;
    *status = PEDP_PREPROCESS_OK;
    if (stage_counts) stage_counts[0] = stage_counts[1] = stage_counts[2] = stage_counts[3] = 0;
    if (N < 3) { *status = PEDP_PREPROCESS_DEGENERATE; return PEDP_OK; }
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    const bool nrm = prm->first_frame != 0;
    const bool box = (prm->flags & PEDP_PREPROCESS_BOX) != 0;
    const bool seen = box || report != nullptr;  // someone reads the refit plane and the average normal (box cut / INFO lines)
    const bool carry = nrm && !box;              // remove_points_below_plane returns points only (:375-377)
    const double avg_voxel = prm->average_normal_voxel > 0.0 ? prm->average_normal_voxel : 10.0;
    if (report) for (int k = 0; k < PEDP_PREPROCESS_REPORT_DOUBLES; ++k) report[k] = 0.0;
    Chain ch;
    ch.report = report;
    double *d_in = const_cast<double *>(pts);
    if (!pts_on_device) PEDP_TRY(upload_in(c, pts, nullptr, N, &d_in, nullptr));
    // ---- voxel grid
    double *v_pts = nullptr, *v_nrm = nullptr;
    int64_t m1 = 0;
    PEDP_TRY(voxel_core(c, d_in, nullptr, N, prm->voxel_size, &v_pts, &v_nrm, &m1, ch.box_lo, ch.box_hi, "pedp_preprocess_source"));
    if (stage_counts) stage_counts[0] = m1;
    if (m1 < 3) { *status = PEDP_PREPROCESS_DEGENERATE; return PEDP_OK; }
    PEDP_TRY(chain_reserve(c, m1, ch));
    PEDP_HIP_CHECK(hipMemcpyAsync(ch.A_pts, v_pts, sizeof(double) * 3 * (size_t)m1, hipMemcpyDeviceToDevice, c->stream));
    // ---- table plane: the best of the sampled planes, kept on the device (sb->best: untouched by the stages between)
    int best_t = -1;
    double best[4] = {0, 0, 0, 0};
    PEDP_TRY(plane_best_core(c, ch.A_pts, m1, prm->plane_distance, prm->plane_iterations, prm->seed, &best_t, best, ch.sb->best));
    // ---- someone reads the plane segment_plane returns (the best plane refit over its inliers): refit on the device,
    // behind the plane kernels; the result is picked up after the stream's next wait (refit_collect)
    if (seen) {
        PEDP_TRY(refit_core(c, ch.A_pts, m1, ch.sb->best, prm->plane_distance, ch.sb->refit, pedp_pinned_at<double>(c, pedp_pinned::REFIT)));
        ch.refit_pending = true;
    }
    // ---- normals of the down-sampled cloud (they orient the final ones)
    if (nrm) {
        double *n_out_d = nullptr;
        PEDP_TRY(normals_core(c, ch.A_pts, m1, prm->normal_radius, prm->normal_max_nn, nullptr, ch.box_lo, ch.box_hi, &n_out_d));
        PEDP_HIP_CHECK(hipMemcpyAsync(ch.A_nrm, n_out_d, sizeof(double) * 3 * (size_t)m1, hipMemcpyDeviceToDevice, c->stream));
    }
    // ---- compute_average_normal (:314-321): the normals' voxel averages on a 10-unit grid, their mean in row order
    // (numpy's reduction over axis 0 adds row by row).  The caller normalises it -- numpy's norm is the caller's.
    // Enqueued here, picked up after the stream's next wait (average_collect).
    if (seen && nrm) {
        PEDP_TRY(average_normal_core(c, ch.A_pts, ch.A_nrm, m1, avg_voxel, ch.box_lo, ch.box_hi, ch.sb,
                                     pedp_pinned_at<double>(c, pedp_pinned::AVERAGE_NORMAL), &ch.avg_pending));
        if (!ch.avg_pending) PEDP_TRY(average_by_sort(c, ch, m1, avg_voxel));
    }
    // ---- the table removed: the half space below the plane (box) or the plane's inliers
    int64_t m2 = m1;
    if (box) {
        PEDP_HIP_CHECK(hipStreamSynchronize(c->stream));
        PEDP_TRY(average_collect(c, ch, m1, avg_voxel));
        refit_collect(c, ch);
        PEDP_TRY(halfspace_flags(c, ch, m1, nrm, status));
        if (*status != PEDP_PREPROCESS_OK) return PEDP_OK;
    } else {  // (no plane found: nothing removed, like select_by_index of an empty list)
        hipLaunchKernelGGL(plane_keep_best_kernel, dim3((unsigned)((m1 + 255) / 256)), dim3(256), 0, c->stream, ch.A_pts, m1,
                           (const double *)ch.sb->best, prm->plane_distance, ch.flag);
    }
    PEDP_TRY(select_core(c, ch.A_pts, carry ? ch.A_nrm : nullptr, m1, ch.flag, ch.B_pts, ch.B_nrm, &m2));
    PEDP_TRY(average_collect(c, ch, m1, avg_voxel));  // (select_core has waited for the stream)
    refit_collect(c, ch);
    if (report) for (int k = 0; k < 3; ++k) report[4 + k] = ch.avg[k];
    if (stage_counts) stage_counts[1] = m2;
    if (m2 == 0) { *status = PEDP_PREPROCESS_NO_CLUSTER; return PEDP_OK; }
    // ---- DBSCAN, largest cluster
    int64_t m3 = 0;
    PEDP_TRY(largest_cluster_flags(c, ch, m2, prm));
    PEDP_TRY(select_core(c, ch.B_pts, carry ? ch.B_nrm : nullptr, m2, ch.flag, ch.C_pts, ch.C_nrm, &m3));
    if (stage_counts) stage_counts[2] = m3;
    if (m3 == 0) { *status = PEDP_PREPROCESS_NO_CLUSTER; return PEDP_OK; }  // every label was noise
    // ---- statistical outlier filter
    int64_t m4 = 0;
    bool any = false;
    PEDP_TRY(outlier_flags(c, ch, m3, prm, &any));
    if (any) PEDP_TRY(select_core(c, ch.C_pts, carry ? ch.C_nrm : nullptr, m3, ch.flag, ch.A_pts, ch.A_nrm, &m4));
    if (stage_counts) stage_counts[3] = m4;
    *n_out = m4;
    PEDP_REQUIRE(m4 <= capacity, "pedp_preprocess_source: %lld points exceed the output capacity %lld", (long long)m4, (long long)capacity);
    if (m4 == 0) return PEDP_OK;
    // ---- normals of the processed cloud, oriented like the ones it carries
    if (nrm) {
        double lo[3], hi[3], *n_fin = nullptr;
        PEDP_TRY(bounds_device(c, ch.A_pts, m4, ch.sb->part, lo, hi));
        PEDP_TRY(normals_core(c, ch.A_pts, m4, prm->normal_radius, prm->normal_max_nn, carry ? ch.A_nrm : nullptr, lo, hi, &n_fin));
        PEDP_TRY(pedp_download(c, out_normals, n_fin, sizeof(double) * 3 * (size_t)m4));
    }
    PEDP_TRY(pedp_download(c, out_pts, ch.A_pts, sizeof(double) * 3 * (size_t)m4));
    PEDP_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PEDP_OK;
}

}  // extern "C"


// the 64-bit key sort's entry points (pedp_internal.h; "The 64-bit key sort" above)
int pedp_sort_keys64_begin(pedp_ctx_t c, int64_t N, int bits, unsigned long long **d_keys) {
    return sort64_begin(c, N, sort_plan(N, bits), d_keys);
}
int pedp_sort_keys64_run(pedp_ctx_t c, int64_t N, int bits, int32_t *d_perm) { return sort64_run(c, N, sort_plan(N, bits), d_perm); }
int pedp_sort_keys64_exact_begin(pedp_ctx_t c, int64_t N, int bits, unsigned long long **d_keys) {
    return sort64_begin(c, N, sort_plan_exact(N, bits), d_keys);
}
int pedp_sort_keys64_exact_run(pedp_ctx_t c, int64_t N, int bits, int32_t *d_perm) {
    return sort64_run(c, N, sort_plan_exact(N, bits), d_perm);
}
