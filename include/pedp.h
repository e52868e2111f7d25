/*
 * pedp.h -- C ABI of libpedp_hip.so: the MI355X (gfx950) implementation of the
 * reference's geometric hot path, behind plain pointers and sizes.
 *
 * The reference binds no FFI on this path today: both stages are Python calls into
 * the Open3D wheel.  Each entry point below names the reference call it replaces
 * (paths relative to the reference repository); INTEGRATION.md shows the ctypes
 * stub a maintainer adds on the reference side.  The library occupies the
 * reference's native-extension slot (import-with-fallback convention of
 * Utils.py:41-57, where mycpp and bundlesdf.mycuda are loaded) and additionally
 * exports cluster_poses so estimater.py:118 keeps working without mycpp.
 *
 * Conventions
 *   - every function returns PEDP_OK (0) or a negative pedp_status; the message of
 *     the last failure on the calling thread is pedp_last_error().
 *   - `mem` arguments: PEDP_HOST = the array pointers are host memory (the call
 *     copies, runs, copies back and returns after completion); PEDP_DEVICE = they
 *     are device memory on the context's GPU (the call only enqueues work on the
 *     context's stream; use pedp_ctx_synchronize or the stream to wait).
 *   - the callee never frees or retains caller arrays; handles own device copies.
 *   - one context = one device + one HIP stream; a context is not thread-safe,
 *     different contexts are independent.
 */
#ifndef PEDP_H
#define PEDP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    PEDP_OK = 0,
    PEDP_ERR_BAD_ARG = -1,
    PEDP_ERR_NO_NORMALS = -2, /* point-to-plane needs target normals (Open3D raises) */
    PEDP_ERR_HIP = -3,
    PEDP_ERR_ALLOC = -4,
    PEDP_ERR_COLLECTIVE = -5 /* the caller's all-reduce hook or an RCCL call failed */
} pedp_status;

enum { PEDP_HOST = 0, PEDP_DEVICE = 1 };
enum { PEDP_POINT_TO_PLANE = 0, PEDP_POINT_TO_POINT = 1 };

typedef struct pedp_ctx_s *pedp_ctx_t;
typedef struct pedp_mesh_s *pedp_mesh_t;
typedef struct pedp_rayset_s *pedp_rayset_t;
typedef struct pedp_cloud_s *pedp_cloud_t;

int pedp_version(void);
const char *pedp_last_error(void);
int pedp_device_count(int *count);

/* stream: a hipStream_t the caller owns (e.g. torch.cuda.current_stream().cuda_stream),
 * or NULL to let the context create its own. */
int pedp_ctx_create(int device, void *stream, pedp_ctx_t *out);
void pedp_ctx_destroy(pedp_ctx_t ctx);
int pedp_ctx_synchronize(pedp_ctx_t ctx);

/* ---------------------------------------------------------------- ray projection
 * Replaces src/defect_projection.py:245-256:
 *     t_mesh = o3d.t.geometry.TriangleMesh.from_legacy(mesh)        -> pedp_mesh_create
 *     scene = o3d.t.geometry.RaycastingScene(); scene.add_triangles(t_mesh)
 *     intersections = scene.cast_rays(o3d_rays)                     -> pedp_raycast
 * verts: V x 3 float32 (from_legacy's cast), tris: F x 3 uint32, both host memory.
 */
int pedp_mesh_create(pedp_ctx_t ctx, const float *verts, int64_t V, const uint32_t *tris,
                     int64_t F, pedp_mesh_t *out);
void pedp_mesh_destroy(pedp_mesh_t mesh);
int pedp_mesh_size(pedp_mesh_t mesh, int64_t *V, int64_t *F);

/* cast_rays: rays6 = N x [ox oy oz dx dy dz] float32 (directions are used as given,
 * not re-normalised; tnear = 0, tfar = +inf, no culling).  Outputs, all length N:
 * t_hit (+inf on miss), prim_id (0xFFFFFFFF on miss), uv (N x 2, nullable; 0 on miss).
 * Closest hit; ties: smaller t, then smaller triangle index. */
int pedp_raycast(pedp_ctx_t ctx, pedp_mesh_t mesh, const float *rays6, int64_t N, int mem,
                 float *t_hit, uint32_t *prim_id, float *uv);

/* Tuning knobs of the sweep (0 = keep default): triangle chunks per ray block
 * (multiple of 8: chunk c is served by XCD c % 8) and sweep variant:
 *   0 auto (2 below 16,384 rays, else 4; 3 for a ray count whose last variant-4 cast had to be
 *     completed by the exhaustive sweep)
 *   1 every ray against every triangle: rays of one origin on the matrix pipe (bf16 MFMA filter with a proven
 *     slack, the exact test on the pairs that pass it), other rays on the packed fp32 loop of variant 5
 *   2 triangle-per-lane with a wavefront-wide min-t reduction
 *   3 ray-per-lane with conservative cluster culling when all rays share one origin
 *     (falls back to 1 on the device otherwise)
 *   4 triangle-driven: rays of one origin threaded into a grid of directions, every triangle
 *     tested against the rays in the cells its image covers (completed by 1 on the device when
 *     the rays do not share an origin, leave the grid's half space or crowd a cell).
 *   5 every ray against every triangle on the vector pipe (ray per lane, packed fp32; round 3's exhaustive kernel)
 * All variants return identical bits. */
int pedp_raycast_configure(pedp_ctx_t ctx, int tri_chunks, int variant);
/* A camera's rays as a resident object.  A camera sends the same rays every frame (the reference generates them from the
 * pixel grid in the camera's frame and moves the MESH, src/defect_projection.py:196-223, :549-550): a ray set copies
 * the N x 6 float32 [origin | direction] rows once and builds, once, what the triangle-driven ray stage (variant 4)
 * derives from the rays alone -- the frame, the grid over the mapped directions, the cells' chains.  A cast against a
 * ray set is then the triangle kernels and the result kernel only: four launches, the rays never re-read
 * (pedp_raycast reads them twice and rebuilds the chains per call).  Results are those of pedp_raycast, bit for bit;
 * rays the grid cannot serve (origins that differ, directions outside the frame's half space, crowded cells) are cast
 * by pedp_raycast's other variants from the resident copy.  mem: where rays6 / the outputs live. */
int pedp_rayset_create(pedp_ctx_t ctx, const float *rays6, int64_t N, int mem, pedp_rayset_t *out);
void pedp_rayset_destroy(pedp_rayset_t rays);
int pedp_raycast_rayset(pedp_ctx_t ctx, pedp_mesh_t mesh, pedp_rayset_t rays, int mem, float *t_hit, uint32_t *prim_id, float *uv);
/* how the last cast against the set was answered: *variant 4 (the grid) with *grid_status 0, or the variant
 * pedp_raycast fell back to with the reason the grid gave (bits as in pedp_raycast_last_variant) */
int pedp_rayset_last_variant(pedp_rayset_t rays, int *variant, int *grid_status);

/* Diagnostics of variant 1's matrix-pipe filter (tests): for N host rays of ONE origin, the filter's score of every (ray,
 * triangle) pair -- >= 0: the pair goes to the exact test -- and the slack inside that score; N x F float32 each, host. */
int pedp_debug_mfma_scores(pedp_ctx_t ctx, pedp_mesh_t mesh, const float *rays6, int64_t N, float *score, float *slack);

/* Which variant the last pedp_raycast of this context ran and, for variant 4, whether the grid
 * answered the cast (grid_status 0) or the exhaustive sweep had to (bit 0 origins differ, 1 a ray
 * outside the half space, 2 a crowded cell, 3 item table full).  Synchronises the stream. */
int pedp_raycast_last_variant(pedp_ctx_t ctx, int *variant, int *grid_status);
/* Diagnostics of the triangle-driven ray stage, for the tests that MEASURE its margin: runs a variant-4 cast of the N
 * host rays; tri_out = F x 12 floats per triangle [live, every-cell, fx0, fx1, fy0, fy1: the bounding rectangle of its
 * mapped corners in cell units before widening, mx, my: the margins, x0, x1, y0, y1: the cells visited]; ray_out = N x 3
 * [kind (1 = mapped), continuous cell coordinate x, y]; grid = [GX, GY, grid_status]. */
int pedp_debug_rast_rects(pedp_ctx_t ctx, pedp_mesh_t mesh, const float *rays6, int64_t N, float *tri_out, float *ray_out,
                          int *grid);

/* Milliseconds the last pedp_raycast spent in its sweep stage -- for variant 4 the bounds, chain, triangle
 * and tile kernels, for variant 3 the direction binning, cull masks, segment table and the sweep itself (HIP events on the context's stream,
 * around everything between the operand set-up and the final t / id / uv write-out);
 * synchronises on the second event. */
int pedp_raycast_last_sweep_ms(pedp_ctx_t ctx, float *ms);

/* ---------------------------------------------------------------- all-hits queries
 * RaycastingScene.count_intersections / test_occlusions / list_intersections on the mesh handle.  A ray intersects a
 * triangle exactly when the cast's own test accepts the pair (edges inclusive: a ray through a shared edge intersects
 * both triangles); its t is the float32 quotient the cast forms, its (u, v) the cast's.  Rays with a zero, NaN or
 * infinite direction intersect nothing.  rays6, N, mem as in pedp_raycast; N = 0 does nothing (a list: ray_splits[0] =
 * 0, total 0); a mesh without triangles, or N >= 2^31 - 16, is PEDP_ERR_BAD_ARG.  The _rayset forms take a resident ray
 * set in the place of rays6, N.  Path: pedp_raycast_configure's variant -- 0: the grid of variant 4 from 16,384 rays on
 * and for a ray set (the exhaustive path once a query's grid pass has given up on those rays), 4: the grid, 1, 2, 3,
 * 5: every ray against every triangle.  Rays the grid cannot hold are completed exhaustively on the device in the same
 * call.  Every path gives identical bits.  The casts' state (a ray set's keys, the grid's headers, the casts' status
 * words and automatic variant choice) is left as a cast expects it.
 *
 * counts: int32 per ray, the number of intersecting triangles. */
int pedp_count_intersections(pedp_ctx_t ctx, pedp_mesh_t mesh, const float *rays6, int64_t N, int mem, int32_t *counts);
int pedp_count_intersections_rayset(pedp_ctx_t ctx, pedp_mesh_t mesh, pedp_rayset_t rays, int mem, int32_t *counts);
/* occluded: one byte per ray, 1 when an intersecting triangle has tnear <= t <= tfar (float32 compare, both ends
 * inclusive; a NaN bound gives 0), else 0. */
int pedp_test_occlusions(pedp_ctx_t ctx, pedp_mesh_t mesh, const float *rays6, int64_t N, int mem, float tnear, float tfar,
                         uint8_t *occluded);
int pedp_test_occlusions_rayset(pedp_ctx_t ctx, pedp_mesh_t mesh, pedp_rayset_t rays, int mem, float tnear, float tfar,
                                uint8_t *occluded);
/* Every intersection: ray_splits (N + 1; ray i owns entries ray_splits[i] .. ray_splits[i + 1] - 1), and per entry ray_ids,
 * t_hit, prim_ids, uvs (x 2).  Within a ray the entries are ordered by t, then by triangle index -- the order of the
 * cast's key, so a ray's first entry is its pedp_raycast result bit for bit.  The outputs hold `capacity` entries;
 * *total (host) is always reported and ray_splits always complete; if total > capacity nothing else is written and the
 * call returns PEDP_ERR_BAD_ARG, like pedp_project_heatmap.  The call waits for the stream once (total sizes the rest). */
int pedp_list_intersections(pedp_ctx_t ctx, pedp_mesh_t mesh, const float *rays6, int64_t N, int mem, int64_t capacity,
                            int64_t *ray_splits, int64_t *ray_ids, float *t_hit, uint32_t *prim_ids, float *uvs, int64_t *total);
int pedp_list_intersections_rayset(pedp_ctx_t ctx, pedp_mesh_t mesh, pedp_rayset_t rays, int mem, int64_t capacity,
                                   int64_t *ray_splits, int64_t *ray_ids, float *t_hit, uint32_t *prim_ids, float *uvs,
                                   int64_t *total);
/* How the last all-hits query of this context was answered: *path 4 (the grid; *grid_status 0, or why the exhaustive
 * completion had to answer instead, bits as in pedp_raycast_last_variant) or 1 (every ray against every triangle).
 * Synchronises the stream. */
int pedp_intersections_last_path(pedp_ctx_t ctx, int *path, int *grid_status);

/* ---------------------------------------------------------------- fused defect projection
 * the per-frame work around cast_rays moved onto the device.
 *
 * Posable mesh.  Replaces the per-frame `copy.deepcopy(mesh)` + `mesh.transform(T)` +
 * `TriangleMesh.from_legacy(mesh)` chain (src/pose_estimation.py:406-409,
 * src/defect_projection.py:549-550, :245; poses composed in run.py:95-119): the model-frame
 * float64 vertices stay resident, pedp_mesh_set_pose forms T * (x, y, z, 1) in float64 (fixed
 * operation order), divides by the fourth component, casts to float32 and rebuilds the triangle
 * records and culling spheres on the device.  T: row-major 4x4 float64 on the host, NULL =
 * identity.  set_pose only enqueues work on the context's stream. */
int pedp_mesh_create_posable(pedp_ctx_t ctx, const double *verts, int64_t V, const uint32_t *tris,
                             int64_t F, pedp_mesh_t *out);
int pedp_mesh_set_pose(pedp_mesh_t mesh, const double T[16]);
/* transform_object(reader.target_mesh, T) (src/pose_estimation.py:406-409; run.py:109-110, :179-181) for the viewer's
 * copy of the mesh: the V x 3 float64 vertices T * (x, y, z, 1) / w of a posable mesh's model, the arithmetic
 * pedp_mesh_set_pose starts from, before the float32 cast.  The mesh's own pose is not changed.  out: host
 * (returns after completion) or device memory. */
int pedp_mesh_posed_vertices(pedp_mesh_t mesh, const double T[16], int mem, double *out);

/* Pinhole intrinsics as read from PinholeCameraIntrinsic.intrinsic_matrix
 * (src/defect_projection.py:209-212) plus the heat map's size. */
typedef struct {
    double fx, fy, cx, cy;
    int32_t width, height;
} pedp_pinhole;

/* heatmap_to_points + compute_rays + intersect_rays_with_mesh in one call
 * (src/defect_projection.py:165-179, :196-223, :225-266):
 *   select pixels with heatmap > threshold in row-major order (np.where); per pixel
 *   d = (xn, yn, 1) / sqrt((xn*xn + yn*yn) + 1), xn = (x - cx) / fx, yn = (y - cy) / fy in float64;
 *   [origin | d] cast to float32 and cast against the mesh (same sweep as pedp_raycast);
 *   rays with t_hit != inf are kept in order; point = origin + d * t_hit in float64.
 * heatmap: height x width float64, row-major.  origin: 3 float64 on the host (the reference passes
 * zeros).  Outputs hold `capacity` rows: points capacity x 3 f64, intensities f64, pixels
 * capacity x 2 int32 (x, y; nullable), prim_id u32 (nullable).  n_rays / n_hits are host
 * scalars (the call synchronises the stream).  PEDP_DEVICE: heatmap and the output arrays are
 * device memory.  If n_hits > capacity nothing is written, n_hits is still reported and the call
 * returns PEDP_ERR_BAD_ARG; capacity = width * height always suffices. */
int pedp_project_heatmap(pedp_ctx_t ctx, pedp_mesh_t mesh, const pedp_pinhole *cam, const double *heatmap,
                         double threshold, const double origin[3], int mem, int64_t capacity,
                         double *points, double *intensities, int32_t *pixels, uint32_t *prim_id,
                         int64_t *n_rays, int64_t *n_hits);

/* The same with what the reference does to the hits right after (src/defect_projection.py:268-294
 * create_intersection_pcd; run.py:118, :200 `.transform(reader.color_to_depth)`), and with the heat map where and as
 * it is.  opts (NULL = the call above):
 *   heat_f32   the heat map is float32: compared with the threshold in float32, the threshold rounded to float32 (what
 *              numpy's `heatmap > threshold` does with a Python number: an entry equal to float32(0.3) is not above
 *              0.3); the intensities are its values widened exactly to float64
 *   heat_mem   PEDP_HOST / PEDP_DEVICE for the heat map alone (a detector's output already on the GPU, or a map
 *              kept resident between detections, run.py:66, :147), whatever `mem` says about the outputs
 *   jet_lut    256 x 3 float64 on the host: matplotlib's `jet` lookup table (pedp_hip.ray_projection builds it);
 *   colors     capacity x 3 float64 (where `mem` says): jet_lut[clip(trunc(s * 256), 0, 255)] of the min-max
 *              normalised hit intensities s = (I - min I) / (max I - min I), float64, one rounding per operation;
 *              equal intensities divide by zero like the reference (NaN -> black).  Both NULL: no colours.
 *   post       4x4 float64 on the host (nullable): the hit points are moved by it -- ((T0 x + T1 y) + T2 z) + T3 per
 *              row, pedp_transform_points' order -- before they are written. */
typedef struct {
    int32_t heat_f32;
    int32_t heat_mem;
    const double *jet_lut;
    double *colors;
    const double *post;
} pedp_project_opts;
int pedp_project_heatmap_ex(pedp_ctx_t ctx, pedp_mesh_t mesh, const pedp_pinhole *cam, const void *heatmap,
                            double threshold, const double origin[3], int mem, int64_t capacity,
                            double *points, double *intensities, int32_t *pixels, uint32_t *prim_id,
                            int64_t *n_rays, int64_t *n_hits, const pedp_project_opts *opts);

/* ---------------------------------------------------------------- depth pre-filters
 * the reference's warp-lang kernels (CUDA-only JIT) and its depth back-projection.
 * Images are H x W float32, row-major; PEDP_HOST copies in and out and returns after completion,
 * PEDP_DEVICE only enqueues on the context's stream.  Defaults of the reference in brackets.
 *
 * erode_depth (Utils.py:356-396; estimater.py:171, :255): a pixel becomes 0 when more than
 * ratio_thres [0.8] of its (2 radius + 1)^2 window [radius 2] is invalid (< 0.001 or >= zfar
 * [100]) or differs from the centre by more than depth_diff_thres [0.001]; else it is kept. */
int pedp_erode_depth(pedp_ctx_t ctx, const float *depth, int H, int W, int radius, float depth_diff_thres,
                     float ratio_thres, float zfar, int mem, float *out);
/* bilateral_filter_depth (Utils.py:304-357; estimater.py:172, :256): mean of the valid window
 * pixels, then a Gaussian (sigmaD [2] in pixels, sigmaR [100000] in depth) weighted average over
 * the valid pixels within 0.01 of that mean; float32, window walked column by column. */
int pedp_bilateral_filter_depth(pedp_ctx_t ctx, const float *depth, int H, int W, int radius, float zfar,
                                float sigmaD, float sigmaR, int mem, float *out);
/* depth2xyzmap (Utils.py:401-420; run.py:89, estimater.py:175, :212), uvs=None form: xyz is
 * H x W x 3 float32, ((u - cx) z / fx, (v - cy) z / fy, z) formed in float64; depth < 0.001 -> 0.
 * K: row-major 3 x 3 float64 on the host. */
int pedp_depth2xyzmap(pedp_ctx_t ctx, const float *depth, int H, int W, const double K[9], int mem, float *xyz);
/* depth2xyzmap_batch (Utils.py:423-442; estimater.py:259): B images, Ks = B x 9 float32 on the
 * host, float32 arithmetic, invalid = depth < 0.001 or depth > zfar. */
int pedp_depth2xyzmap_batch(pedp_ctx_t ctx, const float *depths, int B, int H, int W, const float *Ks, float zfar,
                            int mem, float *xyz);

/* The depth entry of a camera frame in ONE call (estimater.py:255-259 and the scene cloud run.py's loop works on):
 *     erode_depth -> bilateral_filter_depth -> depth2xyzmap_batch (one image, float32) -> the pixels with z >= z_min in
 *     row-major order as float64 points scaled by `scale` (metres -> millimetres: 1000)
 * -- the kernels of the three calls above back to back on the context's stream, one upload of the image (depth_mem =
 * PEDP_HOST), no trip to the host between them, one 4-byte read-back (the count).  d_filtered (H x W float32) and d_xyz
 * (H x W x 3 float32) are DEVICE memory, nullable (library scratch is used instead); d_points: DEVICE memory for
 * H x W x 3 float64, the first n_points rows are written (what torch's `xyz[xyz[..., 2] >= z_min].double() * scale`
 * gives).  Results are those of the single calls bit for bit. */
typedef struct {
    int32_t erode_radius;
    float erode_diff, erode_ratio, erode_zfar;      /* erode_depth(radius, depth_diff_thres, ratio_thres, zfar) */
    int32_t bilateral_radius;
    float bilateral_zfar, sigmaD, sigmaR;            /* bilateral_filter_depth(radius, zfar, sigmaD, sigmaR) */
    float K[9];                                      /* intrinsics of depth2xyzmap_batch (float32, row-major) */
    float xyz_zfar;                                  /* its zfar (inf: none) */
    float z_min;                                     /* validity of a back-projected point: 0.001 */
    double scale;
} pedp_depth_entry_params;
int pedp_depth_to_scene(pedp_ctx_t ctx, const float *depth, int H, int W, int depth_mem, const pedp_depth_entry_params *prm,
                        float *d_filtered, float *d_xyz, double *d_points, int64_t *n_points);

/* ---------------------------------------------------------------- point-cloud operations
 * the Open3D calls preprocess_source chains (src/pose_estimation.py:186-268),
 * restated from the published open3d==0.18.0 algorithms.  Host arrays only (N x 3 float64); the
 * calls return after completion.  Where Open3D's result depends on something that cannot be
 * recovered (hash-map order, random_device seed, thread interleaving) the rule used is stated.
 *
 *   non-finite   a cloud with a NaN or infinite coordinate, in any row, is refused by every operation of this
 *                section that takes points -- pedp_voxel_down_sample[_device_in], pedp_cluster_dbscan,
 *                pedp_knn_mean_distance, pedp_estimate_normals, pedp_fpfh, pedp_segment_plane and
 *                pedp_preprocess_source[_ex], host or device array alike: PEDP_ERR_BAD_ARG, "<entry point>:
 *                non-finite coordinates", outputs untouched except counters set to 0, the context stays usable.
 *                (Open3D's result on such input is undefined -- integer casts of NaN -- and the depth entry never
 *                produces such rows.)  The test rides on the bounding-box pass every operation starts with and
 *                comes before any kernel that turns a coordinate into an index.  Normals, `prior` and feature rows
 *                are NOT checked: a non-finite normal or prior gives non-finite values in the rows that read it;
 *                for feature rows see pedp_feature_match.
 *
 * voxel_down_sample (:204-205): voxel index floor((p - (min_bound - voxel/2)) / voxel) per axis;
 * a voxel's points (and normals, nullable) are summed in point order and divided by the count.
 * Output order: ascending (ix, iy, iz) (Open3D: unordered_map order).  capacity = N always fits. */
int pedp_voxel_down_sample(pedp_ctx_t ctx, const double *pts, const double *normals, int64_t N, double voxel_size,
                           double *out_pts, double *out_normals, int64_t capacity, int64_t *n_out);

/* The same grid over points that are already on the device (N x 3 float64 device memory, e.g. the output of
 * pedp_depth2xyzmap_batch turned into millimetres by the caller): the scene of a frame then never visits the
 * host at full resolution.  Voxel averages come back to host memory like above; no normals.  The caller
 * orders its own work on the array before the call (the library reads it on the context's stream). */
int pedp_voxel_down_sample_device_in(pedp_ctx_t ctx, const double *d_pts, int64_t N, double voxel_size, double *out_pts,
                                     int64_t capacity, int64_t *n_out);
/* cluster_dbscan (:284): neighbours are points with d^2 < eps^2 (itself included), core points
 * have >= min_points neighbours; labels as Open3D's breadth-first sweep assigns them: clusters
 * numbered by their smallest core index, a border point takes the smallest id among its core
 * neighbours, noise is -1.  The labels are a function of (pts, eps, min_points) alone: which grid the
 * library picks for the search (cells below eps / sqrt(3), or cells of eps doubled until they fit the
 * budget, over the cloud's own box or a larger one) does not change them. */
int pedp_cluster_dbscan(pedp_ctx_t ctx, const double *pts, int64_t N, double eps, int min_points, int32_t *labels);
/* Per-point part of remove_statistical_outlier (:308-312): mean distance to the k nearest
 * neighbours (the point itself is one of them), summed in ascending order; the global mean /
 * deviation / threshold over N doubles is host arithmetic (pedp_hip.cloud_ops). */
int pedp_knn_mean_distance(pedp_ctx_t ctx, const double *pts, int64_t N, int k, double *avg);
/* estimate_normals with KDTreeSearchParamHybrid(radius, max_nn) (:301-306, callers :174, :216, :250-251):
 * neighbours = the max_nn nearest points with d^2 < radius^2 (itself included) in ascending
 * (d^2, index); >= 3 of them give the covariance (nine cumulants) whose smallest eigenvector
 * (Open3D's non-iterative FastEigen3x3) is the normal, otherwise (0, 0, 1).  prior (nullable,
 * N x 3): existing normals; the result is flipped to agree with them, as Open3D does. */
int pedp_estimate_normals(pedp_ctx_t ctx, const double *pts, int64_t N, double radius, int max_nn, const double *prior,
                          double *normals);

/* o3d.pipelines.registration.compute_fpfh_feature(cloud, KDTreeSearchParamHybrid(radius, max_nn))
 * (src/pose_estimation.py:132-137, :175-180, :255-260): out = N x 33 float64 (row i = column i of
 * Open3D's Feature.data).  The cloud's normals are required.  Restated from the published
 * open3d==0.18.0 Feature.cpp (parity unpinned); max_nn <= 128.  Feature.cpp orders a pair of points by
 * acos(|a1|) > acos(|a2|); where the two arguments are a few ulp apart (points with one normal, lattices)
 * the order is decided with a correctly rounded acos, so it does not depend on a libm's last bit. */
int pedp_fpfh(pedp_ctx_t ctx, const double *pts, const double *normals, int64_t N, double radius, int max_nn, double *out);

/* The correspondences of registration_ransac_based_on_feature_matching (src/pose_estimation.py:482-501):
 * idx[i] = the target feature nearest to source feature i (squared L2 over the 33 components in
 * float64, ties to the lower index; -1 when there is no target).  Feature rows are not checked: a
 * target row whose squared distance to the source row is NaN or +inf (a NaN or infinite component) is
 * never the nearest, and a source row for which that holds of every target gets -1 -- the
 * registration's rule for non-finite rows. */
int pedp_feature_match(pedp_ctx_t ctx, const double *fs, int64_t Ns, const double *ft, int64_t Nt, int32_t *idx);
/* segment_plane with ransac_n = 3 (:323-329).  Iteration t samples three distinct indices from a
 * counter-based generator of (seed, t); plane through them; inliers |n.p + d| < threshold; the best
 * iteration has the most inliers (earliest on ties); all iterations are evaluated (Open3D:
 * random_device samples, probabilistic early stop); num_iterations <= 4,194,240 (65535 slabs of 64
 * iterations: one launch's blocks in y), likewise pedp_preprocess_source's plane_iterations.
 * Returns, like Open3D, the inliers of the best sampled plane (ascending) and the plane refitted to
 * them (GetPlaneFromPoints).  The refit equals Open3D's up to summation rounding: Open3D keeps running
 * sums, the library adds blocks of 256 points. */
int pedp_segment_plane(pedp_ctx_t ctx, const double *pts, int64_t N, double distance_threshold, int num_iterations,
                       uint64_t seed, double plane[4], int32_t *inliers, int64_t *n_inliers);

/* preprocess_source of a frame in one call (src/pose_estimation.py:186-268; every branch run.py can take except
 * param['mesh']), the scene staying on the device between the stages:
 *     voxel_down_sample(down_sample) :204-205 -> segment_plane :323-329 -> [i == 0: estimate_normals of the
 *     down-sampled cloud :216] -> select_by_index(inliers, invert=True) :234 -> cluster_dbscan(eps 10, 10) +
 *     largest cluster :270-299 -> remove_statistical_outlier(75, 0.01) :308-312 -> [i == 0: estimate_normals
 *     of the result :250-251, oriented like the ones it carries]
 * The kernels and rules of the single operations above; results are bit for bit those of calling them one
 * after the other.  pts: N x 3 float64, host memory or (pts_on_device != 0) device memory that the caller has
 * ordered before the call.  out_pts / out_normals (normals only when first_frame): capacity x 3 float64 host
 * arrays; capacity = N always fits.  stage_counts (nullable): points after the voxel grid, the plane removal,
 * the cluster selection, the outlier filter.  status: PEDP_PREPROCESS_OK, _NO_CLUSTER (nothing left after the
 * plane, or DBSCAN found noise only -- the reference prints "No valid clusters found." and fails on None),
 * _DEGENERATE (fewer than three points) or _AMBIGUOUS (box cut only: the plane normal is perpendicular to the
 * average normal within rounding, the caller's own arithmetic decides the flip); n_out is 0 for those three.
 *
 * The background cloud run.py passes (run.py:99-101, :154-156) has no entry here: without param['box'] nothing of
 * it is read (:232-236 overwrite the cut), with param['box'] background_removal returns its input (:386-388), and
 * its down-sampled copy and normals (:204, :252) are locals of the reference's function.
 *
 * flags & PEDP_PREPROCESS_BOX: param['box'] -- the plane's inliers stay, the cloud is cut by the half space
 * remove_points_below_plane keeps (:366-378: signed distance <= 0 to the refit plane, flipped towards the average
 * normal by flip_plane_normal_if_needed :342-359); like the reference's, the cut cloud carries no normals, so the
 * final ones (first frame) take Open3D's default orientation.
 *
 * pedp_preprocess_source_ex, report (nullable): what the reference's two INFO lines print (:220, :356) and the box
 * cut uses --
 *     [0..3] the plane segment_plane returns (refit over the best plane's inliers, unflipped)
 *     [4..6] mean normal of the down-sampled cloud on the 10-unit grid, NOT normalised (first frame; else 1, 1, 1)
 *     [7]    box cut only: 1 if the plane was flipped        [8] inliers of the refit   [9] voxels of the 10-unit grid
 * Without a report and without the box flag none of this is computed (nothing can observe it). */
typedef struct pedp_preprocess_params {
    double voxel_size;          /* params['down_sample'] */
    double plane_distance;      /* params['plane_removal']['distance_threshold'] */
    int32_t plane_iterations;   /* params['plane_removal']['num_iterations'] */
    int32_t first_frame;        /* i == 0 */
    uint64_t seed;              /* segment_plane's sampler (see pedp_segment_plane) */
    double normal_radius;       /* estimate_normals: 2 */
    int32_t normal_max_nn;      /*                   5 */
    int32_t cluster_min_points; /* filter_largest_cluster: 10 */
    double cluster_eps;         /*                         10 */
    int32_t outlier_neighbors;  /* remove_statistical_outliers: 75 */
    int32_t flags;              /* PEDP_PREPROCESS_BOX */
    double outlier_std_ratio;   /*                              0.01 */
    double average_normal_voxel; /* compute_average_normal's grid: 10 (0 = that default) */
} pedp_preprocess_params;
#define PEDP_PREPROCESS_BOX 1
#define PEDP_PREPROCESS_OK 0
#define PEDP_PREPROCESS_NO_CLUSTER 1
#define PEDP_PREPROCESS_DEGENERATE 2
#define PEDP_PREPROCESS_AMBIGUOUS 3
#define PEDP_PREPROCESS_REPORT_DOUBLES 12
int pedp_preprocess_source(pedp_ctx_t ctx, const double *pts, int64_t N, int pts_on_device, const pedp_preprocess_params *prm,
                           double *out_pts, double *out_normals, int64_t capacity, int64_t *n_out, int64_t stage_counts[4],
                           int *status);
int pedp_preprocess_source_ex(pedp_ctx_t ctx, const double *pts, int64_t N, int pts_on_device, const pedp_preprocess_params *prm,
                              double *out_pts, double *out_normals, int64_t capacity, int64_t *n_out, int64_t stage_counts[4],
                              int *status, double report[PEDP_PREPROCESS_REPORT_DOUBLES]);

/* ---------------------------------------------------------------- ICP
 * Replaces src/pose_estimation.py:519-521 and :654-660:
 *     o3d.pipelines.registration.registration_icp(source, target, max_corr_dist, init,
 *         TransformationEstimationPointToPlane()[, ICPConvergenceCriteria(max_iteration=1)])
 * Clouds: N x 3 float64 host arrays (Open3D's Vector3dVector); normals nullable.
 */
int pedp_cloud_create(pedp_ctx_t ctx, const double *pts, const double *normals, int64_t N,
                      pedp_cloud_t *out);
/* The same from DEVICE memory (N x 3 float64 on the context's GPU, e.g. a torch tensor built from
 * depth2xyzmap's output): device-to-device copies on the context's stream, the bounding box by a reduction on the
 * device behind them (no read-back; centroid and magnitudes only when the cloud is first used as a target).
 * The caller orders its own work on the arrays BEFORE the call (the library reads them on the context's stream);
 * the call returns when the copies are complete -- the arrays may then be freed or overwritten at once -- while the
 * box reduction may still be running. */
int pedp_cloud_create_device(pedp_ctx_t ctx, const double *d_pts, const double *d_normals, int64_t N,
                             pedp_cloud_t *out);
void pedp_cloud_destroy(pedp_cloud_t cloud);
int pedp_cloud_size(pedp_cloud_t cloud, int64_t *N, int *has_normals);

/* Order of a cloud's rows in the pack it gets as a registration TARGET (sorted operand, tile spheres, sorted rows).
 * Any partition of the target's rows into tiles of 16 gives the same results in every bit; the order decides how many
 * tiles a pass has to look at.  HILBERT: runs of the cloud's spatial order (five launches).  COMPACT: a balanced k-d
 * split of that order (csrc/icp/target_order.h), about a third fewer tiles listed per pass on a surface model, built
 * on the device (1.4 ms of kernel time for 50,000 rows on an MI355X).  AUTO (default): Hilbert for the
 * first registration against the handle; from the second on -- a call of pedp_icp, pedp_icp_begin or
 * pedp_icp_batched[_ex] that comes after one whose passes were all enqueued -- the compact order if the target has at
 * least 16,384 finite rows; the pack is rewritten where it is, in front of that call's passes.  The environment
 * variable PEDP_ICP_TARGET_ORDER=hilbert|compact, read once per process, decides for every cloud left in AUTO.
 * A change of mode takes effect at the cloud's next use as a target: a pack in the other order is rewritten in place
 * (buffers keep their addresses).  No counterpart in the reference (src/pose_estimation.py:447-453 calls Open3D). */
#define PEDP_TARGET_ORDER_AUTO 0
#define PEDP_TARGET_ORDER_HILBERT 1
#define PEDP_TARGET_ORDER_COMPACT 2
int pedp_cloud_set_target_order(pedp_cloud_t cloud, int mode);
/* in_force: the order of the pack the cloud holds now (HILBERT / COMPACT), 0 while it has none. */
int pedp_cloud_target_order(pedp_cloud_t cloud, int *in_force);

/* Optional hook called once per correspondence pass with a DEVICE pointer to the
 * n-double partial-sum packet of this rank; it must enqueue an in-place sum over all
 * ranks on `stream` (RCCL all-reduce through torch.distributed) and return 0. */
typedef int (*pedp_allreduce_fn)(void *user, double *dev_packet, int n, void *stream);

typedef struct {
    double max_correspondence_distance;
    int estimator;           /* PEDP_POINT_TO_PLANE (reference default) / PEDP_POINT_TO_POINT */
    int max_iteration;       /* Open3D default 30 */
    double relative_fitness; /* Open3D default 1e-6; negative disables the early exit */
    double relative_rmse;    /* Open3D default 1e-6 */
    pedp_allreduce_fn allreduce; /* NULL on one GPU */
    void *allreduce_user;
    int64_t n_source_global; /* fitness denominator when the scene is sharded; 0 = local N */
    int use_comm;            /* 1: sum the packet over the ranks of the context's own RCCL
                                communicator (pedp_comm_create) on the stream, no host hook */
} pedp_icp_params;

/* init / T_out: row-major 4x4 float64, source -> target (scene -> model), host memory.
 * corr (nullable, host, N_source): target index per source point or -1.
 * trace (nullable, host): (max_iteration + 1) x 18 doubles [fitness, rmse, T] per pass. */
int pedp_icp(pedp_ctx_t ctx, pedp_cloud_t source, pedp_cloud_t target,
             const pedp_icp_params *params, const double init[16], double T_out[16],
             double *fitness, double *inlier_rmse, int32_t *n_iter_done, int32_t *corr,
             double *trace);

/* pedp_icp in two halves.  pedp_icp_begin enqueues every pass of the registration on the context's stream and returns at
 * once (passes after convergence are no-ops on the device: the host does not look at the criteria in between);
 * pedp_icp_end waits for them and hands the result over -- the same bits as pedp_icp's.  What the host does in between
 * (enqueueing a frame's ray stage on ANOTHER context, bench.py's step) overlaps with the registration instead of waiting in
 * front of it.  Between the two calls the registration's workspace, the first 8,192 bytes of the context's page-locked block
 * and the two clouds belong to the pending registration.  Every call that shares them is refused: a second pedp_icp_begin,
 * pedp_icp, pedp_icp_batched(_ex), pedp_nn, pedp_icp_configure, pedp_ransac_hypotheses, pedp_cloud_set_target_order and
 * pedp_debug_target_pack return
 * PEDP_ERR_BAD_ARG, and so do the calls that say so at their own declaration (the closest-point, defect-map and pose-error
 * calls in PEDP_HOST mode and their statistics, which would only wait for the stream).  Every other call of this header
 * keeps to state of its own that the stream orders -- the ray caster, the projection, the depth entry and filters, the
 * point-cloud operations and pedp_preprocess_source, pedp_cloud_create(_device), the renderer, crops, pose arithmetic,
 * statistics and the network kernels -- and may be used on the context in between: it gives the bits it gives on a fresh
 * context, and the registration ends with pedp_icp's bits (tests/test_call_history_gpu.py runs each of them in that
 * window; DESIGN.md s4.19 lists what each touches).  A PEDP_HOST call among them returns after the registration's passes,
 * so only PEDP_DEVICE calls overlap with it.  Destroying the context or either cloud with a registration pending is an
 * error of the caller.  want_trace: pedp_icp_end's `trace` may be non-null.  The reference has no counterpart (registration_icp is one blocking call,
 * src/pose_estimation.py:447-453). */
int pedp_icp_begin(pedp_ctx_t ctx, pedp_cloud_t source, pedp_cloud_t target, const pedp_icp_params *params,
                   const double init[16], int want_trace);
int pedp_icp_end(pedp_ctx_t ctx, double T_out[16], double *fitness, double *inlier_rmse, int32_t *n_iter_done,
                 int32_t *corr, double *trace);

/* Batched refine (FoundationPose hypothesis sizing, estimater.py:104-122): B start
 * poses share one source and one target; no early exit across the batch.  Up to 8 registrations
 * are in flight on internal streams (each replaying one captured hipGraph per pose); the call
 * returns when all are complete.  Results equal B separate pedp_icp calls on the same handles bit
 * for bit (the float64 sums follow the scene's cached spatial order; a different order -- another
 * handle, another region of start poses -- gives the same correspondences and poses equal to
 * rounding). */
int pedp_icp_batched(pedp_ctx_t ctx, pedp_cloud_t source, pedp_cloud_t target,
                     const pedp_icp_params *params, const double *inits /* B x 16 */, int B,
                     double *T_out /* B x 16 */, double *fitness /* B */,
                     double *inlier_rmse /* B */);

/* The same with one parameter struct per start pose (prms[B]): radius and convergence criteria may
 * differ from pose to pose (estimator and max_iteration may not), each registration stops by its
 * own criteria, n_iter_done (nullable, B) receives the iteration counts.  This is the form
 * improve_result's randomised restarts take (src/pose_estimation.py:577-613: every restart has its
 * own distance threshold and Open3D's default criteria). */
int pedp_icp_batched_ex(pedp_ctx_t ctx, pedp_cloud_t source, pedp_cloud_t target,
                        const pedp_icp_params *prms /* B */, const double *inits /* B x 16 */, int B,
                        double *T_out /* B x 16 */, double *fitness /* B */, double *inlier_rmse /* B */,
                        int32_t *n_iter_done /* B, nullable */);

/* One exact nearest-neighbour pass (the correspondence step alone): for every source
 * point transformed by T, the index of the closest target point and the squared
 * distance, float64-exact (ties: lowest index).  idx/d2: host arrays, length N.
 * Non-finite rows (here and in every registration): a target row with a NaN or infinite
 * coordinate is never a neighbour (the target's centroid, box and operand are made of its finite
 * rows), and a source row with one has none (idx -1, d2 +inf; no correspondence).
 * PEDP_ERR_BAD_ARG while a registration is pending on ctx (pedp_icp_begin). */
int pedp_nn(pedp_ctx_t ctx, pedp_cloud_t source, pedp_cloud_t target, const double T[16],
            int32_t *idx, double *d2);
/* Milliseconds of the last TIMED MFMA sweep kernel on this context (HIP events on the stream,
 * directly around the kernel): the sweep of pedp_nn, or of the pass selected by pedp_icp_configure. */
int pedp_nn_last_sweep_ms(pedp_ctx_t ctx, float *ms);

/* RANSAC draws of registration_ransac_based_on_feature_matching (src/pose_estimation.py:482-501,
 * ransac_n = 3): iteration itr0 + k, k = 0 .. count-1, takes three correspondences
 * (corr[i] = target point of source point i, e.g. from pedp_feature_match) with replacement, fits
 * Umeyama without scaling and applies the reference's three checkers in its order
 * (CorrespondenceCheckerBasedOnEdgeLength(edge_similarity), ...BasedOnDistance(max_distance),
 * ...BasedOnNormal(normal_angle, radians; skipped when a cloud has no normals)).  accepted[k] = 1 when
 * all pass; T[16 k ..] = the fitted source -> target transformation either way.  The draw is a
 * counter-based function of (seed, iteration) (Open3D's random_device-seeded engines are not
 * recoverable); count <= 2^22 per call. */
int pedp_ransac_hypotheses(pedp_ctx_t ctx, pedp_cloud_t source, pedp_cloud_t target, const int32_t *corr, uint64_t seed,
                           int64_t itr0, int count, double edge_similarity, double max_distance, double normal_angle,
                           uint8_t *accepted, double *T);

/* Measurement knobs of pedp_icp / pedp_icp_batched on this context.
 *   exhaustive = 1: no culling -- every scene point stays a candidate and the MFMA kernel sweeps
 *     every (scene point, target point) pair in every pass (the all-pairs workload of SURVEY s8d);
 *     correspondences and poses are identical to the culled run, only the work differs.
 *   timed_pass >= 0: record HIP events around the sweep kernel of that correspondence pass (read
 *     with pedp_nn_last_sweep_ms); -2: around the sweep kernel of every fourth pass from pass 1 on
 *     (up to eight), pedp_nn_last_sweep_ms then reports their mean; -3 (fused path): ONE pair of
 *     events around all the passes' launches of a registration, pedp_nn_last_sweep_ms reports the
 *     span divided by the number of launches -- the mean launch-to-launch time of the pass kernel,
 *     boundaries included; -1 = none.
 * "Sweep kernel": nn_sweep_kernel on the segmented path, icp_pass_kernel (the whole pass: per-chunk
 * work, sweep included, and its close by the last workgroup) on the fused path of radius-limited
 * registrations. */
int pedp_icp_configure(pedp_ctx_t ctx, int exhaustive, int timed_pass);

/* Work statistics of the last pedp_icp on this context: correspondence passes run, (scene,
 * target) pairs the MFMA sweep evaluated (scene points farther than the radius from the
 * target's bounding box are dropped before the sweep), and points whose fp32 filter was
 * ambiguous and went through the exact float64 brute-force kernel. */
int pedp_icp_last_stats(pedp_ctx_t ctx, int64_t *passes, int64_t *pairs_swept, int64_t *fallback_points);

/* Passes of the last single pedp_icp on this context that ran under a visit plan: with more live scene chunks than
 * CUs (and at most twice as many) the workgroup that is through first ranks the chunks by the time the pass before
 * spent on them and hands the lightest ones to the workgroup positions that share a CU.  Scheduling only -- partial
 * sums stay indexed by live rank, results do not change in any bit (PEDP_ICP_NO_VISIT_PLAN=1 switches it off;
 * tests/test_icp_gpu.py compares).  No counterpart in the reference (src/pose_estimation.py:447-453 calls Open3D). */
int pedp_icp_last_planned_passes(pedp_ctx_t ctx, int64_t *planned);

/* Registration graphs captured and instantiated on `ctx` and its sub-contexts since the context was created (the
 * per-pose graph of a batch on the segmented path, the group graphs of a fused batch).  A count that stands still
 * over a call means the call replayed what it had (tests: a target whose order changes keeps its graphs). */
int pedp_icp_graph_captures(pedp_ctx_t ctx, int64_t *captures);

/* The serial part of a pass and of a registration, for the last single registration collected on `ctx`.
 * wide_closes: passes whose close ran in its wide form -- the first look at the sign-off counters requested with the
 * partial sums' loads, the three sincos of the update on three lanes, the sixteen entries of the new pose on sixteen --
 * each output by the same sequence of float64 operations as on one lane (PEDP_ICP_SERIAL_CLOSE=1: one lane, 0 here).
 * bracket: bit 0 -- the start state was fetched from the context's page-locked block by a kernel that also zeroes the
 * tickets, sign-off counters, live masks and the visit plan (one launch in front of pass 0 instead of a copy and a
 * fill); bit 1 -- the final state was written into that block by the workgroup that ended the registration, no copy
 * behind the last pass (PEDP_ICP_COPY_BRACKET=1: copies and fill as before, 0 here).  Results do not change in any
 * bit either way (tests/test_icp_serial_path_gpu.py compares).  Between pedp_icp_begin and pedp_icp_end the device
 * writes the page-locked block at a time of its own choosing: every entry point that touches the block's first 4 KB
 * or the ICP workspace returns PEDP_ERR_BAD_ARG while a registration is pending. */
int pedp_icp_last_serial_path(pedp_ctx_t ctx, int64_t *wide_closes, int64_t *bracket);

/* Passes of the last single registration collected on `ctx` that were closed at the head of the next launch: a steady
 * pass of a fused registration ends with its partial sums, and every workgroup of the next launch sums them, solves
 * and updates the pose before it transforms its chunk -- no ticket, no sign-off, no state handed over inside a launch.
 * Rebuild passes and the last pass close in their own launch: passes - rebuild passes - 1 here.  0 with
 * PEDP_ICP_HEAD_CLOSE=0, with PEDP_ICP_SERIAL_CLOSE=1 or PEDP_ICP_COPY_BRACKET=1, for batches and sharded registrations.
 * rebuilds (may be null): rebuilds of the live chunk set that registration asked for after pass 0 (fused path).
 * launches (may be null): passes the last single registration enqueued on `ctx` -- max_iteration + 1, fewer where
 * pedp_icp's early-exit look (every 8th pass) saw the registration done.
 * Results do not change in any bit (tests/test_icp_head_close_gpu.py compares). */
int pedp_icp_last_head_closed(pedp_ctx_t ctx, int64_t *head_closed, int64_t *rebuilds, int64_t *launches);

/* Candidate slots of the last single registration collected on `ctx`, summed over its passes, whose nearest-neighbour
 * search a certificate replaced (`slots`), and those that searched (`searched_slots`, may be null).  A pass leaves, per
 * scene point, a lower bound on the distance to every target point other than the neighbour it found; while the point's
 * motion since keeps that neighbour strictly inside the bound it is still the unique nearest neighbour, and a wave whose
 * slots are all proven so skips culling, sweep and selection.  Rebuild passes, batches, sharded registrations and
 * PEDP_ICP_CERT=0 certify nothing: 0 slots (and, for all but the first, 0 searched slots: they are not counted there).
 * Results do not change in any bit (tests/test_icp_certificate_gpu.py compares). */
int pedp_icp_last_certified(pedp_ctx_t ctx, int64_t *slots, int64_t *searched_slots);

/* Passes of the last single registration collected on `ctx` that ran inside a steady launch (`passes`), and how often such
 * a launch handed the registration back to the generic pass kernel (`handbacks`, may be null).  A registration that closes
 * its passes at the head of the next launch and keeps certificates (the two read-outs above) runs its passes from
 * PEDP_ICP_STEADY_FROM (default 5) on in ONE launch of a resident grid: per pass a bounded device-wide hand-over of the
 * partial sums replaces the launch boundary, one workgroup per CU closes the pass itself (below), and a slot without a certificate runs
 * the exact search.  The launch hands back when a close asks for a rebuild of the live set or more than 1/8 of a pass's
 * candidate slots searched; pedp_icp_end / pedp_icp then run two generic launches and the steady launch again.
 * PEDP_ICP_STEADY=0 (read once per process): 0 passes; so do batches, sharded registrations, captured graphs, a timed_pass
 * other than -1 and -3, and pedp_icp with criteria >= 0 (its early-exit look needs launches to look behind).
 * One steady launch per device is in flight per process (a second registration at the same time keeps to generic launches);
 * where several PROCESSES register on one device at once, set PEDP_ICP_STEADY=0: two resident grids can keep each other out,
 * which the bounded hand-over ends with PEDP_ERR_HIP.
 * PEDP_ICP_STEADY_GRID=n caps the launch's workgroups (tests).  Results do not change in any bit
 * (tests/test_icp_steady_gpu.py compares). */
int pedp_icp_last_steady(pedp_ctx_t ctx, int64_t *passes, int64_t *handbacks);

/* Workgroups of the last steady launch of the last single registration collected on `ctx` that FOLLOWED: they closed no pass
 * themselves but took the closed state from a record one of the closers published (csrc/icp/steady_pass.h).  The ranks below
 * min(ranks, closers) close, the others follow; `closers` is the device's CU count, or PEDP_ICP_STEADY_CLOSERS=n (read once
 * per process; unset or 0: the CU count; n at least the launch's grid: every rank closes, 0 followers; small n: tests).
 * 0 where no steady launch ran.  Results do not change in any bit (tests/test_icp_steady_followers_gpu.py compares).
 *
 * PEDP_ICP_STEADY_GROUPS=1|2 (read once per process) sets the wave groups of a steady launch's workgroups.  1: a workgroup of
 * eight waves is a rank, up to two workgroups per CU.  2: a workgroup of sixteen waves holds two ranks, one per wave group of
 * eight, one workgroup per CU; it closes a pass once, on all its threads, and its second group goes on from the state in the
 * workgroup's LDS -- closer and follower above are then WORKGROUPS, `closers` counts workgroups, and `followers` reads ranks
 * minus closing workgroups (a second group closes nothing itself).  PEDP_ICP_STEADY_GRID=n stays n workgroups, so the ranks are
 * min(live chunks, groups x n).  Unset or 0: two groups where the scene has more chunks of 128 points than the device has CUs
 * -- only there a CU would hold two ranks -- and PEDP_ICP_STEADY_GRID is unset, else one group.  Results do not change in any
 * bit (tests/test_icp_steady_groups_gpu.py compares). */
int pedp_icp_last_steady_followers(pedp_ctx_t ctx, int64_t *followers);

/* Closes of the last single registration collected on `ctx` whose 6x6 point-to-plane system was solved with a row per
 * lane of the closing wave (csrc/icp/solve_lanes.h): the pivot exchanges -- they follow from the six input diagonals
 * alone -- are played through first, lane i < 6 then holds the row that ends up at position i, b and y of that row, and
 * a step of the LDLT is at most five multiply-add pairs and one division on all rows at once.  Each output is computed
 * by the sequence of float64 operations the one-lane solve uses.  A pass counts when it is point-to-plane, has correspondences and does not stop: passes - 1 for
 * a registration that runs all its passes (a fused batch: the total over its poses); 0 for point-to-point, with PEDP_ICP_LANE_SOLVE=0 (read once per process:
 * the solve on one lane, as before) and with PEDP_ICP_SERIAL_CLOSE=1.  Results do not change in any bit
 * (tests/test_icp_lane_solve_gpu.py compares). */
int pedp_icp_last_lane_solves(pedp_ctx_t ctx, int64_t *lane_solves);

/* Both device forms of the close's 6x6 solve on n systems (tests compare them with each other and with the oracle):
 * A (float64 x 36 per system, row-major, both triangles) and b (float64 x 6) on the host; x_lanes / ok_lanes from the
 * row-per-lane form, a wave per system, x_one / ok_one from the one-lane form, a thread per system (float64 x 6 and
 * one int32 per system each; ok = 0: a NaN or infinite solution, and x = 0). */
int pedp_debug_solve6(pedp_ctx_t ctx, int64_t n, const double *A, const double *b, double *x_lanes, int32_t *ok_lanes,
                      double *x_one, int32_t *ok_one);

/* The live list of a rebuild pass's close (csrc/icp/live_list.h) on mask words of the caller's: n_lw words (uint64, bit b of
 * word w: chunk 64 w + b is live) on the host, in one workgroup of `threads` = 512 (the close inside a pass launch: coherent
 * loads, 2,048 entries of the list in LDS) or 1,024 (icp_finish_kernel: plain loads, 8,192 entries).  list_out (int32 x 64 n_lw)
 * gets the set bits' positions, ascending, in its first *n_live_out entries; the rest is left as it was. */
int pedp_debug_live_list(pedp_ctx_t ctx, const unsigned long long *mask_words, int n_lw, int threads, int32_t *list_out, int32_t *n_live_out);

/* Diagnostics of the dense sweep's bf16 form (tests measure its error against float64): for n_src scene rows (b.x, b.y, b.z, .)
 * = (-2 s') and n_tgt model rows (t'.x, t'.y, t'.z, |t'|^2), float32 x 4 each on the host, counts multiples of 16,
 * g[i * n_tgt + j] = |t'_j|^2 - 2 s'_i . t'_j exactly as the sweep's v_mfma_f32_16x16x32_bf16 produces it (same operand packing). */
int pedp_debug_nn_bf16(pedp_ctx_t ctx, const float *src4, int64_t n_src, const float *tgt4, int64_t n_tgt, float *g);

/* Read-out of a target's pack for tests: rows = its finite rows, pad_rows = rows of the padded operand; tile_perm
 * (int32 x N: original index of pack row k), tgt4 (float32 x 4 x pad_rows: centred x y z, |.|^2), and the spheres
 * (float32 x 4: centre, radius; radius < 0: no rows) of every 16 rows (pad_rows / 16), every 64 rows (pad_rows / 64)
 * and every 1024 rows (ceil(pad_rows / 1024)).  Any array may be null.  The cloud must have been a target. */
int pedp_debug_target_pack(pedp_ctx_t ctx, pedp_cloud_t cloud, int64_t *rows, int64_t *pad_rows, int32_t *tile_perm,
                           float *tgt4, float *sph16, float *sph64, float *sph1024);

/* Which way a registration runs: the library's one decision (csrc/pedp_icp.hip: icp_decide_path), exposed for tests.
 * No context, no GPU.  Every flag is 0 or 1. */
typedef struct pedp_icp_switches {  /* the environment switches, read once per process: PEDP_ICP_<FIELD>, PEDP_NN_F32 */
    int nn_f32, unfused_finish, no_visit_plan, serial_close, copy_bracket; /* on when set to a number other than 0 */
    int head_close, cert, steady;                                          /* on unless set to 0 */
    int steady_from;  /* default 5 */
    int steady_grid;  /* cap of a steady launch's workgroups (tests); 0: none */
    int target_order; /* PEDP_TARGET_ORDER_*: hilbert | compact decide for every cloud in automatic mode */
    int steady_closers; /* workgroups of a steady launch that close a pass themselves; 0: the device's CU count */
    int steady_groups;  /* wave groups (ranks) per workgroup of a steady launch, 1 or 2; 0: by the scene's size (below) */
    int lane_solve;     /* PEDP_ICP_LANE_SOLVE: 0 the close's 6x6 solve on one lane, 1 (default) a row per lane of the closing wave */
    int pass_grid;      /* PEDP_ICP_PASS_GRID: cap of a generic pass launch's workgroups with chunks (tests); 0: none.  The path does not depend on it */
} pedp_icp_switches;
typedef struct pedp_icp_path_inputs {
    int64_t n_source, n_target; /* source points, finite target rows */
    double radius;              /* max_correspondence_distance */
    int unit_size;              /* MFMA tiles per target unit: 1 while radius^2 < diag^2 / 16, else (and exhaustive) 4 */
    int poses;                  /* start poses that share the launches */
    int timed_pass;             /* pedp_icp_configure */
    int exhaustive;
    int exchange;               /* an all-reduce hook or the communicator sums the packet over ranks */
    int batch;                  /* a group of a fused batch: the batch's own kernels move its states */
    int early_exit;             /* pedp_icp with criteria >= 0 looks at `done` behind every 8th launch */
    int no_steady;              /* the caller needs generic launches only (a captured graph, a mixed batch) */
    int resident;               /* the steady kernel's grid can be resident on the device */
} pedp_icp_path_inputs;
typedef struct pedp_icp_path {  /* DESIGN 4.2 has the table */
    int fused;          /* passes are launches of the fused pass kernel (else: the segmented kernels) */
    int dev_result;     /* the workgroup that ends the registration writes the final state to the host's block */
    int copy_bracket;   /* copies and a fill bracket the passes (else: one start kernel in front of pass 0) */
    int head;           /* steady passes stay open; the next launch closes them at its head */
    int certify, plan;  /* the passes keep certificates / a visit plan */
    int serial_close;   /* the close of a pass on one lane */
    int unfused_finish; /* a launch of the finish kernel closes every pass */
    int exchange;       /* the packet is summed over ranks between the sums and the solve */
    int steady;         /* the passes from steady_from on run in one resident launch, if the device's is free */
    int steady_from;
    int lane_solve;     /* the wide close solves its 6x6 system a row per lane (never with serial_close) */
} pedp_icp_path;
/* switches null: those this process read from its environment. */
int pedp_debug_icp_path(const pedp_icp_switches *switches, const pedp_icp_path_inputs *inputs, pedp_icp_path *path);

/* ---------------------------------------------------------------- multi-GPU collectives
 * One process per GPU.  The reference has no distributed path; these entry points
 * exist so that the two exchange steps of the sharded path run inside the library, on
 * the context's stream, over RCCL/xGMI: the all-gather of the ray shards' hit records and the
 * per-pass all-reduce of the ICP packet (pedp_icp_params.use_comm).  RCCL is bound at run time.
 * Rendezvous is the host's business: rank 0 makes the id, the host side hands the same 128 bytes
 * to every rank (pedp_hip.dist does it through torch.distributed), every rank calls create. */
enum { PEDP_COMM_ID_BYTES = 128 };
int pedp_comm_unique_id(uint8_t id[PEDP_COMM_ID_BYTES]);
int pedp_comm_create(pedp_ctx_t ctx, const uint8_t id[PEDP_COMM_ID_BYTES], int nranks, int rank);
int pedp_comm_destroy(pedp_ctx_t ctx);
int pedp_comm_size(pedp_ctx_t ctx, int *nranks, int *rank);
/* Device pointers; only enqueue on the context's stream.  allgather: every rank contributes
 * bytes_per_rank bytes, recv holds nranks * bytes_per_rank in rank order. */
int pedp_comm_allgather(pedp_ctx_t ctx, const void *send, void *recv, int64_t bytes_per_rank);
int pedp_comm_allreduce_f64(pedp_ctx_t ctx, double *buf, int64_t n);

/* ---------------------------------------------------------------- mesh renderer
 * Replaces nvdiffrast on FoundationPose's render path (Utils.py nvdiffrast_render :133-220, callers
 * predict_pose_refine.py:49, predict_score.py:79; the dr.rasterize / interpolate / texture calls of run.py:34 and
 * estimater.py:100, :166).  Forward only, no antialiasing; the contract (clip space, pixel centres, coverage,
 * visibility, rast_out, lighting) is DESIGN.md s"Renderer".  All arrays float32 / int32, row-major; every pointer is
 * host or device memory by `mem`. */
typedef struct pedp_render_params {
    int H, W;              /* image size of the intrinsics (bbox2d lives in it) */
    int out_h, out_w;      /* rendered size (output_size) */
    float proj[16];        /* OpenGL projection, row-major (host value) */
    int use_light;         /* colour = colour * w_ambient + diffuse * light_color * w_diffuse */
    int light_mode;        /* 0: light_dir, 1: light_pos (per-vertex direction light_pos - xyz) */
    float light_dir[3], light_pos[3];
    int has_light_color;   /* 0: light_color is the colour itself */
    float light_color[3];
    float w_ambient, w_diffuse;
} pedp_render_params;

/* N poses (ob_in_cam, N x 16) of one mesh (verts / vnormals V x 3, faces F x 3, vcolor V x 3 in [0,1] or per-vertex
 * uv V x 2 + texture tex_h x tex_w x 3), bbox2d N x 4 (umin, vmin, umax, vmax) or null.  Writes color N x out_h x
 * out_w x 3, depth N x out_h x out_w, and where not null normal and xyz (N x out_h x out_w x 3), rows already flipped
 * (output row 0 = image row 0).  F = 0 or V = 0 gives zeros. */
int pedp_render(pedp_ctx_t ctx, const float *verts, int64_t V, const int32_t *faces, int64_t F, const float *vnormals,
                const float *vcolor, const float *uv, const float *tex, int tex_h, int tex_w, const float *poses,
                const float *bbox2d, int N, const pedp_render_params *prm, int mem, float *color, float *depth,
                float *normal, float *xyz);
/* dr.rasterize, instanced mode: pos N x V x 4 clip space -> rast N x H x W x 4 (u, v, z/w, triangle id + 1), GL row order. */
int pedp_rasterize(pedp_ctx_t ctx, const float *pos, int N, int64_t V, const int32_t *tri, int64_t F, int H, int W, int mem,
                   float *rast);
/* dr.interpolate: attr V x A (attr_batched = 0) or N x V x A -> out N x H x W x A; zero where rast has no triangle. */
int pedp_interpolate(pedp_ctx_t ctx, const float *attr, int attr_batched, int64_t V, int A, const float *rast, int N, int H,
                     int W, const int32_t *tri, int64_t F, int mem, float *out);
/* dr.texture, filter 'linear', boundary 'wrap': tex tex_n x th x tw x C (tex_n 1 or N), uv N x H x W x 2 -> out N x H x W x C. */
int pedp_texture(pedp_ctx_t ctx, const float *tex, int tex_n, int th, int tw, int C, const float *uv, int N, int H, int W,
                 int mem, float *out);
/* Poses per chunk of the renderer's workspace (0: as many as 128 MB of per-pixel keys hold). */
int pedp_render_configure(pedp_ctx_t ctx, int pose_chunk);

/* ---------------------------------------------------------------- crop batches (kornia warp_perspective)
 * Replaces kornia.geometry.transform.warp_perspective (kornia 0.7.2) and FoundationPose's make_crop_data_batch
 * (predict_pose_refine.py:26-88, predict_score.py:57-112, with compute_crop_window_tf_batch of Utils.py:577-621 and
 * the datasets' transform_batch, h5_dataset.py:79-180).  The contract is DESIGN.md s4.9: per pose one float64 map from
 * output pixel to grid_sample pixel coordinate, evaluated in float64 per pixel, cast to float32, then grid_sample's
 * float32 bilinear (zeros padding, corners nw, ne, sw, se, no FMA) or nearest (round half to even).  A singular or
 * non-finite M gives zeros.  Every pointer is host or device memory by `mem`. */
enum { PEDP_U8 = 0, PEDP_F32 = 1 };

/* A strided N x C x H x W image: element (n, c, y, x) at data + n*sn + c*sc + y*sy + x*sx elements of `dtype`
 * (PEDP_U8 or PEDP_F32).  Strides are >= 0; sn = 0 is a batch expanded from one image, and H x W x C storage behind a
 * permuted view is sc = 1, sy = W*C, sx = C. */
typedef struct pedp_image {
    const void *data;
    int dtype;
    int N, C, H, W;
    int64_t sn, sc, sy, sx;
} pedp_image;

/* warp_perspective(src, M, (out_h, out_w), mode, 'zeros', align_corners): M B x 9 float32 (source pixel -> output
 * pixel), src N = B or 1, mode 0 bilinear / 1 nearest.  out: B x C x out_h x out_w float32, contiguous. */
int pedp_warp_perspective(pedp_ctx_t ctx, const pedp_image *src, const float *M, int B, int out_h, int out_w, int mode,
                          int align_corners, int mem, float *out);

/* compute_crop_window_tf_batch(method='box_3d'): poses B x 16 float32 (by `mem`), K 9 float32 host values (read during
 * the call, whatever `mem` says), radius = float32(mesh_diameter * crop_ratio / 2), out_w x out_h the crop size.
 * tf_to_crops B x 9 float32; bbox2d B x 4 (the crop corners (0, 0) and (corner_u, corner_v) through the float64 inverse
 * of tf_to_crops, cast to float32) or null.  The scales are out_w * float32(1 / (right - left)), as torch computes a
 * number divided by a tensor. */
int pedp_crop_window(pedp_ctx_t ctx, const float *poses, int B, const float *K, float radius, int out_w, int out_h,
                     float corner_u, float corner_v, int mem, float *tf_to_crops, float *bbox2d);

typedef struct pedp_crop_params {
    int variant;        /* 0: refiner (predict_pose_refine.py), 1: scorer (predict_score.py) */
    int normalize_xyz;  /* cfg['normalize_xyz'] */
    int use_normal;     /* refiner: write normalB from the normal source */
    int B;              /* poses */
    int H, W;           /* full frame */
    int out_h, out_w;   /* crop (input_resize) */
    float K[9];         /* float32 intrinsics (scorer: the back-projection of the depth round trip) */
    float mesh_diameter;
} pedp_crop_params;

/* One fused pass over every pose: the B side (rgbB bilinear / 255; refiner xyzB nearest from `xyz` and, under
 * use_normal, normalB nearest from `normal`; scorer depthB nearest from `depth` and xyzB through the crop -> frame ->
 * crop round trip) and the A side (rgbA = (rgb_r * 255) / 255, xyzA from xyz_r; "/ 255" is torch's product with
 * float32(1 / 255)), with transform_batch's xyz
 * normalisation on both xyz maps.  Sources are one H x W frame each (their sn is ignored); rgb_r and xyz_r are the
 * renderer's B x out_h x out_w x 3 outputs.  tf_to_crops B x 9, poses B x 16 float32.  Outputs B x C x out_h x out_w
 * float32 (C = 3, depthB C = 1); null where the variant has none. */
int pedp_crop_batch(pedp_ctx_t ctx, const pedp_crop_params *prm, const float *tf_to_crops, const float *poses,
                    const pedp_image *rgb, const pedp_image *xyz, const pedp_image *normal, const pedp_image *depth,
                    const float *rgb_r, const float *xyz_r, int mem, float *rgbA, float *rgbB, float *xyzA, float *xyzB,
                    float *normalB, float *depthB);

/* The crop batch with the network's inputs packed: predict_pose_refine.py:187-188 and predict_score.py:188-189 build
 * A = torch.cat([rgbAs, xyz_mapAs], 1) and B = torch.cat([rgbBs, xyz_mapBs], 1) from pedp_crop_batch's outputs.  Same
 * arguments and values as pedp_crop_batch, but the A side goes into one B x 6 x out_h x out_w float32 buffer (channels
 * rgbA 0-2, xyzA 3-5) and the B side into another (rgbB, xyzB); normalB and depthB as pedp_crop_batch. */
int pedp_crop_batch_packed(pedp_ctx_t ctx, const pedp_crop_params *prm, const float *tf_to_crops, const float *poses,
                           const pedp_image *rgb, const pedp_image *xyz, const pedp_image *normal, const pedp_image *depth,
                           const float *rgb_r, const float *xyz_r, int mem, float *A, float *B, float *normalB, float *depthB);

/* ---------------------------------------------------------------- pose arithmetic (pytorch3d, compute_mesh_diameter)
 * The contract is DESIGN.md s4.10: float32 with no contraction, every sum in the order written, tanh / sin / cos in
 * float64 rounded once to float32.  The rotations restate pytorch3d 0.7's so3_exp_map and rotation_6d_to_matrix (parity
 * with pytorch3d unpinned: it is not installed where this library runs). */
enum { PEDP_TRANS_TRACKNET = 0, PEDP_TRANS_RAW = 1 };
enum { PEDP_ROT_AXIS_ANGLE = 0, PEDP_ROT_6D = 1 };

typedef struct pedp_pose_update_params {
    int trans_rep;              /* cfg['trans_rep']: PEDP_TRANS_TRACKNET or PEDP_TRANS_RAW (deepim is not supported) */
    int rot_rep;                /* cfg['rot_rep']: PEDP_ROT_AXIS_ANGLE or PEDP_ROT_6D */
    int normalize_xyz;          /* cfg['normalize_xyz'] */
    float trans_normalizer[3];  /* float32(cfg['trans_normalizer']), one value repeated or three */
    float rot_normalizer;       /* float32(cfg['rot_normalizer']) */
    double mesh_diameter;       /* under normalize_xyz the translation is multiplied by float32(mesh_diameter / 2) */
} pedp_pose_update_params;

/* Replaces predict_pose_refine.py:195-231 (the tanh scaling, pytorch3d's so3_exp_map(...).permute(0, 2, 1) or
 * rotation_6d_to_matrix(...).permute(0, 2, 1), the diameter scale) and egocentric_delta_pose_to_pose (Utils.py:848-855),
 * one lane per pose.  trans B x 3, rot B x 3 (axis-angle) or B x 6 (6d), poseA B x 16 float32 -> poses B x 16 (may be
 * poseA itself); trans_delta B x 3 and rot_mat_delta B x 9 (the predictor's last_trans_update / last_rot_update) or null.
 * Every pointer is host or device memory by `mem`. */
int pedp_pose_update(pedp_ctx_t ctx, const pedp_pose_update_params *prm, int B, const float *trans, const float *rot,
                     const float *poseA, int mem, float *poses, float *trans_delta, float *rot_mat_delta);

/* Replaces compute_mesh_diameter's `np.linalg.norm(pts[None] - pts[:, None], axis=-1).max()` (Utils.py:559-574): pts
 * n x 3 float64 (host or device by `mem`) -> *out = sqrt(max over i, j of (dx^2 + dy^2) + dz^2), bit for bit numpy's
 * value; NaN if any coordinate is not finite (numpy's diagonal inf - inf), 0 for n = 1; n = 0 is an error.  *out is host
 * memory; the call returns once it is written. */
int pedp_max_pair_distance(pedp_ctx_t ctx, const double *pts, int64_t n, int mem, double *out);

/* ---------------------------------------------------------------- pose errors (add_err, adds_err)
 * ADD and ADD-S of B predicted poses against a ground truth (Utils.py:232-253), one float64 per pose.  The contract is
 * DESIGN.md s4.15:
 *   arithmetic   float64, no contraction, every sum in the order written, no floating-point atomics: a rerun, another
 *                batch size and another position in the batch give the same bits
 *   transform    q_k = ((R_k0 x + R_k1 y) + R_k2 z) + t_k for a model point (x, y, z); the bottom row of a pose is not read
 *   ADD          e = (1 / N) sum_i sqrt((dx^2 + dy^2) + dz^2), d = pred p_i - gt p_i
 *   ADD-S        e = (1 / N) sum_i sqrt(min_j ((dx^2 + dy^2) + dz^2)), d = pred p_j - gt p_i: the nearest transformed
 *                pred point of every transformed gt point (the reference's tree holds the pred points)
 *   mean         the terms in chunks of 256 points, a chunk's sum in a fixed tree, the chunks' sums added in index order,
 *                one division by N: the order depends on N alone (DESIGN.md states it, tests/_metrics_ref.py restates it)
 *   symmetries   S > 0: the error of pose b is the minimum over s of e(pred_b . sym_s, gt), the 4 x 4 product's rows
 *                0 .. 2 formed as ((P_i0 s_0j + P_i1 s_1j) + P_i2 s_2j) + P_i3 s_3j; S = 0 multiplies nothing, and S = 1
 *                with the identity gives the same bits as S = 0
 *   non-finite   a pose is NaN if a transformed coordinate it reads (pred or gt side, any symmetry) is not finite, which
 *                every NaN / infinite entry of the pose, the ground truth, a symmetry or a point causes; the other poses
 *                are not touched
 * pts N x 3; preds B x 16 and gts G x 16 row-major 4 x 4, G = 1 (one ground truth for all) or G = B; sym S x 16 or null
 * with S = 0; kind PEDP_ERR_ADD or PEDP_ERR_ADDS; out B doubles.  Every pointer is host or device memory by `mem`;
 * PEDP_DEVICE only enqueues on the context's stream.  N = 0, N > 2^22, B > 65535, S > 65535 or G not in {1, B} is
 * PEDP_ERR_BAD_ARG; B = 0 does nothing.  The partial sums live in a workspace of their own (64 MB at most unless
 * one pose alone needs more: more poses go in slabs), so PEDP_DEVICE calls are allowed while a registration is pending on ctx (pedp_icp_begin); PEDP_HOST
 * calls, which use the context's staging buffers and wait on its stream, are PEDP_ERR_BAD_ARG then. */
enum { PEDP_ERR_ADD = 0, PEDP_ERR_ADDS = 1 };

int pedp_pose_errors(pedp_ctx_t ctx, const double *pts, int64_t N, const double *preds, int B, const double *gts, int G,
                     const double *sym, int S, int kind, int mem, double *out);

/* ---------------------------------------------------------------- closest points of the mesh (compute_closest_points)
 * The closest point of the mesh, as currently posed, to each of N points: RaycastingScene.compute_closest_points /
 * compute_distance on the handle the ray caster uses.  The contract is DESIGN.md s4.16:
 *   triangle     the record the ray caster tests, as stored: a = v0, ab = e1, ac = e2, float32 values promoted to float64;
 *                the vertices are a, a + ab, a + ac.  Pad records and records whose m = e2 x e1 is all zero (degenerate: no
 *                ray can hit them either) are skipped
 *   arithmetic   float64, no contraction, every expression in the order written; dot(x, y) = (x0 y0 + x1 y1) + x2 y2.
 *                With ap = p - a, bp = ap - ab, cp = ap - ac: d1 = ab.ap, d2 = ac.ap, d3 = ab.bp, d4 = ac.bp, d5 = ab.cp,
 *                d6 = ac.cp, vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4.  The first matching rule gives (v, w):
 *                  1  d1 <= 0 && d2 <= 0                          (0, 0)
 *                  2  d3 >= 0 && d4 <= d3                         (1, 0)
 *                  3  vc <= 0 && d1 >= 0 && d3 <= 0               (d1 / (d1 - d3), 0)
 *                  4  d6 >= 0 && d5 <= d6                         (0, 1)
 *                  5  vb <= 0 && d2 >= 0 && d6 <= 0               (0, d2 / (d2 - d6))
 *                  6  va <= 0 && d4 - d3 >= 0 && d5 - d6 >= 0     e = (d4 - d3) / ((d4 - d3) + (d5 - d6)), (1 - e, e)
 *                  7  otherwise                                   den = 1 / ((va + vb) + vc), (vb den, vc den)
 *                c = (a + ab v) + ac w componentwise, r = p - c, d^2 = (r0^2 + r1^2) + r2^2
 *   selection    the minimum d^2 wins, ties go to the lowest triangle index; a NaN d^2 never wins.  dist = sqrt(d^2),
 *                uv = (v, w), side = the sign (-1 / 0 / +1) of r . (ab x ac) with the cross product formed as
 *                (x1 y2 - x2 y1, x2 y0 - x0 y2, x0 y1 - x1 y0): the side of the chosen face's normal, exact where the closest
 *                point lies inside a face and a convention on edges and vertices
 *   non-finite   a point with a NaN / infinite coordinate gets NaN in closest, dist and uv, 0xFFFFFFFF in prim_id and 0 in
 *                side; the other points are not touched.  If no triangle is left (all skipped, F = 0, or every d^2 is
 *                +inf or NaN): dist = +inf, prim_id = 0xFFFFFFFF, closest and uv NaN, side 0
 *   determinism  a point's outputs depend on that point and the mesh's records alone: not on N, its position in the
 *                batch, its neighbours, the handle's history or `exhaustive`; the culled search (the default) returns
 *                the bits of the exhaustive one in every output
 * pts N x 3; every output may be null.  All pointers are host or device memory by `mem`; PEDP_DEVICE only enqueues on the
 * context's stream.  N = 0 does nothing; N > 2^24 is PEDP_ERR_BAD_ARG.  The call's workspace (one counter, and the
 * staging of a host-memory call) is its own, so PEDP_DEVICE calls are allowed while a registration is pending on ctx
 * (pedp_icp_begin); PEDP_HOST calls and pedp_closest_last_stats, which wait on the context's stream, are
 * PEDP_ERR_BAD_ARG then.
 * pedp_closest_configure: exhaustive = 1 tests every point against every triangle (the yardstick), 0 culls on the
 * mesh's bounding spheres, with a wave per point up to 16384 points and a lane per point above; 2 and 3 are 0 with
 * the lane-per-point or the wave-per-point kernel at every N (for tests and measurements: the bits are the same).  pedp_closest_last_stats: the point-triangle pairs the last call on ctx evaluated (finite
 * points x unskipped triangles tested; it waits for the stream). */
int pedp_closest_points(pedp_ctx_t ctx, pedp_mesh_t mesh, const double *pts, int64_t N, int mem, double *closest,
                        double *dist, uint32_t *prim_id, double *uv, int8_t *side);
int pedp_closest_configure(pedp_ctx_t ctx, int exhaustive);
int pedp_closest_last_stats(pedp_ctx_t ctx, int64_t *pairs_tested);
/* The unit normals (ab x ac) / |ab x ac| of the N triangles listed in prim_id (the cross product as above, the length as
 * sqrt((x^2 + y^2) + z^2), one division per component), N x 3 float64; NaN for an id >= F and for a degenerate record.
 * Memory, bounds and the pending-registration rule as pedp_closest_points. */
int pedp_mesh_face_normals(pedp_ctx_t ctx, pedp_mesh_t mesh, const uint32_t *prim_id, int64_t N, int mem, double *normals);

/* ---------------------------------------------------------------- robust best fit of a cloud to the mesh's surface
 * Iteratively re-weighted Gauss-Newton of N points onto the mesh as posed: the pose correction T (row-major 4 x 4) that
 * brings the points onto the surface itself, with a loss that keeps a defect from pulling the pose.  The whole loop runs
 * on the device; the contract is DESIGN.md s4.21.  State: T, float64, starting from `init` (HOST memory whatever `mem` is,
 * read before the call returns; null: the identity).  Pass p = 0, 1, ...:
 *   search     for every finite row p_i of pts (never rewritten): q_i = R p_i + t of the current T, each component
 *              ((T[4k] x + T[4k+1] y) + T[4k+2] z) + T[4k+3]; (c_i, d_i, face_i) of q_i from the search of
 *              pedp_closest_points (the same point_triangle, selection and culling margin).  A non-finite row, and a row
 *              with no triangle, takes no part
 *   row        an inlier has d_i <= gate; every other row adds nothing to any sum.  r = q - c (the bits the search formed),
 *              n = r / d componentwise when d > 0, else the unit normal of face_i as pedp_mesh_face_normals forms it.
 *              weight w: PEDP_FIT_L2 1; PEDP_FIT_HUBER 1 if d <= scale, else scale / d; PEDP_FIT_TUKEY
 *              t t with t = 1 - u u, u = d / scale, if d < scale, else 0.  J = [q x n, n] (the cross product as above),
 *              wJ = w J componentwise
 *   sums       the packet: [0, 21) wJ_a J_b for a <= b row by row of the upper triangle, [21, 27) wJ_a d, [27] d d,
 *              [28] 1 (their sum is K), [29] w.  Blocks of 256 consecutive points; inside a block the 64 rows of each
 *              quarter by a butterfly (l with l ^ 32, then ^ 16, 8, 4, 2, 1), the quarters as (s0 + s1) + (s2 + s3); then
 *              the blocks in index order, starting from 0.  No floating-point atomics: the packet's bits depend on the
 *              points, the records and T alone, not on the search kernel, the context's history or `mem`
 *   close      fitness = K / (finite rows), rmse = sqrt(packet[27] / K), both 0 when K = 0; trace row p (if asked for):
 *              fitness, rmse, T as the pass found it, 18 doubles like pedp_icp's.  The loop ends when p == max_iteration,
 *              when K == 0, or when p > 0 and |fitness - previous| < relative_fitness and |rmse - previous| <
 *              relative_rmse.  Otherwise x = solve(A, -b) by pedp_icp's pivoted LDLT, upd = its T(x) (Rz Ry Rx of x[2],
 *              x[1], x[0] and the translation x[3..5]), T <- upd T.  A non-finite x or T ends the loop with T unchanged and
 *              `singular` set; so does a pass whose sums are not finite (a pose thrown far off by a rank-deficient solve):
 *              T, fitness, rmse and the packet are then those of the last pass that could be closed
 * scale is in the mesh's units and must be positive for HUBER and TUKEY (ignored for L2); gate >= 0 (+inf: none);
 * 0 <= max_iteration <= 1000.  pts, T_out (16), stats_out (PEDP_FIT_STATS_DOUBLES) and trace_out (18 x (max_iteration + 1),
 * rows behind the last pass left as they were (PEDP_DEVICE) or zero (PEDP_HOST)) are host or device memory by `mem`; the
 * three outputs may be null.  stats_out: [0] fitness and [1] rmse of the last pass, [2] its index (the updates applied),
 * [3] K, [4] sum of w, [5] 1 if a solve was singular, [6] finite rows, [7] 0, [8, 38) the packet of the last pass, [38, 40) 0.
 * All passes are enqueued without a host wait (a device flag turns the launches behind the last pass into early exits);
 * PEDP_DEVICE only enqueues, PEDP_HOST reads the results back once at the end.  N = 0 gives T = init and zero statistics;
 * N > 2^24 is PEDP_ERR_BAD_ARG.  The workspace is the call's own (not pedp_icp's), but a context holds one of it and the
 * passes are ordered on its stream: while a registration is pending on ctx (pedp_icp_begin) the call is
 * PEDP_ERR_BAD_ARG in either memory form. */
enum { PEDP_FIT_L2 = 0, PEDP_FIT_HUBER = 1, PEDP_FIT_TUKEY = 2 };
#define PEDP_FIT_STATS_DOUBLES 40
int pedp_fit_to_surface(pedp_ctx_t ctx, pedp_mesh_t mesh, const double *pts, int64_t N, int mem, const double *init, int loss,
                        double scale, double gate, int max_iteration, double relative_fitness, double relative_rmse,
                        double *T_out, double *stats_out, double *trace_out);

/* ---------------------------------------------------------------- the defect map: per-face accumulation and regions
 * What the projected heat maps of many frames say about the CAD model itself: per face the peak intensity, the hits and
 * the frames that saw it, and the connected regions of the marked faces with their sizes.  It stands in the place of
 * run.py:61, :119, :196-201, which keep a growing list of hit clouds and move every one of them at every detection:
 * triangle indices keep the input's order in every mesh handle whatever the pose, so a map kept per face in the MODEL
 * frame is a constant-size object that never needs a transform.  The contract is DESIGN.md s4.17.
 *
 * pedp_defect_map_create: verts V x 3 float64 and tris F x 3 on the host, the model frame.  A mesh handle keeps neither,
 * so the map takes them itself; it is tied to a mesh only by the shared triangle order.  An index >= V is
 * PEDP_ERR_BAD_ARG; F = 0 is allowed; F > 2^28 is PEDP_ERR_BAD_ARG.  Built on the device and kept resident, float64, no
 * contraction, every expression in the order written (a, b, c: the face's corners):
 *   area[f]      0.5 * sqrt((n0^2 + n1^2) + n2^2), n = ab x ac formed as (x1 y2 - x2 y1, x2 y0 - x0 y2, x0 y1 - x1 y0),
 *                ab = b - a, ac = c - a
 *   centroid[f]  ((a + b) + c) / 3 componentwise
 *   box[f]       minimum and maximum of the corners per axis, -0 below +0; a NaN coordinate takes no part
 *   weld         w[v] = the lowest index of a vertex whose three coordinates compare equal with == (so -0 equals +0, and a
 *                vertex with a NaN is welded to nothing): OBJ files duplicate vertices along UV seams, and a defect
 *                must not fall apart there
 *   adjacency    two faces are neighbours iff they share an unordered edge {w_i, w_j} with w_i != w_j; any number of
 *                faces may share an edge and are then all neighbours of each other; a face's edge with w_i == w_j is
 *                no edge
 * The call returns after the build; it waits on the context's stream, so it is PEDP_ERR_BAD_ARG while a registration is
 * pending on ctx (pedp_icp_begin).
 *
 * pedp_defect_map_add is one OBSERVATION (one frame's hits): for every row with prim_id < F and a non-NaN intensity
 *   peak[f] = max(peak[f], intensity) with +0 above -0;  hits[f] += 1 (64-bit);  frames[f] += 1 ONCE per observation
 * whatever the number of rows on f.  Rows with 0xFFFFFFFF (a miss), any other id >= F or a NaN intensity are ignored and
 * counted.  n = 0 still counts as an observation.  PEDP_DEVICE only enqueues on the context's stream and is allowed
 * while a registration is pending on the context (pedp_icp_begin); PEDP_HOST is PEDP_ERR_BAD_ARG then.  Runs of equal
 * ids in neighbouring rows (hits arrive in pixel order) are combined inside a wave before the atomics.  There is no
 * floating-point atomic: the maximum is an integer atomic max on an order-preserving 64-bit key, the counts are integer
 * atomics.  The per-face state after a sequence of calls is a function of the multiset of rows of each observation
 * alone: not of the rows' order, of how an observation's rows sit in memory, or of the handle's history before the
 * last pedp_defect_map_clear (which forgets everything, the observation count included).
 * pedp_defect_map_faces: F values each, every pointer nullable, host or device memory by `mem`; a face never hit reads
 * peak 0, hits 0, frames 0 (PEDP_HOST and a pending registration: as for add).  pedp_defect_map_stats: observations, rows taken and rows ignored since the last clear (it
 * waits on the stream: PEDP_ERR_BAD_ARG while a registration is pending).
 *
 * pedp_defect_map_regions:
 *   1  a face is MARKED iff hits > 0 && peak > threshold && frames >= min_frames (strictly above the threshold, like
 *      heatmap_to_points)
 *   2  the marking is grown `grow` times (0 <= grow <= 64): a face is marked after a round if it or one of its
 *      neighbours was marked before the round.  This bridges the faces that lie BETWEEN two pixels' rays on a mesh
 *      whose triangles are smaller than a pixel's footprint
 *   3  regions are the connected components of the marked faces under the adjacency, numbered 0 ... R - 1 by their
 *      lowest face index
 * labels (F x int32, nullable): the region of each face or -1.  table (nullable with capacity 0): one row per region.
 * If R > capacity nothing is written to table, n_regions still reports R and the call returns PEDP_ERR_BAD_ARG, like
 * pedp_project_heatmap; capacity = F always suffices.  n_regions is a host scalar, so the call waits on the stream, and
 * like pedp_closest_last_stats it is PEDP_ERR_BAD_ARG while a registration is pending on the context.  The workspace is
 * the map's own (its two sorts use the context's pooled sort buffers, like every sort of the library): never the pinned
 * result block, never the ICP workspace.  area and moment are floating-point sums formed in a fixed order: the same bits on
 * every call for the same per-face state. */
typedef struct pedp_defect_map_s *pedp_defect_map_t;
typedef struct pedp_defect_region {
    int32_t first_face;    /* the region's lowest face index */
    int32_t n_faces;       /* faces after the growth */
    int32_t n_seed_faces;  /* faces marked before the growth */
    int32_t max_frames;    /* largest `frames` among the faces */
    int64_t hits;          /* sum of the faces' hits */
    double area;           /* sum of the faces' areas */
    double centroid[3];    /* moment / area; NaN for a region of zero area */
    double moment[3];      /* sum of area * centroid over the faces: the centroid's numerators */
    double peak;           /* maximum over its faces with hits */
    double lo[3], hi[3];   /* the box of its faces' vertices */
} pedp_defect_region;
int pedp_defect_map_create(pedp_ctx_t ctx, const double *verts, int64_t V, const uint32_t *tris, int64_t F, pedp_defect_map_t *out);
int pedp_defect_map_destroy(pedp_defect_map_t map);
int pedp_defect_map_size(pedp_defect_map_t map, int64_t *V, int64_t *F);
int pedp_defect_map_add(pedp_defect_map_t map, const uint32_t *prim_id, const double *intensity, int64_t n, int mem);
int pedp_defect_map_clear(pedp_defect_map_t map);
int pedp_defect_map_faces(pedp_defect_map_t map, int mem, double *peak, int64_t *hits, int32_t *frames);
int pedp_defect_map_stats(pedp_defect_map_t map, int64_t *observations, int64_t *rows_added, int64_t *rows_ignored);
int pedp_defect_map_regions(pedp_defect_map_t map, double threshold, int32_t min_frames, int32_t grow, int mem, int32_t *labels,
                            int64_t capacity, pedp_defect_region *table, int64_t *n_regions);

/* ---------------------------------------------------------------- the coverage map: which faces were seen, and how well
 * The defect map says which faces are defective; it cannot say whether the whole part was looked at: a face with
 * peak 0, hits 0, frames 0 is either clean or never seen.  The coverage map keeps, per face of the model, the evidence
 * that the camera observed it.  The reference has no counterpart (run.py shows hit clouds and never says what was not
 * inspected); the contract is DESIGN.md s4.20.
 *
 * pedp_coverage_create lays the coverage state over the faces of a defect map and borrows its areas, centroids, boxes,
 * adjacency and region scratch: one weld and one adjacency per model.  The map must outlive the coverage handle; the
 * handle lives on the map's context.  The map's own per-face state is neither read nor written by any call here.
 * PEDP_ERR_BAD_ARG while a registration is pending on the context.
 *
 * pedp_coverage_add is one VIEW (one camera frame).  mesh: a handle of the map's context with the map's F, posed as the
 * frame sees it, in the camera's frame.  cam: the pinhole whose pixel rays from the origin were cast against it (fx, fy
 * positive); t_hit height x width float32 and prim_id height x width uint32 are that cast's results, row-major, pixel
 * i = y width + x.  depth (nullable): height x width float32, the sensor's image; mask (nullable): height x width
 * uint8; status (nullable): height x width uint8, the class of every pixel.  prm (NULL without depth: depth_scale 1,
 * min_cos 0, z_min 0.001): depth_tol, in mesh units, is the sensor's and has no default.  Per pixel, float64, no
 * contraction, every expression in the order written:
 *   d        the ray that was cast: (xn, yn, 1) / sqrt((xn xn + yn yn) + 1), xn = (x - cx) / fx, yn = (y - cy) / fy
 *            (pedp_project_heatmap's arithmetic), each component rounded to float32 and widened again
 *   z_hit    t_hit d_z;   z_meas = (double)depth depth_scale
 *   n        the unit normal (ab x ac) / |ab x ac| of record prim_id as posed, as pedp_mesh_face_normals forms it
 *   cos      min(|(n_x d_x + n_y d_y) + n_z d_z|, 1); 0 for a record that no ray can hit or a normal that is NaN
 *   footprint  ((z_hit z_hit) d_z) / ((fx fy) cos): the area of surface one pixel covers, t^2 dOmega / cos with
 *            dOmega = d_z^3 / (fx fy); +inf at cos = 0
 * The pixel gets exactly one class, the first of these rules that holds:
 *   0 MASKED    a mask is given and mask[i] == 0
 *   1 MISS      prim_id >= F (0xFFFFFFFF included), or t_hit is not finite
 *   2 NO_DEPTH  depth is given and it is not true that depth[i] >= z_min (float32, as pedp_depth_to_scene compares),
 *               or the depth is infinite; NaN falls here
 *   3 OCCLUDED  depth is given and z_meas - z_hit < -depth_tol: something stands in front of the surface
 *   4 BEHIND    depth is given and z_meas - z_hit > depth_tol: the sensor looked through where the model has surface
 *   5 GRAZING   cos < min_cos
 *   6 SEEN      otherwise; a difference of exactly depth_tol is SEEN
 * For the SEEN pixels on face f: pixels[f] += 1 (64-bit); views[f] += 1 ONCE per view; best_cos[f] is raised to cos;
 * min_footprint[f] is lowered to the footprint (a NaN footprint -- t_hit = 0 at cos = 0 -- takes no part).  For the
 * OCCLUDED pixels on f: blocked[f] += 1.  Seven 64-bit class counters and the view count are kept per handle.  Integer
 * atomics only, as for pedp_defect_map_add: the maximum on the order-preserving key, the minimum on the bits of the
 * non-negative double, counts, and the view stamp; runs of equal faces in neighbouring pixels are combined inside a
 * wave before the atomics.  The state after a sequence of views is a function of each view's pixels alone: not of their
 * order, of how they sit in memory, or of the handle's history before the last pedp_coverage_clear.
 * PEDP_DEVICE only enqueues on the context's stream, has no workspace and is allowed while a registration is pending on
 * the context (pedp_icp_begin); PEDP_HOST copies in and out, returns after completion and is PEDP_ERR_BAD_ARG then.
 * PEDP_ERR_BAD_ARG also when the mesh's F is not the map's, when the mesh is of another context, when depth is given
 * and depth_tol is negative or NaN (or prm is NULL), and when min_cos is outside [0, 1].
 *
 * pedp_coverage_faces: F values each, every pointer nullable, host or device memory by `mem`; a face never seen reads
 * pixels 0, views 0, best_cos 0.0, min_footprint +inf, blocked 0.  pedp_coverage_stats: the views and the pixels of each
 * class since the last clear (classes nullable; with it the call waits on the stream: PEDP_ERR_BAD_ARG while a
 * registration is pending).
 *
 * A face is COVERED under criteria c iff views >= c.min_views && pixels >= c.min_pixels && best_cos >= c.min_cos &&
 * min_footprint <= c.max_footprint on the values pedp_coverage_faces reads; NULL means 1, 1, 0, +inf.
 * pedp_coverage_summary: the covered faces, their area and the model's area.  The two areas are summed in s4.17's
 * block-and-butterfly order over the faces in face order (blocks of 4096 consecutive faces): the same bits on every call
 * for the same per-face state.  It waits on the stream (PEDP_ERR_BAD_ARG while a registration is pending).
 * pedp_coverage_regions: the connected regions of the UNCOVERED faces (covered = 0: where to point the camera next) or of
 * the covered ones (covered != 0), through the body of pedp_defect_map_regions: growth, numbering by the lowest face,
 * the table's sums, the overflow rule (R > capacity) and the pending rule are that call's.  In a row, hits is the sum of
 * the faces' pixels, max_frames the largest views, peak the largest best_cos over the faces with pixels (0 if none). */
typedef struct pedp_coverage_s *pedp_coverage_t;
typedef struct pedp_coverage_view {
    double depth_scale;    /* z_meas = (double)depth * depth_scale: 1000 for metres against a mesh in millimetres */
    double depth_tol;      /* mesh units; >= 0 whenever depth is given */
    double min_cos;        /* 0 ... 1 */
    float z_min;           /* validity of a depth: 0.001 */
} pedp_coverage_view;
typedef struct pedp_coverage_criteria {
    int32_t min_views;
    int64_t min_pixels;
    double min_cos, max_footprint;
} pedp_coverage_criteria;
typedef struct pedp_coverage_totals {
    int64_t covered_faces, faces;
    double covered_area, total_area;
} pedp_coverage_totals;
int pedp_coverage_create(pedp_defect_map_t map, pedp_coverage_t *out);
int pedp_coverage_destroy(pedp_coverage_t cov);
int pedp_coverage_add(pedp_coverage_t cov, pedp_mesh_t mesh, const pedp_pinhole *cam, const float *t_hit, const uint32_t *prim_id,
                      const float *depth, const uint8_t *mask, const pedp_coverage_view *prm, int mem, uint8_t *status);
int pedp_coverage_clear(pedp_coverage_t cov);
int pedp_coverage_faces(pedp_coverage_t cov, int mem, int64_t *pixels, int32_t *views, double *best_cos, double *min_footprint,
                        int64_t *blocked);
int pedp_coverage_stats(pedp_coverage_t cov, int64_t *views, int64_t classes[7]);
int pedp_coverage_summary(pedp_coverage_t cov, const pedp_coverage_criteria *c, pedp_coverage_totals *out);
int pedp_coverage_regions(pedp_coverage_t cov, const pedp_coverage_criteria *c, int covered, int32_t grow, int mem, int32_t *labels,
                          int64_t capacity, pedp_defect_region *table, int64_t *n_regions);

/* ---------------------------------------------------------------- next-best-view planning over the coverage map
 * pedp_coverage_regions says where the part was not looked at; the view plan turns that into the next camera poses: it
 * keeps what each of a set of CANDIDATE views would add to the coverage map, scores all of them against a working copy of
 * the map's state, and picks greedily.  The coverage map itself is never written by any call here.  The contract is
 * DESIGN.md s4.22.
 *
 * pedp_view_plan_create: room for `capacity` (>= 1) candidates over the faces of `cov`, on its context: one allocation of
 * capacity F 20 bytes of observation columns plus the working state and the sums' scratch; a failed allocation is
 * PEDP_ERR_HIP.  The plan starts without candidates and with the working state of a map that saw nothing.  The coverage
 * handle must outlive the plan.  PEDP_ERR_BAD_ARG while a registration is pending on the context.
 * pedp_view_plan_clear forgets the candidates (the working state stays).
 *
 * pedp_view_plan_observe appends one candidate and returns its index: mesh, cam, t_hit, prim_id and min_cos are those of
 * a pedp_coverage_add WITHOUT depth and mask, and the candidate's row holds, per face f, what that view would add:
 *   cpix[f]  the SEEN pixels on f (uint32)      ckey[f]  the largest key of their cosines (0: none)
 *   cfp[f]   the bits of their smallest footprint (all ones: none)
 * by the per-pixel rule of pedp_coverage_add, bit for bit (one routine serves both).  Integer atomics only.  The checks
 * are pedp_coverage_add's, and the plan must not be full.  PEDP_DEVICE only enqueues and is allowed while a registration
 * is pending; PEDP_HOST copies in, returns after completion and is PEDP_ERR_BAD_ARG then.
 * pedp_view_plan_candidate reads row v back in the units of pedp_coverage_faces (pixels, best_cos 0.0 / min_footprint
 * +inf where the view sees nothing of the face); every pointer nullable, host or device memory by `mem`.
 *
 * The WORKING STATE w is the plan's own copy of the map's per-face pixels, views, best and minfp.
 * pedp_view_plan_reset: w := the coverage map's state now.  pedp_view_plan_commit: candidate v is MERGED into w, per face
 *   pixels += cpix;  views += (cpix > 0);  key = max(key, ckey);  fp = min(fp, cfp) on the bits
 * which is the state pedp_coverage_add of that view would leave.  Both only enqueue.
 *
 * PROGRESS of a face under criteria c (NULL: 1, 1, 0, +inf) is the integer
 *   n = (pixels >= c.min_pixels && best_cos >= c.min_cos && min_footprint <= c.max_footprint)
 *         ? (c.min_views <= 0 ? 1 : min(views, c.min_views)) : 0,      m = max(c.min_views, 1)
 * so n == m exactly when the face is covered.  The GAIN of candidate v against w: per face D = n(w merged with v) - n(w)
 * (>= 0; 0 wherever cpix is 0), the term (area[f] (double)D) / (double)m (+0 where D is 0), and
 *   gain_area[v]   the sum of the terms in s4.17's block-and-butterfly order over the faces in face order (blocks of
 *                  4096 consecutive faces, lane l adds l, l + 64, ... one after the other from +0, the butterfly xor
 *                  32 ... 1 adds the lanes, one wave adds the block sums the same way); no floating-point atomic
 *   gain_faces[v]  the faces with n(w) < m and n(merged) == m
 * With min_views 1 the gain is the area pedp_coverage_add at that pose would newly cover; with min_views 2 a first
 * qualifying view earns half a face's area.  pedp_view_plan_score: both for every candidate (n values each, either
 * pointer nullable), host or device memory; PEDP_DEVICE only enqueues.
 *
 * pedp_view_plan_select: w := the map's state, no candidate chosen; then at most k rounds: score the candidates not yet
 * chosen; among those whose gain_area is > min_gain take the largest, the lowest index among equals (a NaN never wins);
 * if there is none, stop; else record (index, gain_area, gain_faces), merge the candidate into w and mark it chosen.  The
 * rounds are enqueued back to back, the choice and the stop are made on the device, and the host waits once.  order,
 * gain_area and gain_faces (room for min(k, candidates) entries each, nullable) get the *n_selected recorded rounds;
 * totals (nullable) the summary of w afterwards, as pedp_coverage_summary forms it.  w stays as the rounds left it.
 * pedp_view_plan_select, and _candidate / _score / _observe with PEDP_HOST, wait on the stream: PEDP_ERR_BAD_ARG while a
 * registration is pending. */
typedef struct pedp_view_plan_s *pedp_view_plan_t;
int pedp_view_plan_create(pedp_coverage_t cov, int64_t capacity, pedp_view_plan_t *out);
int pedp_view_plan_destroy(pedp_view_plan_t plan);
int pedp_view_plan_clear(pedp_view_plan_t plan);
int pedp_view_plan_observe(pedp_view_plan_t plan, pedp_mesh_t mesh, const pedp_pinhole *cam, const float *t_hit, const uint32_t *prim_id,
                           double min_cos, int mem, int64_t *index);
int pedp_view_plan_candidate(pedp_view_plan_t plan, int64_t v, int mem, int64_t *pixels, double *best_cos, double *min_footprint);
int pedp_view_plan_reset(pedp_view_plan_t plan);
int pedp_view_plan_commit(pedp_view_plan_t plan, int64_t v);
int pedp_view_plan_score(pedp_view_plan_t plan, const pedp_coverage_criteria *c, int mem, double *gain_area, int64_t *gain_faces);
int pedp_view_plan_select(pedp_view_plan_t plan, const pedp_coverage_criteria *c, int64_t k, double min_gain, int32_t *order,
                          double *gain_area, int64_t *gain_faces, int64_t *n_selected, pedp_coverage_totals *totals);

/* ---------------------------------------------------------------- the solid: signed distance and occupancy
 * RaycastingScene.compute_signed_distance / compute_occupancy on the mesh handle: whether a point lies inside the CAD
 * solid (a dent, missing material) or outside it (a burr, excess material), which `side` above cannot tell away from
 * the inside of a face.  The contract is DESIGN.md s4.18.
 *
 * pedp_solid_create: the topology of the model, built once from verts V x 3 float64 and tris F x 3 on the host (the
 * arrays a mesh handle or a defect map is made from), independent of any pose.  Bounds and errors as
 * pedp_defect_map_create; the weld and the edge slots are the defect map's (one implementation):
 *   weld         as above: == on the positions, -0 equals +0, a vertex with a NaN welds to nothing
 *   edge slot    3 f + k joins corners k and (k + 1) % 3 of face f.  The slots of one unordered pair of welded vertices
 *                form an edge: one slot is a BOUNDARY edge, three or more a NON-MANIFOLD edge, two are TWINS if the two
 *                faces run through the edge in opposite directions and a FLIPPED edge if in the same
 *   volume       the sum over the faces of a . (b x c) / 6 on the float64 vertices (cross and dot as above), in a fixed
 *                order: thread t of a block of 256 adds its faces t, t + 256, ... of the block's 4096 one after the
 *                other, the threads' sums are added pairwise (t with t + 128, t + 64, ... t + 1), and one block adds
 *                the blocks' sums in the same way.  No floating-point atomic
 * Creation succeeds on any mesh; `closed` says whether the mesh bounds a solid (a check of a CAD export on its own).
 * The handle keeps the index buffer, the welded id of every corner, the twin of every edge slot and, per welded vertex,
 * its corners sorted by (face, corner).  The call waits on the context's stream (PEDP_ERR_BAD_ARG while a registration
 * is pending on ctx).
 *
 * pedp_signed_distance: the closest point c of every point p is the one of the search above (the same kernels, the same
 * cull, the same expressions), and the rule 1 ... 7 that decided (v, w) for the chosen triangle names the closest
 * FEATURE, whose angle-weighted pseudonormal N (Baerentzen & Aanaes 2005) is formed from the mesh's records AS POSED,
 * with n(f) = (ab x ac) / |ab x ac| as pedp_mesh_face_normals forms it:
 *   rule 7           the face: N = n(f)
 *   rules 3, 6, 5    the edge slots 0, 1, 2: N = n(f) + n(face of the twin slot) componentwise
 *   rules 1, 2, 4    the corners 0, 1, 2: N = the sum, over the corners of the welded vertex in (face, corner) order
 *                    starting from 0, of n(g) angle, with angle = atan2(|q x s|, q . s) between the record's two edges
 *                    that leave the corner: (ab, ac), (ac - ab, -ab), (-ac, ab - ac) for corner 0, 1, 2
 *   A record that the search skips, or whose ab x ac has no length, adds nothing to an edge's or a vertex's N.
 *   sign             s = ((p - c) . N) orientation; sdist = s < 0 ? -dist : dist, so s == 0 counts as outside;
 *                    |sdist| has the bits of pedp_closest_points' dist.  occupancy = sdist < 0.  feature = 0 / 1 / 2
 *                    for face / edge / vertex.  normal = (N / sqrt(N . N)) orientation: the outward unit pseudonormal
 *                    (NaN where N is zero)
 *   non-finite       a point with a NaN / infinite coordinate: sdist NaN, occupancy 0, feature 255, normal NaN; no
 *                    triangle left (F = 0, all skipped): sdist +inf, occupancy 0, feature 255, normal NaN
 *   determinism      as pedp_closest_points: a point's outputs depend on that point, the records and the solid alone
 * The sign is exact -- it IS the inside / outside of the solid -- for a closed, consistently oriented mesh and a point
 * that is not on the surface; where rounding moves a point from one of Ericson's regions to a neighbouring one the two
 * features' pseudonormals give the same sign, by continuity.  For a point within rounding of the surface itself
 * (dist of the order of the records' float32 resolution) the sign is a convention, as `side` is on edges and vertices.
 * PEDP_ERR_BAD_ARG: the solid is not closed (boundary, non-manifold or flipped edges) or has orientation 0, unless
 * F = 0; solid F != mesh F; a posable mesh, which keeps its index buffer, whose indices differ from the solid's
 * (compared on the device at the first call with that mesh, which therefore waits on the stream); a mesh or a solid
 * of another context; N > 2^24; a registration pending on ctx -- in either memory: the workspace (the vertices' table
 * and the search's outputs) is the solid's own and is sized by V and N, so that the call may have to wait for the
 * device to grow it.  Never the pinned result block, never the ICP workspace.  pts N x 3; every output may be null;
 * all pointers host or device memory by `mem`; PEDP_DEVICE only enqueues on the context's stream (after the first call). */
typedef struct pedp_solid_s *pedp_solid_t;
typedef struct pedp_solid_info {
    int64_t V, F, welded_vertices, edges;
    int64_t boundary_edges;     /* edges with one face */
    int64_t nonmanifold_edges;  /* edges with three or more faces */
    int64_t flipped_edges;      /* two-face edges that both faces run through in the same direction */
    int64_t degenerate_faces;   /* two corners weld to one vertex */
    int32_t closed;             /* 1 iff the three edge counts above are all zero and F > 0 */
    int32_t orientation;        /* sign of volume: +1 normals point out, -1 in, 0 */
    double  volume;             /* sum over faces of a . (b x c) / 6, float64, fixed order */
} pedp_solid_info;
int pedp_solid_create(pedp_ctx_t ctx, const double *verts, int64_t V, const uint32_t *tris, int64_t F, pedp_solid_t *out);
int pedp_solid_destroy(pedp_solid_t solid);
int pedp_solid_get_info(pedp_solid_t solid, pedp_solid_info *out);
int pedp_signed_distance(pedp_ctx_t ctx, pedp_mesh_t mesh, pedp_solid_t solid, const double *pts, int64_t N, int mem,
                         double *sdist, int8_t *occupancy, uint8_t *feature, double *normal);

/* ---------------------------------------------------------------- the deviation map: per-face statistics of signed deviation
 * How far off is the part on this face, measured over everything the camera saw, and how certain is that?  The defect
 * map keeps a PEAK per face, which a noisy measurement biases upwards with every frame; the deviation map keeps the
 * count, sum, sum of squares, extremes and frames of the SIGNED distance per face, so that noise shrinks with sqrt(n),
 * the sign and the millimetres are kept, and a region has a volume of excess or missing material.  The reference has no
 * counterpart; the contract is DESIGN.md s4.23.
 *
 * pedp_deviation_map_create lays the state over the faces of a defect map and borrows its areas, adjacency and region
 * scratch, as pedp_coverage_create does; the map must outlive the handle.  It allocates device memory (PEDP_ERR_BAD_ARG
 * while a registration is pending on the context).
 *
 * pedp_deviation_map_add is one OBSERVATION: one frame's rows (prim_id, d), d the signed distance in the mesh's unit,
 * negative inside the solid.  A row is TAKEN iff prim_id < F, d is not NaN and |d| <= gate; gate is per call,
 * 0 <= gate <= 1024, anything else (NaN included) is PEDP_ERR_BAD_ARG.  Rows with a bad id or a NaN d are IGNORED,
 * the other rows with |d| > gate (+-inf included) are GATED; both are counted.  n = 0 still counts as an observation.
 * A taken row is quantised, q = rint(d 2^20) as int64, round half to even (the product is exact in float64, |q| <= 2^30),
 * and the face's state takes it with integer atomics alone:
 *   n += 1 (int64)   S1 += q (int64)   S2 += q q, exact in 128 bits, kept as two uint64 sums of (q q & 0xFFFFFFFF) and
 *   (q q >> 32)   qmin = min(qmin, q)   qmax = max(qmax, q)   frames += 1 ONCE per observation (the defect map's stamp)
 * Runs of equal ids in neighbouring rows are combined inside a wave before the atomics (integer sums are exact and
 * associative: no bit changes).  The state after any sequence of calls is a function of the multiset of taken rows of
 * each observation alone: not of the rows' order, of how they sit in memory, of host or device memory, or of the
 * handle's history before the last pedp_deviation_map_clear.  PEDP_DEVICE only enqueues and is allowed while a
 * registration is pending; PEDP_HOST is PEDP_ERR_BAD_ARG then.
 *
 * pedp_deviation_map_add_points is one observation made from a frame's points with ONE search: pedp_closest_launch on
 * pts (N x 3 float64, the mesh's frame), the solid's vertex pseudonormals, and one kernel that signs the distance of
 * every point exactly as pedp_signed_distance does (one routine) and feeds the row (prim_id, sdist) to the accumulation
 * above; no N-sized result is written.  The checks are pedp_signed_distance's, and the mesh's F must be the map's.
 * origin (nullable, 3 doubles in HOST memory whatever `mem` is): the camera centre in the mesh's frame; a row with a
 * closest feature of pseudonormal N is then taken only if ((origin - c) . N) orientation > 0 -- a depth point cannot
 * have been measured on a surface that faces away -- and is otherwise counted as BACKFACING, before the gate.  The
 * workspace is the handle's own, sized by V and N: PEDP_ERR_BAD_ARG while a registration is pending, in either memory.
 *
 * pedp_deviation_map_faces: F values each, every pointer nullable, host or device memory by `mem`:
 *   n, frames, s1 = S1, s2_hi / s2_lo = S2 as (hi64, lo64)
 *   min = qmin 2^-20, max = qmax 2^-20 (exact);  mean = ((double)S1 / (double)n) 2^-20
 *   std = sqrt(var), var = (D(n S2 - S1 S1) / ((double)n (double)n)) 2^-40 with the integer formed exactly in 128 bits
 *   and D the double nearest to it, ties to even; valid for n < 2^33, above that std is NaN
 * A face with n = 0 reads n 0, frames 0 and NaN for mean, std, min and max.
 * pedp_deviation_map_stats: observations, rows taken, ignored, gated and backfacing since the last clear (waits on the
 * stream unless only observations is asked for).
 *
 * Criteria (NULL: threshold 0, z 0, min_samples 1, min_frames 1, sign 0).  A face is MARKED iff n >= min_samples and
 * frames >= min_frames and the sign test holds -- sign 0: |mean| > threshold; +1: mean > threshold (excess material);
 * -1: mean < -threshold (missing material); another sign is PEDP_ERR_BAD_ARG -- and, when z > 0, also
 * |mean| sqrt((double)n) > z std: significance against the face's own spread.  A face with n = 0 is never marked.
 * pedp_deviation_map_regions: growth, components, numbering, labels and the capacity rule are pedp_defect_map_regions'
 * (one body), with hits = n, frames, and peak = the largest |mean| over the faces with n > 0.  A row is a
 * pedp_defect_region followed by measured_area (sum of area over the region's faces with n > 0), volume (sum of
 * area mean over the same faces: unit^3, signed), mean = volume / measured_area, min_mean and max_mean (NaN when no face
 * of the region has n > 0).  The two sums are formed in the order in which the body sums `area`.
 * pedp_deviation_map_summary: over the MEASURED faces (n > 0 and n >= min_samples) their number and area, the
 * area-weighted mean (sum area mean / measured_area) and RMS (sqrt(sum area mean^2 / measured_area)) of the face means,
 * the largest |mean| and the lowest face that has it (-1: none); the marked faces and their area; the model's area.  The
 * sums take their terms in pedp_coverage_summary's order: the same bits on every call.  Both calls wait on the stream
 * (PEDP_ERR_BAD_ARG while a registration is pending). */
typedef struct pedp_deviation_map_s *pedp_deviation_map_t;
typedef struct pedp_deviation_criteria {
    double threshold, z;
    int64_t min_samples;
    int32_t min_frames, sign;
} pedp_deviation_criteria;
typedef struct pedp_deviation_region {
    pedp_defect_region region;
    double measured_area, volume, mean, min_mean, max_mean;
} pedp_deviation_region;
typedef struct pedp_deviation_totals {
    int64_t faces, measured_faces, marked_faces, max_face;
    double total_area, measured_area, marked_area, mean, rms, max_abs_mean;
} pedp_deviation_totals;
int pedp_deviation_map_create(pedp_defect_map_t map, pedp_deviation_map_t *out);
int pedp_deviation_map_destroy(pedp_deviation_map_t dev);
int pedp_deviation_map_clear(pedp_deviation_map_t dev);
int pedp_deviation_map_add(pedp_deviation_map_t dev, const uint32_t *prim_id, const double *d, int64_t n, double gate, int mem);
int pedp_deviation_map_add_points(pedp_deviation_map_t dev, pedp_mesh_t mesh, pedp_solid_t solid, const double *pts, int64_t N, int mem,
                                  double gate, const double *origin);
int pedp_deviation_map_faces(pedp_deviation_map_t dev, int mem, int64_t *n, int32_t *frames, int64_t *s1, uint64_t *s2_hi, uint64_t *s2_lo,
                             double *min, double *max, double *mean, double *std);
int pedp_deviation_map_stats(pedp_deviation_map_t dev, int64_t *observations, int64_t *rows_taken, int64_t *rows_ignored,
                             int64_t *rows_gated, int64_t *rows_backfacing);
int pedp_deviation_map_summary(pedp_deviation_map_t dev, const pedp_deviation_criteria *c, pedp_deviation_totals *out);
int pedp_deviation_map_regions(pedp_deviation_map_t dev, const pedp_deviation_criteria *c, int32_t grow, int mem, int32_t *labels,
                               int64_t capacity, pedp_deviation_region *table, int64_t *n_regions);

/* ---------------------------------------------------------------- mesh refinement: faces split to a maximum edge length
 * The defect, coverage and deviation maps and the view planner speak per FACE of the model, so a face is the smallest
 * thing they can say anything about -- and a CAD export makes a flat side two triangles.  pedp_mesh_refine gives a model
 * a resolution: every edge longer than max_edge is bisected, round after round, until none is left, and every refined
 * face carries the face of the input it came from, so that each map can be laid over the refined model and read back
 * per CAD face.  The reference prepares a second model file offline for the same need (datareader.py:720-724).  The
 * contract is DESIGN.md s4.25.  Everything is float64, no contraction, every expression in the order written.
 *
 * pedp_mesh_refine: verts V x 3 float64, tris F x 3, host or device memory by `mem`; max_edge > 0; max_faces caps the
 * number of faces of the result (and of the input).  PEDP_ERR_BAD_ARG: an index >= V, a vertex with a non-finite
 * coordinate, max_edge that is not a positive finite number, F > 2^28, V > 2^32 - 2.
 *   weld         w[v] = the lowest index of a vertex at v's position, compared with == (the defect map's weld, one
 *                implementation); a vertex made by a round is unique: w[v] = v
 *   one round    over the current vertices and faces:
 *     long edge    edge (a, b) of a face is LONG iff (dx dx + dy dy) + dz dz > max_edge max_edge with d = b - a.  The
 *                  test is bit-symmetric in a and b, so the faces at an edge always agree, also where the input
 *                  duplicates vertices along the edge (OBJ exports with split normals do)
 *     vertices     every distinct long edge, told apart by its key (min(w_a, w_b), max(w_a, w_b)), gets ONE new vertex
 *                  at 0.5 (a + b) per component (symmetric too); the new vertices follow all existing ones in ascending
 *                  key order
 *     children     every face is replaced, in place in the face order, by 1 ... 4 children that keep its winding;
 *                  corners keep their own indices, not the welded ones.  With edge k = (c_k, c_(k+1)%3):
 *                    none long    the face itself
 *                    one long     rotated so that it is edge 0, m its midpoint: (c0, m, c2), (m, c1, c2)
 *                    two long     rotated so that the short edge is edge 2, m0 = mid(c0, c1), m1 = mid(c1, c2):
 *                                 (m0, c1, m1), then (c0, m0, c2), (m0, m1, c2) if |m0 - c2|^2 <= |m1 - c0|^2 (the same
 *                                 squared-length expression), else (c0, m0, m1), (c0, m1, c2)
 *                    three long   (c0, m0, m2), (m0, c1, m1), (m2, m1, c2), (m0, m1, m2)
 *     parents      parent_face of a child is its parent's; initially parent_face[f] = f
 *   rounds       repeat until a round finds no long edge; a mesh without one is returned unchanged after 0 rounds.  They
 *                end: a 1- or 3-split makes no inner edge longer than max_edge or half an edge of the parent, and a
 *                2-split's diagonal is a median, at most sqrt(3) / 2 of the parent's longest edge.  More faces than
 *                max_faces after a round, more than 64 rounds or more than 2^32 - 2 vertices: PEDP_ERR_BAD_ARG, *out
 *                stays null and *faces_reached (nullable) reports that round's face count; on success it is F_out
 * What follows: the input's V vertices are kept, in order; parent_face is non-decreasing, so the children of an input
 * face are a contiguous run; the surface is unchanged (a new vertex is the midpoint of two vertices of one face); a closed,
 * consistently oriented input stays so, both sides of every edge hold bit-identical points, and they still do after
 * rounding to the mesh handle's float32 records, which is what pedp_solid_create needs.  The result is a pure function of
 * the arrays and max_edge: the same bits on every call and on any context, whatever the context did before (new
 * vertices are numbered by the stable pooled sort, children are placed by a scan; the only atomics are integer minima).
 * Per round the host reads two counts to size the round's outputs, so the call waits on the context's stream:
 * PEDP_ERR_BAD_ARG while a registration is pending on ctx (pedp_icp_begin).  The handle keeps the result on the device.
 *
 * pedp_refined_size: the result's vertex and face counts and the number of rounds that split something.
 * pedp_refined_read: verts V_out x 3, tris F_out x 3, parent_face F_out, each nullable, host or device memory by `mem`;
 * PEDP_DEVICE only enqueues copies on the context's stream; PEDP_HOST is PEDP_ERR_BAD_ARG while a registration is pending.
 * pedp_refined_reduce: folds child_values (F_out) to parent_values (F) over each input face's run, in ascending child
 * index, starting from the run's first value y_0 (every input face has a child): PEDP_REDUCE_SUM acc = acc + y;
 * PEDP_REDUCE_MAX acc = y where y > acc or y is a NaN; PEDP_REDUCE_MIN likewise with <.  A lane per input face; mem as
 * for pedp_refined_read. */
typedef struct pedp_refined_s *pedp_refined_t;
enum { PEDP_REDUCE_MAX = 0, PEDP_REDUCE_MIN = 1, PEDP_REDUCE_SUM = 2 };
int pedp_mesh_refine(pedp_ctx_t ctx, const double *verts, int64_t V, const uint32_t *tris, int64_t F, int mem, double max_edge,
                     int64_t max_faces, pedp_refined_t *out, int64_t *faces_reached);
int pedp_refined_size(pedp_refined_t refined, int64_t *V_out, int64_t *F_out, int32_t *rounds);
int pedp_refined_read(pedp_refined_t refined, int mem, double *verts, uint32_t *tris, int32_t *parent_face);
int pedp_refined_reduce(pedp_refined_t refined, int op, int mem, const double *child_values, double *parent_values);
int pedp_refined_destroy(pedp_refined_t refined);

/* ---------------------------------------------------------------- surface sampling: uniform and Poisson-disk model clouds
 * The cloud of the model's surface (model.ply, the ICP target and the pose errors' points) made from the model's mesh,
 * in the place of Open3D's sample_points_uniformly / sample_points_poisson_disk (src/pose_estimation.py:453-464).
 * Everything is a pure function of (mesh, seed, spacing): the same bits on every call and context.  float64, no fused
 * multiply-add, every sum and product in the order written.  The contract is DESIGN.md s4.26:
 *   generator   Philox4x32-10.  Sample k (a uint64, global: a call for [first, first + n) returns that slice of one
 *               endless sequence, k wrapping at 2^64) draws x = philox(counter (k_lo, k_hi, 0, 0), key (seed_lo, seed_hi))
 *               and y = philox(counter (k_lo, k_hi, 1, 0), the same key).
 *   face        area_f = 0.5 * sqrt((cx^2 + cy^2) + cz^2) of c = e1 x e2, e1 = v1 - v0, e2 = v2 - v0; amax the largest
 *               finite area; w_f = (uint64) floor((area_f / amax) * 2^32), 0 for an area that is 0 or not finite; C the
 *               inclusive integer prefix sum of w, W its total; t = mulhi64((x0 << 32) | x1, W); the face is the first f
 *               with C[f] > t.  A face of weight 0 is never chosen (info: unsampled_faces).
 *   point       u1 = (((x2 << 32) | x3) >> 11) * 2^-53, u2 = (((y0 << 32) | y1) >> 11) * 2^-53, s = sqrt(u1), a = 1 - s,
 *               b = s * (1 - u2), c = s * u2, p = (a * v0 + b * v1) + c * v2 per component.  barycentric = (a, b, c).
 *   normal      PEDP_SAMPLE_NORMALS_VERTEX: (a * n0 + b * n1) + c * n2 of the vertex normals, not renormalised;
 *               PEDP_SAMPLE_NORMALS_TRIANGLE: c / sqrt((cx^2 + cy^2) + cz^2) of the face's e1 x e2.
 *   thinning    S(r) of points p_i, i < M: point i has the key (z_i << 32) | (i mod 2^32), the lower key wins; z_i = y2 of
 *               a mesh sample's own draw, and word 0 of philox(counter (i_lo, i_hi, 2, 0), key seed) for a given cloud.
 *               i and j conflict iff ((dx^2 + dy^2) + dz^2) < r * r (strict).  S(r) is what a visit in ascending key
 *               order keeps that keeps a point iff it conflicts with no kept point.  The device finds it in rounds
 *               of final decisions (REMOVED once a conflicting lower key is KEPT, KEPT once all conflicting lower keys
 *               are REMOVED), so it depends on no schedule; the rounds it took are reported, not part of the contract.
 *               No two points of S(r) are closer than r, and every point is closer than r to one of S(r).
 *   count       M = init_factor * N samples k = 0 .. M - 1; r bisected on [0, 2 * sqrt(area / N)] for 24 halvings,
 *               mid = 0.5 * (lo + hi), |S(mid)| >= N ? lo = mid : hi = mid; r* = the final lo; of S(r*) the N lowest
 *               keys.  area = the faces' areas summed in face order.  Always exactly N points, none closer than r*.
 *   spacing     S(r) of M = ceil((init_factor * area) / (r * r)) samples k = 0 .. M - 1 (at least 1).
 *
 * pedp_mesh_sampler_create: verts V x 3 float64, tris F x 3 (1 <= F <= 2^24), vertex_normals V x 3 or null, all in host
 * or device memory by `mem`; the handle keeps copies and the prefix sum on the device.  PEDP_ERR_BAD_ARG for an index
 * outside the vertices, a non-finite coordinate, or W = 0 (no face has an area).  The call waits on the context's stream.
 * pedp_mesh_sample: samples [first, first + n) to points n x 3, face_ids n, barycentric n x 3, normals_out n x 3 (each
 * but points nullable; normals_out needed unless normals is PEDP_SAMPLE_NORMALS_NONE).  PEDP_DEVICE only enqueues.
 * pedp_points_thin: S(spacing) of a given cloud (n x 3, finite), spacing >= 0: the kept indices in ascending order to
 * kept (capacity entries), their number to *count -- larger than capacity: come back with that many.
 * pedp_points_thin_count: the count form on a given cloud, bisected on [0, spacing_max]: exactly number_of_points (<= n)
 * indices in ascending order to kept, r* to *spacing, the last thinning's rounds, and the thinnings run to *probes.
 * pedp_mesh_sample_disk: the count form (number_of_points >= 1, spacing < 0) or the spacing form (number_of_points 0,
 * spacing > 0) on the mesh; the draw and the kept set stay on the device in the handle until the next call.  *count kept
 * samples of *drawn, *spacing_out = r* or the spacing given.  pedp_mesh_sample_disk_read: the kept samples in ascending
 * sample index: points, face_ids, barycentric, normals_out (only after a draw with normals), sample_index, each nullable.
 * The thinning calls read a few counters per group of rounds: they wait on the context's stream and are
 * PEDP_ERR_BAD_ARG while a registration is pending on it. */
typedef struct pedp_mesh_sampler_s *pedp_mesh_sampler_t;
enum { PEDP_SAMPLE_NORMALS_NONE = 0, PEDP_SAMPLE_NORMALS_VERTEX = 1, PEDP_SAMPLE_NORMALS_TRIANGLE = 2 };
typedef struct {
    int64_t vertices, faces;
    int64_t unsampled_faces;   /* faces of weight 0: no area, or below 2^-32 of the largest */
    uint64_t total_weight;     /* W */
    double area;               /* the faces' areas summed in face order */
    double largest_area;       /* amax */
    int32_t has_vertex_normals;
    int32_t reserved;
} pedp_mesh_sampler_info_t;
int pedp_mesh_sampler_create(pedp_ctx_t ctx, const double *verts, int64_t V, const uint32_t *tris, int64_t F, const double *vertex_normals,
                             int mem, pedp_mesh_sampler_t *out);
int pedp_mesh_sampler_destroy(pedp_mesh_sampler_t sampler);
int pedp_mesh_sampler_info(pedp_mesh_sampler_t sampler, pedp_mesh_sampler_info_t *info);
int pedp_mesh_sample(pedp_mesh_sampler_t sampler, uint64_t seed, uint64_t first, int64_t n, int normals, int mem, double *points,
                     int32_t *face_ids, double *barycentric, double *normals_out);
int pedp_points_thin(pedp_ctx_t ctx, const double *points, int64_t n, double spacing, uint64_t seed, int mem, int64_t capacity, int32_t *kept,
                     int64_t *count, int32_t *rounds);
int pedp_points_thin_count(pedp_ctx_t ctx, const double *points, int64_t n, int64_t number_of_points, double spacing_max, uint64_t seed,
                           int mem, int32_t *kept, double *spacing, int32_t *rounds, int32_t *probes);
int pedp_mesh_sample_disk(pedp_mesh_sampler_t sampler, uint64_t seed, int64_t number_of_points, double spacing, int64_t init_factor,
                          int normals, int64_t *count, int64_t *drawn, double *spacing_out, int32_t *rounds, int32_t *probes);
int pedp_mesh_sample_disk_read(pedp_mesh_sampler_t sampler, int mem, double *points, int32_t *face_ids, double *barycentric,
                               double *normals_out, int32_t *sample_index);

/* ---------------------------------------------------------------- mask / depth statistics (guess_translation, register's gate)
 * What estimater.py:135-147 and :182-183 take from a frame with np.where, np.median and a sum, in one call on the device.
 * The contract is DESIGN.md s4.11.  With pos = mask > 0, truthy = mask.astype(bool) (for a float32 mask they differ on
 * negative and NaN entries) and near = depth >= float32(0.001) (false for NaN):
 *   n_pos, umin, umax, vmin, vmax   count and box of pos (u = column, v = row); the box is -1 when n_pos = 0
 *   n_valid                         count of near & pos
 *   n_med, median                   count of truthy & near and numpy's median of those depths bit for bit: the middle
 *                                   element, or (a + b) / 2 in float32 of the two middle ones; NaN when n_med = 0 */
typedef struct pedp_mask_depth_record {
    int32_t n_pos, n_valid, n_med;
    int32_t umin, umax, vmin, vmax;
    float median;
} pedp_mask_depth_record;

/* depth H x W float32 and mask H x W of mask_dtype (PEDP_U8: uint8 or bool bytes; PEDP_F32), both contiguous, host or
 * device memory by `mem`; H * W <= 4096 * 4096.  *out is host memory; the call returns once it is written.  Integer
 * atomics only: the record does not depend on scheduling. */
int pedp_mask_depth_stats(pedp_ctx_t ctx, const float *depth, const void *mask, int mask_dtype, int H, int W, int mem,
                          pedp_mask_depth_record *out);

/* ---------------------------------------------------------------- 3x3 convolution of the networks' residual blocks
 * The contract is DESIGN.md s4.12: stride 1, padding 1, NHWC float16 in and out, float32 accumulation in a fixed order
 * (two calls give the same bits), device memory only, on the context's stream.  Cin and Cout are multiples of 32 up to
 * 512 (PEDP_ERR_BAD_ARG otherwise); N, H, W >= 1. */
typedef struct pedp_conv3x3_params {
    int32_t N, H, W;         /* x is N x H x W x Cin, dense */
    int32_t Cin, Cout;
    int32_t y_ld, y_c0;      /* y[pixel * y_ld + y_c0 + co]: the destination's channel stride (>= y_c0 + Cout) and offset */
    int32_t res_ld, res_c0;  /* the same for the residual (ignored when it is null) */
    int32_t relu;            /* 0: identity */
} pedp_conv3x3_params;

/* Replaces the fold of `bn(conv(x))` in eval mode: with s = gamma / sqrt(var + eps) in float32, w_packed[co][tap][ci] =
 * float16(w[co][ci][tap] * s[co]) (Cout x 9 x Cin, tap = 3 * ky + kx) and bias[co] = (b[co] - mean[co]) * s[co] + beta[co].
 * w is the Conv2d weight Cout x Cin x 3 x 3 float32, b its bias or null (zeros); gamma, beta, mean, var are the
 * BatchNorm2d's weight, bias, running_mean and running_var, or all null for a plain convolution (s = 1, bias = b). */
int pedp_conv3x3_pack(pedp_ctx_t ctx, int Cin, int Cout, const float *w, const float *b, const float *gamma, const float *beta,
                      const float *mean, const float *var, float eps, void *w_packed, float *bias);

/* Replaces `relu(bn(F.conv2d(x, w, b, stride=1, padding=1)) + residual)` (ResnetBasicBlock.forward, network_modules.py:94-111)
 * on channels-last float16 tensors: y = act(conv(x, w_packed) + bias [+ residual]).  x, w_packed and bias 16-byte
 * aligned, y and residual 8-byte aligned; residual may be y itself (each element is read by the lane that then writes it),
 * x may not. */
int pedp_conv3x3_f16(pedp_ctx_t ctx, const pedp_conv3x3_params *prm, const void *x, const void *w_packed, const float *bias,
                     const void *residual, void *y);

/* ---------------------------------------------------------------- the encoders' stride-2 convolutions
 * The other three convolutions of an encoder, with the arithmetic of the block kernel: float16 products,
 * float32 accumulation in an order fixed by the shape, float32 bias with the BatchNorm folded in, optional ReLU, one
 * rounding to float16 into NHWC y.  Device memory only, on the context's stream.  Two forms are built, everything else is
 * PEDP_ERR_BAD_ARG:
 *   3 x 3, stride 2, padding 1   x N x H x W x Cin float16 (PEDP_NHWC, PEDP_F16), Cin and Cout multiples of 32 up to 512
 *   7 x 7, stride 2, padding 3   x N x Cin x H x W float32 or float16 (PEDP_NCHW), Cin 1 .. 8, Cout a multiple of 32 up
 *                                to 512; float32 input is rounded to float16 (to nearest even) before the products
 * y is N x OH x OW with OH = (H + 2 * pad - KH) / stride + 1 (floor), OW likewise. */
enum { PEDP_NHWC = 0, PEDP_NCHW = 1 };
enum { PEDP_F16 = 2 };       /* with PEDP_U8 and PEDP_F32 above */
typedef struct pedp_conv2d_params {
    int32_t N, H, W;         /* of the input */
    int32_t Cin, Cout;
    int32_t KH, KW, stride, pad;
    int32_t layout, dtype;   /* of the input: PEDP_NHWC / PEDP_NCHW, PEDP_F16 / PEDP_F32 */
    int32_t N0;              /* images 0 .. N0 come from x, N0 .. N from x2 (7 x 7 only; N0 = N or 0 when x2 is null) */
    int32_t y_ld, y_c0;      /* y[pixel * y_ld + y_c0 + co], as in pedp_conv3x3_params */
    int32_t relu;            /* 0: identity */
} pedp_conv2d_params;

/* pedp_conv3x3_pack for a KH x KW kernel (3 x 3 or 7 x 7): the same float32 fold of `ConvBNReLU`'s BatchNorm2d
 * (network_modules.py:37-50) into w Cout x Cin x KH x KW.  3 x 3: w_packed is Cout x 9 x Cin as above.  7 x 7 (Cin <= 8):
 * w_packed is Cout x 416 float16, [co][8 * (7 * ky + kx) + ci], zero for ci >= Cin and past tap 48. */
int pedp_conv2d_pack(pedp_ctx_t ctx, int Cin, int Cout, int KH, int KW, const float *w, const float *b, const float *gamma,
                     const float *beta, const float *mean, const float *var, float eps, void *w_packed, float *bias);

/* Replaces `ConvBNReLU.forward` (network_modules.py:37-50: `relu(bn(F.conv2d(x, w, b, stride=2, padding=(k - 1) // 2)))`)
 * of the encoders' three stride-2 layers under float16 autocast, and for the 7 x 7 one the `torch.cat([A, B], 0)` in front
 * of it (refine_network.py:80, score_network.py:66): x2, when not null, holds images N0 .. N.  x (3 x 3), w_packed and bias
 * 16-byte aligned, y 8-byte aligned; y may not overlap an input.  residual must be null: the stride-2 layers add none. */
int pedp_conv2d_f16(pedp_ctx_t ctx, const pedp_conv2d_params *prm, const void *x, const void *x2, const void *w_packed,
                    const float *bias, const void *residual, void *y);

/* ---------------------------------------------------------------- multi-head attention core of the networks' heads
 * The contract is DESIGN.md s4.13: O = softmax(scale * Q K^T) V per (batch, head) without an S x S matrix in memory; float16
 * operands, float32 scores, running maximum and sum, the probabilities rounded to float16 for the product with V, float32
 * accumulation, one rounding to float16 into o.  No mask, no dropout.  The summation order is fixed (no atomics, the key
 * axis is not split across workgroups): two calls give the same bits.  Device memory only, on the context's stream, no
 * host wait.  D = 128 is the only head dimension built (PEDP_ERR_BAD_ARG otherwise); B, H >= 1, 1 <= S <= 4096. */
typedef struct pedp_mha_params {
    int32_t B, S, H, D;              /* batch, tokens, heads, head dimension */
    int32_t q_ld, k_ld, v_ld, o_ld;  /* elements from token s to token s + 1 of each operand (>= H * D, multiples of 8) */
    float scale;                     /* of the scores before the softmax: 1 / sqrt(D) for nn.MultiheadAttention */
} pedp_mha_params;

/* Replaces the middle of `nn.MultiheadAttention.forward` / `F.multi_head_attention_forward` in eval mode between the two
 * projections, i.e. `F.scaled_dot_product_attention(q, k, v)` on B x H x S x D views, or with need_weights=True (what
 * score_network.py:77 and :88 call) `softmax(baddbmm(q, k^T))`, `bmm(p, v)` and the head-averaged B x S x S weights, which
 * are not formed here.  Element (b, s, h, d) of an operand x is x[(b * S + s) * x_ld + h * D + d]: with q, k = q + E and
 * v = q + 2E, E = H * D, and q_ld = k_ld = v_ld = 3E the operands are read in place from the packed in-projection output
 * B x S x 3E; three separate tensors work the same way.  q, k, v and o are 16-byte aligned; o's bytes may not overlap an
 * input's (from its first element to its last), PEDP_ERR_BAD_ARG otherwise.  Rows >= S of no operand are touched. */
int pedp_mha_f16(pedp_ctx_t ctx, const pedp_mha_params *prm, const void *q, const void *k, const void *v, void *o);

/* ---------------------------------------------------------------- linear layers of the networks' heads
 * The contract is DESIGN.md s4.14: Y[M x N] = epilogue(X[M x K] W^T + bias) with float16 X (row stride x_ld, read in
 * place) and W (N x K row-major, `nn.Linear.weight` as stored), float32 bias (may be null), float32 accumulation on the
 * matrix cores, the epilogue in float32 and one rounding to float16.  K is not split and nothing is added atomically:
 * two calls give the same bits.  Device memory only, on the context's stream, no host wait. */
#define PEDP_LINEAR_PLAIN 0  /* y = acc + bias */
#define PEDP_LINEAR_RELU 1   /* y = max(acc + bias, 0) */
#define PEDP_LINEAR_ADD_LN 2 /* y = LayerNorm(res + (acc + bias)) * gamma + beta over the whole row; N == 512 only */
typedef struct pedp_linear_params {
    int32_t M, N, K;           /* M >= 1; N and K multiples of 64 (K <= 8192) */
    int32_t x_ld, y_ld;        /* elements from row r to row r + 1 (multiples of 8, at least K and N) */
    int32_t res_ld;            /* ADD_LN: the same for res */
    int32_t epilogue;          /* PEDP_LINEAR_* */
    int32_t pos_rows;          /* rows of the position table */
    int32_t pos_period;        /* S: row r takes table row r % S (1 <= S <= pos_rows) */
    int32_t pos_a;             /* ADD_LN: nonzero adds the table to X as well as to res (then K == N) */
    float eps;                 /* ADD_LN: of the variance, `nn.LayerNorm.eps` */
} pedp_linear_params;

/* Replaces `F.linear` of the heads' projections and feed-forward, and with ADD_LN the `norm(x + linear(...))` that follows
 * it in a post-norm nn.TransformerEncoderLayer.  pos, when not null, is a float32 table pos_rows x K: row r of the X
 * operand is half(float(x[r]) + pos[r % S]), formed on the way into the product and never written to memory (the
 * `tokens + pe` of a _PositionTable).  In ADD_LN pos (pos_rows x N) is added in float32 to the residual row, and to X
 * only if pos_a is set; res is float16 with row stride res_ld, gamma and beta (may be null) are float32, mean and biased
 * variance are float32 sums over all N columns.  Every array is 16-byte aligned.  y may not overlap an input, except
 * that ADD_LN takes y == res with y_ld == res_ld (each element is read and then written by the same lane).  Rows >= M
 * of no array are touched.  Anything else is PEDP_ERR_BAD_ARG before the context or the device is used. */
int pedp_linear_f16(pedp_ctx_t ctx, const pedp_linear_params *prm, const void *x, const void *w, const float *bias,
                    const void *res, const float *pos, const float *gamma, const float *beta, void *y);

typedef struct pedp_token_pool_params {
    int32_t B, S;              /* groups, consecutive rows per group */
    int32_t E;                 /* channels: 512 only */
    int32_t x_ld;              /* elements from row r to row r + 1 (a multiple of 8, at least E) */
    int32_t n_out;             /* rows of w (1 .. 8); 0 without w */
} pedp_token_pool_params;

/* The float32 mean over each group's S rows of x (float16), in a fixed order.  w == null: out is B x E float16, the
 * `.mean(1)` of score_network.py:74.  Otherwise out is B x n_out float16, mean w^T + bias in float32 rounded once: a
 * Linear and the mean commute, so this is `Linear(512, n)(x).mean(1)` of refine_network.py:90-91, and with S = 1 the
 * Linear itself (score_network.py:88).  w (n_out x E) and bias (may be null) are float32; x, w, bias 16-byte aligned. */
int pedp_token_pool_f16(pedp_ctx_t ctx, const pedp_token_pool_params *prm, const void *x, const float *w, const float *bias,
                        void *out);

/* ---------------------------------------------------------------- cluster_poses
 * Replaces mycpp.cluster_poses (mycpp/src/app/pybind_api.cpp:24-68; caller
 * estimater.py:118).  Host only.  poses: n x 16 float32 row-major, syms: s x 16.
 * keep_idx: caller array of n ints, receives the indices of the kept poses. */
int pedp_cluster_poses(float angle_diff_deg, float dist_diff, const float *poses, int n,
                       const float *syms, int s, int32_t *keep_idx, int *n_keep);

/* ---------------------------------------------------------------- page-locked host memory
 * Result arrays a caller allocates anew for every frame are paid for twice: the pages of a fresh allocation fault in one
 * by one while the result is copied into them (0.15 ms per megabyte measured inside the frame chain), and a pageable
 * destination goes through the library's staging buffer.  pedp_host_alloc hands out page-locked memory (hipHostMalloc)
 * that downloads reach directly; pedp_hip keeps a pool of such blocks under its result arrays (_lib.host_array). */
int pedp_host_alloc(size_t bytes, void **out);
void pedp_host_free(void *p);

/* ---------------------------------------------------------------- rigid transform of host arrays
 * What o3d.geometry.PointCloud.transform / TriangleMesh.transform do to the holders' float64 arrays on the path
 * (src/pose_estimation.py:406-409 transform_object, :815-816; run.py:118, :197, :200): out_i = R in_i + t with
 * ((T0 x + T1 y) + T2 z) + T3 per row, one rounding per operation (the oracle's order); rotate_only != 0 leaves the
 * translation out (normals).  Host only, out may be in.  A numpy (N, 3) @ (3, 3) product takes ten times as long
 * (a BLAS call with inner dimension 3) and its rounding depends on the BLAS build. */
int pedp_transform_points(const double T[16], const double *in, int64_t n, int rotate_only, double *out);

#ifdef __cplusplus
}
#endif
#endif
