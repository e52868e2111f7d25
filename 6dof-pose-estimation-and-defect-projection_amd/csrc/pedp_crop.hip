// Crop batches of FoundationPose's render-and-compare step: the device half of crop.py.
//
//   map_prep_kernel     per pose: warp_perspective's float64 map from output pixel to grid_sample pixel coordinate
//   warp_kernel         one lane per output pixel of one pose: the coordinate once, then every channel (bilinear or nearest)
//   window_kernel       per pose: compute_crop_window_tf_batch(method='box_3d') in float32, and the renderer's bbox2d
//   crop_prep_kernel    per pose: the maps of tf_to_crops (frame -> crop) and of its inverse (crop -> frame), pose translation
//   crop_kernel         one lane per crop pixel of one pose: every B-side map from the shared full-frame sources with one
//                       coordinate, the A-side normalisation of the rendered maps, transform_batch on both xyz maps
//
// A workgroup covers 256 consecutive pixels of one pose (blockIdx.y), so the pose's map is uniform and the stores of
// every NCHW plane are contiguous along x.  The sources are one 640 x 480 frame each (a few MB): they stay in L2 / MALL
// while all poses gather from them.
//
// Arithmetic: the maps and the per-pixel coordinate in float64, cast to float32; grid_sample's float32
// weights and sums in a fixed order with no FMA (-ffp-contract=off).  tests/_crop_ref.py restates it operation for
// operation.
#include "pedp_internal.h"
#include <algorithm>
#include <cmath>

namespace {

constexpr int CB = 256;              // threads per workgroup = pixels per tile
constexpr int MAX_GRID_Y = 65535;    // poses per launch
// transform_batch's `/ 255.0`: torch divides a CUDA tensor by a Python scalar as a product with the float32 reciprocal
constexpr float INV255 = 1.0f / 255.0f;

// Output pixel (x, y) -> grid_sample pixel coordinate:
//   X = (s[0] x + s[1] y) + s[2],  Y = (s[3] x + s[4] y) + s[5],  Z = (s[6] x + s[7] y) + s[8]
//   ix = X / Z + bx, iy = Y / Z + by  where |Z| > 1e-8, else X + bx, Y + by.
struct PoseMap {
    double s[9];
    double bx, by;
    double ok;  // 1: M invertible and finite
};

struct Img {
    const void *p;
    int u8;
    int C, H, W;
    int64_t sn, sc, sy, sx;
};

__host__ __device__ inline Img make_img(const pedp_image &d, const void *p) {
    return Img{p, d.dtype == PEDP_U8 ? 1 : 0, d.C, d.H, d.W, d.sn, d.sc, d.sy, d.sx};
}

__device__ __forceinline__ float load(const Img &im, int64_t off) {
    return im.u8 ? (float)((const uint8_t *)im.p)[off] : ((const float *)im.p)[off];
}

// Float64 inverse of a 3 x 3 (adjugate / determinant); returns the determinant.
__host__ __device__ inline double inv3(const double *m, double *r) {
    const double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[2] * m[7] - m[1] * m[8], c02 = m[1] * m[5] - m[2] * m[4];
    const double c10 = m[5] * m[6] - m[3] * m[8], c11 = m[0] * m[8] - m[2] * m[6], c12 = m[2] * m[3] - m[0] * m[5];
    const double c20 = m[3] * m[7] - m[4] * m[6], c21 = m[1] * m[6] - m[0] * m[7], c22 = m[0] * m[4] - m[1] * m[3];
    const double det = (m[0] * c00 + m[1] * c10) + m[2] * c20;
    r[0] = c00 / det; r[1] = c01 / det; r[2] = c02 / det;
    r[3] = c10 / det; r[4] = c11 / det; r[5] = c12 / det;
    r[6] = c20 / det; r[7] = c21 / det; r[8] = c22 / det;
    return det;
}

// kornia: A = N(h_out, w_out) M N(H, W)^-1, grid = A^-1 applied to the normalised output meshgrid, then grid_sample's
// unnormalisation.  The output-side normalisation cancels; what is left is N(H, W) M^-1 followed by
// ix = a x_n + b  (align_corners: a = (W-1)/2, else a = W/2; b = (W-1)/2).
__device__ inline PoseMap make_map(const float *Mf, int H, int W, int align_corners) {
    double m[9], r[9];
    bool fin = true;
    for (int k = 0; k < 9; ++k) {
        m[k] = (double)Mf[k];
        fin = fin && isfinite(m[k]);
    }
    const double det = inv3(m, r);
    PoseMap pm;
    pm.ok = (fin && det != 0.0 && isfinite(det)) ? 1.0 : 0.0;
    const double nx = 2.0 / (W == 1 ? 1e-14 : (double)(W - 1)), ny = 2.0 / (H == 1 ? 1e-14 : (double)(H - 1));
    const double ax = align_corners ? (double)(W - 1) / 2.0 : (double)W / 2.0;
    const double ay = align_corners ? (double)(H - 1) / 2.0 : (double)H / 2.0;
    for (int j = 0; j < 3; ++j) {
        pm.s[j] = ax * (nx * r[j] - r[6 + j]);
        pm.s[3 + j] = ay * (ny * r[3 + j] - r[6 + j]);
        pm.s[6 + j] = r[6 + j];
    }
    pm.bx = (double)(W - 1) / 2.0;
    pm.by = (double)(H - 1) / 2.0;
    return pm;
}

__device__ __forceinline__ void map_coord(const PoseMap &m, int x, int y, float *ix, float *iy) {
    const double xd = (double)x, yd = (double)y;
    const double X = (m.s[0] * xd + m.s[1] * yd) + m.s[2];
    const double Y = (m.s[3] * xd + m.s[4] * yd) + m.s[5];
    const double Z = (m.s[6] * xd + m.s[7] * yd) + m.s[8];
    if (fabs(Z) > 1e-8) {
        *ix = (float)(X / Z + m.bx);
        *iy = (float)(Y / Z + m.by);
    } else {
        *ix = (float)(X + m.bx);
        *iy = (float)(Y + m.by);
    }
}

// grid_sample nearest: nearbyint (half to even), zero outside.  Returns false where the sample is outside.
__device__ __forceinline__ bool nearest_index(float ix, float iy, int H, int W, int *xi, int *yi) {
    const float xr = rintf(ix), yr = rintf(iy);
    if (!(xr >= 0.f && xr <= (float)(W - 1) && yr >= 0.f && yr <= (float)(H - 1))) return false;
    *xi = (int)xr;
    *yi = (int)yr;
    return true;
}

struct Bilin {
    int x0, y0;
    float w[4];   // nw, ne, sw, se
    bool any;     // some corner inside
};

__device__ __forceinline__ Bilin bilinear_setup(float ix, float iy, int H, int W) {
    Bilin b;
    const float x0f = floorf(ix), y0f = floorf(iy);
    b.any = x0f >= -1.f && x0f <= (float)(W - 1) && y0f >= -1.f && y0f <= (float)(H - 1);
    if (!b.any) return b;
    b.x0 = (int)x0f;
    b.y0 = (int)y0f;
    const float x1f = x0f + 1.f, y1f = y0f + 1.f;
    b.w[0] = (x1f - ix) * (y1f - iy);
    b.w[1] = (ix - x0f) * (y1f - iy);
    b.w[2] = (x1f - ix) * (iy - y0f);
    b.w[3] = (ix - x0f) * (iy - y0f);
    return b;
}

__device__ __forceinline__ float bilinear_sample(const Img &im, int64_t base, const Bilin &b) {
    float acc = 0.f;
    if (!b.any) return acc;
    const bool xin0 = b.x0 >= 0, xin1 = b.x0 + 1 <= im.W - 1, yin0 = b.y0 >= 0, yin1 = b.y0 + 1 <= im.H - 1;
    const int64_t o00 = base + (int64_t)b.y0 * im.sy + (int64_t)b.x0 * im.sx;
    if (yin0 && xin0) acc = acc + load(im, o00) * b.w[0];
    if (yin0 && xin1) acc = acc + load(im, o00 + im.sx) * b.w[1];
    if (yin1 && xin0) acc = acc + load(im, o00 + im.sy) * b.w[2];
    if (yin1 && xin1) acc = acc + load(im, o00 + im.sy + im.sx) * b.w[3];
    return acc;
}

__global__ __launch_bounds__(64) void map_prep_kernel(const float *__restrict__ M, int B, int H, int W, int align_corners,
                                                      PoseMap *__restrict__ maps) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    maps[b] = make_map(M + 9 * (size_t)b, H, W, align_corners);
}

template <int NEAREST>
__global__ __launch_bounds__(CB) void warp_kernel(Img src, const PoseMap *__restrict__ maps, int b0, int oh, int ow,
                                                  float *__restrict__ out) {
    const int hw = oh * ow;
    const int q = blockIdx.x * CB + threadIdx.x;
    if (q >= hw) return;
    const int b = b0 + blockIdx.y;
    const PoseMap &m = maps[b];
    const int y = q / ow, x = q - y * ow;
    float *o = out + (size_t)b * src.C * hw + q;
    const int64_t nbase = (int64_t)b * src.sn;
    float ix = 0.f, iy = 0.f;
    map_coord(m, x, y, &ix, &iy);
    if (m.ok == 0.0) {
        for (int c = 0; c < src.C; ++c) o[(size_t)c * hw] = 0.f;
        return;
    }
    if (NEAREST) {
        int xi, yi;
        const bool in = nearest_index(ix, iy, src.H, src.W, &xi, &yi);
        const int64_t off = nbase + (in ? (int64_t)yi * src.sy + (int64_t)xi * src.sx : 0);
        for (int c = 0; c < src.C; ++c) o[(size_t)c * hw] = in ? load(src, off + (int64_t)c * src.sc) : 0.f;
    } else {
        const Bilin bl = bilinear_setup(ix, iy, src.H, src.W);
        for (int c = 0; c < src.C; ++c) o[(size_t)c * hw] = bilinear_sample(src, nbase + (int64_t)c * src.sc, bl);
    }
}

// compute_crop_window_tf_batch(method='box_3d'), float32 in the reference's order (no FMA):
//   pts = t + {0, +-r x, +-r y}, (u, v, w) = K pts row by row ((K0 X + K1 Y) + K2 Z), uv = (u / w, v / w),
//   radius = max |uv - uv_centre|, left/right/top/bottom = round(centre -+ radius) (half to even),
//   tf = diag(out_w * (1 / (right - left)), out_h * (1 / (bottom - top)), 1) . [[1, 0, -left], [0, 1, -top], [0, 0, 1]]
//   (3 x 3 product, each entry ((a0 b0 + a1 b1) + a2 b2)).  `out_size[0] / (right - left)` divides a Python number by a
//   tensor, which torch computes as the float32 reciprocal times the number (Tensor.__rdiv__).
struct Intrinsics {
    float k[9];
};

__global__ __launch_bounds__(64) void window_kernel(const float *__restrict__ poses, int B, Intrinsics Kv, float r,
                                                    int out_w, int out_h, float cu, float cv, float *__restrict__ tf_out,
                                                    float *__restrict__ bbox) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const float *p = poses + 16 * (size_t)b;
    const float *K = Kv.k;
    const float off[5][2] = {{0.f, 0.f}, {r, 0.f}, {-r, 0.f}, {0.f, r}, {0.f, -r}};
    float uv[5][2];
    for (int k = 0; k < 5; ++k) {
        const float X = p[3] + off[k][0], Y = p[7] + off[k][1], Z = p[11] + 0.f;
        const float u = (K[0] * X + K[1] * Y) + K[2] * Z;
        const float v = (K[3] * X + K[4] * Y) + K[5] * Z;
        const float w = (K[6] * X + K[7] * Y) + K[8] * Z;
        uv[k][0] = u / w;
        uv[k][1] = v / w;
    }
    float rad = 0.f;
    bool nan = false;  // torch.max propagates NaN
    for (int k = 0; k < 5; ++k)
        for (int j = 0; j < 2; ++j) {
            const float a = fabsf(uv[k][j] - uv[0][j]);
            nan = nan || a != a;
            rad = fmaxf(rad, a);
        }
    if (nan) rad = __builtin_nanf("");
    const float left = rintf(uv[0][0] - rad), right = rintf(uv[0][0] + rad);
    const float top = rintf(uv[0][1] - rad), bottom = rintf(uv[0][1] + rad);
    const float sx = (1.0f / (right - left)) * (float)out_w, sy = (1.0f / (bottom - top)) * (float)out_h;
    const float nt[9] = {sx, 0.f, 0.f, 0.f, sy, 0.f, 0.f, 0.f, 1.f};
    const float t[9] = {1.f, 0.f, -left, 0.f, 1.f, -top, 0.f, 0.f, 1.f};
    float tf[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) tf[3 * i + j] = (nt[3 * i] * t[j] + nt[3 * i + 1] * t[3 + j]) + nt[3 * i + 2] * t[6 + j];
    for (int k = 0; k < 9; ++k) tf_out[9 * (size_t)b + k] = tf[k];
    if (bbox) {
        double m[9], inv[9];
        for (int k = 0; k < 9; ++k) m[k] = (double)tf[k];
        inv3(m, inv);
        float *o = bbox + 4 * (size_t)b;
        o[0] = (float)((inv[0] * 0.0 + inv[1] * 0.0) + inv[2]);
        o[1] = (float)((inv[3] * 0.0 + inv[4] * 0.0) + inv[5]);
        o[2] = (float)((inv[0] * (double)cu + inv[1] * (double)cv) + inv[2]);
        o[3] = (float)((inv[3] * (double)cu + inv[4] * (double)cv) + inv[5]);
    }
}

struct CropPose {
    PoseMap k1;  // tf_to_crops on the frame: crop pixel -> frame coordinate
    PoseMap k2;  // crop_to_ori = float32(inverse(tf_to_crops)) on the crop: frame pixel -> crop coordinate
    float t[4];  // poseA[:3, 3]
};

__global__ __launch_bounds__(64) void crop_prep_kernel(const float *__restrict__ tf, const float *__restrict__ poses, int B, int H,
                                                       int W, int oh, int ow, CropPose *__restrict__ out) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const float *M = tf + 9 * (size_t)b;
    CropPose cp;
    cp.k1 = make_map(M, H, W, 0);
    double m[9], inv[9];
    for (int k = 0; k < 9; ++k) m[k] = (double)M[k];
    inv3(m, inv);
    float c2o[9];
    for (int k = 0; k < 9; ++k) c2o[k] = (float)inv[k];
    cp.k2 = make_map(c2o, oh, ow, 0);
    const float *p = poses + 16 * (size_t)b;
    cp.t[0] = p[3];
    cp.t[1] = p[7];
    cp.t[2] = p[11];
    cp.t[3] = 0.f;
    out[b] = cp;
}

struct CropArgs {
    Img rgb, xyz, normal, depth;
    const float *rgb_r, *xyz_r;
    float *rgbA, *rgbB, *xyzA, *xyzB, *normalB, *depthB;
    size_t pstride;    // floats from one pose's rgbA / rgbB / xyzA / xyzB plane to the next: 3 h w, packed 6 h w
    float K[9];
    float inv_r;       // 1 / (float32(diameter) / 2)
    float z_invalid;   // refiner 0.001, scorer 0.1
    int normalize, use_normal;
    int H, W, oh, ow;
};

// transform_batch on one xyz pixel (h5_dataset.py:79-116 refiner, :137-180 scorer): the invalid test on z before the
// translation, x - t, then under normalize_xyz x * inv_r and a channel is zeroed where z failed or its own |x| >= 2.
__device__ __forceinline__ void xyz_transform(const CropArgs &a, const float *t, float v[3]) {
    const bool zbad = v[2] < a.z_invalid;
    for (int c = 0; c < 3; ++c) v[c] = v[c] - t[c];
    if (a.normalize)
        for (int c = 0; c < 3; ++c) {
            v[c] = v[c] * a.inv_r;
            if (zbad || fabsf(v[c]) >= 2.f) v[c] = 0.f;
        }
}

__device__ __forceinline__ bool frame_index(const PoseMap &m, int x, int y, int H, int W, int *xi, int *yi) {
    float ix, iy;
    map_coord(m, x, y, &ix, &iy);
    return m.ok != 0.0 && nearest_index(ix, iy, H, W, xi, yi);
}

template <int SCORER>
__global__ __launch_bounds__(CB) void crop_kernel(CropArgs a, const CropPose *__restrict__ poses, int b0) {
    const int hw = a.oh * a.ow;
    const int q = blockIdx.x * CB + threadIdx.x;
    if (q >= hw) return;
    const int b = b0 + blockIdx.y;
    const CropPose &cp = poses[b];
    const int y = q / a.ow, x = q - y * a.ow;
    const size_t p3 = (size_t)b * a.pstride + q;   // rgbA / rgbB / xyzA / xyzB
    const size_t n3 = (size_t)b * 3 * hw + q;       // normalB

    // B side: one coordinate for every map
    float ix = 0.f, iy = 0.f;
    map_coord(cp.k1, x, y, &ix, &iy);
    const bool ok = cp.k1.ok != 0.0;
    {
        Bilin bl = bilinear_setup(ix, iy, a.H, a.W);
        bl.any = bl.any && ok;
        for (int c = 0; c < 3; ++c) a.rgbB[p3 + (size_t)c * hw] = bilinear_sample(a.rgb, (int64_t)c * a.rgb.sc, bl) * INV255;
    }
    int xo = 0, yo = 0;
    const bool in = ok && nearest_index(ix, iy, a.H, a.W, &xo, &yo);
    float v[3] = {0.f, 0.f, 0.f};
    if (!SCORER) {
        if (in) {
            const int64_t off = (int64_t)yo * a.xyz.sy + (int64_t)xo * a.xyz.sx;
            for (int c = 0; c < 3; ++c) v[c] = load(a.xyz, off + c * a.xyz.sc);
        }
        if (a.use_normal) {
            const int64_t off = (int64_t)yo * a.normal.sy + (int64_t)xo * a.normal.sx;
            for (int c = 0; c < 3; ++c) a.normalB[n3 + (size_t)c * hw] = in ? load(a.normal, off + c * a.normal.sc) : 0.f;
        }
    } else {
        a.depthB[(size_t)b * hw + q] = in ? load(a.depth, (int64_t)yo * a.depth.sy + (int64_t)xo * a.depth.sx) : 0.f;
        // crop -> frame -> crop round trip: frame pixel o, crop pixel c = nearest(k2(o)), frame pixel o' = nearest(k1(c))
        if (in) {
            float z = 0.f;
            int xc, yc, xo2, yo2;
            if (frame_index(cp.k2, xo, yo, a.oh, a.ow, &xc, &yc) && frame_index(cp.k1, xc, yc, a.H, a.W, &xo2, &yo2))
                z = load(a.depth, (int64_t)yo2 * a.depth.sy + (int64_t)xo2 * a.depth.sx);
            // depth2xyzmap_batch at pixel o (zfar = inf)
            if (!((z < 0.001f) || (z > INFINITY))) {
                v[0] = ((float)xo - a.K[2]) * z / a.K[0];
                v[1] = ((float)yo - a.K[5]) * z / a.K[4];
                v[2] = z;
            }
        }
    }
    xyz_transform(a, cp.t, v);
    for (int c = 0; c < 3; ++c) a.xyzB[p3 + (size_t)c * hw] = v[c];

    // A side: the renderer's N x h x w x 3 maps into NCHW
    const float *rr = a.rgb_r + 3 * ((size_t)b * hw + q);
    for (int c = 0; c < 3; ++c) a.rgbA[p3 + (size_t)c * hw] = (rr[c] * 255.f) * INV255;
    const float *xr = a.xyz_r + 3 * ((size_t)b * hw + q);
    float u[3] = {xr[0], xr[1], xr[2]};
    xyz_transform(a, cp.t, u);
    for (int c = 0; c < 3; ++c) a.xyzA[p3 + (size_t)c * hw] = u[c];
}

size_t a256(size_t b) { return (b + 255) & ~(size_t)255; }

// Elements an image's storage spans (the batch stride counted only when `batched`).
size_t span(const pedp_image &d, bool batched) {
    size_t n = 1 + (size_t)(d.C - 1) * d.sc + (size_t)(d.H - 1) * d.sy + (size_t)(d.W - 1) * d.sx;
    if (batched) n += (size_t)(d.N - 1) * d.sn;
    return n;
}

int check_image(const pedp_image *d, const char *who, const char *what) {
    PEDP_REQUIRE(d && d->data, "%s: null %s", who, what);
    PEDP_REQUIRE(d->dtype == PEDP_U8 || d->dtype == PEDP_F32, "%s: %s dtype %d (uint8 or float32)", who, what, d->dtype);
    PEDP_REQUIRE(d->N > 0 && d->C > 0 && d->H > 0 && d->W > 0 && d->H <= 16384 && d->W <= 16384 && d->C <= 4096,
                 "%s: bad %s shape %d x %d x %d x %d", who, what, d->N, d->C, d->H, d->W);
    PEDP_REQUIRE(d->sn >= 0 && d->sc >= 0 && d->sy >= 0 && d->sx >= 0, "%s: negative %s stride", who, what);
    return PEDP_OK;
}

// Host-memory calls: every input and output through crop_io.
struct Stage {
    pedp_ctx_s *c;
    int mem;
    char *base = nullptr;
    size_t off = 0;
    int rc = PEDP_OK;
    const void *in(const void *src, size_t bytes) {
        if (mem == PEDP_DEVICE || !src || rc) return src;
        char *d = base + off;
        off += a256(bytes);
        rc = pedp_upload(c, d, src, bytes);
        return d;
    }
    float *out(float *dst, size_t count) {
        if (mem == PEDP_DEVICE || !dst) return dst;
        float *d = (float *)(base + off);
        off += a256(sizeof(float) * count);
        return d;
    }
};

size_t esize(const pedp_image &d) { return d.dtype == PEDP_U8 ? 1 : 4; }

}  // namespace

extern "C" {

int pedp_warp_perspective(pedp_ctx_t c, const pedp_image *src, const float *M, int B, int out_h, int out_w, int mode,
                          int align_corners, int mem, float *out) {
    const char *who = "pedp_warp_perspective";
    PEDP_REQUIRE(c, "%s: null context", who);
    PEDP_REQUIRE(mem == PEDP_HOST || mem == PEDP_DEVICE, "%s: bad mem flag %d", who, mem);
    PEDP_REQUIRE(mode == 0 || mode == 1, "%s: mode %d (0 bilinear, 1 nearest)", who, mode);
    PEDP_REQUIRE(B >= 0 && out_h > 0 && out_w > 0 && out_h <= 16384 && out_w <= 16384, "%s: bad sizes", who);
    int rc = check_image(src, who, "source");
    if (rc) return rc;
    PEDP_REQUIRE(src->N == B || src->N == 1, "%s: %d source images for %d matrices", who, src->N, B);
    const size_t hw = (size_t)out_h * out_w, nout = (size_t)B * src->C * hw;
    PEDP_REQUIRE(nout <= ((size_t)1 << 34), "%s: output too large", who);
    if (B == 0) return PEDP_OK;
    PEDP_REQUIRE(M && out, "%s: null matrices or output", who);
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    pedp_image s = *src;
    if (s.N == 1) s.sn = 0;
    const size_t sbytes = esize(s) * span(s, true);
    if (mem == PEDP_HOST) {
        rc = c->crop_io.reserve(a256(sbytes) + a256(36 * (size_t)B) + a256(4 * nout));
        if (rc) return rc;
    }
    Stage sg{c, mem, (char *)c->crop_io.ptr};
    const void *d_src = sg.in(s.data, sbytes);
    const float *d_M = (const float *)sg.in(M, 36 * (size_t)B);
    float *d_out = sg.out(out, nout);
    if (sg.rc) return sg.rc;
    rc = c->crop_ws.reserve(sizeof(PoseMap) * (size_t)B);
    if (rc) return rc;
    PoseMap *maps = (PoseMap *)c->crop_ws.ptr;
    hipLaunchKernelGGL(map_prep_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, c->stream, d_M, B, s.H, s.W, align_corners,
                       maps);
    const Img im = make_img(s, d_src);
    for (int b0 = 0; b0 < B; b0 += MAX_GRID_Y) {
        const dim3 grid((unsigned)((hw + CB - 1) / CB), (unsigned)std::min(MAX_GRID_Y, B - b0));
        if (mode == 1)
            hipLaunchKernelGGL(warp_kernel<1>, grid, dim3(CB), 0, c->stream, im, maps, b0, out_h, out_w, d_out);
        else
            hipLaunchKernelGGL(warp_kernel<0>, grid, dim3(CB), 0, c->stream, im, maps, b0, out_h, out_w, d_out);
        PEDP_HIP_CHECK(hipGetLastError());
    }
    if (mem == PEDP_HOST) return pedp_download(c, out, d_out, sizeof(float) * nout);
    return PEDP_OK;
}

int pedp_crop_window(pedp_ctx_t c, const float *poses, int B, const float *K, float radius, int out_w, int out_h, float corner_u,
                     float corner_v, int mem, float *tf_to_crops, float *bbox2d) {
    const char *who = "pedp_crop_window";
    PEDP_REQUIRE(c, "%s: null context", who);
    PEDP_REQUIRE(mem == PEDP_HOST || mem == PEDP_DEVICE, "%s: bad mem flag %d", who, mem);
    PEDP_REQUIRE(B >= 0 && out_w > 0 && out_h > 0, "%s: bad sizes", who);
    if (B == 0) return PEDP_OK;
    PEDP_REQUIRE(poses && K && tf_to_crops, "%s: null poses, K or output", who);
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    Intrinsics Kv;
    for (int k = 0; k < 9; ++k) Kv.k[k] = K[k];  // host values, passed by value: no copy on the stream
    if (mem == PEDP_HOST) {
        const int rc = c->crop_io.reserve(a256(64 * (size_t)B) + a256(36 * (size_t)B) + a256(16 * (size_t)B));
        if (rc) return rc;
    }
    Stage sg{c, mem, (char *)c->crop_io.ptr};
    const float *d_p = (const float *)sg.in(poses, 64 * (size_t)B);
    float *d_tf = sg.out(tf_to_crops, 9 * (size_t)B);
    float *d_bb = sg.out(bbox2d, 4 * (size_t)B);
    if (sg.rc) return sg.rc;
    hipLaunchKernelGGL(window_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, c->stream, d_p, B, Kv, radius, out_w, out_h,
                       corner_u, corner_v, d_tf, d_bb);
    PEDP_HIP_CHECK(hipGetLastError());
    if (mem == PEDP_HOST) {
        int rc = pedp_download(c, tf_to_crops, d_tf, 36 * (size_t)B);
        if (!rc && bbox2d) rc = pedp_download(c, bbox2d, d_bb, 16 * (size_t)B);
        return rc;
    }
    return PEDP_OK;
}

}  // extern "C"

namespace {

// pedp_crop_batch and, with `packed`, pedp_crop_batch_packed: rgbA / rgbB are then the A / B buffers (B x 6 x h x w) and
// xyzA / xyzB are ignored (the planes at channel 3 of each).
int crop_batch(pedp_ctx_t c, const char *who, bool packed, const pedp_crop_params *prm, const float *tf_to_crops,
               const float *poses, const pedp_image *rgb, const pedp_image *xyz, const pedp_image *normal,
               const pedp_image *depth, const float *rgb_r, const float *xyz_r, int mem, float *rgbA, float *rgbB, float *xyzA,
               float *xyzB, float *normalB, float *depthB) {
    PEDP_REQUIRE(c && prm, "%s: null context or parameters", who);
    PEDP_REQUIRE(mem == PEDP_HOST || mem == PEDP_DEVICE, "%s: bad mem flag %d", who, mem);
    PEDP_REQUIRE(prm->variant == 0 || prm->variant == 1, "%s: variant %d (0 refiner, 1 scorer)", who, prm->variant);
    const int B = prm->B, H = prm->H, W = prm->W, oh = prm->out_h, ow = prm->out_w;
    PEDP_REQUIRE(B >= 0 && H > 0 && W > 0 && oh > 0 && ow > 0 && H <= 16384 && W <= 16384 && oh <= 16384 && ow <= 16384,
                 "%s: bad sizes", who);
    const bool scorer = prm->variant == 1, use_normal = !scorer && prm->use_normal;
    const size_t hw = (size_t)oh * ow, n3 = (size_t)B * 3 * hw;
    PEDP_REQUIRE(n3 <= ((size_t)1 << 34), "%s: output too large", who);
    if (B == 0) return PEDP_OK;
    int rc = check_image(rgb, who, "rgb");
    if (!rc) rc = scorer ? check_image(depth, who, "depth") : check_image(xyz, who, "xyz map");
    if (!rc && use_normal) rc = check_image(normal, who, "normal map");
    if (rc) return rc;
    PEDP_REQUIRE(rgb->C == 3 && rgb->H == H && rgb->W == W, "%s: rgb must be %d x %d x 3", who, H, W);
    if (scorer) {
        PEDP_REQUIRE(depth->C == 1 && depth->H == H && depth->W == W, "%s: depth must be %d x %d", who, H, W);
    } else {
        PEDP_REQUIRE(xyz->C == 3 && xyz->H == H && xyz->W == W, "%s: xyz map must be %d x %d x 3", who, H, W);
        PEDP_REQUIRE(!use_normal || (normal->C == 3 && normal->H == H && normal->W == W), "%s: normal map must be %d x %d x 3",
                     who, H, W);
    }
    PEDP_REQUIRE(tf_to_crops && poses && rgb_r && xyz_r && rgbA && rgbB && (packed || (xyzA && xyzB)), "%s: null array", who);
    PEDP_REQUIRE(scorer ? depthB != nullptr : (!use_normal || normalB != nullptr), "%s: null output", who);
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    const pedp_image *srcs[4] = {rgb, scorer ? nullptr : xyz, use_normal ? normal : nullptr, scorer ? depth : nullptr};
    size_t sb[4] = {0, 0, 0, 0};
    for (int k = 0; k < 4; ++k)
        if (srcs[k]) sb[k] = esize(*srcs[k]) * span(*srcs[k], false);
    if (mem == PEDP_HOST) {
        size_t need = a256(36 * (size_t)B) + a256(64 * (size_t)B) + 2 * a256(12 * (size_t)B * hw) + 4 * a256(4 * n3) +
                      (use_normal ? a256(4 * n3) : 0) + (scorer ? a256(4 * (size_t)B * hw) : 0);
        for (int k = 0; k < 4; ++k) need += a256(sb[k]);
        rc = c->crop_io.reserve(need);
        if (rc) return rc;
    }
    Stage sg{c, mem, (char *)c->crop_io.ptr};
    CropArgs a;
    const void *d_src[4];
    for (int k = 0; k < 4; ++k) d_src[k] = srcs[k] ? sg.in(srcs[k]->data, sb[k]) : nullptr;
    const Img none{nullptr, 0, 0, 0, 0, 0, 0, 0, 0};
    a.rgb = make_img(*rgb, d_src[0]);
    a.xyz = srcs[1] ? make_img(*xyz, d_src[1]) : none;
    a.normal = srcs[2] ? make_img(*normal, d_src[2]) : none;
    a.depth = srcs[3] ? make_img(*depth, d_src[3]) : none;
    const float *d_tf = (const float *)sg.in(tf_to_crops, 36 * (size_t)B);
    const float *d_poses = (const float *)sg.in(poses, 64 * (size_t)B);
    a.rgb_r = (const float *)sg.in(rgb_r, 4 * n3);
    a.xyz_r = (const float *)sg.in(xyz_r, 4 * n3);
    if (packed) {
        a.rgbA = sg.out(rgbA, 2 * n3);
        a.rgbB = sg.out(rgbB, 2 * n3);
        a.xyzA = a.rgbA + 3 * hw;
        a.xyzB = a.rgbB + 3 * hw;
        a.pstride = 6 * hw;
    } else {
        a.rgbA = sg.out(rgbA, n3);
        a.rgbB = sg.out(rgbB, n3);
        a.xyzA = sg.out(xyzA, n3);
        a.xyzB = sg.out(xyzB, n3);
        a.pstride = 3 * hw;
    }
    a.normalB = use_normal ? sg.out(normalB, n3) : nullptr;
    a.depthB = scorer ? sg.out(depthB, (size_t)B * hw) : nullptr;
    if (sg.rc) return sg.rc;
    for (int k = 0; k < 9; ++k) a.K[k] = prm->K[k];
    a.inv_r = 1.0f / (prm->mesh_diameter / 2.0f);
    a.z_invalid = scorer ? 0.1f : 0.001f;
    a.normalize = prm->normalize_xyz != 0;
    a.use_normal = use_normal;
    a.H = H; a.W = W; a.oh = oh; a.ow = ow;
    rc = c->crop_ws.reserve(sizeof(CropPose) * (size_t)B);
    if (rc) return rc;
    CropPose *cp = (CropPose *)c->crop_ws.ptr;
    hipLaunchKernelGGL(crop_prep_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, c->stream, d_tf, d_poses, B, H, W, oh, ow, cp);
    for (int b0 = 0; b0 < B; b0 += MAX_GRID_Y) {
        const dim3 grid((unsigned)((hw + CB - 1) / CB), (unsigned)std::min(MAX_GRID_Y, B - b0));
        if (scorer)
            hipLaunchKernelGGL(crop_kernel<1>, grid, dim3(CB), 0, c->stream, a, cp, b0);
        else
            hipLaunchKernelGGL(crop_kernel<0>, grid, dim3(CB), 0, c->stream, a, cp, b0);
        PEDP_HIP_CHECK(hipGetLastError());
    }
    if (mem == PEDP_HOST) {
        const size_t nab = packed ? 2 * n3 : n3;
        float *outs[6] = {rgbA, rgbB, packed ? nullptr : xyzA, packed ? nullptr : xyzB, a.normalB ? normalB : nullptr,
                          a.depthB ? depthB : nullptr};
        const float *devs[6] = {a.rgbA, a.rgbB, a.xyzA, a.xyzB, a.normalB, a.depthB};
        const size_t cnt[6] = {nab, nab, n3, n3, n3, (size_t)B * hw};
        for (int k = 0; k < 6 && !rc; ++k)
            if (outs[k]) rc = pedp_download(c, outs[k], devs[k], sizeof(float) * cnt[k]);
    }
    return rc;
}

}  // namespace

extern "C" {

int pedp_crop_batch(pedp_ctx_t c, const pedp_crop_params *prm, const float *tf_to_crops, const float *poses, const pedp_image *rgb,
                    const pedp_image *xyz, const pedp_image *normal, const pedp_image *depth, const float *rgb_r,
                    const float *xyz_r, int mem, float *rgbA, float *rgbB, float *xyzA, float *xyzB, float *normalB,
                    float *depthB) {
    return crop_batch(c, "pedp_crop_batch", false, prm, tf_to_crops, poses, rgb, xyz, normal, depth, rgb_r, xyz_r, mem, rgbA,
                      rgbB, xyzA, xyzB, normalB, depthB);
}

int pedp_crop_batch_packed(pedp_ctx_t c, const pedp_crop_params *prm, const float *tf_to_crops, const float *poses,
                           const pedp_image *rgb, const pedp_image *xyz, const pedp_image *normal, const pedp_image *depth,
                           const float *rgb_r, const float *xyz_r, int mem, float *A, float *B, float *normalB, float *depthB) {
    return crop_batch(c, "pedp_crop_batch_packed", true, prm, tf_to_crops, poses, rgb, xyz, normal, depth, rgb_r, xyz_r, mem, A,
                      B, nullptr, nullptr, normalB, depthB);
}

}  // extern "C"
