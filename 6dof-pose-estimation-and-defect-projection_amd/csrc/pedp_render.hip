// Batched mesh renderer: the device half of render.py (nvdiffrast_render and the dr.* shim).
//
// One render call, per chunk of poses, all on the context's stream with no host wait in between:
//   pose_prep_kernel   per pose: clip matrix  projection . glcam_in_cvcam . ob_in_cam  and the bbox2d window
//   memset             per-pixel 64-bit keys := ~0 (background)
//   raster_kernel      one lane per (pose, triangle): homogeneous edge functions (Olano & Greer), a conservative
//                      pixel rectangle, and for every covered pixel centre an atomicMin of
//                      key = orderable(z/w) << 32 | triangle id.  Rectangles above BIG_RECT pixels go to a list ...
//   raster_big_kernel  ... that whole workgroups cover, so that one large triangle does not hold up a wave
//   resolve_kernel     one lane per output pixel: the winning triangle's perspective-correct barycentrics again
//                      (the same arithmetic as the coverage test), interpolated xyz / colour or texture / normal,
//                      the lighting, written straight into the flipped row order render.py returns.
// The minimum of the keys does not depend on the order of the atomics: results are deterministic.
//
// The arithmetic is float32 (edge functions float64) in a fixed order with no FMA (-ffp-contract=off, IEEE division and sqrt); the numpy
// restatement in tests/_render_ref.py repeats it operation for operation.  DESIGN.md s"Renderer" states the contract.
#include "pedp_internal.h"
#include <algorithm>

namespace {

constexpr int RB = 256;                        // threads per workgroup
constexpr int BIG_RECT = 64;                   // rectangles with more pixels go to the one-wave-per-triangle pass
constexpr int BIG_WG = 64;                     // that pass: one wave per list entry (the entries' chains of dependent loads
                                               // are latency-bound: more, smaller workgroups keep more of them in flight)
constexpr unsigned long long BIG_CAP = 1u << 20;  // big-list entries per chunk; beyond it a lane covers its own rectangle
constexpr size_t KEY_BUDGET = 128u << 20;      // key bytes per chunk when no chunk size is configured
constexpr unsigned long long EMPTY = ~0ull;
constexpr int PREC = 24;                       // pose record: clip matrix (16), has_bbox, sx, ox, sy, oy, pad

struct ClipSrc {
    const float *pos;    // shim: N x V x 4 clip-space positions (null in the fused path)
    const float *verts;  // fused: V x 3 model vertices
    const float *prec;   // fused: pose records
    int64_t V;
};

struct Tri {
    double c[3][3];  // edge coefficients (cross products of the (x, y, w) vertices), sign-normalised
    float z[3], w[3];
    int r0, r1, c0, c1;  // conservative pixel rectangle (GL rows)
};

__device__ inline float4 clip_vertex(const ClipSrc &s, int n, int64_t i) {
    if (s.pos) {
        const float *p = s.pos + ((int64_t)n * s.V + i) * 4;
        return make_float4(p[0], p[1], p[2], p[3]);
    }
    const float *m = s.prec + (int64_t)n * PREC;
    const float *v = s.verts + 3 * i;
    const float x = v[0], y = v[1], z = v[2];
    float cx = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
    float cy = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
    const float cz = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
    const float cw = ((m[12] * x + m[13] * y) + m[14] * z) + m[15];
    if (m[16] != 0.f) {  // bbox2d window: row vector times tf (only its four non-trivial entries)
        cx = cx * m[17] + cw * m[18];
        cy = cy * m[19] + cw * m[20];
    }
    return make_float4(cx, cy, cz, cw);
}

// In float64: the products of float32 coordinates are exact, so a shared edge's coefficients in its two triangles are
// exact negations; and the edge functions' rounding stays far below the float32 positions' own, so that the signs
// around a vertex stay consistent (float32 edge functions leave pixel centres at vertices uncovered).
__device__ inline void cross3(double ax, double ay, double aw, double bx, double by, double bw, double *o) {
    o[0] = ay * bw - aw * by;
    o[1] = aw * bx - ax * bw;
    o[2] = ax * by - ay * bx;
}

__device__ inline float pixel_ndc(int i, int n) { return (float)(2 * i + 1) / (float)n - 1.0f; }

// Column range of pixel centres whose NDC lies in [lo, hi], widened by one pixel and clamped to [0, n-1].
__device__ inline void ndc_span(float lo, float hi, int n, int *a, int *b) {
    const float fn = (float)n;
    float l = ((lo + 1.0f) * fn - 1.0f) * 0.5f, h = ((hi + 1.0f) * fn - 1.0f) * 0.5f;
    l = fmaxf(fminf(floorf(l) - 1.0f, fn), -1.0f);  // in float first: no out-of-range conversion
    h = fmaxf(fminf(ceilf(h) + 1.0f, fn), -1.0f);
    *a = max((int)l, 0);
    *b = min((int)h, n - 1);
}

// Triangle setup.  false: culled (bad index, all vertices outside one clip plane, degenerate, or no pixel).
__device__ inline bool tri_setup(const ClipSrc &s, const int32_t *faces, int64_t t, int n, int H, int W, Tri &T) {
    const int32_t i0 = faces[3 * t], i1 = faces[3 * t + 1], i2 = faces[3 * t + 2];
    if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= s.V || i1 >= s.V || i2 >= s.V) return false;
    const float4 a = clip_vertex(s, n, i0), b = clip_vertex(s, n, i1), d = clip_vertex(s, n, i2);
    // trivial rejects: every point of the triangle (a convex combination) is outside the same clip plane
    if (a.x > a.w && b.x > b.w && d.x > d.w) return false;
    if (a.x < -a.w && b.x < -b.w && d.x < -d.w) return false;
    if (a.y > a.w && b.y > b.w && d.y > d.w) return false;
    if (a.y < -a.w && b.y < -b.w && d.y < -d.w) return false;
    if (a.z > a.w && b.z > b.w && d.z > d.w) return false;
    if (a.z < -a.w && b.z < -b.w && d.z < -d.w) return false;
    if (a.w <= 0.f && b.w <= 0.f && d.w <= 0.f) return false;
    cross3(b.x, b.y, b.w, d.x, d.y, d.w, T.c[0]);
    cross3(d.x, d.y, d.w, a.x, a.y, a.w, T.c[1]);
    cross3(a.x, a.y, a.w, b.x, b.y, b.w, T.c[2]);
    const double det = (T.c[0][0] * (double)a.x + T.c[0][1] * (double)a.y) + T.c[0][2] * (double)a.w;
    if (!(det != 0.0) || !isfinite(det)) return false;
    if (det < 0.0)
        for (int k = 0; k < 3; ++k)
            for (int j = 0; j < 3; ++j) T.c[k][j] = -T.c[k][j];
    T.z[0] = a.z; T.z[1] = b.z; T.z[2] = d.z;
    T.w[0] = a.w; T.w[1] = b.w; T.w[2] = d.w;
    if (a.w > 0.f && b.w > 0.f && d.w > 0.f) {
        const float ax = a.x / a.w, bx = b.x / b.w, dx = d.x / d.w;
        const float ay = a.y / a.w, by = b.y / b.w, dy = d.y / d.w;
        ndc_span(fminf(fminf(ax, bx), dx), fmaxf(fmaxf(ax, bx), dx), W, &T.c0, &T.c1);
        ndc_span(fminf(fminf(ay, by), dy), fmaxf(fmaxf(ay, by), dy), H, &T.r0, &T.r1);
    } else {  // a vertex at or behind the eye: the projection is unbounded, test the whole image
        T.c0 = 0; T.c1 = W - 1;
        T.r0 = 0; T.r1 = H - 1;
    }
    return T.c0 <= T.c1 && T.r0 <= T.r1;
}

// Coverage of one pixel centre (px, py): inclusive edges, interpolated w > 0, -1 <= z/w <= 1.
__device__ inline bool cover(const Tri &T, float px, float py, float *u, float *v, float *zd) {
    const double x = px, y = py;
    const double e0 = (T.c[0][0] * x + T.c[0][1] * y) + T.c[0][2];
    const double e1 = (T.c[1][0] * x + T.c[1][1] * y) + T.c[1][2];
    const double e2 = (T.c[2][0] * x + T.c[2][1] * y) + T.c[2][2];
    if (!(e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0)) return false;
    const double S = (e0 + e1) + e2;
    if (!(S > 0.0)) return false;
    const float bu = (float)(e0 / S), bv = (float)(e1 / S);  // float32 from here on
    const float bt = (1.0f - bu) - bv;
    const float zc = (bu * T.z[0] + bv * T.z[1]) + bt * T.z[2];
    const float wc = (bu * T.w[0] + bv * T.w[1]) + bt * T.w[2];
    if (!(wc > 0.f)) return false;
    const float q = zc / wc;
    if (!(q >= -1.0f && q <= 1.0f)) return false;
    *u = bu; *v = bv; *zd = q;
    return true;
}

__device__ inline unsigned orderable(float f) {
    const unsigned b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ inline void cover_pixel(const Tri &T, uint32_t t, int r, int c, int H, int W, unsigned long long *keys) {
    float u, v, zd;
    if (!cover(T, pixel_ndc(c, W), pixel_ndc(r, H), &u, &v, &zd)) return;
    const unsigned long long key = ((unsigned long long)orderable(zd) << 32) | t;
    unsigned long long *k = keys + (int64_t)r * W + c;
    // the stored key only ever decreases: a stale read can only make this lane try an atomic it did not need
    if (key < __hip_atomic_load(k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(k, key);
}

__global__ void __launch_bounds__(RB) raster_kernel(ClipSrc s, const int32_t *faces, int64_t F, int n0, int H, int W,
                                                    unsigned long long *keys, unsigned long long *big,
                                                    unsigned long long *big_n, unsigned long long big_cap) {
    const int64_t t = (int64_t)blockIdx.x * RB + threadIdx.x;
    if (t >= F) return;
    const int n = n0 + (int)blockIdx.y;
    Tri T;
    if (!tri_setup(s, faces, t, n, H, W, T)) return;
    unsigned long long *kp = keys + (int64_t)blockIdx.y * H * W;
    const int cw = T.c1 - T.c0 + 1;
    if ((int64_t)cw * (T.r1 - T.r0 + 1) > BIG_RECT) {
        const unsigned long long slot = atomicAdd(big_n, 1ull);
        if (slot < big_cap) {
            big[slot] = ((unsigned long long)blockIdx.y << 32) | (unsigned long long)t;
            return;
        }
    }
    for (int r = T.r0; r <= T.r1; ++r)
        for (int c = T.c0; c <= T.c1; ++c) cover_pixel(T, (uint32_t)t, r, c, H, W, kp);
}

__global__ void __launch_bounds__(BIG_WG) raster_big_kernel(ClipSrc s, const int32_t *faces, int n0, int H, int W,
                                                        unsigned long long *keys, const unsigned long long *big,
                                                        const unsigned long long *big_n, unsigned long long big_cap) {
    const unsigned long long cnt = min(*big_n, big_cap);
    for (unsigned long long e = blockIdx.x; e < cnt; e += gridDim.x) {
        const unsigned long long rec = big[e];
        const int p = (int)(rec >> 32);
        const int64_t t = (int64_t)(rec & 0xFFFFFFFFull);
        Tri T;
        if (!tri_setup(s, faces, t, n0 + p, H, W, T)) continue;
        unsigned long long *kp = keys + (int64_t)p * H * W;
        const int cw = T.c1 - T.c0 + 1;
        const int area = cw * (T.r1 - T.r0 + 1);  // <= H x W < 2^31
        for (int i = threadIdx.x; i < area; i += BIG_WG)
            cover_pixel(T, (uint32_t)t, T.r0 + i / cw, T.c0 + i % cw, H, W, kp);
    }
}

// pose record n: clip matrix M = P . G . T with G = diag(1, -1, -1, 1), and the bbox2d window (l, t, r, b) -> sx, ox, sy, oy
__global__ void pose_prep_kernel(pedp_render_params prm, const float *poses, const float *bbox, int N, float *prec) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const float *T = poses + 16 * (int64_t)n;
    float G[16];
    for (int j = 0; j < 4; ++j) {
        G[j] = T[j];
        G[4 + j] = -T[4 + j];
        G[8 + j] = -T[8 + j];
        G[12 + j] = T[12 + j];
    }
    float *o = prec + (int64_t)n * PREC;
    const float *P = prm.proj;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j)
            o[4 * i + j] = ((P[4 * i] * G[j] + P[4 * i + 1] * G[4 + j]) + P[4 * i + 2] * G[8 + j]) + P[4 * i + 3] * G[12 + j];
    for (int k = 16; k < PREC; ++k) o[k] = 0.f;
    if (bbox) {
        const float Wf = (float)prm.W, Hf = (float)prm.H;
        const float *bb = bbox + 4 * (int64_t)n;
        const float l = bb[0], t = Hf - bb[1], r = bb[2], b = Hf - bb[3];
        o[16] = 1.f;
        o[17] = Wf / (r - l);
        o[18] = ((Wf - r) - l) / (r - l);
        o[19] = Hf / (t - b);
        o[20] = ((Hf - t) - b) / (t - b);
    }
}

__device__ inline float lerp3(float u, float v, float t, float a0, float a1, float a2) { return (u * a0 + v * a1) + t * a2; }

__device__ inline void normalize3(float *x) {
    const float n = sqrtf((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]);
    const float d = fmaxf(n, 1e-12f);
    x[0] = x[0] / d; x[1] = x[1] / d; x[2] = x[2] / d;
}

__device__ inline float clamp01(float x) { return x < 0.f ? 0.f : (x > 1.f ? 1.f : x); }

__device__ inline int wrap_index(float f, int n) {
    float m = fmodf(f, (float)n);
    if (m < 0.f) m += (float)n;
    const int i = (int)m;
    return (i >= 0 && i < n) ? i : 0;
}

// Bilinear sample, texel centres at +0.5, wrap addressing.  tex: th x tw x C.
__device__ inline void tex_sample(const float *tex, int th, int tw, int C, float u, float v, float *out) {
    const float x = u * (float)tw - 0.5f, y = v * (float)th - 0.5f;
    if (!(fabsf(x) < 1e8f && fabsf(y) < 1e8f)) {
        for (int ch = 0; ch < C; ++ch) out[ch] = 0.f;
        return;
    }
    const float x0 = floorf(x), y0 = floorf(y);
    const float fx = x - x0, fy = y - y0;
    const int ix0 = wrap_index(x0, tw), iy0 = wrap_index(y0, th);
    const int ix1 = ix0 + 1 == tw ? 0 : ix0 + 1, iy1 = iy0 + 1 == th ? 0 : iy0 + 1;
    const float *r0 = tex + (int64_t)iy0 * tw * C, *r1 = tex + (int64_t)iy1 * tw * C;
    for (int ch = 0; ch < C; ++ch) {
        const float t00 = r0[ix0 * C + ch], t10 = r0[ix1 * C + ch], t01 = r1[ix0 * C + ch], t11 = r1[ix1 * C + ch];
        const float a = t00 + (t10 - t00) * fx, b = t01 + (t11 - t01) * fx;
        out[ch] = a + (b - a) * fy;
    }
}

struct MeshArgs {
    const float *verts, *vnormals, *vcolor, *uv, *tex;
    const int32_t *faces;
    int64_t V, F;
    int tex_h, tex_w;
};

struct OutArgs {
    float *color, *depth, *normal, *xyz;
};

__global__ void __launch_bounds__(RB) resolve_kernel(ClipSrc s, MeshArgs m, pedp_render_params prm, const float *poses,
                                                     int n0, const unsigned long long *keys, OutArgs out) {
    const int H = prm.out_h, W = prm.out_w;
    const int64_t pix = (int64_t)blockIdx.x * RB + threadIdx.x;
    if (pix >= (int64_t)H * W) return;
    const int n = n0 + (int)blockIdx.y;
    const int orow = (int)(pix / W), c = (int)(pix % W);
    const int r = H - 1 - orow;  // GL row of this output row (the output is flipped)
    const int64_t o = ((int64_t)n * H + orow) * W + c;
    const unsigned long long key = keys[((int64_t)blockIdx.y * H + r) * W + c];
    float u = 0.f, v = 0.f, zd;
    Tri T;
    bool hit = false;
    const int64_t t = (int64_t)(key & 0xFFFFFFFFull);
    if (key != EMPTY && t < m.F && tri_setup(s, m.faces, t, n, H, W, T))
        hit = cover(T, pixel_ndc(c, W), pixel_ndc(r, H), &u, &v, &zd);
    if (!hit) {
        for (int k = 0; k < 3; ++k) out.color[3 * o + k] = 0.f;
        out.depth[o] = 0.f;
        if (out.normal)
            for (int k = 0; k < 3; ++k) out.normal[3 * o + k] = 0.f;
        if (out.xyz)
            for (int k = 0; k < 3; ++k) out.xyz[3 * o + k] = 0.f;
        return;
    }
    const float bt = (1.0f - u) - v;
    const int32_t idx[3] = {m.faces[3 * t], m.faces[3 * t + 1], m.faces[3 * t + 2]};
    const float *P = poses + 16 * (int64_t)n;
    float pc[3][3], nc[3][3];
    const bool want_n = out.normal || prm.use_light;
    for (int k = 0; k < 3; ++k) {
        const float *p = m.verts + 3 * (int64_t)idx[k];
        for (int i = 0; i < 3; ++i) pc[k][i] = ((P[4 * i] * p[0] + P[4 * i + 1] * p[1]) + P[4 * i + 2] * p[2]) + P[4 * i + 3];
        if (want_n) {
            const float *q = m.vnormals + 3 * (int64_t)idx[k];
            for (int i = 0; i < 3; ++i) nc[k][i] = (P[4 * i] * q[0] + P[4 * i + 1] * q[1]) + P[4 * i + 2] * q[2];
        }
    }
    float xyz[3], col[3];
    for (int i = 0; i < 3; ++i) xyz[i] = lerp3(u, v, bt, pc[0][i], pc[1][i], pc[2][i]);
    if (m.tex) {
        float uv[2];
        for (int i = 0; i < 2; ++i)
            uv[i] = lerp3(u, v, bt, m.uv[2 * (int64_t)idx[0] + i], m.uv[2 * (int64_t)idx[1] + i], m.uv[2 * (int64_t)idx[2] + i]);
        tex_sample(m.tex, m.tex_h, m.tex_w, 3, uv[0], uv[1], col);
    } else {
        for (int i = 0; i < 3; ++i)
            col[i] = lerp3(u, v, bt, m.vcolor[3 * (int64_t)idx[0] + i], m.vcolor[3 * (int64_t)idx[1] + i], m.vcolor[3 * (int64_t)idx[2] + i]);
    }
    if (prm.use_light) {
        float dif[3];
        for (int k = 0; k < 3; ++k) {
            float nh[3] = {nc[k][0], nc[k][1], nc[k][2]}, l[3];
            normalize3(nh);
            for (int i = 0; i < 3; ++i) l[i] = prm.light_mode == 0 ? -prm.light_dir[i] : prm.light_pos[i] - pc[k][i];
            normalize3(l);
            dif[k] = clamp01((nh[0] * l[0] + nh[1] * l[1]) + nh[2] * l[2]);
        }
        const float d = lerp3(u, v, bt, dif[0], dif[1], dif[2]);
        for (int i = 0; i < 3; ++i) {
            const float lc = prm.has_light_color ? prm.light_color[i] : col[i];
            col[i] = col[i] * prm.w_ambient + (d * lc) * prm.w_diffuse;
        }
    }
    for (int i = 0; i < 3; ++i) out.color[3 * o + i] = clamp01(col[i]);
    out.depth[o] = xyz[2];
    if (out.xyz)
        for (int i = 0; i < 3; ++i) out.xyz[3 * o + i] = xyz[i];
    if (out.normal) {
        float nm[3];
        for (int i = 0; i < 3; ++i) nm[i] = lerp3(u, v, bt, nc[0][i], nc[1][i], nc[2][i]);
        normalize3(nm);
        for (int i = 0; i < 3; ++i) out.normal[3 * o + i] = nm[i];
    }
}

// dr.rasterize's output, GL row order: (u, v, z/w, triangle id + 1), zero on the background
__global__ void __launch_bounds__(RB) rast_out_kernel(ClipSrc s, const int32_t *faces, int64_t F, int n0, int H, int W,
                                                      const unsigned long long *keys, float *rast) {
    const int64_t pix = (int64_t)blockIdx.x * RB + threadIdx.x;
    if (pix >= (int64_t)H * W) return;
    const int n = n0 + (int)blockIdx.y;
    const int r = (int)(pix / W), c = (int)(pix % W);
    const unsigned long long key = keys[(int64_t)blockIdx.y * H * W + pix];
    const int64_t t = (int64_t)(key & 0xFFFFFFFFull);
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    Tri T;
    float u, v, zd;
    if (key != EMPTY && t < F && tri_setup(s, faces, t, n, H, W, T) && cover(T, pixel_ndc(c, W), pixel_ndc(r, H), &u, &v, &zd))
        o = make_float4(u, v, zd, (float)(t + 1));
    reinterpret_cast<float4 *>(rast)[((int64_t)n * H * W) + pix] = o;
}

__global__ void __launch_bounds__(RB) interpolate_kernel(const float *attr, int attr_batched, int64_t V, int A,
                                                         const float *rast, int64_t HW, int64_t total, const int32_t *tri,
                                                         int64_t F, float *out) {
    const int64_t p = (int64_t)blockIdx.x * RB + threadIdx.x;
    if (p >= total) return;
    const float4 r = reinterpret_cast<const float4 *>(rast)[p];
    float *o = out + p * A;
    int32_t idx[3] = {-1, -1, -1};
    if (r.w >= 1.0f && r.w <= (float)F) {
        const int64_t t = (int64_t)r.w - 1;  // (float)F rounds above F for some F > 2^24: t == F must not be read
        if (t < F)
            for (int k = 0; k < 3; ++k) idx[k] = tri[3 * t + k];
    }
    if (idx[0] < 0 || idx[1] < 0 || idx[2] < 0 || idx[0] >= V || idx[1] >= V || idx[2] >= V) {
        for (int a = 0; a < A; ++a) o[a] = 0.f;
        return;
    }
    const float *base = attr + (attr_batched ? (p / HW) * V * A : 0);
    const float bt = (1.0f - r.x) - r.y;
    for (int a = 0; a < A; ++a)
        o[a] = lerp3(r.x, r.y, bt, base[(int64_t)idx[0] * A + a], base[(int64_t)idx[1] * A + a], base[(int64_t)idx[2] * A + a]);
}

__global__ void __launch_bounds__(RB) texture_kernel(const float *tex, int tex_batched, int th, int tw, int C,
                                                     const float *uv, int64_t HW, int64_t total, float *out) {
    const int64_t p = (int64_t)blockIdx.x * RB + threadIdx.x;
    if (p >= total) return;
    const float *t = tex + (tex_batched ? (p / HW) * th * tw * C : 0);
    float tmp[16];
    tex_sample(t, th, tw, C, uv[2 * p], uv[2 * p + 1], tmp);
    for (int ch = 0; ch < C; ++ch) out[p * C + ch] = tmp[ch];
}

// ---------------------------------------------------------------- host side

size_t a256(size_t b) { return (b + 255) & ~(size_t)255; }

// Inputs of a host-memory call are uploaded into `io` one after the other; device-memory calls use the caller's pointers.
struct Staging {
    pedp_ctx_s *c;
    int mem;
    char *base = nullptr;
    size_t off = 0;
    int rc = PEDP_OK;
    template <class T>
    const T *in(const T *src, size_t count) {
        if (mem == PEDP_DEVICE || !src || rc) return src;
        T *d = (T *)(base + off);
        off += a256(sizeof(T) * count);
        rc = pedp_upload(c, d, src, sizeof(T) * count);
        return d;
    }
    template <class T>
    T *out(T *dst, size_t count) {
        if (mem == PEDP_DEVICE || !dst) return dst;
        T *d = (T *)(base + off);
        off += a256(sizeof(T) * count);
        return d;
    }
};

int zero_fill(pedp_ctx_s *c, int mem, void *p, size_t bytes) {
    if (!p || !bytes) return PEDP_OK;
    if (mem == PEDP_HOST) {
        memset(p, 0, bytes);
        return PEDP_OK;
    }
    PEDP_HIP_CHECK(hipMemsetAsync(p, 0, bytes, c->stream));
    return PEDP_OK;
}

int pose_chunk(pedp_ctx_s *c, int N, int H, int W) {
    int64_t nc = c->render_chunk > 0 ? c->render_chunk : (int64_t)(KEY_BUDGET / (sizeof(unsigned long long) * (size_t)H * W));
    nc = std::max<int64_t>(1, std::min<int64_t>({nc, (int64_t)N, 65535}));
    return (int)nc;
}

// Keys + big list for one chunk of `nc` poses, after `extra` bytes of the call's own at the front of render_ws.
int reserve_raster(pedp_ctx_s *c, int nc, int H, int W, int64_t F, size_t extra, unsigned long long **keys,
                   unsigned long long **big, unsigned long long **big_n, unsigned long long *cap, char **front) {
    *cap = std::min<unsigned long long>((unsigned long long)nc * (unsigned long long)F, BIG_CAP);
    const size_t s_keys = a256(sizeof(unsigned long long) * (size_t)nc * H * W);
    const size_t s_big = a256(sizeof(unsigned long long) * (size_t)*cap);
    int st = c->render_ws.reserve(a256(extra) + s_keys + s_big + 256);
    if (st) return st;
    char *b = (char *)c->render_ws.ptr;
    *front = b;
    b += a256(extra);
    *keys = (unsigned long long *)b;
    *big = (unsigned long long *)(b + s_keys);
    *big_n = (unsigned long long *)(b + s_keys + s_big);
    return PEDP_OK;
}

int raster_chunk(pedp_ctx_s *c, const ClipSrc &s, const int32_t *faces, int64_t F, int n0, int nc, int H, int W,
                 unsigned long long *keys, unsigned long long *big, unsigned long long *big_n, unsigned long long cap) {
    PEDP_HIP_CHECK(hipMemsetAsync(keys, 0xFF, sizeof(unsigned long long) * (size_t)nc * H * W, c->stream));
    PEDP_HIP_CHECK(hipMemsetAsync(big_n, 0, sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(raster_kernel, dim3((unsigned)((F + RB - 1) / RB), (unsigned)nc), dim3(RB), 0, c->stream, s, faces, F, n0,
                       H, W, keys, big, big_n, cap);
    const unsigned g = (unsigned)std::max<unsigned long long>(1, std::min<unsigned long long>(cap, 16384));
    hipLaunchKernelGGL(raster_big_kernel, dim3(g), dim3(BIG_WG), 0, c->stream, s, faces, n0, H, W, keys, (const unsigned long long *)big,
                       (const unsigned long long *)big_n, cap);
    PEDP_HIP_CHECK(hipGetLastError());
    return PEDP_OK;
}

int check_out_size(int N, int H, int W, const char *who) {
    PEDP_REQUIRE(N >= 0 && H > 0 && W > 0 && H <= 16384 && W <= 16384, "%s: bad batch or resolution (N %d, %d x %d)", who, N, H, W);
    PEDP_REQUIRE((int64_t)N * H * W <= ((int64_t)1 << 34), "%s: N x H x W too large", who);
    return PEDP_OK;
}

}  // namespace

extern "C" {

int pedp_render_configure(pedp_ctx_t c, int pose_chunk) {
    PEDP_REQUIRE(c, "pedp_render_configure: null context");
    PEDP_REQUIRE(pose_chunk >= 0 && pose_chunk <= 65535, "pedp_render_configure: pose_chunk %d out of range", pose_chunk);
    c->render_chunk = pose_chunk;
    return PEDP_OK;
}

int pedp_render(pedp_ctx_t c, const float *verts, int64_t V, const int32_t *faces, int64_t F, const float *vnormals,
                const float *vcolor, const float *uv, const float *tex, int tex_h, int tex_w, const float *poses,
                const float *bbox2d, int N, const pedp_render_params *prm, int mem, float *color, float *depth,
                float *normal, float *xyz) {
    const char *who = "pedp_render";
    PEDP_REQUIRE(c && prm, "%s: null context or parameters", who);
    PEDP_REQUIRE(mem == PEDP_HOST || mem == PEDP_DEVICE, "%s: bad mem flag %d", who, mem);
    int rc = check_out_size(N, prm->out_h, prm->out_w, who);
    if (rc) return rc;
    PEDP_REQUIRE(V >= 0 && F >= 0 && V < ((int64_t)1 << 31) && F < ((int64_t)1 << 31), "%s: bad mesh size", who);
    PEDP_REQUIRE(prm->H > 0 && prm->W > 0, "%s: bad image size", who);
    PEDP_REQUIRE(prm->light_mode == 0 || prm->light_mode == 1, "%s: bad light mode", who);
    PEDP_REQUIRE(N == 0 || (poses && color && depth), "%s: null poses or outputs", who);
    const bool textured = tex != nullptr;
    if (V > 0 && F > 0) {
        PEDP_REQUIRE(verts && faces, "%s: null mesh arrays", who);
        PEDP_REQUIRE(vnormals || !(prm->use_light || normal), "%s: null vertex normals", who);
        PEDP_REQUIRE(textured ? (uv && tex_h > 0 && tex_w > 0 && (int64_t)tex_h * tex_w < ((int64_t)1 << 30)) : vcolor != nullptr,
                     "%s: need vertex colours or uv + texture", who);
    }
    const int H = prm->out_h, W = prm->out_w;
    const size_t npix = (size_t)N * H * W;
    if (N == 0) return PEDP_OK;
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    if (V == 0 || F == 0) {
        rc = zero_fill(c, mem, color, sizeof(float) * 3 * npix);
        if (!rc) rc = zero_fill(c, mem, depth, sizeof(float) * npix);
        if (!rc) rc = zero_fill(c, mem, normal, sizeof(float) * 3 * npix);
        if (!rc) rc = zero_fill(c, mem, xyz, sizeof(float) * 3 * npix);
        return rc;
    }
    // host memory: every input and output through render_io
    const bool want_n = prm->use_light != 0;
    if (mem == PEDP_HOST) {
        const size_t need = 3 * a256(12 * V) + a256(12 * F) + a256(8 * V) + a256(12 * (size_t)tex_h * tex_w) + a256(64 * (size_t)N) +
                            a256(16 * (size_t)N) + 3 * a256(12 * npix) + a256(4 * npix);
        rc = c->render_io.reserve(need);
        if (rc) return rc;
    }
    Staging sg{c, mem, (char *)c->render_io.ptr};
    const float *d_verts = sg.in(verts, 3 * V);
    const int32_t *d_faces = sg.in(faces, 3 * F);
    const float *d_vn = want_n || normal ? sg.in(vnormals, 3 * V) : nullptr;
    const float *d_vc = textured ? nullptr : sg.in(vcolor, 3 * V);
    const float *d_uv = textured ? sg.in(uv, 2 * V) : nullptr;
    const float *d_tex = textured ? sg.in(tex, 3 * (size_t)tex_h * tex_w) : nullptr;
    const float *d_poses = sg.in(poses, 16 * (size_t)N);
    const float *d_bbox = sg.in(bbox2d, 4 * (size_t)N);
    // the normal map is written where the caller passes one (render.py asks for it under get_normal or use_light)
    OutArgs o{sg.out(color, 3 * npix), sg.out(depth, npix), sg.out(normal, 3 * npix), sg.out(xyz, 3 * npix)};
    if (sg.rc) return sg.rc;

    const int nc = pose_chunk(c, N, H, W);
    unsigned long long *keys, *big, *big_n, cap;
    char *front;
    rc = reserve_raster(c, nc, H, W, F, sizeof(float) * PREC * (size_t)N, &keys, &big, &big_n, &cap, &front);
    if (rc) return rc;
    float *prec = (float *)front;
    hipLaunchKernelGGL(pose_prep_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, c->stream, *prm, d_poses, d_bbox, N, prec);
    ClipSrc s{nullptr, d_verts, prec, V};
    MeshArgs m{d_verts, d_vn, d_vc, d_uv, d_tex, d_faces, V, F, tex_h, tex_w};
    for (int n0 = 0; n0 < N; n0 += nc) {
        const int k = std::min(nc, N - n0);
        rc = raster_chunk(c, s, d_faces, F, n0, k, H, W, keys, big, big_n, cap);
        if (rc) return rc;
        hipLaunchKernelGGL(resolve_kernel, dim3((unsigned)((H * W + RB - 1) / RB), (unsigned)k), dim3(RB), 0, c->stream, s, m, *prm,
                           d_poses, n0, (const unsigned long long *)keys, o);
        PEDP_HIP_CHECK(hipGetLastError());
    }
    if (mem == PEDP_HOST) {
        rc = pedp_download(c, color, o.color, sizeof(float) * 3 * npix);
        if (!rc) rc = pedp_download(c, depth, o.depth, sizeof(float) * npix);
        if (!rc && o.normal) rc = pedp_download(c, normal, o.normal, sizeof(float) * 3 * npix);
        if (!rc && xyz) rc = pedp_download(c, xyz, o.xyz, sizeof(float) * 3 * npix);
    }
    return rc;
}

int pedp_rasterize(pedp_ctx_t c, const float *pos, int N, int64_t V, const int32_t *tri, int64_t F, int H, int W, int mem,
                   float *rast) {
    const char *who = "pedp_rasterize";
    PEDP_REQUIRE(c, "%s: null context", who);
    PEDP_REQUIRE(mem == PEDP_HOST || mem == PEDP_DEVICE, "%s: bad mem flag %d", who, mem);
    int rc = check_out_size(N, H, W, who);
    if (rc) return rc;
    PEDP_REQUIRE(V >= 0 && F >= 0 && V < ((int64_t)1 << 31) && F < ((int64_t)1 << 31), "%s: bad mesh size", who);
    PEDP_REQUIRE((int64_t)N * V < ((int64_t)1 << 40), "%s: N x V too large", who);
    const size_t npix = (size_t)N * H * W;
    if (N == 0) return PEDP_OK;
    PEDP_REQUIRE(rast, "%s: null output", who);
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    if (V == 0 || F == 0) return zero_fill(c, mem, rast, sizeof(float) * 4 * npix);
    PEDP_REQUIRE(pos && tri, "%s: null positions or triangles", who);
    if (mem == PEDP_HOST) {
        rc = c->render_io.reserve(a256(16 * (size_t)N * V) + a256(12 * (size_t)F) + a256(16 * npix));
        if (rc) return rc;
    }
    Staging sg{c, mem, (char *)c->render_io.ptr};
    const float *d_pos = sg.in(pos, 4 * (size_t)N * V);
    const int32_t *d_tri = sg.in(tri, 3 * (size_t)F);
    float *d_rast = sg.out(rast, 4 * npix);
    if (sg.rc) return sg.rc;
    const int nc = pose_chunk(c, N, H, W);
    unsigned long long *keys, *big, *big_n, cap;
    char *front;
    rc = reserve_raster(c, nc, H, W, F, 0, &keys, &big, &big_n, &cap, &front);
    if (rc) return rc;
    ClipSrc s{d_pos, nullptr, nullptr, V};
    for (int n0 = 0; n0 < N; n0 += nc) {
        const int k = std::min(nc, N - n0);
        rc = raster_chunk(c, s, d_tri, F, n0, k, H, W, keys, big, big_n, cap);
        if (rc) return rc;
        hipLaunchKernelGGL(rast_out_kernel, dim3((unsigned)((H * W + RB - 1) / RB), (unsigned)k), dim3(RB), 0, c->stream, s, d_tri, F,
                           n0, H, W, (const unsigned long long *)keys, d_rast);
        PEDP_HIP_CHECK(hipGetLastError());
    }
    if (mem == PEDP_HOST) return pedp_download(c, rast, d_rast, sizeof(float) * 4 * npix);
    return PEDP_OK;
}

int pedp_interpolate(pedp_ctx_t c, const float *attr, int attr_batched, int64_t V, int A, const float *rast, int N, int H, int W,
                     const int32_t *tri, int64_t F, int mem, float *out) {
    const char *who = "pedp_interpolate";
    PEDP_REQUIRE(c, "%s: null context", who);
    PEDP_REQUIRE(mem == PEDP_HOST || mem == PEDP_DEVICE, "%s: bad mem flag %d", who, mem);
    int rc = check_out_size(N, H, W, who);
    if (rc) return rc;
    PEDP_REQUIRE(V >= 0 && F >= 0 && V < ((int64_t)1 << 31) && F < ((int64_t)1 << 31) && A > 0 && A <= 1024, "%s: bad sizes", who);
    const size_t npix = (size_t)N * H * W;
    if (N == 0) return PEDP_OK;
    PEDP_REQUIRE(rast && out, "%s: null rast or output", who);
    PEDP_REQUIRE((attr || V == 0) && (tri || F == 0), "%s: null attributes or triangles", who);
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    const size_t s_attr = (size_t)(attr_batched ? N : 1) * V * A;
    if (mem == PEDP_HOST) {
        rc = c->render_io.reserve(a256(4 * s_attr) + a256(12 * (size_t)F) + a256(16 * npix) + a256(4 * npix * A));
        if (rc) return rc;
    }
    Staging sg{c, mem, (char *)c->render_io.ptr};
    const float *d_attr = sg.in(attr, s_attr);
    const int32_t *d_tri = sg.in(tri, 3 * (size_t)F);
    const float *d_rast = sg.in(rast, 4 * npix);
    float *d_out = sg.out(out, npix * A);
    if (sg.rc) return sg.rc;
    hipLaunchKernelGGL(interpolate_kernel, dim3((unsigned)((npix + RB - 1) / RB)), dim3(RB), 0, c->stream, d_attr, attr_batched, V, A,
                       d_rast, (int64_t)H * W, (int64_t)npix, d_tri, F, d_out);
    PEDP_HIP_CHECK(hipGetLastError());
    if (mem == PEDP_HOST) return pedp_download(c, out, d_out, sizeof(float) * A * npix);
    return PEDP_OK;
}

int pedp_texture(pedp_ctx_t c, const float *tex, int tex_n, int th, int tw, int C, const float *uv, int N, int H, int W, int mem,
                 float *out) {
    const char *who = "pedp_texture";
    PEDP_REQUIRE(c, "%s: null context", who);
    PEDP_REQUIRE(mem == PEDP_HOST || mem == PEDP_DEVICE, "%s: bad mem flag %d", who, mem);
    int rc = check_out_size(N, H, W, who);
    if (rc) return rc;
    PEDP_REQUIRE(th > 0 && tw > 0 && (int64_t)th * tw < ((int64_t)1 << 30) && C > 0 && C <= 16, "%s: bad texture size", who);
    PEDP_REQUIRE(tex_n == 1 || tex_n == N, "%s: %d textures for %d images", who, tex_n, N);
    const size_t npix = (size_t)N * H * W;
    if (N == 0) return PEDP_OK;
    PEDP_REQUIRE(tex && uv && out, "%s: null arrays", who);
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    const size_t s_tex = (size_t)tex_n * th * tw * C;
    if (mem == PEDP_HOST) {
        rc = c->render_io.reserve(a256(4 * s_tex) + a256(8 * npix) + a256(4 * npix * C));
        if (rc) return rc;
    }
    Staging sg{c, mem, (char *)c->render_io.ptr};
    const float *d_tex = sg.in(tex, s_tex);
    const float *d_uv = sg.in(uv, 2 * npix);
    float *d_out = sg.out(out, npix * C);
    if (sg.rc) return sg.rc;
    hipLaunchKernelGGL(texture_kernel, dim3((unsigned)((npix + RB - 1) / RB)), dim3(RB), 0, c->stream, d_tex, tex_n > 1 ? 1 : 0, th, tw,
                       C, d_uv, (int64_t)H * W, (int64_t)npix, d_out);
    PEDP_HIP_CHECK(hipGetLastError());
    if (mem == PEDP_HOST) return pedp_download(c, out, d_out, sizeof(float) * C * npix);
    return PEDP_OK;
}

}  // extern "C"
