// The 7x7, stride-2, pad-3 convolution that opens FoundationPose's shared encoder, for Cin <= 8:
// NCHW float32 or float16 crops, read from two base pointers (images 0 .. N0 from the first, N0 .. N from the second),
// to NHWC float16.  Included by pedp_conv.hip, inside its anonymous namespace.
//
//   K axis        (ky, kx, ci padded to 8): one 16-byte slot per tap, 49 taps = 392 halves, padded with zero weights to
//                 416 = 13 steps of v_mfma_f32_16x16x32_f16.  In a step, the lanes of quarter q = lane >> 4 carry tap
//                 4 * step + q: an operand fragment is the 8 channels of one input pixel.
//   tile          one workgroup (4 waves) per 8 x 16 output pixels of one image x 64 output channels.  The 21 x 37 input
//                 patch under the tile is staged once into LDS as one half8 per pixel (float32 rounded to nearest even on
//                 the way, zeros outside the image and for channels >= Cin): 13440 bytes.  Even and odd columns of a patch
//                 row lie apart (slots 0 .. 18 and 20 .. 37 of a 40-slot row), so the 16 pixels of a fragment, two input
//                 columns apart, read 16 consecutive slots.
//   waves         2 along the channels x 2 along the pixels: 32 channels x 64 pixels (four tile rows) each, 2 x 4
//                 accumulators.  A wave's weights, 2 x 13 fragments, are read once from global memory into registers; the
//                 pixel fragments are one ds_read_b128 each, straight from the patch: nothing is gathered per tap.
//   order         every output element is the sum of its 13 steps in turn, in float32: fixed by the shape alone.
constexpr int STEM_TH = 8, STEM_TW = 16;            // output tile
constexpr int STEM_PH = 2 * STEM_TH + 5;            // patch rows (21)
constexpr int STEM_PW = 2 * STEM_TW + 5;            // patch columns (37)
constexpr int STEM_ROW = 40;                        // 16-byte slots of a patch row in LDS: even columns at 0, odd at 20
constexpr int STEM_ODD = 20;
constexpr int STEM_K = 416;                         // packed row: 52 taps x 8 channels, taps 49 .. 51 zero
constexpr int STEM_KSTEPS = STEM_K / 32;
constexpr int STEM_BN = 64;                         // output channels per workgroup

struct StemArgs {
    int N, N0, H, W, Cin, Cout, OH, OW;
    int y_ld, y_c0, relu;
    int tiles_x, tiles_y, c_tiles;
};

template <typename T>
__global__ __launch_bounds__(THREADS) void stem_kernel(StemArgs a, const T *__restrict__ xa, const T *__restrict__ xb,
                                                       const _Float16 *__restrict__ wp, const float *__restrict__ bias,
                                                       _Float16 *__restrict__ y) {
    __shared__ __attribute__((aligned(16))) _Float16 patch[STEM_PH * STEM_ROW * 8];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    unsigned b = blockIdx.x;
    const int c0 = (int)(b % a.c_tiles) * STEM_BN;
    b /= a.c_tiles;
    const int ox0 = (int)(b % a.tiles_x) * STEM_TW;
    b /= a.tiles_x;
    const int oy0 = (int)(b % a.tiles_y) * STEM_TH;
    const int img = (int)(b / a.tiles_y);
    const size_t plane = (size_t)a.H * a.W;
    const T *src = img < a.N0 ? xa + (size_t)img * a.Cin * plane : xb + (size_t)(img - a.N0) * a.Cin * plane;

    // the patch: one thread per input pixel, its channels gathered from the planes (threads run along a row)
    const int iy0 = 2 * oy0 - 3, ix0 = 2 * ox0 - 3;
    for (int p = t; p < STEM_PH * STEM_PW; p += THREADS) {
        const int py = p / STEM_PW, px = p - py * STEM_PW;
        const int iy = iy0 + py, ix = ix0 + px;
        half8 v = {};
        if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) {
            const T *s = src + (size_t)iy * a.W + ix;
            for (int ci = 0; ci < 8; ++ci)
                if (ci < a.Cin) v[ci] = (_Float16)s[(size_t)ci * plane];
        }
        *(half8 *)(patch + (py * STEM_ROW + (px & 1) * STEM_ODD + (px >> 1)) * 8) = v;
    }

    const int wc = wave >> 1, wpx = wave & 1;
    const int fr = lane & 15, fq = lane >> 4;
    half8 fw[2][STEM_KSTEPS];
    for (int i = 0; i < 2; ++i) {
        const int co = c0 + wc * 32 + i * 16 + fr;
        for (int s = 0; s < STEM_KSTEPS; ++s) {
            half8 z = {};
            fw[i][s] = co < a.Cout ? *(const half8 *)(wp + (size_t)co * STEM_K + s * 32 + fq * 8) : z;
        }
    }
    float4v acc[2][4];
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 4; ++j) acc[i][j] = float4v{0.f, 0.f, 0.f, 0.f};
    __syncthreads();

    // slot of output pixel (ty, tx) under tap (ky, kx): (2 ty + ky) * ROW + (kx & 1) * ODD + (kx >> 1) + tx
    const int base = (2 * wpx * 4) * STEM_ROW + fr;
#pragma unroll
    for (int s = 0; s < STEM_KSTEPS; ++s) {
        const int tap = 4 * s + fq, tp = tap < 49 ? tap : 48;  // taps 49 .. 51 pad K: their address stays inside the patch
        const int ky = tp / 7, kx = tp - ky * 7;
        const int off = base + ky * STEM_ROW + (kx & 1) * STEM_ODD + (kx >> 1);
        half8 fx[4];
        for (int j = 0; j < 4; ++j) {
            half8 z = {};
            fx[j] = tap < 49 ? *(const half8 *)(patch + (off + 2 * j * STEM_ROW) * 8) : z;
        }
        for (int i = 0; i < 2; ++i)
            for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fw[i][s], fx[j], acc[i][j], 0, 0, 0);
    }

    // result fragment (i, j): row = output channel i*16 + fq*4 + reg, column = pixel (tile row wpx*4 + j, column fr)
    const int ox = ox0 + fr;
    for (int j = 0; j < 4; ++j) {
        const int oy = oy0 + wpx * 4 + j;
        if (oy >= a.OH || ox >= a.OW) continue;
        const size_t m = ((size_t)img * a.OH + oy) * a.OW + ox;
        for (int i = 0; i < 2; ++i) {
            const int co = c0 + wc * 32 + i * 16 + fq * 4;
            if (co >= a.Cout) continue;  // Cout is a multiple of 32: a group of four is inside or outside as a whole
            const float4v v = acc[i][j] + *(const float4v *)(bias + co);
            half4 o;
            for (int e = 0; e < 4; ++e) o[e] = (_Float16)(a.relu ? fmaxf(v[e], 0.f) : v[e]);
            *(half4 *)(y + m * a.y_ld + a.y_c0 + co) = o;
        }
    }
}
