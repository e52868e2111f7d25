// The convolutions of FoundationPose's encoders as implicit GEMMs on the matrix cores: the pad-1 3x3
// convolution with stride 1 (the residual blocks) or 2 (the two that halve the resolution), y = act(conv(x, w') + b'
// [+ residual]), NHWC float16 in and out, float32 accumulation; and the 7x7 stride-2 stem on NCHW crops (conv/stem.h).
//
//   pack_kernel   folds eval-mode BatchNorm into the weights and the bias in float32 and writes the weights as
//                 Cout x KH*KW x Cin float16 (tap-major, channels innermost): the GEMM's K axis is then contiguous per
//                 row.  The stem's form pads the channels to 8 and the row to 416 with zeros.
//   conv_kernel   one workgroup (4 waves) per tile of 128 output pixels x 128 output channels.  M is the flattened
//                 N*OH*OW pixel index, so a tile may straddle two images; a tap outside its own image loads zeros: tap
//                 (ky, kx) of output pixel (oy, ox) reads input (S * oy + ky - 1, S * ox + kx - 1).  A K step
//                 is one tap and 32 * KC input channels: both operands go global -> registers -> LDS in 16-byte pieces
//                 along the channel axis (two LDS buffers, one barrier per step; the next step's loads are in flight
//                 while this step's MFMAs run).  Rows are 64 bytes in LDS with the 16-byte slot XORed by (row >> 2) & 3,
//                 so the 16 rows a ds_read_b128 group touches fall on 16 different slots.
//                 The weights are the MFMA's A operand and the pixels its B operand: of v_mfma_f32_16x16x32_f16's result
//                 a lane then holds four consecutive output channels of one pixel, which is one 8-byte residual read and one
//                 8-byte store.  Each output element is read (residual) and written by one lane, so the residual may be
//                 the destination.  No atomics, no split of K across workgroups: the summation order is fixed.
#include "pedp_internal.h"
#include <hip/hip_fp16.h>

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "pedp_conv.hip uses v_mfma_f32_16x16x32_f16: build with --offload-arch=gfx950"
#endif

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float float4v __attribute__((ext_vector_type(4)));

constexpr int BM = 128;       // output pixels per workgroup
constexpr int BN = 128;       // output channels per workgroup
constexpr int THREADS = 256;  // 4 waves: 2 along the channels x 2 along the pixels, 64 x 64 each
constexpr int SUB = BM * 32;  // halves of one 128-row x 32-channel LDS image

struct ConvArgs {
    int N, H, W, Cin, Cout;
    int y_ld, y_c0, res_ld, res_c0, relu;
    long long M;  // N * OH * OW
    int OH, OW;   // (H + 2 - 3) / S + 1: H, W at stride 1
};

// 16-byte slot of (row, chunk) in a 128 x 32-half image, in halves
__device__ __forceinline__ int lds_off(int row, int chunk) { return row * 32 + ((chunk ^ ((row >> 2) & 3)) << 3); }

template <int KC, int S>
__global__ __launch_bounds__(THREADS) void conv_kernel(ConvArgs a, const _Float16 *__restrict__ x,
                                                       const _Float16 *__restrict__ wp, const float *__restrict__ bias,
                                                       const _Float16 *res, _Float16 *y) {
    // [buffer][operand: 0 weights, 1 pixels][KC][128 rows][32 halves]
    __shared__ __attribute__((aligned(16))) _Float16 lds[2 * 2 * KC * SUB];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int n_tiles = (a.Cout + BN - 1) / BN;
    const long long m0 = (long long)(blockIdx.x / n_tiles) * BM;
    const int c0 = (int)(blockIdx.x % n_tiles) * BN;
    const int K = 9 * a.Cin;

    // staging: thread t carries rows (t >> 2) and (t >> 2) + 64 of both operands, 16-byte chunk t & 3 of every 32 channels
    const int srow = t >> 2, chunk = t & 3;
    int py[2], px[2];    // the input pixel under the output pixel's centre tap
    long long pbase[2];  // element offset of that pixel's channel 0, or -1 past the end
    const _Float16 *wrow[2];
    for (int r = 0; r < 2; ++r) {
        const long long m = m0 + srow + 64 * r;
        if (m < a.M) {
            const long long img = m / ((long long)a.OH * a.OW);
            const int rem = (int)(m - img * a.OH * a.OW);
            py[r] = rem / a.OW;
            px[r] = rem - py[r] * a.OW;
            if (S == 1) {
                pbase[r] = m * a.Cin;
            } else {
                py[r] *= S;
                px[r] *= S;
                pbase[r] = ((img * a.H + py[r]) * a.W + px[r]) * a.Cin;
            }
        } else {
            py[r] = px[r] = 0;
            pbase[r] = -1;
        }
        const int co = c0 + srow + 64 * r;
        wrow[r] = co < a.Cout ? wp + (size_t)co * K : nullptr;
    }

    const int csteps = a.Cin / (32 * KC);
    const int steps = 9 * csteps;
    half8 gw[2][KC], gx[2][KC];

    auto gload = [&](int s) {
        const int tap = s / csteps, cb = (s - tap * csteps) * (32 * KC) + chunk * 8;
        const int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
        for (int r = 0; r < 2; ++r) {
            const int iy = py[r] + dy, ix = px[r] + dx;
            const bool in = pbase[r] >= 0 && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
            const _Float16 *xs = x + (in ? pbase[r] + ((long long)dy * a.W + dx) * a.Cin + cb : 0);
            const _Float16 *ws = wrow[r] ? wrow[r] + (size_t)tap * a.Cin + cb : wp;
            for (int k = 0; k < KC; ++k) {
                half8 z = {};
                gx[r][k] = in ? *(const half8 *)(xs + 32 * k) : z;
                gw[r][k] = wrow[r] ? *(const half8 *)(ws + 32 * k) : z;
            }
        }
    };
    auto lstore = [&](int buf) {
        _Float16 *b = lds + buf * (2 * KC * SUB);
        for (int r = 0; r < 2; ++r)
            for (int k = 0; k < KC; ++k) {
                const int o = k * SUB + lds_off(srow + 64 * r, chunk);
                *(half8 *)(b + o) = gw[r][k];
                *(half8 *)(b + KC * SUB + o) = gx[r][k];
            }
    };

    float4v acc[4][4];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) acc[i][j] = float4v{0.f, 0.f, 0.f, 0.f};
    const int wc = wave >> 1, wpx = wave & 1;  // the wave's 64 channels / 64 pixels of the tile
    const int fr = lane & 15, fq = lane >> 4;

    gload(0);
    lstore(0);
    __syncthreads();
    for (int s = 0; s < steps; ++s) {
        const int buf = s & 1;
        if (s + 1 < steps) gload(s + 1);
        const _Float16 *b = lds + buf * (2 * KC * SUB);
        for (int k = 0; k < KC; ++k) {
            half8 fw[4], fx[4];
            for (int i = 0; i < 4; ++i) {
                fw[i] = *(const half8 *)(b + k * SUB + lds_off(wc * 64 + i * 16 + fr, fq));
                fx[i] = *(const half8 *)(b + (KC + k) * SUB + lds_off(wpx * 64 + i * 16 + fr, fq));
            }
            for (int i = 0; i < 4; ++i)
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fw[i], fx[j], acc[i][j], 0, 0, 0);
        }
        if (s + 1 < steps) lstore(buf ^ 1);  // the other buffer: its readers passed the barrier that ended step s - 1
        __syncthreads();
    }

    // result fragment (i, j): row = output channel i*16 + fq*4 + reg, column = pixel j*16 + fr
    for (int j = 0; j < 4; ++j) {
        const long long m = m0 + wpx * 64 + j * 16 + fr;
        if (m >= a.M) continue;
        for (int i = 0; i < 4; ++i) {
            const int co = c0 + wc * 64 + i * 16 + fq * 4;
            if (co >= a.Cout) continue;  // Cout is a multiple of 32: a group of four is inside or outside as a whole
            const float4v bv = *(const float4v *)(bias + co);
            float4v v = acc[i][j] + bv;
            if (res) {
                const half4 rv = *(const half4 *)(res + (size_t)m * a.res_ld + a.res_c0 + co);
                for (int e = 0; e < 4; ++e) v[e] += (float)rv[e];
            }
            half4 o;
            for (int e = 0; e < 4; ++e) o[e] = (_Float16)(a.relu ? fmaxf(v[e], 0.f) : v[e]);
            *(half4 *)(y + (size_t)m * a.y_ld + a.y_c0 + co) = o;
        }
    }
}

struct PackArgs {
    int Cin, Cout, taps, CinP, Kp, has_bn;  // a packed row: Kp halves, tap-major, CinP >= Cin channels per tap
    float eps;
};

// one thread per packed weight; the first Cout threads also write the bias
__global__ void pack_kernel(PackArgs a, const float *__restrict__ w, const float *__restrict__ b, const float *__restrict__ gamma,
                            const float *__restrict__ beta, const float *__restrict__ mean, const float *__restrict__ var,
                            _Float16 *__restrict__ wp, float *__restrict__ bp) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = (long long)a.Cout * a.Kp;
    if (i >= total) return;
    const int k = (int)(i % a.Kp), co = (int)(i / a.Kp);
    const int ci = k % a.CinP, tap = k / a.CinP;
    const float scale = a.has_bn ? gamma[co] / sqrtf(var[co] + a.eps) : 1.0f;
    const bool real = ci < a.Cin && tap < a.taps;  // the rest pads the channels and the row with zeros
    wp[i] = real ? (_Float16)(w[((size_t)co * a.Cin + ci) * a.taps + tap] * scale) : (_Float16)0.0f;
    if (i < a.Cout) {
        const int c = (int)i;
        const float sc = a.has_bn ? gamma[c] / sqrtf(var[c] + a.eps) : 1.0f;
        const float b0 = b ? b[c] : 0.0f;
        bp[c] = a.has_bn ? (b0 - mean[c]) * sc + beta[c] : b0;
    }
}

bool channels_ok(int c) { return c >= 32 && c <= 512 && c % 32 == 0; }

#include "conv/stem.h"

int pack(pedp_ctx_t c, const char *who, int Cin, int Cout, int KH, int KW, const float *w, const float *b, const float *gamma,
         const float *beta, const float *mean, const float *var, float eps, void *w_packed, float *bias) {
    PEDP_REQUIRE(c, "%s: null context", who);
    const bool stem = KH == 7 && KW == 7;
    PEDP_REQUIRE(stem || (KH == 3 && KW == 3), "%s: a %d x %d kernel (3 x 3 and 7 x 7 are built)", who, KH, KW);
    PEDP_REQUIRE(channels_ok(Cout) && (stem ? Cin >= 1 && Cin <= 8 : channels_ok(Cin)),
                 "%s: Cin = %d, Cout = %d (multiples of 32 up to 512; Cin 1 .. 8 for 7 x 7)", who, Cin, Cout);
    PEDP_REQUIRE(w && w_packed && bias, "%s: null array", who);
    const bool bn = gamma || beta || mean || var;
    PEDP_REQUIRE(!bn || (gamma && beta && mean && var), "%s: BatchNorm needs weight, bias, running_mean and running_var", who);
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    PackArgs a{Cin, Cout, KH * KW, stem ? 8 : Cin, stem ? STEM_K : 9 * Cin, bn ? 1 : 0, eps};
    const long long total = (long long)Cout * a.Kp;
    hipLaunchKernelGGL(pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, a, w, b, gamma, beta, mean, var,
                       (_Float16 *)w_packed, bias);
    PEDP_HIP_CHECK(hipGetLastError());
    return PEDP_OK;
}

// what the 3x3 entry points share: the checks on the destination, the residual and the pointers, and the launch
template <int S>
int conv3x3(pedp_ctx_t c, const char *who, int N, int H, int W, int Cin, int Cout, int y_ld, int y_c0, int res_ld, int res_c0,
            int relu, const void *x, const void *w_packed, const float *bias, const void *residual, void *y) {
    PEDP_REQUIRE(channels_ok(Cin) && channels_ok(Cout), "%s: Cin = %d, Cout = %d (multiples of 32 up to 512)", who, Cin, Cout);
    PEDP_REQUIRE(N >= 1 && H >= 1 && W >= 1, "%s: N x H x W = %d x %d x %d", who, N, H, W);
    PEDP_REQUIRE(y_c0 >= 0 && y_c0 % 4 == 0 && y_ld % 4 == 0 && y_ld >= y_c0 + Cout,
                 "%s: y_ld = %d, y_c0 = %d for Cout = %d (multiples of 4, y_c0 + Cout <= y_ld)", who, y_ld, y_c0, Cout);
    PEDP_REQUIRE(!residual || (res_c0 >= 0 && res_c0 % 4 == 0 && res_ld % 4 == 0 && res_ld >= res_c0 + Cout),
                 "%s: res_ld = %d, res_c0 = %d for Cout = %d", who, res_ld, res_c0, Cout);
    PEDP_REQUIRE(x && w_packed && bias && y, "%s: null array", who);
    PEDP_REQUIRE(((uintptr_t)x | (uintptr_t)w_packed | (uintptr_t)bias) % 16 == 0 && ((uintptr_t)y | (uintptr_t)residual) % 8 == 0,
                 "%s: x, w_packed and bias must be 16-byte aligned, y and residual 8-byte aligned", who);
    const int OH = (H - 1) / S + 1, OW = (W - 1) / S + 1;  // (H + 2 - 3) / S + 1
    const long long M = (long long)N * OH * OW;
    const long long tiles = ((M + BM - 1) / BM) * ((Cout + BN - 1) / BN);
    PEDP_REQUIRE(tiles <= 0x7FFFFFFFLL, "%s: %lld tiles", who, tiles);
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    ConvArgs a{N, H, W, Cin, Cout, y_ld, y_c0, res_ld, res_c0, relu != 0, M, OH, OW};
    const _Float16 *xs = (const _Float16 *)x, *ws = (const _Float16 *)w_packed, *rs = (const _Float16 *)residual;
    if (Cin % 64 == 0)
        hipLaunchKernelGGL((conv_kernel<2, S>), dim3((unsigned)tiles), dim3(THREADS), 0, c->stream, a, xs, ws, bias, rs, (_Float16 *)y);
    else
        hipLaunchKernelGGL((conv_kernel<1, S>), dim3((unsigned)tiles), dim3(THREADS), 0, c->stream, a, xs, ws, bias, rs, (_Float16 *)y);
    PEDP_HIP_CHECK(hipGetLastError());
    return PEDP_OK;
}

int stem(pedp_ctx_t c, const char *who, const pedp_conv2d_params *p, const void *x, const void *x2, const void *w_packed,
         const float *bias, void *y) {
    PEDP_REQUIRE(p->layout == PEDP_NCHW && (p->dtype == PEDP_F32 || p->dtype == PEDP_F16),
                 "%s: the 7 x 7 convolution reads NCHW float32 or float16 (layout = %d, dtype = %d)", who, p->layout, p->dtype);
    PEDP_REQUIRE(p->Cin >= 1 && p->Cin <= 8 && channels_ok(p->Cout), "%s: Cin = %d (1 .. 8), Cout = %d (multiples of 32 up to 512)",
                 who, p->Cin, p->Cout);
    PEDP_REQUIRE(p->N >= 1 && p->H >= 1 && p->W >= 1, "%s: N x H x W = %d x %d x %d", who, p->N, p->H, p->W);
    PEDP_REQUIRE(x2 ? (p->N0 >= 0 && p->N0 <= p->N) : (p->N0 == p->N || p->N0 == 0),
                 "%s: N0 = %d of N = %d images in the first tensor%s", who, p->N0, p->N, x2 ? "" : " (and no second one)");
    PEDP_REQUIRE(p->y_c0 >= 0 && p->y_c0 % 4 == 0 && p->y_ld % 4 == 0 && p->y_ld >= p->y_c0 + p->Cout,
                 "%s: y_ld = %d, y_c0 = %d for Cout = %d (multiples of 4, y_c0 + Cout <= y_ld)", who, p->y_ld, p->y_c0, p->Cout);
    PEDP_REQUIRE(x && w_packed && bias && y, "%s: null array", who);
    const uintptr_t el = p->dtype == PEDP_F32 ? 4 : 2;
    PEDP_REQUIRE(((uintptr_t)w_packed | (uintptr_t)bias) % 16 == 0 && (uintptr_t)y % 8 == 0 && ((uintptr_t)x | (uintptr_t)x2) % el == 0,
                 "%s: w_packed and bias must be 16-byte aligned, y 8-byte aligned, x to its element", who);
    const int OH = (p->H - 1) / 2 + 1, OW = (p->W - 1) / 2 + 1;  // (H + 6 - 7) / 2 + 1
    StemArgs a{p->N, x2 ? p->N0 : p->N, p->H, p->W, p->Cin, p->Cout, OH, OW, p->y_ld, p->y_c0, p->relu != 0,
               (OW + STEM_TW - 1) / STEM_TW, (OH + STEM_TH - 1) / STEM_TH, (p->Cout + STEM_BN - 1) / STEM_BN};
    const long long tiles = (long long)p->N * a.tiles_y * a.tiles_x * a.c_tiles;
    PEDP_REQUIRE(tiles <= 0x7FFFFFFFLL, "%s: %lld tiles", who, tiles);
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    const _Float16 *ws = (const _Float16 *)w_packed;
    if (p->dtype == PEDP_F32)
        hipLaunchKernelGGL(stem_kernel<float>, dim3((unsigned)tiles), dim3(THREADS), 0, c->stream, a, (const float *)x,
                           (const float *)x2, ws, bias, (_Float16 *)y);
    else
        hipLaunchKernelGGL(stem_kernel<_Float16>, dim3((unsigned)tiles), dim3(THREADS), 0, c->stream, a, (const _Float16 *)x,
                           (const _Float16 *)x2, ws, bias, (_Float16 *)y);
    PEDP_HIP_CHECK(hipGetLastError());
    return PEDP_OK;
}

}  // namespace

extern "C" {

int pedp_conv3x3_pack(pedp_ctx_t c, int Cin, int Cout, const float *w, const float *b, const float *gamma, const float *beta,
                      const float *mean, const float *var, float eps, void *w_packed, float *bias) {
    return pack(c, "pedp_conv3x3_pack", Cin, Cout, 3, 3, w, b, gamma, beta, mean, var, eps, w_packed, bias);
}

int pedp_conv3x3_f16(pedp_ctx_t c, const pedp_conv3x3_params *prm, const void *x, const void *w_packed, const float *bias,
                     const void *residual, void *y) {
    const char *who = "pedp_conv3x3_f16";
    PEDP_REQUIRE(c && prm, "%s: null context or parameters", who);
    return conv3x3<1>(c, who, prm->N, prm->H, prm->W, prm->Cin, prm->Cout, prm->y_ld, prm->y_c0, prm->res_ld, prm->res_c0, prm->relu, x,
                      w_packed, bias, residual, y);
}

int pedp_conv2d_pack(pedp_ctx_t c, int Cin, int Cout, int KH, int KW, const float *w, const float *b, const float *gamma,
                     const float *beta, const float *mean, const float *var, float eps, void *w_packed, float *bias) {
    return pack(c, "pedp_conv2d_pack", Cin, Cout, KH, KW, w, b, gamma, beta, mean, var, eps, w_packed, bias);
}

int pedp_conv2d_f16(pedp_ctx_t c, const pedp_conv2d_params *prm, const void *x, const void *x2, const void *w_packed,
                    const float *bias, const void *residual, void *y) {
    const char *who = "pedp_conv2d_f16";
    PEDP_REQUIRE(c && prm, "%s: null context or parameters", who);
    PEDP_REQUIRE(!residual, "%s: no residual is added by the stride-2 convolutions", who);
    if (prm->KH == 7 && prm->KW == 7 && prm->stride == 2 && prm->pad == 3) return stem(c, who, prm, x, x2, w_packed, bias, y);
    PEDP_REQUIRE(prm->KH == 3 && prm->KW == 3 && prm->stride == 2 && prm->pad == 1,
                 "%s: %d x %d, stride %d, padding %d (built: 3 x 3 / 2 / 1 and 7 x 7 / 2 / 3; stride 1 is pedp_conv3x3_f16)", who,
                 prm->KH, prm->KW, prm->stride, prm->pad);
    PEDP_REQUIRE(prm->layout == PEDP_NHWC && prm->dtype == PEDP_F16 && !x2 && (prm->N0 == prm->N || prm->N0 == 0),
                 "%s: the 3 x 3 convolution reads one NHWC float16 tensor (layout = %d, dtype = %d, N0 = %d)", who, prm->layout,
                 prm->dtype, prm->N0);
    return conv3x3<2>(c, who, prm->N, prm->H, prm->W, prm->Cin, prm->Cout, prm->y_ld, prm->y_c0, 0, 0, prm->relu, x, w_packed, bias,
                      nullptr, y);
}

}  // extern "C"
