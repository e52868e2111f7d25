// Stride-1, pad-1 3x3 convolution of FoundationPose's residual blocks as an implicit GEMM on the matrix cores
// (DESIGN.md s4.12): y = act(conv(x, w') + b' [+ residual]), NHWC float16 in and out, float32 accumulation.
//
//   pack_kernel   folds eval-mode BatchNorm into the weights and the bias in float32 and writes the weights as
//                 Cout x 9 x Cin float16 (tap-major, channels innermost): the GEMM's K axis is then contiguous per row
//   conv_kernel   one workgroup (4 waves) per tile of 128 output pixels x 128 output channels.  M is the flattened
//                 N*H*W pixel index, so a tile may straddle two images; a tap outside its own image loads zeros.  A K step
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
    long long M;  // N * H * W
};

// 16-byte slot of (row, chunk) in a 128 x 32-half image, in halves
__device__ __forceinline__ int lds_off(int row, int chunk) { return row * 32 + ((chunk ^ ((row >> 2) & 3)) << 3); }

template <int KC>
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
    int py[2], px[2];
    long long pbase[2];  // element offset of the pixel's own channel 0, or -1 past the end
    const _Float16 *wrow[2];
    for (int r = 0; r < 2; ++r) {
        const long long m = m0 + srow + 64 * r;
        if (m < a.M) {
            const long long img = m / ((long long)a.H * a.W);
            const int rem = (int)(m - img * a.H * a.W);
            py[r] = rem / a.W;
            px[r] = rem - py[r] * a.W;
            pbase[r] = m * a.Cin;
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
    int Cin, Cout, has_bn;
    float eps;
};

// one thread per packed weight; the first Cout threads also write the bias
__global__ void pack_kernel(PackArgs a, const float *__restrict__ w, const float *__restrict__ b, const float *__restrict__ gamma,
                            const float *__restrict__ beta, const float *__restrict__ mean, const float *__restrict__ var,
                            _Float16 *__restrict__ wp, float *__restrict__ bp) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = (long long)a.Cout * 9 * a.Cin;
    if (i >= total) return;
    const int ci = (int)(i % a.Cin), tap = (int)((i / a.Cin) % 9), co = (int)(i / (9LL * a.Cin));
    const float scale = a.has_bn ? gamma[co] / sqrtf(var[co] + a.eps) : 1.0f;
    wp[i] = (_Float16)(w[((size_t)co * a.Cin + ci) * 9 + tap] * scale);
    if (i < a.Cout) {
        const int c = (int)i;
        const float sc = a.has_bn ? gamma[c] / sqrtf(var[c] + a.eps) : 1.0f;
        const float b0 = b ? b[c] : 0.0f;
        bp[c] = a.has_bn ? (b0 - mean[c]) * sc + beta[c] : b0;
    }
}

bool channels_ok(int c) { return c >= 32 && c <= 512 && c % 32 == 0; }

}  // namespace

extern "C" {

int pedp_conv3x3_pack(pedp_ctx_t c, int Cin, int Cout, const float *w, const float *b, const float *gamma, const float *beta,
                      const float *mean, const float *var, float eps, void *w_packed, float *bias) {
    const char *who = "pedp_conv3x3_pack";
    PEDP_REQUIRE(c, "%s: null context", who);
    PEDP_REQUIRE(channels_ok(Cin) && channels_ok(Cout), "%s: Cin = %d, Cout = %d (multiples of 32 up to 512)", who, Cin, Cout);
    PEDP_REQUIRE(w && w_packed && bias, "%s: null array", who);
    const bool bn = gamma || beta || mean || var;
    PEDP_REQUIRE(!bn || (gamma && beta && mean && var), "%s: BatchNorm needs weight, bias, running_mean and running_var", who);
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    PackArgs a{Cin, Cout, bn ? 1 : 0, eps};
    const long long total = (long long)Cout * 9 * Cin;
    hipLaunchKernelGGL(pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, a, w, b, gamma, beta, mean, var,
                       (_Float16 *)w_packed, bias);
    PEDP_HIP_CHECK(hipGetLastError());
    return PEDP_OK;
}

int pedp_conv3x3_f16(pedp_ctx_t c, const pedp_conv3x3_params *prm, const void *x, const void *w_packed, const float *bias,
                     const void *residual, void *y) {
    const char *who = "pedp_conv3x3_f16";
    PEDP_REQUIRE(c && prm, "%s: null context or parameters", who);
    PEDP_REQUIRE(channels_ok(prm->Cin) && channels_ok(prm->Cout), "%s: Cin = %d, Cout = %d (multiples of 32 up to 512)", who,
                 prm->Cin, prm->Cout);
    PEDP_REQUIRE(prm->N >= 1 && prm->H >= 1 && prm->W >= 1, "%s: N x H x W = %d x %d x %d", who, prm->N, prm->H, prm->W);
    PEDP_REQUIRE(prm->y_c0 >= 0 && prm->y_c0 % 4 == 0 && prm->y_ld % 4 == 0 && prm->y_ld >= prm->y_c0 + prm->Cout,
                 "%s: y_ld = %d, y_c0 = %d for Cout = %d (multiples of 4, y_c0 + Cout <= y_ld)", who, prm->y_ld, prm->y_c0, prm->Cout);
    PEDP_REQUIRE(!residual || (prm->res_c0 >= 0 && prm->res_c0 % 4 == 0 && prm->res_ld % 4 == 0 && prm->res_ld >= prm->res_c0 + prm->Cout),
                 "%s: res_ld = %d, res_c0 = %d for Cout = %d", who, prm->res_ld, prm->res_c0, prm->Cout);
    PEDP_REQUIRE(x && w_packed && bias && y, "%s: null array", who);
    PEDP_REQUIRE(((uintptr_t)x | (uintptr_t)w_packed | (uintptr_t)bias) % 16 == 0 && ((uintptr_t)y | (uintptr_t)residual) % 8 == 0,
                 "%s: x, w_packed and bias must be 16-byte aligned, y and residual 8-byte aligned", who);
    const long long M = (long long)prm->N * prm->H * prm->W;
    const long long tiles = ((M + BM - 1) / BM) * ((prm->Cout + BN - 1) / BN);
    PEDP_REQUIRE(tiles <= 0x7FFFFFFFLL, "%s: %lld tiles", who, tiles);
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    ConvArgs a{prm->N, prm->H, prm->W, prm->Cin, prm->Cout, prm->y_ld, prm->y_c0, prm->res_ld, prm->res_c0, prm->relu != 0, M};
    const _Float16 *xs = (const _Float16 *)x, *ws = (const _Float16 *)w_packed, *rs = (const _Float16 *)residual;
    if (prm->Cin % 64 == 0)
        hipLaunchKernelGGL(conv_kernel<2>, dim3((unsigned)tiles), dim3(THREADS), 0, c->stream, a, xs, ws, bias, rs, (_Float16 *)y);
    else
        hipLaunchKernelGGL(conv_kernel<1>, dim3((unsigned)tiles), dim3(THREADS), 0, c->stream, a, xs, ws, bias, rs, (_Float16 *)y);
    PEDP_HIP_CHECK(hipGetLastError());
    return PEDP_OK;
}

}  // extern "C"
