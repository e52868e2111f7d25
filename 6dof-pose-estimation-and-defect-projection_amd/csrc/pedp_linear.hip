// The linear layers of the networks' heads, Y = epilogue(X W^T + bias), on the matrix cores: float16
// operands read in place, float32 accumulation, the epilogue on the accumulators, one rounding to float16.
//
//   linear_kernel   one workgroup (4 waves) per tile of BM rows x BN columns, the waves stacked along the rows.  X and W
//                   are both K-contiguous, so both go global -> registers -> LDS in 16-byte pieces of a row (two LDS
//                   buffers, one barrier per K tile; the next tile's loads are in flight while this tile's MFMAs run and
//                   are written after them) and both are read back with ds_read_b128 in the same fragment shape.  The
//                   16-byte slot of a row is XORed with a function of the row so that the lanes one ds_read_b128 serves
//                   together fall on 16 different slots of the 256-byte bank row.
//                   The product is formed as W X^T: of v_mfma_f32_16x16x32_f16's result a lane then holds four CONSECUTIVE
//                   columns of ONE row (row lane & 15, columns 16 j + 4 (lane >> 4) ...), so bias, gamma, beta, the
//                   residual and the result move as 16- and 8-byte pieces, and a row's statistics are sums inside a lane
//                   followed by two shuffles.
//                     PLAIN / RELU   BM 128 (32 rows per wave), BN 128, K tile 64; 64 accumulator registers per lane
//                     ADD_LN         BM 64 (16 rows per wave), BN 512 = the whole row, K tile 32; 128 accumulator registers
//                   The position table is added while X is staged (float32 add, one rounding to float16) and, in ADD_LN,
//                   to the residual in float32.  Tails: a row >= M is never loaded (zeros go to LDS) and never stored; a W
//                   row >= N is zeros and its columns are skipped.  No atomics, K is not split: the order of the sums
//                   depends on the shape alone.
//   pool_kernel     one workgroup per group of S rows: float32 column sums in a fixed order (thread t sums the rows
//                   (t >> 6) + 4 i of the 8 channels 8 (t & 63) ..., the four partial sums are added as (0 + 1) + (2 + 3)),
//                   divided by S, then either rounded to float16 or multiplied with up to 8 float32 weight rows.
#include "pedp_internal.h"
#include <hip/hip_fp16.h>
#include <cmath>

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "pedp_linear.hip uses v_mfma_f32_16x16x32_f16: build with --offload-arch=gfx950"
#endif

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float float4v __attribute__((ext_vector_type(4)));

constexpr int THREADS = 256;       // 4 waves
constexpr int LN_N = 512;          // the only row length ADD_LN is built for
constexpr int POOL_E = 512;        // channels of the pooled tokens
constexpr int POOL_MAX_OUT = 8;

struct LinArgs {
    int M, N, K, nn;               // nn: column tiles
    long long x_ld, y_ld, res_ld;
    int period;                    // of the position table's rows
    int pos_a;                     // the table is added to X
    float eps;
};

// halves from an image's start to 16-byte chunk `ch` of row `row`; rows of BK halves
template <int BK> __device__ __forceinline__ int lds_off(int row, int ch);
template <> __device__ __forceinline__ int lds_off<64>(int row, int ch) { return row * 64 + ((ch ^ ((row >> 1) & 7)) << 3); }
template <> __device__ __forceinline__ int lds_off<32>(int row, int ch) {
    return row * 32 + ((ch ^ ((0x78 >> (2 * ((row >> 2) & 3))) & 3)) << 3);
}

// EPI: PEDP_LINEAR_*; POS: a position table is given
template <int EPI, bool POS>
__global__ __launch_bounds__(THREADS, 1) void linear_kernel(LinArgs a, const _Float16 *__restrict__ x, const _Float16 *__restrict__ w,
                                                            const float *__restrict__ bias, const _Float16 *res,
                                                            const float *__restrict__ pos, const float *__restrict__ gamma,
                                                            const float *__restrict__ beta, _Float16 *y) {
    constexpr bool LN = EPI == PEDP_LINEAR_ADD_LN;
    constexpr int MI = LN ? 1 : 2;             // 16-row blocks per wave
    constexpr int NJ = LN ? LN_N / 16 : 8;     // 16-column blocks per wave
    constexpr int BK = LN ? 32 : 64;
    constexpr int BM = 64 * MI, BN = 16 * NJ, CH = BK / 8;
    constexpr int AC = BM * CH / THREADS, BC = BN * CH / THREADS;   // 16-byte chunks per thread and K tile
    constexpr int IMG = (BM + BN) * BK;        // halves of one buffer: X rows, then W rows
    __shared__ __attribute__((aligned(16))) _Float16 lds[2 * IMG];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int nt = (int)blockIdx.x % a.nn, mt = (int)blockIdx.x / a.nn;
    const int m0 = mt * BM, n0 = nt * BN;
    const int jmax = LN ? NJ : min(NJ, (a.N - n0) / 16);   // wave-uniform: N is a multiple of 64

    // staging: chunk q = t + 256 r of an operand's tile is 16-byte chunk q % CH of row q / CH
    const int srow = t / CH, sch = t % CH;
    half8 gx[AC], gw[BC];
    float4v gp[POS ? AC : 1][2];
    int prow[AC];
    #pragma unroll
    for (int r = 0; r < AC; ++r) prow[r] = POS ? (m0 + srow + (THREADS / CH) * r) % a.period : 0;
    auto gload = [&](int kt) {
        const int k = kt * BK + sch * 8;
        #pragma unroll
        for (int r = 0; r < AC; ++r) {
            const int row = m0 + srow + (THREADS / CH) * r;
            const bool in = row < a.M;
            half8 z = {};
            gx[r] = in ? *(const half8 *)(x + (size_t)row * a.x_ld + k) : z;
            if constexpr (POS) {
                if (a.pos_a) {
                    const float *p = pos + (size_t)prow[r] * a.K + k;
                    float4v zf = {0.f, 0.f, 0.f, 0.f};
                    gp[r][0] = in ? *(const float4v *)p : zf;
                    gp[r][1] = in ? *(const float4v *)(p + 4) : zf;
                }
            }
        }
        #pragma unroll
        for (int r = 0; r < BC; ++r) {
            const int row = n0 + srow + (THREADS / CH) * r;
            half8 z = {};
            gw[r] = row < a.N ? *(const half8 *)(w + (size_t)row * a.K + k) : z;
        }
    };
    auto lstore = [&](int buf) {
        _Float16 *xb = lds + buf * IMG, *wb = xb + BM * BK;
        #pragma unroll
        for (int r = 0; r < AC; ++r) {
            half8 v = gx[r];
            if constexpr (POS) {
                if (a.pos_a) {
                    #pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = (_Float16)((float)v[e] + gp[r][e >> 2][e & 3]);
                }
            }
            *(half8 *)(xb + lds_off<BK>(srow + (THREADS / CH) * r, sch)) = v;
        }
        #pragma unroll
        for (int r = 0; r < BC; ++r) *(half8 *)(wb + lds_off<BK>(srow + (THREADS / CH) * r, sch)) = gw[r];
    };

    float4v acc[MI][NJ];   // [row block][column block]: row = 16 i + fr, columns 16 j + 4 fq + reg
    #pragma unroll
    for (int i = 0; i < MI; ++i)
        #pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = float4v{0.f, 0.f, 0.f, 0.f};

    const int tiles = a.K / BK;
    gload(0);
    lstore(0);
    __syncthreads();
    for (int kt = 0; kt < tiles; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < tiles) gload(kt + 1);
        const _Float16 *xb = lds + buf * IMG, *wb = xb + BM * BK;
        #pragma unroll
        for (int ks = 0; ks < BK / 32; ++ks) {
            half8 xf[MI];
            #pragma unroll
            for (int i = 0; i < MI; ++i) xf[i] = *(const half8 *)(xb + lds_off<BK>(wave * 16 * MI + 16 * i + fr, 4 * ks + fq));
            #pragma unroll
            for (int j = 0; j < NJ; ++j) {
                if (j < jmax) {
                    const half8 wf = *(const half8 *)(wb + lds_off<BK>(16 * j + fr, 4 * ks + fq));
                    #pragma unroll
                    for (int i = 0; i < MI; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf, xf[i], acc[i][j], 0, 0, 0);
                }
            }
        }
        if (kt + 1 < tiles) lstore(buf ^ 1);   // the other buffer: its readers passed the barrier that ended tile kt - 1
        __syncthreads();
    }

    if constexpr (!LN) {
        #pragma unroll
        for (int i = 0; i < MI; ++i) {
            const int row = m0 + wave * 16 * MI + 16 * i + fr;
            if (row >= a.M) continue;
            _Float16 *dst = y + (size_t)row * a.y_ld + n0 + 4 * fq;
            #pragma unroll
            for (int j = 0; j < NJ; ++j) {
                if (j < jmax) {
                    float4v v = acc[i][j];
                    if (bias) v += *(const float4v *)(bias + n0 + 16 * j + 4 * fq);
                    half4 r;
                    #pragma unroll
                    for (int e = 0; e < 4; ++e) r[e] = (_Float16)(EPI == PEDP_LINEAR_RELU ? fmaxf(v[e], 0.f) : v[e]);
                    *(half4 *)(dst + 16 * j) = r;
                }
            }
        }
    } else {
        const int row = m0 + wave * 16 + fr;
        const bool in = row < a.M;
        const _Float16 *rr = res + (size_t)(in ? row : 0) * a.res_ld + 4 * fq;
        const float *pr = POS ? pos + (size_t)((in ? row : 0) % a.period) * LN_N + 4 * fq : nullptr;
        float sum = 0.f;
        #pragma unroll
        for (int j = 0; j < NJ; ++j) {
            float4v v = acc[0][j];
            if (bias) v += *(const float4v *)(bias + 16 * j + 4 * fq);
            float4v r = {0.f, 0.f, 0.f, 0.f};
            if (in) {
                const half4 h = *(const half4 *)(rr + 16 * j);
                r = float4v{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
                if constexpr (POS) r += *(const float4v *)(pr + 16 * j);
            }
            v = in ? r + v : r;
            acc[0][j] = v;
            sum += (v[0] + v[1]) + (v[2] + v[3]);
        }
        sum += __shfl_xor(sum, 16);
        sum += __shfl_xor(sum, 32);
        const float mean = sum / (float)LN_N;
        float sq = 0.f;
        #pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const float4v d = acc[0][j] - mean;
            acc[0][j] = d;
            sq += (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
        }
        sq += __shfl_xor(sq, 16);
        sq += __shfl_xor(sq, 32);
        const float rstd = 1.0f / sqrtf(sq / (float)LN_N + a.eps);
        if (!in) return;
        _Float16 *dst = y + (size_t)row * a.y_ld + 4 * fq;
        #pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const float4v g = *(const float4v *)(gamma + 16 * j + 4 * fq);
            const float4v v = acc[0][j] * rstd * g;
            float4v b = {0.f, 0.f, 0.f, 0.f};
            if (beta) b = *(const float4v *)(beta + 16 * j + 4 * fq);
            half4 r;
            #pragma unroll
            for (int e = 0; e < 4; ++e) r[e] = (_Float16)(v[e] + b[e]);
            *(half4 *)(dst + 16 * j) = r;
        }
    }
}

struct PoolArgs {
    int S, n_out;                  // n_out == 0: the means themselves
    long long x_ld;
};

__global__ __launch_bounds__(THREADS) void pool_kernel(PoolArgs a, const _Float16 *__restrict__ x, const float *__restrict__ w,
                                                       const float *__restrict__ bias, _Float16 *__restrict__ out) {
    __shared__ float part[4][POOL_E];
    __shared__ float dots[POOL_MAX_OUT][4];
    const int t = threadIdx.x, c = t & 63, ph = t >> 6, lane = t & 63;
    const size_t g = blockIdx.x;
    const _Float16 *src = x + g * a.S * a.x_ld + 8 * c;
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int r = ph; r < a.S; r += 4) {
        const half8 v = *(const half8 *)(src + (size_t)r * a.x_ld);
        #pragma unroll
        for (int e = 0; e < 8; ++e) s[e] += (float)v[e];
    }
    #pragma unroll
    for (int e = 0; e < 8; ++e) part[ph][8 * c + e] = s[e];
    __syncthreads();
    // thread t owns channels 2 t and 2 t + 1 from here on
    float m[2];
    #pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int ch = 2 * t + e;
        m[e] = ((part[0][ch] + part[1][ch]) + (part[2][ch] + part[3][ch])) / (float)a.S;
    }
    if (a.n_out == 0) {
        out[g * POOL_E + 2 * t] = (_Float16)m[0];
        out[g * POOL_E + 2 * t + 1] = (_Float16)m[1];
        return;
    }
    for (int o = 0; o < a.n_out; ++o) {
        float d = m[0] * w[o * POOL_E + 2 * t] + m[1] * w[o * POOL_E + 2 * t + 1];
        #pragma unroll
        for (int sh = 1; sh < 64; sh <<= 1) d += __shfl_xor(d, sh);
        if (lane == 0) dots[o][ph] = d;
    }
    __syncthreads();
    if (t < a.n_out) {
        const float d = (dots[t][0] + dots[t][1]) + (dots[t][2] + dots[t][3]);
        out[g * a.n_out + t] = (_Float16)(bias ? d + bias[t] : d);
    }
}

bool overlap(const void *x, long long nx, const void *y, long long ny) {
    if (!x || !y) return false;
    const uintptr_t a = (uintptr_t)x, b = (uintptr_t)y;
    return a < b + (uintptr_t)ny && b < a + (uintptr_t)nx;
}

// bytes from the first element of `rows` rows of `ld` elements, `used` of them used, to one past the last
long long extent(long long rows, long long ld, long long used, int size) { return ((rows - 1) * ld + used) * size; }

template <int EPI>
void launch_linear(bool has_pos, unsigned blocks, hipStream_t s, const LinArgs &a, const void *x, const void *w, const float *bias,
                   const void *res, const float *pos, const float *gamma, const float *beta, void *y) {
    if (has_pos)
        hipLaunchKernelGGL((linear_kernel<EPI, true>), dim3(blocks), dim3(THREADS), 0, s, a, (const _Float16 *)x, (const _Float16 *)w,
                           bias, (const _Float16 *)res, pos, gamma, beta, (_Float16 *)y);
    else
        hipLaunchKernelGGL((linear_kernel<EPI, false>), dim3(blocks), dim3(THREADS), 0, s, a, (const _Float16 *)x, (const _Float16 *)w,
                           bias, (const _Float16 *)res, pos, gamma, beta, (_Float16 *)y);
}

}  // namespace

extern "C" {

int pedp_linear_f16(pedp_ctx_t c, const pedp_linear_params *prm, const void *x, const void *w, const float *bias, const void *res,
                    const float *pos, const float *gamma, const float *beta, void *y) {
    const char *who = "pedp_linear_f16";
    PEDP_REQUIRE(c && prm, "%s: null context or parameters", who);
    const int epi = prm->epilogue;
    const bool ln = epi == PEDP_LINEAR_ADD_LN;
    PEDP_REQUIRE(epi == PEDP_LINEAR_PLAIN || epi == PEDP_LINEAR_RELU || ln, "%s: epilogue %d", who, epi);
    PEDP_REQUIRE(prm->M >= 1 && prm->K >= 64 && prm->K % 64 == 0 && prm->K <= 8192 && prm->N >= 64 && prm->N % 64 == 0,
                 "%s: M = %d, N = %d, K = %d (M >= 1; N and K multiples of 64, K <= 8192)", who, prm->M, prm->N, prm->K);
    PEDP_REQUIRE(x && w && y, "%s: null array", who);
    PEDP_REQUIRE(prm->x_ld >= prm->K && prm->x_ld % 8 == 0 && prm->y_ld >= prm->N && prm->y_ld % 8 == 0,
                 "%s: row strides %d (x, K = %d) and %d (y, N = %d) must be multiples of 8 and at least the row", who, prm->x_ld,
                 prm->K, prm->y_ld, prm->N);
    if (ln) {
        PEDP_REQUIRE(prm->N == LN_N, "%s: ADD_LN is built for N = %d only, got %d", who, LN_N, prm->N);
        PEDP_REQUIRE(res && gamma, "%s: ADD_LN needs res and gamma", who);
        PEDP_REQUIRE(prm->res_ld >= prm->N && prm->res_ld % 8 == 0, "%s: res_ld = %d (a multiple of 8, at least N)", who, prm->res_ld);
        PEDP_REQUIRE(std::isfinite(prm->eps) && prm->eps >= 0.f, "%s: eps", who);
    } else {
        PEDP_REQUIRE(!res && !gamma && !beta, "%s: res, gamma and beta belong to ADD_LN", who);
    }
    const bool pos_a = pos && (!ln || prm->pos_a);
    if (pos) {
        PEDP_REQUIRE(prm->pos_period >= 1 && prm->pos_rows >= prm->pos_period, "%s: pos with period %d and %d rows (1 <= period <= rows)",
                     who, prm->pos_period, prm->pos_rows);
        PEDP_REQUIRE(!(ln && pos_a) || prm->K == prm->N, "%s: one table for x and res needs K == N", who);
    }
    const uintptr_t al = (uintptr_t)x | (uintptr_t)w | (uintptr_t)y | (uintptr_t)bias | (uintptr_t)res | (uintptr_t)pos |
                         (uintptr_t)gamma | (uintptr_t)beta;
    PEDP_REQUIRE(al % 16 == 0, "%s: every array must be 16-byte aligned", who);
    const long long M = prm->M, N = prm->N, K = prm->K, ny = extent(M, prm->y_ld, N, 2);
    const bool in_place = ln && res == y && prm->res_ld == prm->y_ld;   // a lane reads the residual elements it then writes
    PEDP_REQUIRE(!overlap(y, ny, x, extent(M, prm->x_ld, K, 2)) && !overlap(y, ny, w, N * K * 2) && !overlap(y, ny, bias, N * 4) &&
                     (in_place || !overlap(y, ny, res, ln ? extent(M, prm->res_ld, N, 2) : 0)) &&
                     !overlap(y, ny, pos, (long long)prm->pos_rows * (pos_a ? K : N) * 4) && !overlap(y, ny, gamma, N * 4) &&
                     !overlap(y, ny, beta, N * 4),
                 "%s: y overlaps an input", who);
    const int bm = ln ? 64 : 128, bn = ln ? LN_N : 128;
    const int nn = (prm->N + bn - 1) / bn;
    const long long blocks = ((M + bm - 1) / bm) * nn;
    PEDP_REQUIRE(blocks <= 0x7FFFFFFFLL, "%s: %lld workgroups", who, blocks);
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    LinArgs a{prm->M, prm->N, prm->K, nn, prm->x_ld, prm->y_ld, ln ? prm->res_ld : 0, pos ? prm->pos_period : 1, pos_a ? 1 : 0,
              prm->eps};
    if (epi == PEDP_LINEAR_PLAIN)
        launch_linear<PEDP_LINEAR_PLAIN>(pos != nullptr, (unsigned)blocks, c->stream, a, x, w, bias, res, pos, gamma, beta, y);
    else if (epi == PEDP_LINEAR_RELU)
        launch_linear<PEDP_LINEAR_RELU>(pos != nullptr, (unsigned)blocks, c->stream, a, x, w, bias, res, pos, gamma, beta, y);
    else
        launch_linear<PEDP_LINEAR_ADD_LN>(pos != nullptr, (unsigned)blocks, c->stream, a, x, w, bias, res, pos, gamma, beta, y);
    PEDP_HIP_CHECK(hipGetLastError());
    return PEDP_OK;
}

int pedp_token_pool_f16(pedp_ctx_t c, const pedp_token_pool_params *prm, const void *x, const float *w, const float *bias, void *out) {
    const char *who = "pedp_token_pool_f16";
    PEDP_REQUIRE(c && prm, "%s: null context or parameters", who);
    PEDP_REQUIRE(prm->B >= 1 && prm->S >= 1 && (long long)prm->B * prm->S <= 0x7FFFFFFFLL, "%s: B = %d, S = %d", who, prm->B, prm->S);
    PEDP_REQUIRE(prm->E == POOL_E, "%s: E = %d (only %d is built)", who, prm->E, POOL_E);
    PEDP_REQUIRE(prm->x_ld >= prm->E && prm->x_ld % 8 == 0, "%s: x_ld = %d (a multiple of 8, at least E)", who, prm->x_ld);
    PEDP_REQUIRE(x && out, "%s: null array", who);
    PEDP_REQUIRE(w ? prm->n_out >= 1 && prm->n_out <= POOL_MAX_OUT : prm->n_out == 0 && !bias,
                 "%s: n_out = %d (1 .. %d with w; 0 and no bias without)", who, prm->n_out, POOL_MAX_OUT);
    PEDP_REQUIRE(((uintptr_t)x | (uintptr_t)w | (uintptr_t)bias) % 16 == 0 && (uintptr_t)out % 2 == 0,
                 "%s: x, w and bias must be 16-byte aligned, out 2-byte", who);
    const long long no = (long long)prm->B * (w ? prm->n_out : POOL_E) * 2;
    PEDP_REQUIRE(!overlap(out, no, x, extent((long long)prm->B * prm->S, prm->x_ld, POOL_E, 2)) &&
                     !overlap(out, no, w, (long long)prm->n_out * POOL_E * 4) && !overlap(out, no, bias, prm->n_out * 4LL),
                 "%s: out overlaps an input", who);
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    PoolArgs a{prm->S, w ? prm->n_out : 0, prm->x_ld};
    hipLaunchKernelGGL(pool_kernel, dim3((unsigned)prm->B), dim3(THREADS), 0, c->stream, a, (const _Float16 *)x, w, bias, (_Float16 *)out);
    PEDP_HIP_CHECK(hipGetLastError());
    return PEDP_OK;
}

}  // extern "C"
