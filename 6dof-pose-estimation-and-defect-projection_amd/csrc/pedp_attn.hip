// Multi-head attention core of the networks' heads, O = softmax(scale * Q K^T) V per (batch, head), flash-style on the
// matrix cores: float16 operands read in place from the packed in-projection output, float32 scores and
// statistics, no S x S matrix in memory.  Head dimension 128 only.
//
//   mha_kernel   one workgroup (4 waves) per (batch, head) and 128 query rows, 32 per wave as two blocks of 16.  Q stays in
//                registers as the MFMA's B operand.  K and V tiles of 64 keys go global -> registers -> LDS in 16-byte
//                pieces (two LDS buffers, one barrier per tile; the next tile's loads are in flight while this tile's MFMAs
//                run and are written after them).  K rows are 256 bytes in LDS with the 16-byte slot XORed by row & 15, so
//                the 16 rows of a ds_read_b128 group fall on 16 different slots; V rows are 256 bytes with the slot XORed by
//                ((row & 3) << 2) | ((row >> 2) & 3) and are read transposed by ds_read_b64_tr_b16.
//                Scores are computed as K Q^T: of v_mfma_f32_16x16x32_f16's result a lane holds four keys of ONE query row,
//                the row's statistics are shared by the four lanes with the same lane & 15, and the 16 probabilities a lane
//                holds per tile are, in its own registers, the B operand of V^T P^T.  That product's k axis runs over the
//                keys in the permuted order the lanes hold them, and the transposed V reads fetch the keys in that order.
//                The result O^T keeps the query row on lane & 15, so the rescale by exp(m_old - m_new) is lane-local, and a
//                lane ends with four consecutive channels per block: one 8-byte store.
//                Tails: a key row >= S is never loaded (zeros go to LDS) and its score is -inf before the maximum, so its
//                probability is exactly 0; a query row >= S is computed on zeros and not stored.  The first tile always holds
//                key 0, so every running maximum is finite after it.  The maximum is rescaled at every tile (no deferred
//                rescale).  No atomics, no split of the key axis: the summation order is fixed.
#include "pedp_internal.h"
#include <hip/hip_fp16.h>
#include <cmath>

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "pedp_attn.hip uses v_mfma_f32_16x16x32_f16 and ds_read_b64_tr_b16: build with --offload-arch=gfx950"
#endif

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float float4v __attribute__((ext_vector_type(4)));

constexpr int D = 128;             // head dimension
constexpr int BK = 64;             // keys per tile
constexpr int BQ = 128;            // query rows per workgroup
constexpr int QW = 32;             // query rows per wave: two 16-row blocks
constexpr int THREADS = 256;       // 4 waves
constexpr int TILE = BK * D;       // halves of one 64-row x 128-channel LDS image

struct MhaArgs {
    int S, H, nq;                  // nq: query tiles per (batch, head)
    long long q_ld, k_ld, v_ld, o_ld;
    float c;                       // scale * log2(e): probabilities are exp2(c * score - max)
};

// halves from the image's start to 16-byte chunk `ch` (0..15) of row `row`
__device__ __forceinline__ int k_off(int row, int ch) { return row * D + ((ch ^ (row & 15)) << 3); }
__device__ __forceinline__ int v_off(int row, int ch) { return row * D + ((ch ^ (((row & 3) << 2) | ((row >> 2) & 3))) << 3); }

// ds_read_b64_tr_b16: the wave's 16-lane group reads a block of 4 rows x 16 columns; lane 4q + p of the group passes the address
// of row q, columns 4p .. 4p + 3, and lane i receives column i of the four rows.  Needs every lane of the wave active.
__device__ __forceinline__ half4 lds_read_tr(const _Float16 *p) {
    typedef short short4v __attribute__((__vector_size__(4 * sizeof(short))));
    const short4v r = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4v *)p);
    return __builtin_bit_cast(half4, r);
}

__global__ __launch_bounds__(THREADS, 2) void mha_kernel(MhaArgs a, const _Float16 *__restrict__ q, const _Float16 *__restrict__ k,
                                                         const _Float16 *__restrict__ v, _Float16 *__restrict__ o) {
    // [buffer][0: K, 1: V][64 rows][128 halves]
    __shared__ __attribute__((aligned(16))) _Float16 lds[2 * 2 * TILE];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    int blk = (int)blockIdx.x;
    const int qt = blk % a.nq;
    blk /= a.nq;
    const int h = blk % a.H, b = blk / a.H;
    const size_t row0 = (size_t)b * a.S;  // the batch's first row in every operand
    const _Float16 *qh = q + row0 * a.q_ld + h * D, *kh = k + row0 * a.k_ld + h * D, *vh = v + row0 * a.v_ld + h * D;
    _Float16 *oh = o + row0 * a.o_ld + h * D;
    const int q0 = qt * BQ + wave * QW;
    const bool active = q0 < a.S;  // wave-uniform: a wave whose rows all lie past S only helps to stage

    // Q as the B operand: lane holds Q[q0 + 16 i + fr][32 ks + 8 fq ..]
    half8 qf[2][4];
    #pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = q0 + 16 * i + fr;
        #pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            half8 z = {};
            qf[i][ks] = row < a.S ? *(const half8 *)(qh + (size_t)row * a.q_ld + 32 * ks + 8 * fq) : z;
        }
    }

    // staging: thread t carries 16-byte chunk t & 15 of rows (t >> 4) + 16 r, r = 0..3, of both tiles
    const int srow = t >> 4, chunk = t & 15;
    half8 gk[4], gv[4];
    auto gload = [&](int tile) {
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int key = tile * BK + srow + 16 * r;
            half8 z = {};
            const bool in = key < a.S;
            gk[r] = in ? *(const half8 *)(kh + (size_t)key * a.k_ld + chunk * 8) : z;
            gv[r] = in ? *(const half8 *)(vh + (size_t)key * a.v_ld + chunk * 8) : z;
        }
    };
    auto lstore = [&](int buf) {
        _Float16 *kb = lds + buf * (2 * TILE), *vb = kb + TILE;
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
            *(half8 *)(kb + k_off(srow + 16 * r, chunk)) = gk[r];
            *(half8 *)(vb + v_off(srow + 16 * r, chunk)) = gv[r];
        }
    };

    float4v acc[2][8];  // O^T: [query block][channel block], row = channel 4 fq + reg, column = query fr
    #pragma unroll
    for (int i = 0; i < 2; ++i)
        #pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = float4v{0.f, 0.f, 0.f, 0.f};
    float m[2] = {-INFINITY, -INFINITY};  // running maximum of c * score, the same in the four lanes of a query row
    float l[2] = {0.f, 0.f};              // this lane's share of the running sum

    const int tiles = (a.S + BK - 1) / BK;
    gload(0);
    lstore(0);
    __syncthreads();
    for (int tile = 0; tile < tiles; ++tile) {
        const int buf = tile & 1;
        if (tile + 1 < tiles) gload(tile + 1);
        if (active) {
            const _Float16 *kb = lds + buf * (2 * TILE), *vb = kb + TILE;
            // scores: s[i][j][e] = score of key 16 j + 4 fq + e against query row 16 i + fr
            float4v s[2][4];
            #pragma unroll
            for (int j = 0; j < 4; ++j) {
                half8 kf[4];
                #pragma unroll
                for (int ks = 0; ks < 4; ++ks) kf[ks] = *(const half8 *)(kb + k_off(16 * j + fr, 4 * ks + fq));
                #pragma unroll
                for (int i = 0; i < 2; ++i) {
                    float4v c = {0.f, 0.f, 0.f, 0.f};
                    #pragma unroll
                    for (int ks = 0; ks < 4; ++ks) c = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[ks], qf[i][ks], c, 0, 0, 0);
                    s[i][j] = c;
                }
            }
            const int key0 = tile * BK + 4 * fq;
            const bool tail = tile * BK + BK > a.S;
            half8 pf[2][2];  // P^T as the B operand: element e of k step u is key 32 u + 16 (e >> 2) + 4 fq + (e & 3)
            #pragma unroll
            for (int i = 0; i < 2; ++i) {
                float mx = -INFINITY;
                #pragma unroll
                for (int j = 0; j < 4; ++j)
                    #pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float x = s[i][j][e] * a.c;
                        if (tail && key0 + 16 * j + e >= a.S) x = -INFINITY;
                        s[i][j][e] = x;
                        mx = fmaxf(mx, x);
                    }
                mx = fmaxf(mx, __shfl_xor(mx, 16));
                mx = fmaxf(mx, __shfl_xor(mx, 32));
                const float mn = fmaxf(m[i], mx);  // finite: tile 0 holds key 0
                const float alpha = __builtin_amdgcn_exp2f(m[i] - mn);
                m[i] = mn;
                float sum = 0.f;
                #pragma unroll
                for (int j = 0; j < 4; ++j)
                    #pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float p = __builtin_amdgcn_exp2f(s[i][j][e] - mn);
                        sum += p;
                        pf[i][j >> 1][4 * (j & 1) + e] = (_Float16)p;
                    }
                l[i] = l[i] * alpha + sum;
                #pragma unroll
                for (int j = 0; j < 8; ++j) acc[i][j] *= alpha;
            }
            // O^T += V^T P^T
            #pragma unroll
            for (int j = 0; j < 8; ++j) {
                half8 vf[2];
                #pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int row = 32 * u + 4 * fq + (fr >> 2), ch = 2 * j + ((fr >> 1) & 1), sub = 4 * (fr & 1);
                    const half4 lo = lds_read_tr(vb + v_off(row, ch) + sub);
                    const half4 hi = lds_read_tr(vb + v_off(row + 16, ch) + sub);
                    vf[u] = half8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                }
                #pragma unroll
                for (int i = 0; i < 2; ++i)
                    #pragma unroll
                    for (int u = 0; u < 2; ++u) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf[u], pf[i][u], acc[i][j], 0, 0, 0);
            }
        }
        if (tile + 1 < tiles) lstore(buf ^ 1);  // the other buffer: its readers passed the barrier that ended tile - 1
        __syncthreads();
    }

    if (!active) return;
    #pragma unroll
    for (int i = 0; i < 2; ++i) {
        float sum = l[i];
        sum += __shfl_xor(sum, 16);
        sum += __shfl_xor(sum, 32);
        const int row = q0 + 16 * i + fr;
        if (row >= a.S) continue;
        const float inv = 1.0f / sum;
        _Float16 *dst = oh + (size_t)row * a.o_ld + 4 * fq;
        #pragma unroll
        for (int j = 0; j < 8; ++j) {
            half4 r;
            #pragma unroll
            for (int e = 0; e < 4; ++e) r[e] = (_Float16)(acc[i][j][e] * inv);
            *(half4 *)(dst + 16 * j) = r;
        }
    }
}

// bytes from an operand's first element to one past its last: rows * S of `ld` elements, H * D of them used
long long extent(const pedp_mha_params *p, long long ld) {
    return (((long long)p->B * p->S - 1) * ld + (long long)p->H * p->D) * 2;
}

bool overlap(const void *x, long long nx, const void *y, long long ny) {
    const uintptr_t a = (uintptr_t)x, b = (uintptr_t)y;
    return a < b + (uintptr_t)ny && b < a + (uintptr_t)nx;
}

}  // namespace

extern "C" {

int pedp_mha_f16(pedp_ctx_t c, const pedp_mha_params *prm, const void *q, const void *k, const void *v, void *o) {
    const char *who = "pedp_mha_f16";
    PEDP_REQUIRE(c && prm, "%s: null context or parameters", who);
    PEDP_REQUIRE(prm->D == D, "%s: head dimension %d (only %d is built)", who, prm->D, D);
    PEDP_REQUIRE(prm->B >= 1 && prm->H >= 1 && prm->S >= 1 && prm->S <= 4096, "%s: B = %d, H = %d, S = %d (B, H >= 1, 1 <= S <= 4096)",
                 who, prm->B, prm->H, prm->S);
    PEDP_REQUIRE(q && k && v && o, "%s: null array", who);
    const long long e = (long long)prm->H * D;
    PEDP_REQUIRE(e <= 0x7FFFFFFFLL && prm->q_ld >= e && prm->k_ld >= e && prm->v_ld >= e && prm->o_ld >= e &&
                     (prm->q_ld | prm->k_ld | prm->v_ld | prm->o_ld) % 8 == 0,
                 "%s: row strides %d, %d, %d, %d for H * D = %lld (multiples of 8, at least H * D)", who, prm->q_ld, prm->k_ld,
                 prm->v_ld, prm->o_ld, e);
    PEDP_REQUIRE(((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o) % 16 == 0, "%s: q, k, v and o must be 16-byte aligned", who);
    PEDP_REQUIRE(std::isfinite(prm->scale), "%s: scale is not finite", who);
    const long long no = extent(prm, prm->o_ld);
    PEDP_REQUIRE(!overlap(o, no, q, extent(prm, prm->q_ld)) && !overlap(o, no, k, extent(prm, prm->k_ld)) &&
                     !overlap(o, no, v, extent(prm, prm->v_ld)),
                 "%s: o overlaps an input", who);
    const int nq = (prm->S + BQ - 1) / BQ;
    const long long blocks = (long long)prm->B * prm->H * nq;
    PEDP_REQUIRE(blocks <= 0x7FFFFFFFLL, "%s: %lld workgroups", who, blocks);
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    MhaArgs a{prm->S, prm->H, nq, prm->q_ld, prm->k_ld, prm->v_ld, prm->o_ld, prm->scale * 1.44269504088896340736f};
    hipLaunchKernelGGL(mha_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, c->stream, a, (const _Float16 *)q, (const _Float16 *)k,
                       (const _Float16 *)v, (_Float16 *)o);
    PEDP_HIP_CHECK(hipGetLastError());
    return PEDP_OK;
}

}  // extern "C"
