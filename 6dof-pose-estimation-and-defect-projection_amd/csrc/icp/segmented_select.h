// ICP, segmented path, second half: exact selection from the sweep triples, the float64 fallback, and
// the accumulate / reduce kernels that feed the solve.
#pragma once
#include "segmented_sweep.h"

namespace {

// ---- 4. exact selection, four threads per slot (thread gl of a slot reads lane group gl of
// every segment of its block): window = min b1 + 2 eps; every (segment, lane group) whose best
// tile is inside the window has its 4 rows re-scored in float64 (the oracle's formula,
// lexicographic (d^2, index) min); a second tile inside the window sends the slot to
// nn_fallback.
template <int QT>
__global__ __launch_bounds__(256) void nn_select_kernel(
    IcpState *__restrict__ st, const int32_t *__restrict__ blk_segstart, const float *__restrict__ tr_b1,
    const int32_t *__restrict__ tr_t1, const float *__restrict__ tr_b2, const double *__restrict__ tgt,
    const int32_t *__restrict__ tperm /* sorted row -> target index */, int64_t Nt, const double *__restrict__ P,
    const float *__restrict__ eps, const float *__restrict__ S, const int32_t *__restrict__ list, float r2f,
    int32_t *__restrict__ idx_out, double *__restrict__ d2_out, int32_t *__restrict__ fb_list) {
    if (st->done) return;
    const int count = st->n_blocks * (NN_SB * 16);
    const int tid = blockIdx.x * blockDim.x + threadIdx.x;
    const int k = tid >> 2, gl = tid & 3;
    if ((tid & ~63) >= 4 * count) return;  // whole wave beyond the list
    const int kk = k < count ? k : 0;
    const int i = k < count ? list[kk] : -1;
    const bool live = i >= 0;  // dummies carry -1
    const int blk = kk >> 7, slot = kk & 127;
    const int s0 = blk_segstart[blk], s1 = blk_segstart[blk + 1];
    // everything the slot needs later is requested now, ahead of the dependent loads below
    const float e = eps[kk], Si = S[kk];
    const int64_t ip = live ? i : 0;
    const double px = P[3 * ip], py = P[3 * ip + 1], pz = P[3 * ip + 2];
    const float inf = __uint_as_float(0x7F800000u);
    float m = inf, sm = inf, m2 = inf;  // own best b1, own second-best b1, best b2
    int mt = 0;                         // unit of the own best
    for (int sg = s0; sg < s1; sg += 4) {  // four segments per trip: twelve loads in flight
        float v1[4], v2[4];
        int vt[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool in = sg + u < s1;
            const size_t o = ((size_t)(in ? sg + u : s1 - 1) * 4 + gl) * (NN_SB * 16) + slot;
            v1[u] = tr_b1[o];
            v2[u] = tr_b2[o];
            vt[u] = tr_t1[o];
            if (!in) { v1[u] = inf; v2[u] = inf; }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            sm = v1[u] < m ? m : fminf(sm, v1[u]);
            mt = v1[u] < m ? vt[u] : mt;
            m = fminf(m, v1[u]);
            m2 = fminf(m2, v2[u]);
        }
    }
    float mg = fminf(m, __shfl_xor(m, 1, 64)); mg = fminf(mg, __shfl_xor(mg, 2, 64));
    m2 = fminf(m2, __shfl_xor(m2, 1, 64)); m2 = fminf(m2, __shfl_xor(m2, 2, 64));
    const bool maybe = mg + Si <= r2f + 4.0f * e + 4.8e-7f * Si;  // else certainly farther than r
    const float win = mg + 2.0f * e;
    double bd = __longlong_as_double(0x7FF0000000000000ll);
    int bj = 0x7FFFFFFF;
    auto rescore = [&](int unit) {
        const int64_t row0 = (int64_t)unit * (16 * QT) + 4 * gl;  // lane group gl: rows 4gl..4gl+3 of each tile
        for (int u = 0; u < QT; ++u) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t row = row0 + 16 * u + r;
                if (row < Nt) {
                    const int64_t j = tperm[row];
                    lexmin(bd, bj, dist2(px, py, pz, tgt[3 * j], tgt[3 * j + 1], tgt[3 * j + 2]), (int)j);
                }
            }
        }
    };
    if (live && maybe) {
        if (sm <= win) {  // rare: several of this thread's segments have a unit inside the window
            for (int sg = s0; sg < s1; ++sg) {
                const size_t o = ((size_t)sg * 4 + gl) * (NN_SB * 16) + slot;
                if (tr_b1[o] <= win) rescore(tr_t1[o]);
            }
        } else if (m <= win) {
            rescore(mt);
        }
    }
#pragma unroll
    for (int off = 1; off <= 2; off <<= 1) {
        const double od = __shfl_xor(bd, off, 64);
        const int oj = __shfl_xor(bj, off, 64);
        lexmin(bd, bj, od, oj);
    }
    if (live && gl == 0) {
        if (!maybe) {
            idx_out[i] = -1;
            d2_out[i] = __longlong_as_double(0x7FF0000000000000ll);
        } else {
            idx_out[i] = bj;
            d2_out[i] = bd;
            if (m2 <= win) fb_list[atomicAdd(&st->fb_count, 1)] = kk;  // ambiguous: exact search decides
        }
    }
}

// ---- 5. ambiguous slots: exact float64 search, one workgroup (FB_WAVES waves) per slot.
// Candidate tiles are the block's surviving tiles (mask) that also come within r of THIS point
// (lane-parallel sphere test per non-empty mask word); wave w takes the mask words w, w +
// FB_WAVES, ... so the chain of dependent loads per slot is n_words / FB_WAVES long; the waves'
// results meet in LDS.  Rows are scanned 64 at a time.
constexpr int FB_WAVES = 16;
template <int QT>
__global__ __launch_bounds__(FB_WAVES * 64) void nn_fallback_kernel(const IcpState *__restrict__ st,
                                                                   const int32_t *__restrict__ fb_list,
                                                                   const int32_t *__restrict__ list,
                                                                   const unsigned long long *__restrict__ mask, int n_words,
                                                                   const float4 *__restrict__ tile_sph, float r_search,
                                                                   const double *__restrict__ tgt,
                                                                   const int32_t *__restrict__ tperm, int64_t Nt,
                                                                   const double *__restrict__ P,
                                                                   int32_t *__restrict__ idx_out,
                                                                   double *__restrict__ d2_out) {
    if (st->done) return;
    __shared__ double red_d[FB_WAVES];
    __shared__ int red_j[FB_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = st->fb_count;
    const double cx = st->centroid[0], cy = st->centroid[1], cz = st->centroid[2];
    for (int w = blockIdx.x; w < n; w += gridDim.x) {
        const int kk = fb_list[w];
        const int i = list[kk];
        const unsigned long long *mw = mask + (size_t)(kk >> 7) * n_words;
        const double px = P[3 * (int64_t)i], py = P[3 * (int64_t)i + 1], pz = P[3 * (int64_t)i + 2];
        const float sx = (float)(px - cx), sy = (float)(py - cy), sz = (float)(pz - cz);
        const float slack = point_slack(sx, sy, sz);
        double bd = __longlong_as_double(0x7FF0000000000000ll);
        int bj = 0x7FFFFFFF;
        for (int wi = wave; wi < n_words; wi += FB_WAVES) {
            const unsigned long long word = mw[wi];  // wave-uniform
            if (word == 0ull) continue;
            bool keep = false;
            if ((word >> lane) & 1ull) {
                const float4 ts = tile_sph[wi * 64 + lane];
                const float dx = ts.x - sx, dy = ts.y - sy, dz = ts.z - sz;
                const float lim = r_search + ts.w + slack;
                keep = !offset_beyond(dx, dy, dz, lim);
            }
            unsigned long long near = __builtin_amdgcn_ballot_w64(keep);
            while (near != 0ull) {  // wave-uniform: 64 lanes = 64 rows = 64 / (16 QT) units per trip
                constexpr int UPT = 64 / (16 * QT);  // units per trip
                int unit = -1;
#pragma unroll
                for (int g = 0; g < UPT; ++g) {
                    if (near != 0ull) {
                        const int bit = __builtin_ctzll(near);
                        near &= near - 1ull;
                        if (g == lane / (16 * QT)) unit = wi * 64 + bit;
                    }
                }
                const int64_t row = (int64_t)unit * (16 * QT) + (lane % (16 * QT));
                if (unit >= 0 && row < Nt) {
                    const int64_t j = tperm[row];
                    lexmin(bd, bj, dist2(px, py, pz, tgt[3 * j], tgt[3 * j + 1], tgt[3 * j + 2]), (int)j);
                }
            }
        }
#pragma unroll
        for (int off = 1; off <= 32; off <<= 1) {
            double od = __shfl_xor(bd, off, 64);
            int oj = __shfl_xor(bj, off, 64);
            lexmin(bd, bj, od, oj);
        }
        if (lane == 0) { red_d[wave] = bd; red_j[wave] = bj; }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int q = 1; q < FB_WAVES; ++q) lexmin(bd, bj, red_d[q], red_j[q]);
            idx_out[i] = bj;
            d2_out[i] = bd;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------ accumulate

// Packet layout.  point-to-plane: [0..20] upper triangle of J J^T (row-major), [21..26] J r,
// [27] sum d^2, [28] count.  point-to-point: [0..2] sum (s-c), [3..5] sum (t-c),
// [6..14] sum (t-c)(s-c)^T, [27], [28] as above.
__global__ __launch_bounds__(ACC_THREADS) void icp_accumulate_kernel(
    const IcpState *__restrict__ st, int estimator, const double *__restrict__ P, int64_t Ns,
    const double *__restrict__ tgt, const double *__restrict__ nrm, int32_t *__restrict__ idx,
    const double *__restrict__ d2, double r2, double *__restrict__ partials /* ACC_BLOCKS x PACKET */) {
    if (st->done) return;
    double acc[PACKET];
#pragma unroll
    for (int k = 0; k < PACKET; ++k) acc[k] = 0.0;
    const double cx = st->centroid[0], cy = st->centroid[1], cz = st->centroid[2];
    for (int64_t i = (int64_t)blockIdx.x * ACC_THREADS + threadIdx.x; i < Ns; i += (int64_t)ACC_BLOCKS * ACC_THREADS) {
        int j = idx[i];
        if (j < 0) continue;
        double dd = d2[i];
        if (!(dd < r2)) { idx[i] = -1; continue; }  // strict, as SearchHybrid's lower_bound
        double sx = P[3 * i], sy = P[3 * i + 1], sz = P[3 * i + 2];
        double tx = tgt[3 * (int64_t)j], ty = tgt[3 * (int64_t)j + 1], tz = tgt[3 * (int64_t)j + 2];
        if (estimator == PEDP_POINT_TO_PLANE) {
            double nx = nrm[3 * (int64_t)j], ny = nrm[3 * (int64_t)j + 1], nz = nrm[3 * (int64_t)j + 2];
            double r = (sx - tx) * nx + (sy - ty) * ny + (sz - tz) * nz;
            double J[6] = {sy * nz - sz * ny, sz * nx - sx * nz, sx * ny - sy * nx, nx, ny, nz};
            int k = 0;
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int c = a; c < 6; ++c) acc[k++] += J[a] * J[c];
#pragma unroll
            for (int a = 0; a < 6; ++a) acc[21 + a] += J[a] * r;
        } else {
            double s[3] = {sx - cx, sy - cy, sz - cz}, t[3] = {tx - cx, ty - cy, tz - cz};
#pragma unroll
            for (int a = 0; a < 3; ++a) { acc[a] += s[a]; acc[3 + a] += t[a]; }
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[6 + 3 * a + c] += t[a] * s[c];
        }
        acc[27] += dd;
        acc[28] += 1.0;
    }
    __shared__ double sh[ACC_THREADS / 64][PACKET];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < PACKET; ++k) {
        double v = wave_sum(acc[k]);
        if (lane == 0) sh[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < PACKET) {
        double v = 0.0;
        for (int w = 0; w < ACC_THREADS / 64; ++w) v += sh[w][threadIdx.x];
        partials[(size_t)blockIdx.x * PACKET + threadIdx.x] = v;
    }
}

__global__ void icp_reduce_kernel(const IcpState *__restrict__ st, const double *__restrict__ partials,
                                  double *__restrict__ packet) {
    if (st->done) return;
    if (threadIdx.x < PACKET) {
        double v = 0.0;
        for (int b = 0; b < ACC_BLOCKS; ++b) v += partials[(size_t)b * PACKET + threadIdx.x];
        packet[threadIdx.x] = v;
    }
}

}  // namespace
