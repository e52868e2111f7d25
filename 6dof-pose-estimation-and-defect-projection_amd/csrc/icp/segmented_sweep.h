// ICP, segmented path (dense sweeps, large radii), first half: transform + pack, sphere culling, the
// segment table and the two MFMA sweeps (f32 and bf16 operands).
#pragma once
#include "common.h"
#include "slot_math.h"

namespace {

// ------------------------------------------------------------------ transform + pack
// mode 0: P <- T * src (first pass; T = init), mode 1: P <- upd * P.
// A wave takes 128 consecutive points of the scene's spatial order (two per lane).  Points
// farther than r from the target's bounding box (lo, hi) have no neighbour within r
// (d_nn >= d_box) and are written off as "no correspondence" here.  If any point of the wave
// survives, the wave claims one 128-slot scene block (atomic counter), compacts its survivors
// into it, pads the rest with dummies (list = -1) and stores the block's bounding sphere --
// so every scene block of the sweep is one compact patch of space.
struct PackPoint {
    bool cand;
    int i;
    float sx, sy, sz;
};
__device__ __forceinline__ PackPoint pack_one(const IcpState *__restrict__ st, int mode, const double *__restrict__ src,
                                              double *__restrict__ P, const int32_t *__restrict__ perm, int64_t k,
                                              int64_t N, int32_t *__restrict__ idx_out, double *__restrict__ d2_out,
                                              double r2cut, double lox, double loy, double loz, double hix, double hiy,
                                              double hiz) {
    PackPoint o;
    o.cand = false; o.i = -1; o.sx = o.sy = o.sz = 0.f;
    if (k >= N) return o;
    const int64_t i = perm[k];
    const double *M = mode == 0 ? st->T : st->upd;
    const double *in = mode == 0 ? src : P;
    double x = in[3 * i], y = in[3 * i + 1], z = in[3 * i + 2];
    double nx = dadd(dadd(dadd(dmul(M[0], x), dmul(M[1], y)), dmul(M[2], z)), M[3]);
    double ny = dadd(dadd(dadd(dmul(M[4], x), dmul(M[5], y)), dmul(M[6], z)), M[7]);
    double nz = dadd(dadd(dadd(dmul(M[8], x), dmul(M[9], y)), dmul(M[10], z)), M[11]);
    P[3 * i] = nx; P[3 * i + 1] = ny; P[3 * i + 2] = nz;
    double ex = fmax(fmax(lox - nx, nx - hix), 0.0), ey = fmax(fmax(loy - ny, ny - hiy), 0.0),
           ez = fmax(fmax(loz - nz, nz - hiz), 0.0);  // (box_dist2 of slot_math.h)
    o.cand = (ex * ex + ey * ey + ez * ez) <= r2cut;  // r2cut = r^2 (1 + 1e-12): rounding-safe
    o.i = (int)i;
    o.sx = (float)(nx - st->centroid[0]); o.sy = (float)(ny - st->centroid[1]); o.sz = (float)(nz - st->centroid[2]);
    if (!o.cand) {
        idx_out[i] = -1;
        d2_out[i] = __longlong_as_double(0x7FF0000000000000ll);
    }
    return o;
}
__device__ __forceinline__ void pack_store(const PackPoint &p, int slot, float4 *__restrict__ B, float *__restrict__ eps,
                                           float *__restrict__ S, int32_t *__restrict__ list, float Tn, float T2, float r1,
                                           float mi_factor) {
    B[slot] = make_float4(-2.0f * p.sx, -2.0f * p.sy, -2.0f * p.sz, 1.0f);
    // Error bound of the fp32 surrogate relative to the float64 distance, for points whose
    // nearest neighbour is closer than r1 (see DESIGN.md "NN filter bound"):
    //   eps = 2^-23 * (5 * (2*|s'|_1*Tn + T2) + 2*min(r1, |s'|_1 + Tn)*(Tn + |s'|_1))
    float s1 = fabsf(p.sx) + fabsf(p.sy) + fabsf(p.sz);
    float Mi = 2.0f * s1 * Tn + T2;
    // (mi_factor: 5 for the fp32 MFMA's four rounded products and three sums; 34 for the bf16 form's thirty exact products
    // and up to thirty-one fp32 additions inside the matrix pipe, each charged a full ulp of the largest partial sum)
    eps[slot] = 1.1920929e-7f * (mi_factor * Mi + 2.0f * fminf(r1, s1 + Tn) * (Tn + s1)) * 1.0001f;
    S[slot] = p.sx * p.sx + p.sy * p.sy + p.sz * p.sz;
    list[slot] = p.i;
}
__global__ __launch_bounds__(256) void icp_transform_pack_kernel(
    IcpState *__restrict__ st, int mode, const double *__restrict__ src, double *__restrict__ P,
    const int32_t *__restrict__ perm, int64_t N, float4 *__restrict__ B, float *__restrict__ eps, float *__restrict__ S,
    int32_t *__restrict__ list, float4 *__restrict__ blk_sph, int32_t *__restrict__ idx_out,
    double *__restrict__ d2_out, float Tn, float T2, float r1, double r2cut, double lox, double loy, double loz,
    double hix, double hiy, double hiz, float mi_factor) {
    if (st->done) return;
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t k0 = wave * 128 + lane;
    const PackPoint p0 = pack_one(st, mode, src, P, perm, k0, N, idx_out, d2_out, r2cut, lox, loy, loz, hix, hiy, hiz);
    const PackPoint p1 = pack_one(st, mode, src, P, perm, k0 + 64, N, idx_out, d2_out, r2cut, lox, loy, loz, hix, hiy, hiz);
    const unsigned long long m0 = __builtin_amdgcn_ballot_w64(p0.cand), m1 = __builtin_amdgcn_ballot_w64(p1.cand);
    const int c0 = __builtin_popcountll(m0), cnt = c0 + __builtin_popcountll(m1);
    if (cnt == 0) return;  // wave-uniform
    int blk = 0;
    if (lane == 0) blk = atomicAdd(&st->n_blocks, 1);
    blk = __builtin_amdgcn_readfirstlane(blk);
    const unsigned long long lt = (1ull << lane) - 1ull;
    const int base = blk * 128;
    if (p0.cand) pack_store(p0, base + __builtin_popcountll(m0 & lt), B, eps, S, list, Tn, T2, r1, mi_factor);
    if (p1.cand) pack_store(p1, base + c0 + __builtin_popcountll(m1 & lt), B, eps, S, list, Tn, T2, r1, mi_factor);
    for (int s = cnt + lane; s < 128; s += 64) {  // dummies: never inliers, never selected
        B[base + s] = make_float4(0.f, 0.f, 0.f, 1.f);
        eps[base + s] = 0.f;
        S[base + s] = 3e38f;
        list[base + s] = -1;
    }
    // Bounding spheres of the block's eight 16-slot sub-blocks (centred fp32 coordinates).
    // Consecutive NON-EMPTY cells of the space-filling curve can be far apart (the curve
    // leaves a surface and re-enters it elsewhere), so one sphere per 128 slots can be huge;
    // per sub-block the sweep keeps a target tile only if it is near SOME sub-block.
    __shared__ float stage[4][3][128];
    float (*sg)[128] = stage[threadIdx.x >> 6];
    if (p0.cand) { const int sl = __builtin_popcountll(m0 & lt); sg[0][sl] = p0.sx; sg[1][sl] = p0.sy; sg[2][sl] = p0.sz; }
    if (p1.cand) { const int sl = c0 + __builtin_popcountll(m1 & lt); sg[0][sl] = p1.sx; sg[1][sl] = p1.sy; sg[2][sl] = p1.sz; }
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): this wave's LDS writes have landed
    const float big = 3e38f;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int sl = half * 64 + lane;
        const bool real = sl < cnt;
        const float x = real ? sg[0][sl] : 0.f, y = real ? sg[1][sl] : 0.f, z = real ? sg[2][sl] : 0.f;
        float lx = real ? x : big, hx = real ? x : -big, ly = real ? y : big, hy = real ? y : -big, lz = real ? z : big,
              hz = real ? z : -big;
#pragma unroll
        for (int off = 1; off <= 8; off <<= 1) {
            lx = fminf(lx, __shfl_xor(lx, off, 64)); hx = fmaxf(hx, __shfl_xor(hx, off, 64));
            ly = fminf(ly, __shfl_xor(ly, off, 64)); hy = fmaxf(hy, __shfl_xor(hy, off, 64));
            lz = fminf(lz, __shfl_xor(lz, off, 64)); hz = fmaxf(hz, __shfl_xor(hz, off, 64));
        }
        if ((lane & 15) == 0) {
            float4 sp = make_float4(0.f, 0.f, 0.f, -1.f);  // empty sub-block: matches nothing
            if (hx >= lx) {
                const float cx = 0.5f * (lx + hx), cy = 0.5f * (ly + hy), cz = 0.5f * (lz + hz);
                const float ex = hx - cx, ey = hy - cy, ez = hz - cz;
                sp = make_float4(cx, cy, cz, sqrtf(ex * ex + ey * ey + ez * ez) * 1.0001f +
                                                 1e-6f * (fabsf(cx) + fabsf(cy) + fabsf(cz)) + 1e-30f);
            }
            blk_sph[(size_t)blk * NN_SB + (sl >> 4)] = sp;
        }
    }
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// ------------------------------------------------------------------ NN sweep (MFMA)
__device__ __forceinline__ void lexmin(double &d, int &j, double od, int oj) {
    if (od < d || (od == d && oj < j)) { d = od; j = oj; }
}

// ---- 1. cull: which target tiles can matter for which scene block (bit mask per block) ----
// Tile t survives for a block iff for some 16-slot sub-block |c_sub - c_tile| <= r + rad_sub +
// rad_tile (bounding spheres, margins included).  A skipped tile has all its points farther
// than r from all points of the block, so it cannot contain the nearest neighbour of an
// INLIER; for a point without any neighbour within r the answer is "no correspondence"
// whichever tiles were visited.  One wave per (block, CULL_WORDS x 64 tiles): lane l tests tile
// base + l, the ballot IS the mask word.  With r = infinity (pedp_nn) every bit is set: the
// dense all-pairs sweep.
__global__ __launch_bounds__(256) void nn_cull_kernel(const IcpState *__restrict__ st, const float4 *__restrict__ tile_sph,
                                                      int n_tiles, int n_words, const float4 *__restrict__ blk_sph,
                                                      float r_search, unsigned long long *__restrict__ mask,
                                                      int32_t *__restrict__ blk_cnt) {
    if (st->done) return;
    const int lane = threadIdx.x & 63;
    const int wg = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int groups = (n_words + CULL_WORDS - 1) / CULL_WORDS;
    const int blk = wg / groups, grp = wg - blk * groups;
    if (blk >= st->n_blocks) return;  // wave-uniform
    float4 bs[NN_SB];
#pragma unroll
    for (int sb = 0; sb < NN_SB; ++sb) bs[sb] = blk_sph[(size_t)blk * NN_SB + sb];
    int w1 = (grp + 1) * CULL_WORDS;
    if (w1 > n_words) w1 = n_words;
    int cnt = 0;
    for (int wi = grp * CULL_WORDS; wi < w1; ++wi) {
        const int t = wi * 64 + lane;
        const float4 ts = tile_sph[t < n_tiles ? t : 0];
        bool keep = false;
#pragma unroll
        for (int sb = 0; sb < NN_SB; ++sb) {
            const float dx = ts.x - bs[sb].x, dy = ts.y - bs[sb].y, dz = ts.z - bs[sb].z;
            const float lim = r_search + bs[sb].w + ts.w;
            keep |= (bs[sb].w >= 0.f) & !offset_beyond(dx, dy, dz, lim);
        }
        keep = keep && (t < n_tiles) && (ts.w >= 0.f);
        const unsigned long long m = __builtin_amdgcn_ballot_w64(keep);
        if (lane == 0) mask[(size_t)blk * n_words + wi] = m;
        cnt += __builtin_popcountll(m);
    }
    if (lane == 0 && cnt > 0) atomicAdd(&blk_cnt[blk], cnt);
}

// ---- 2. segments: cut every block's survivor list into pieces of seg_len tiles ----
// One workgroup.  seg_len is chosen so that all pieces fit the segment table (max_segs) and
// is at least SEG_MIN: heavy blocks simply get more pieces, so every sweep wave has the same
// amount of work whatever the spatial distribution.
__global__ __launch_bounds__(1024) void nn_segment_kernel(IcpState *__restrict__ st, int32_t *__restrict__ blk_cnt,
                                                          int32_t *__restrict__ blk_segstart, int32_t *__restrict__ seg_blk,
                                                          int32_t *__restrict__ seg_rank0, int32_t *__restrict__ seg_n,
                                                          int max_segs, int SEG_MIN, int NN_LIST) {
    if (st->done) return;
    __shared__ long long red[16];
    __shared__ int scan[1024];
    __shared__ long long total_s;
    const int nb = st->n_blocks, tid = threadIdx.x;
    const int per = (nb + 1023) / 1024;
    const int b0 = tid * per, b1 = (b0 + per < nb) ? b0 + per : nb;
    long long loc = 0;
    for (int b = b0; b < b1; ++b) loc += blk_cnt[b];
    long long v = loc;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) {
        long long t = 0;
        for (int k = 0; k < 16; ++k) t += red[k];
        total_s = t;
    }
    __syncthreads();
    const long long total = total_s;
    long long room = (long long)max_segs - nb;
    if (room < 1) room = 1;
    long long sl = (total + room - 1) / room;
    if (sl < SEG_MIN) sl = SEG_MIN;
    sl = (sl + NN_TU - 1) / NN_TU * NN_TU;
    if (sl > NN_LIST) sl = NN_LIST;  // cannot happen: the host sizes max_segs for the dense case
    const int seg_len = (int)sl;
    int mine = 0;
    for (int b = b0; b < b1; ++b) mine += (blk_cnt[b] + seg_len - 1) / seg_len;
    scan[tid] = mine;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int t = tid >= off ? scan[tid - off] : 0;
        __syncthreads();
        scan[tid] += t;
        __syncthreads();
    }
    int at = scan[tid] - mine;
    for (int b = b0; b < b1; ++b) {
        const int c = blk_cnt[b];
        blk_cnt[b] = 0;  // ready for the next pass
        blk_segstart[b] = at;
        // the block's pieces are made equally long (a 782-unit list is cut 392 + 390, not 424 + 358)
        const int pieces = (c + seg_len - 1) / seg_len;
        const int piece = pieces > 0 ? ((c + pieces - 1) / pieces + NN_TU - 1) / NN_TU * NN_TU : seg_len;
        for (int r0 = 0, k = 0; k < pieces; r0 += piece, ++k) {
            if (at < max_segs) { seg_blk[at] = b; seg_rank0[at] = r0; seg_n[at] = (c - r0 < piece) ? c - r0 : piece; }
            ++at;
        }
    }
    if (tid == 1023) {
        blk_segstart[nb] = scan[1023];
        st->n_segs = scan[1023] < max_segs ? scan[1023] : max_segs;
        st->seg_len = seg_len;
        st->sum_tiles += total;
    }
}

// ---- 3. sweep ----
// Ranks [r0, r0 + n_s) of a block's surviving-unit mask, expanded into an LDS list by one wave
// (prefix popcount over the mask words), followed by 2 G pad units (rows that can never win: the
// last group is filled up with them and the prefetch of the trip after it reads them).
template <int G>
__device__ __forceinline__ void expand_ranks(const unsigned long long *__restrict__ mw, int n_words, int r0, int n_s,
                                             unsigned pad_unit, unsigned *__restrict__ mine, int lane) {
    int running = 0;
    for (int wg = 0; wg < n_words && running < r0 + n_s; wg += 64) {
        unsigned long long word = (wg + lane < n_words) ? mw[wg + lane] : 0ull;
        const int pc = __builtin_popcountll(word);
        int incl = pc;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_up(incl, off, 64);
            if (lane >= off) incl += o;
        }
        int rank = running + incl - pc;
        if (pc > 0 && rank < r0 + n_s && rank + pc > r0) {
            const unsigned tile0 = (unsigned)(wg + lane) * 64u;
            while (word != 0ull) {
                const int bit = __builtin_ctzll(word);
                word &= word - 1ull;
                if (rank >= r0 && rank < r0 + n_s) mine[rank - r0] = tile0 + (unsigned)bit;
                ++rank;
            }
        }
        running += __shfl(incl, 63, 64);
    }
    if (lane < 2 * G) mine[n_s + lane] = pad_unit;
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): the wave's own LDS writes have landed
}

// The MFMA loop of one wave over the n_s units of its LDS list: keeps, per lane and scene
// sub-block, the best unit value b1, its unit t1 and the second-best unit value b2 (running
// across calls).  Per unit (QT MFMA tiles = 16 QT target rows) the values a lane sees are folded
// with two v_min3 per MFMA, and only once per unit the running triple is updated.  The matrix
// pipe works on the next tile while the VALU folds this one (software pipeline), and the A
// operands of a whole group of G units are fetched one group ahead: G QT x NN_SB MFMAs cover the
// load latency.
template <int QT, int G>
__device__ __forceinline__ void sweep_list(const unsigned *__restrict__ mine, int n_s,
                                           const float *__restrict__ tgtf, int frag, const float (&b)[NN_SB],
                                           float (&b1)[NN_SB], int (&t1)[NN_SB], float (&b2)[NN_SB]) {
    if (n_s <= 0) return;
    constexpr int U = G * QT;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    float vq[NN_SB];
#pragma unroll
    for (int sb = 0; sb < NN_SB; ++sb) vq[sb] = __uint_as_float(0x7F800000u);
    float a[U];
    unsigned units[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        units[g] = mine[g];
#pragma unroll
        for (int u = 0; u < QT; ++u) a[g * QT + u] = tgtf[((size_t)units[g] * QT + u) * 64 + frag];
    }
    f32x4 acc[NN_SB];
#pragma unroll
    for (int sb = 0; sb < NN_SB; ++sb) acc[sb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], b[sb], zero, 0, 0, 0);
    for (int k = 0; k < n_s; k += G) {
        float an[U];
        unsigned units_n[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            units_n[g] = mine[k + G + g];  // pad units follow the last real one
#pragma unroll
            for (int u = 0; u < QT; ++u) an[g * QT + u] = tgtf[((size_t)units_n[g] * QT + u) * 64 + frag];
        }
#pragma unroll
        for (int t = 0; t < U; ++t) {
            const int u = t % QT;
            const unsigned unit = units[t / QT];
            const float a_next = (t + 1 < U) ? a[t + 1] : an[0];
#pragma unroll
            for (int sb = 0; sb < NN_SB; ++sb) {
                f32x4 nxt = __builtin_amdgcn_mfma_f32_16x16x4f32(a_next, b[sb], zero, 0, 0, 0);
                const f32x4 cur = acc[sb];
#if PEDP_NN_EXPERIMENT == 1   /* MFMA only (wrong results): pure matrix-pipe rate of this loop shape */
                b1[sb] = fminf(b1[sb], cur[0]);
                acc[sb] = nxt;
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x002, 1, 0);
#else
                // two v_min3 per MFMA (linear nesting is what the compiler turns into v_min3)
                if (u == 0) vq[sb] = fminf(fminf(fminf(cur[0], cur[1]), cur[2]), cur[3]);
                else vq[sb] = fminf(fminf(fminf(fminf(vq[sb], cur[0]), cur[1]), cur[2]), cur[3]);
                if (u == QT - 1) {
                    const float v = vq[sb];
                    t1[sb] = v < b1[sb] ? (int)unit : t1[sb];
                    b2[sb] = __builtin_amdgcn_fmed3f(b1[sb], b2[sb], v);  // b1 <= b2: new second best
                    b1[sb] = fminf(b1[sb], v);
                }
                acc[sb] = nxt;
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                    // 1 MFMA
                if (u == QT - 1) __builtin_amdgcn_sched_group_barrier(0x002, 6, 0);   // then its VALU ops
                else __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
#endif
            }
        }
#pragma unroll
        for (int t = 0; t < U; ++t) a[t] = an[t];
#pragma unroll
        for (int g = 0; g < G; ++g) units[g] = units_n[g];
    }
}

// One wave per segment.
// Triples of segment s: tr_b1 / tr_t1 / tr_b2 [(s * 4 + q) * 128 + slot in block]
template <int QT, int G>
__global__ __launch_bounds__(NN_WAVES * 64) void nn_sweep_kernel(
    const IcpState *__restrict__ st, const float *__restrict__ tgtf /* (n_tiles + pad) x 64, sorted */, int n_tiles,
    int n_words, const unsigned long long *__restrict__ mask, const int32_t *__restrict__ seg_blk,
    const int32_t *__restrict__ seg_rank0, const int32_t *__restrict__ seg_n, const float *__restrict__ srcf /* slots x 4 */,
    float *__restrict__ tr_b1, int32_t *__restrict__ tr_t1, float *__restrict__ tr_b2) {
    __shared__ unsigned surv[NN_WAVES][NN_LIST_TILES / QT + 2 * G];
    if (st->done) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int seg = blockIdx.x * NN_WAVES + wv;
    if (seg >= st->n_segs) return;  // wave-uniform
    const int blk = seg_blk[seg], r0 = seg_rank0[seg], n_s = seg_n[seg];
    const int64_t base = (int64_t)blk * (NN_SB * 16);
    const int frag = (lane & 15) * 4 + (lane >> 4);  // float offset inside a 16-point tile
    unsigned *mine = surv[wv];
    expand_ranks<G>(mask + (size_t)blk * n_words, n_words, r0, n_s, (unsigned)n_tiles, mine, lane);

    float b[NN_SB];
#pragma unroll
    for (int sb = 0; sb < NN_SB; ++sb) b[sb] = srcf[(base + sb * 16) * 4 + frag];
    float b1[NN_SB], b2[NN_SB];
    int t1[NN_SB];
#pragma unroll
    for (int sb = 0; sb < NN_SB; ++sb) { b1[sb] = __uint_as_float(0x7F800000u); b2[sb] = b1[sb]; t1[sb] = n_tiles; }
    sweep_list<QT, G>(mine, n_s, tgtf, frag, b, b1, t1, b2);
    const int q = lane >> 4, j = lane & 15;
#pragma unroll
    for (int sb = 0; sb < NN_SB; ++sb) {
        const size_t o = ((size_t)seg * 4 + q) * (NN_SB * 16) + (size_t)(sb * 16 + j);
        tr_b1[o] = b1[sb];
        tr_t1[o] = t1[sb];
        tr_b2[o] = b2[sb];
    }
}

// ---- 3b. the dense sweep on the bf16 matrix pipe (units of QT = 4 tiles: pedp_nn, large radii, the exhaustive
// configuration).  g(i, j) = |t'_j|^2 - 2 s'_i . t'_j is one K = 32 contraction of v_mfma_f32_16x16x32_bf16 over EXACT
// three-way bf16 pieces (truncation splits: 3 x 8 bits carry an fp32 mantissa): slot k = 9 c + 3 i + j holds piece i of the
// model's t'_c against piece j of the scene's -2 s'_c (27 slots), slots 27..29 the pieces of |t'|^2 against 1, slots 30,
// 31 zero.  Every product is exact; what is left of the error is the pipe's fp32 accumulation of thirty terms, which
// the slot's bound eps charges at a full ulp of the largest partial sum per addition (mi_factor 34 instead of the fp32
// form's 5): g is still a FILTER, winners are re-scored in float64 exactly as before.  16 cycles per MFMA instead of the
// f32-input form's 32, and vector instructions issue beside it (8 of the 16 cycles are free): the fold's three VALU
// operations per MFMA fit.  Same lanes, same triples, same selection and fallback kernels as nn_sweep_kernel.
typedef __bf16 bf8v __attribute__((ext_vector_type(8)));
union BfFrag { bf8v v; unsigned short h[8]; uint4 q; };
__device__ __forceinline__ void split3_bf16(float x, unsigned short (&out)[3]) {  // x = hi + mid + lo exactly (truncation)
    const float hi = __uint_as_float(__float_as_uint(x) & 0xFFFF0000u);
    const float r1 = __fsub_rn(x, hi);
    const float mid = __uint_as_float(__float_as_uint(r1) & 0xFFFF0000u);
    const float lo = __fsub_rn(r1, mid);   // eight significant bits at most: a bf16
    out[0] = (unsigned short)(__float_as_uint(hi) >> 16);
    out[1] = (unsigned short)(__float_as_uint(mid) >> 16);
    out[2] = (unsigned short)(__float_as_uint(lo) >> 16);
}
// A operand: per 16-row tile 64 lanes x 16 B, lane l = (row l & 15, k group l >> 4) holds its eight slots
__global__ void pack_target_bf16_kernel(const float4 *__restrict__ tgt4, int64_t n_rows, uint4 *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_rows * 4) return;
    const int64_t tile = t >> 6;
    const int lane = (int)(t & 63), row = lane & 15, q = lane >> 4;
    const float4 v = tgt4[tile * 16 + row];
    unsigned short pc[4][3];
    split3_bf16(v.x, pc[0]); split3_bf16(v.y, pc[1]); split3_bf16(v.z, pc[2]); split3_bf16(v.w, pc[3]);
    BfFrag f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int k = 8 * q + e;
        f.h[e] = k < 27 ? pc[k / 9][(k % 9) / 3] : (k < 30 ? pc[3][k - 27] : (unsigned short)0);
    }
    out[t] = f.q;
}
#if PEDP_NN_EXPERIMENT == 2   /* timing experiment (wrong results): every wave reads the same unit -- the operand out of L1 */
#define PEDP_BF_UNIT(u) ((u) & 1u)
#else
#define PEDP_BF_UNIT(u) (u)
#endif
template <int QT, int G>
__device__ __forceinline__ void sweep_list_bf16(const unsigned *__restrict__ mine, int n_s, const uint4 *__restrict__ tgtb, int lane,
                                                const bf8v (&b)[NN_SB], float (&b1)[NN_SB], int (&t1)[NN_SB], float (&b2)[NN_SB]) {
    if (n_s <= 0) return;
    constexpr int U = G * QT;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    float vq[NN_SB];
#pragma unroll
    for (int sb = 0; sb < NN_SB; ++sb) vq[sb] = __uint_as_float(0x7F800000u);
    BfFrag a[U];
    unsigned units[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        units[g] = mine[g];
#pragma unroll
        for (int u = 0; u < QT; ++u) a[g * QT + u].q = tgtb[((size_t)PEDP_BF_UNIT(units[g]) * QT + u) * 64 + lane];
    }
    f32x4 acc[NN_SB];
#pragma unroll
    for (int sb = 0; sb < NN_SB; ++sb) acc[sb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0].v, b[sb], zero, 0, 0, 0);
    for (int k = 0; k < n_s; k += G) {
        BfFrag an[U];
        unsigned units_n[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            units_n[g] = mine[k + G + g];  // pad units follow the last real one
#pragma unroll
            for (int u = 0; u < QT; ++u) an[g * QT + u].q = tgtb[((size_t)PEDP_BF_UNIT(units_n[g]) * QT + u) * 64 + lane];
        }
#pragma unroll
        for (int t = 0; t < U; ++t) {
            const int u = t % QT;
            const unsigned unit = units[t / QT];
            const bf8v a_next = (t + 1 < U) ? a[t + 1].v : an[0].v;
#pragma unroll
            for (int sb = 0; sb < NN_SB; ++sb) {
                f32x4 nxt = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_next, b[sb], zero, 0, 0, 0);
                const f32x4 cur = acc[sb];
                if (u == 0) vq[sb] = fminf(fminf(fminf(cur[0], cur[1]), cur[2]), cur[3]);
                else vq[sb] = fminf(fminf(fminf(fminf(vq[sb], cur[0]), cur[1]), cur[2]), cur[3]);
                if (u == QT - 1) {
                    const float v = vq[sb];
                    t1[sb] = v < b1[sb] ? (int)unit : t1[sb];
                    b2[sb] = __builtin_amdgcn_fmed3f(b1[sb], b2[sb], v);
                    b1[sb] = fminf(b1[sb], v);
                }
                acc[sb] = nxt;
#if PEDP_NN_EXPERIMENT != 3
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                    // 1 MFMA
                if (u == QT - 1) __builtin_amdgcn_sched_group_barrier(0x002, 6, 0);   // then its VALU ops
                else __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
#endif
            }
        }
#pragma unroll
        for (int t = 0; t < U; ++t) a[t] = an[t];
#pragma unroll
        for (int g = 0; g < G; ++g) units[g] = units_n[g];
    }
}
// One wave per segment, like nn_sweep_kernel.  (Measured and not kept: the four waves of a workgroup taking the same piece
// of four consecutive blocks and sharing its A operands through LDS, double-buffered, one barrier per 64 MFMAs of every
// wave -- a quarter of the L2 traffic, 9.2 -> 2.3 GB per sweep, but 1.06-1.22 ms against this kernel's 0.84: the barrier,
// the exposed LDS read at the head of every group and the lost cross-group pipelining cost more than the L2 gave back.)
template <int QT, int G>
__global__ __launch_bounds__(NN_WAVES * 64) void nn_sweep_bf16_kernel(
    const IcpState *__restrict__ st, const uint4 *__restrict__ tgtb /* (n_tiles + pad) x 64 lanes x 16 B */, int n_tiles,
    int n_words, const unsigned long long *__restrict__ mask, const int32_t *__restrict__ seg_blk,
    const int32_t *__restrict__ seg_rank0, const int32_t *__restrict__ seg_n, const float4 *__restrict__ src4 /* slots */,
    float *__restrict__ tr_b1, int32_t *__restrict__ tr_t1, float *__restrict__ tr_b2) {
    __shared__ unsigned surv[NN_WAVES][NN_LIST_TILES / QT + 2 * G];
    if (st->done) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int seg = blockIdx.x * NN_WAVES + wv;
    if (seg >= st->n_segs) return;  // wave-uniform
    const int blk = seg_blk[seg], r0 = seg_rank0[seg], n_s = seg_n[seg];
    const int64_t base = (int64_t)blk * (NN_SB * 16);
    unsigned *mine = surv[wv];
    expand_ranks<G>(mask + (size_t)blk * n_words, n_words, r0, n_s, (unsigned)n_tiles, mine, lane);
    const int q = lane >> 4, j = lane & 15;
    bf8v b[NN_SB];
#pragma unroll
    for (int sb = 0; sb < NN_SB; ++sb) {   // the B operand: pieces of the slot's (-2 x', -2 y', -2 z'), ones for |t'|^2's slots
        const float4 sv = src4[base + sb * 16 + j];
        unsigned short ps[3][3];
        split3_bf16(sv.x, ps[0]); split3_bf16(sv.y, ps[1]); split3_bf16(sv.z, ps[2]);
        BfFrag f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = 8 * q + e;
            f.h[e] = k < 27 ? ps[k / 9][k % 3] : (k < 30 ? (unsigned short)0x3F80 : (unsigned short)0);
        }
        b[sb] = f.v;
    }
    float b1[NN_SB], b2[NN_SB];
    int t1[NN_SB];
#pragma unroll
    for (int sb = 0; sb < NN_SB; ++sb) { b1[sb] = __uint_as_float(0x7F800000u); b2[sb] = b1[sb]; t1[sb] = n_tiles; }
    sweep_list_bf16<QT, G>(mine, n_s, tgtb, lane, b, b1, t1, b2);
#pragma unroll
    for (int sb = 0; sb < NN_SB; ++sb) {
        const size_t o = ((size_t)seg * 4 + q) * (NN_SB * 16) + (size_t)(sb * 16 + j);
        tr_b1[o] = b1[sb];
        tr_t1[o] = t1[sb];
        tr_b2[o] = b2[sb];
    }
}

// Diagnostics (tests/test_icp_gpu.py measures the bf16 form's error against float64): g of every (scene row, model row)
// pair as the sweep's MFMA produces it -- one wave per (16 scene rows, 16 model rows), the same operand packing
__global__ __launch_bounds__(64) void nn_bf16_debug_kernel(const uint4 *__restrict__ tgtb, const float4 *__restrict__ src4, int n_src16,
                                                           int n_tgt, float *__restrict__ g_out) {
    const int lane = threadIdx.x, q = lane >> 4, j = lane & 15;
    const int sb = blockIdx.x % n_src16, tile = blockIdx.x / n_src16;
    const float4 sv = src4[(size_t)sb * 16 + j];
    unsigned short ps[3][3];
    split3_bf16(sv.x, ps[0]); split3_bf16(sv.y, ps[1]); split3_bf16(sv.z, ps[2]);
    BfFrag f, a;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int k = 8 * q + e;
        f.h[e] = k < 27 ? ps[k / 9][k % 3] : (k < 30 ? (unsigned short)0x3F80 : (unsigned short)0);
    }
    a.q = tgtb[(size_t)tile * 64 + lane];
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const f32x4 r = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.v, f.v, zero, 0, 0, 0);
#pragma unroll
    for (int e = 0; e < 4; ++e) {   // D: column = scene slot j, row = model row 4 q + e of the tile
        const int row = tile * 16 + 4 * q + e;
        if (row < n_tgt) g_out[((size_t)sb * 16 + j) * n_tgt + row] = r[e];
    }
}

}  // namespace
