// ICP, compact row order of a target pack: a balanced k-d split of the target's finite rows into tiles.
//
// What a wave of a pass culls and sweeps follows the radius of the 16-row tiles (and of the 64- and 1024-row
// groups above them).  Any partition of the rows into groups of 16 gives the same results bit for bit -- the filter
// keeps every tile with a point within reach, the selection is exact and breaks ties by the original index -- so the
// partition is free to be the most compact one.  Runs of the Hilbert order are elongated on a surface; this order
// splits instead:
//
//   start: the rows in the cloud's Hilbert order (positions 0 .. m-1); one segment
//   while a segment has m > 16 rows:
//     axis  = the widest extent (hi - lo in float32) of the segment's centred float32 coordinates, ties to the lowest axis
//     sort the segment's rows by (coordinate on that axis, position so far), -0 counting as +0
//     the left part takes h = u * ceil(m / 2u) rows, u = 1024 if m > 1024, else 64 if m > 64, else 16
//
// so every 1024-, 64- and 16-row boundary is a segment boundary: mask words, the dense sweep's units and the tiles
// are subtrees.  Segments above 1024 rows start on multiples of 1024 and are split level by level with the context's
// pooled radix sort (key = first 1024-row block of the segment | order-preserving bits of the coordinate; the sort
// is stable, which is the tie rule).  From 1024 rows down one workgroup finishes a block in LDS by rank counting.
// Everything is a function of the cloud's data alone, stream-ordered, without read-back.
#pragma once
#include "common.h"

namespace {

constexpr int TORD_BLOCK = 1024;  // rows of a mask word: the top phase's unit, the leaf kernel's block

// the sizes the split takes, on the host too (the number of radix-sorted levels follows from the row count alone)
__host__ __device__ inline int tord_left(int m) {
    const int u = m > 1024 ? 1024 : m > 64 ? 64 : 16;
    return u * ((m + 2 * u - 1) / (2 * u));
}
inline int tord_top_levels(int64_t m) {
    int l = 0;
    while (m > TORD_BLOCK) { m = (int64_t)TORD_BLOCK * ((m + 2 * TORD_BLOCK - 1) / (2 * TORD_BLOCK)); ++l; }
    return l;
}

__device__ __forceinline__ unsigned tord_bits(float v) {
    unsigned b = __float_as_uint(v);
    if (b == 0x80000000u) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ int tord_axis(const float lo[3], const float hi[3]) {
    const float e0 = hi[0] - lo[0], e1 = hi[1] - lo[1], e2 = hi[2] - lo[2];
    int a = 0;
    float e = e0;
    if (e1 > e) { a = 1; e = e1; }
    if (e2 > e) a = 2;
    return a;
}

// every block starts in the one segment of all rows
__global__ void tord_init_kernel(int2 *__restrict__ blk_seg, int n_blocks, int nt) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < n_blocks) blk_seg[b] = make_int2(0, nt);
}

// min / max of six values over the 256 threads of a workgroup (result in every thread)
__device__ __forceinline__ void tord_reduce_box(float lo[3], float hi[3], float (*red)[256]) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int c = 0; c < 3; ++c) { red[c][tid] = lo[c]; red[3 + c][tid] = hi[c]; }
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                red[c][tid] = fminf(red[c][tid], red[c][tid + s]);
                red[3 + c][tid] = fmaxf(red[3 + c][tid], red[3 + c][tid + s]);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) { lo[c] = red[c][0]; hi[c] = red[3 + c][0]; }
    __syncthreads();
}

// A level of the top phase, first half: apply the last sort (cur_out[p] = cur_in[sigma[p]]; no sort yet: the identity)
// and take the box of every 1024-row block.  cur holds positions in the Hilbert pack t4.
__global__ __launch_bounds__(256) void tord_block_box_kernel(const float4 *__restrict__ t4, const int32_t *__restrict__ cur_in,
                                                             const int32_t *__restrict__ sigma, int32_t *__restrict__ cur_out,
                                                             int nt, float *__restrict__ blk_box) {
    __shared__ float red[6][256];
    const int b = blockIdx.x;
    float lo[3] = {3e38f, 3e38f, 3e38f}, hi[3] = {-3e38f, -3e38f, -3e38f};
    for (int r = threadIdx.x; r < TORD_BLOCK; r += 256) {
        const int p = b * TORD_BLOCK + r;
        if (p >= nt) break;
        const int j = sigma ? cur_in[sigma[p]] : p;
        cur_out[p] = j;
        const float4 v = t4[j];
        lo[0] = fminf(lo[0], v.x); hi[0] = fmaxf(hi[0], v.x);
        lo[1] = fminf(lo[1], v.y); hi[1] = fmaxf(hi[1], v.y);
        lo[2] = fminf(lo[2], v.z); hi[2] = fmaxf(hi[2], v.z);
    }
    tord_reduce_box(lo, hi, red);
    if (threadIdx.x < 3) {
        blk_box[6 * b + threadIdx.x] = lo[threadIdx.x];
        blk_box[6 * b + 3 + threadIdx.x] = hi[threadIdx.x];
    }
}

// Second half: the block's segment (all rows of a block share one while segments are above 1024 rows) gets its box
// from its blocks' boxes and its axis from the box; the rows get their keys; the block learns which half it falls in.
// A segment of 1024 rows or fewer is done here: its rows keep their places (equal keys, stable sort).
__global__ __launch_bounds__(256) void tord_key_kernel(const float4 *__restrict__ t4, const int32_t *__restrict__ cur, int nt,
                                                       const float *__restrict__ blk_box, int2 *__restrict__ blk_seg,
                                                       unsigned long long *__restrict__ key) {
    __shared__ float red[6][256];
    const int b = blockIdx.x;
    const int2 seg = blk_seg[b];  // (first row, rows)
    const unsigned long long top = (unsigned long long)(unsigned)(seg.x / TORD_BLOCK) << 32;
    int axis = -1;
    if (seg.y > TORD_BLOCK) {  // (uniform over the workgroup)
        float lo[3] = {3e38f, 3e38f, 3e38f}, hi[3] = {-3e38f, -3e38f, -3e38f};
        const int b0 = seg.x / TORD_BLOCK, b1 = (seg.x + seg.y + TORD_BLOCK - 1) / TORD_BLOCK;
        for (int q = b0 + threadIdx.x; q < b1; q += 256)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                lo[c] = fminf(lo[c], blk_box[6 * q + c]);
                hi[c] = fmaxf(hi[c], blk_box[6 * q + 3 + c]);
            }
        tord_reduce_box(lo, hi, red);
        axis = tord_axis(lo, hi);
    }
    for (int r = threadIdx.x; r < TORD_BLOCK; r += 256) {
        const int p = b * TORD_BLOCK + r;
        if (p >= nt) break;
        unsigned low = 0u;
        if (axis >= 0) {
            const float4 v = t4[cur[p]];
            low = tord_bits(axis == 0 ? v.x : axis == 1 ? v.y : v.z);
        }
        key[p] = top | low;
    }
    if (threadIdx.x == 0 && axis >= 0) {  // (no other workgroup reads this block's entry)
        const int h = tord_left(seg.y);
        blk_seg[b] = b * TORD_BLOCK - seg.x < h ? make_int2(seg.x, h) : make_int2(seg.x + h, seg.y - h);
    }
}

// The levels from 1024 rows down, one workgroup per block, in LDS.  A row counts the rows of its segment that come
// in front of it -- smaller coordinate, or the same and an earlier position -- and moves to that rank.
__global__ __launch_bounds__(256) void tord_leaf_kernel(const float4 *__restrict__ t4, const int32_t *__restrict__ cur_in,
                                                        const int32_t *__restrict__ sigma, const int32_t *__restrict__ perm, int nt,
                                                        int32_t *__restrict__ tile_perm) {
    __shared__ float xyz[2][3][TORD_BLOCK];
    __shared__ int32_t id[2][TORD_BLOCK];
    __shared__ unsigned short sstart[2][TORD_BLOCK], slen[2][TORD_BLOCK];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int m = nt - b * TORD_BLOCK < TORD_BLOCK ? nt - b * TORD_BLOCK : TORD_BLOCK;
    for (int r = tid; r < m; r += 256) {
        const int p = b * TORD_BLOCK + r;
        const int j = sigma ? cur_in[sigma[p]] : p;
        const float4 v = t4[j];
        xyz[0][0][r] = v.x; xyz[0][1][r] = v.y; xyz[0][2][r] = v.z;
        id[0][r] = j;
        sstart[0][r] = 0; slen[0][r] = (unsigned short)m;
    }
    __syncthreads();
    int g = 0;  // the side that holds the rows
    for (;;) {
        int any = 0;
        for (int r = tid; r < m; r += 256) {
            const int s = sstart[g][r], n = slen[g][r];
            int at = r, ns = s, nn = n;
            if (n > 16) {
                any = 1;
                float lo[3] = {3e38f, 3e38f, 3e38f}, hi[3] = {-3e38f, -3e38f, -3e38f};
                for (int q = s; q < s + n; ++q)
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const float v = xyz[g][c][q];
                        lo[c] = fminf(lo[c], v); hi[c] = fmaxf(hi[c], v);
                    }
                const float *ca = xyz[g][tord_axis(lo, hi)];
                const float mine = ca[r];
                int rank = 0;
                for (int q = s; q < s + n; ++q) {
                    const float v = ca[q];
                    rank += (v < mine || (v == mine && q < r)) ? 1 : 0;
                }
                const int h = tord_left(n);
                at = s + rank;
                if (rank < h) nn = h;
                else { ns = s + h; nn = n - h; }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) xyz[g ^ 1][c][at] = xyz[g][c][r];
            id[g ^ 1][at] = id[g][r];
            sstart[g ^ 1][at] = (unsigned short)ns; slen[g ^ 1][at] = (unsigned short)nn;
        }
        g ^= 1;
        if (!__syncthreads_or(any)) break;  // (the barrier between a level's writes and the next level's reads)
    }
    // after the last level nothing moved: both sides hold the final order
    for (int r = tid; r < m; r += 256) tile_perm[b * TORD_BLOCK + r] = perm[id[g][r]];
}

}  // namespace
