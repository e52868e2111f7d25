// Ray stage, variant 3: ray per lane WITH conservative culling when all rays share one origin -- still every
// triangle is accounted for, most of them by a bound instead of a test.  (The auto choice takes it for a ray count
// whose last grid cast had to be completed exhaustively; rays of differing origins fall through to the
// general-origin sweep of ray/sweep_packed.h on the device.)
// Triangles are taken in clusters of 16 consecutive records with a bounding sphere and every 64 clusters in a
// super-cluster sphere (mesh build, ray/mesh_records.h); per call every (super-)cluster gets its cone from the
// shared origin (unit axis v, cos/sin of the half-angle psi); rays are binned by direction (octahedral map,
// 256 x 256 cells in Hilbert-curve order, counting sort) so a packet of 64 consecutive rays covers one small solid
// angle, whose cone (axis a, half-angle theta) is reduced from the actual rays.  A ray of the packet can only hit a
// triangle of a cluster if angle(a, v) <= theta + psi, so clusters with v.a < cos(theta + psi) are dropped:
//   ray_cull_mask_kernel   one wave per packet, super-cluster cones first, then lane l tests
//                          cluster 64 w + l of every surviving word: the ballot IS the mask word
//   ray_segment_kernel     cuts every packet's survivor list into segments of equal length
//                          (device-side scan), so each sweep wave has the same work
//   ray_sweep_seg_kernel   one wave per segment: mask ranks -> LDS cluster list -> the loop body
//                          of the packed shared-origin sweep on those clusters
// Culling is conservative (margins below), so results stay bit-identical to the oracle.
#pragma once
#include "mt.h"
#include "mesh_records.h"
#include "sweep_packed.h"

namespace {

// ------------------------------------------------------------------ culled sweep (shared origin)
constexpr int CL_GROUPS = CL_TRIS / (2 * RPL_PAIRS);     // loop groups per cluster (4)
constexpr int BIN_BITS = 8;                              // 256 x 256 direction cells
constexpr int BIN_CELLS = 1 << (2 * BIN_BITS);

// per call: cone of each cluster seen from the shared origin.  rec[2c] = (vx, vy, vz, cos psi),
// rec[2c+1].x = sin psi.  cos psi = -2: the origin is inside the sphere (never cull);
// cos psi = 2: empty cluster (always cull).
__global__ void cluster_cone_kernel(const float4 *__restrict__ sph, int64_t n_clusters, const float *__restrict__ rays6,
                                    const int *__restrict__ shared_flag, float4 *__restrict__ rec) {
    if (*shared_flag == 0) return;
    int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_clusters) return;
    const float4 s = sph[c];
    float4 a = make_float4(0.f, 0.f, 1.f, -2.f), b = make_float4(0.f, 0.f, 0.f, 0.f);
    if (s.w < 0.f) {
        a.w = 2.f;
    } else {
        float vx = s.x - rays6[0], vy = s.y - rays6[1], vz = s.z - rays6[2];
        float dist = sqrtf(vx * vx + vy * vy + vz * vz);
        if (dist > s.w * 1.0001f && dist > 0.f) {
            float inv = 1.0f / dist;
            float sn = fminf(s.w * inv * 1.0001f, 1.0f);
            a = make_float4(vx * inv, vy * inv, vz * inv, sqrtf(fmaxf(0.f, 1.0f - sn * sn)));
            b.x = sn;
        }
    }
    rec[2 * c] = a;
    rec[2 * c + 1] = b;
}

// ---- direction binning (counting sort by Hilbert-ordered cell of the octahedral map)
__device__ __forceinline__ void octa(float dx, float dy, float dz, float &u, float &v) {
    float n = fabsf(dx) + fabsf(dy) + fabsf(dz);
    float inv = n > 0.f ? 1.0f / n : 0.f;
    float px = dx * inv, py = dy * inv;
    if (dz < 0.f) {
        float qx = (1.0f - fabsf(py)) * (px >= 0.f ? 1.f : -1.f);
        float qy = (1.0f - fabsf(px)) * (py >= 0.f ? 1.f : -1.f);
        px = qx; py = qy;
    }
    u = px; v = py;
}
// Hilbert curve index of cell (x, y) on the 2^BIN_BITS grid.  Consecutive indices are always
// neighbouring cells (no long jumps, unlike Morton order), so ANY run of 64 sorted rays -- one
// wave -- covers a compact patch of directions.
__device__ __forceinline__ unsigned hilbert_index(unsigned x, unsigned y) {
    const unsigned n = 1u << BIN_BITS;
    unsigned d = 0;
#pragma unroll
    for (unsigned s = n >> 1; s > 0; s >>= 1) {
        const unsigned rx = (x & s) ? 1u : 0u, ry = (y & s) ? 1u : 0u;
        d += s * s * ((3u * rx) ^ ry);
        if (ry == 0u) {
            if (rx == 1u) { x = n - 1u - x; y = n - 1u - y; }
            const unsigned t = x; x = y; y = t;
        }
    }
    return d;
}

// The direction order of a frame's rays is kept between calls.  A camera sends the same rays every
// frame, and the order only decides how COMPACT the 64-ray packets are: the culling takes every
// packet's cone from the rays the packet actually holds, so an order computed for other rays of
// the same count is merely less efficient, never wrong.  ray_order_check_kernel compares RAY_SAMPLES
// evenly spaced directions bit for bit with those the kept order was built from; only on a
// mismatch (`stale`) do the four binning kernels below run, otherwise they return at once.
constexpr int RAY_SAMPLES = 4096;
__global__ void ray_order_check_kernel(const float *__restrict__ rays6, int64_t N, float *__restrict__ samples,
                                       int *__restrict__ stale, unsigned *__restrict__ bounds) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s == 0) { bounds[0] = 0xFFFFFFFFu; bounds[1] = 0u; bounds[2] = 0xFFFFFFFFu; bounds[3] = 0u; }
    if (s >= RAY_SAMPLES) return;
    const int64_t i = (int64_t)s * N / RAY_SAMPLES;
    bool diff = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const unsigned now = __float_as_uint(rays6[6 * i + 3 + k]), was = __float_as_uint(samples[3 * s + k]);
        diff |= now != was;
        samples[3 * s + k] = __uint_as_float(now);
    }
    if (__builtin_amdgcn_ballot_w64(diff) != 0ull && (threadIdx.x & 63) == 0) atomicOr(stale, 1);
}

// bounds[0..3] = enc(min u), enc(max u), enc(min v), enc(max v); preset by ray_order_check_kernel.
// Also clears the histogram for ray_count_kernel (one word per thread and trip).
__global__ void ray_bounds_kernel(const float *__restrict__ rays6, int64_t N, const int *__restrict__ stale,
                                  unsigned *__restrict__ bounds, unsigned *__restrict__ hist) {
    if (*stale == 0) return;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < BIN_CELLS; k += gridDim.x * blockDim.x) hist[k] = 0u;
    unsigned lo_u = 0xFFFFFFFFu, hi_u = 0u, lo_v = 0xFFFFFFFFu, hi_v = 0u;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        float u, v;
        octa(rays6[6 * i + 3], rays6[6 * i + 4], rays6[6 * i + 5], u, v);
        if (u == u && v == v) {
            unsigned eu = enc_f(u), ev = enc_f(v);
            lo_u = eu < lo_u ? eu : lo_u; hi_u = eu > hi_u ? eu : hi_u;
            lo_v = ev < lo_v ? ev : lo_v; hi_v = ev > hi_v ? ev : hi_v;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        unsigned t;
        t = __shfl_xor(lo_u, off, 64); lo_u = t < lo_u ? t : lo_u;
        t = __shfl_xor(hi_u, off, 64); hi_u = t > hi_u ? t : hi_u;
        t = __shfl_xor(lo_v, off, 64); lo_v = t < lo_v ? t : lo_v;
        t = __shfl_xor(hi_v, off, 64); hi_v = t > hi_v ? t : hi_v;
    }
    __shared__ unsigned red[4][4];  // [wave][which]: same-address atomics are slow, one set per block
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[wave][0] = lo_u; red[wave][1] = hi_u; red[wave][2] = lo_v; red[wave][3] = hi_v; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            lo_u = red[w][0] < lo_u ? red[w][0] : lo_u; hi_u = red[w][1] > hi_u ? red[w][1] : hi_u;
            lo_v = red[w][2] < lo_v ? red[w][2] : lo_v; hi_v = red[w][3] > hi_v ? red[w][3] : hi_v;
        }
        atomicMin(&bounds[0], lo_u); atomicMax(&bounds[1], hi_u);
        atomicMin(&bounds[2], lo_v); atomicMax(&bounds[3], hi_v);
    }
}

__device__ __forceinline__ unsigned ray_cell(const float *__restrict__ rays6, int64_t i, const unsigned *__restrict__ bounds) {
    float u, v;
    octa(rays6[6 * i + 3], rays6[6 * i + 4], rays6[6 * i + 5], u, v);
    const float u0 = dec_f(bounds[0]), u1 = dec_f(bounds[1]), v0 = dec_f(bounds[2]), v1 = dec_f(bounds[3]);
    const float su = u1 > u0 ? (float)(1 << BIN_BITS) / (u1 - u0) : 0.f, sv = v1 > v0 ? (float)(1 << BIN_BITS) / (v1 - v0) : 0.f;
    int qu = (int)((u - u0) * su), qv = (int)((v - v0) * sv);
    qu = qu < 0 ? 0 : (qu > (1 << BIN_BITS) - 1 ? (1 << BIN_BITS) - 1 : qu);
    qv = qv < 0 ? 0 : (qv > (1 << BIN_BITS) - 1 ? (1 << BIN_BITS) - 1 : qv);
    if (!(u == u) || !(v == v)) { qu = 0; qv = 0; }
    return hilbert_index((unsigned)qu, (unsigned)qv);
}

__global__ void ray_count_kernel(const float *__restrict__ rays6, int64_t N, const int *__restrict__ stale,
                                 const unsigned *__restrict__ bounds, unsigned *__restrict__ hist) {
    if (*stale == 0) return;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) atomicAdd(&hist[ray_cell(rays6, i, bounds)], 1u);
}

// exclusive scan of BIN_CELLS counters, one workgroup of 1024 threads (64 cells each)
__global__ __launch_bounds__(1024) void bin_scan_kernel(const int *__restrict__ stale, unsigned *__restrict__ hist) {
    if (*stale == 0) return;
    __shared__ unsigned part[1024];
    constexpr int PER = BIN_CELLS / 1024;
    unsigned loc[PER], sum = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) { loc[k] = hist[threadIdx.x * PER + k]; sum += loc[k]; }
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        unsigned t = threadIdx.x >= (unsigned)off ? part[threadIdx.x - off] : 0u;
        __syncthreads();
        part[threadIdx.x] += t;
        __syncthreads();
    }
    unsigned run = part[threadIdx.x] - sum;
#pragma unroll
    for (int k = 0; k < PER; ++k) { hist[threadIdx.x * PER + k] = run; run += loc[k]; }
}

__global__ void ray_scatter_kernel(const float *__restrict__ rays6, int64_t N, const int *__restrict__ stale,
                                   const unsigned *__restrict__ bounds, unsigned *__restrict__ cursor /* scanned */,
                                   unsigned *__restrict__ perm) {
    if (*stale == 0) return;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) perm[atomicAdd(&cursor[ray_cell(rays6, i, bounds)], 1u)] = (unsigned)i;
}

__device__ __forceinline__ float wave_sum_f(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ float wave_min_f(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fminf(v, __shfl_xor(v, off, 64));
    return v;
}

// ---- culled sweep in three balanced steps ------------------------------------------------
// 1. ray_cull_mask_kernel: one wave per packet (64 direction-sorted rays): cone of the packet,
//    lane-parallel cluster tests, the ballot of 64 tests IS the mask word of surviving clusters.
// 2. ray_segment_kernel: cuts every packet's survivor list into segments of seg_len clusters
//    (>= RSEG_MIN, chosen on the device so all fit the table).  Packets that look along a
//    surface see hundreds of clusters, most see none: without this step a few waves carried
//    the kernel (0.52 ms); with it every sweep wave has the same amount of work.
// 3. ray_sweep_seg_kernel: one wave per segment, ray per lane, the loop body of the exhaustive
//    kernel on the segment's clusters; packets meet in the same 64-bit atomicMin keys.
constexpr int RSEG_MIN = 16;    // clusters per segment at least (256 triangles)
constexpr int RLIST = 2048;     // most clusters one sweep wave walks (LDS list)

__global__ __launch_bounds__(256) void ray_cull_mask_kernel(const float4 *__restrict__ cones,
                                                            const float4 *__restrict__ scones, int n_clusters,
                                                            int n_words, const float *__restrict__ rays6,
                                                            const unsigned *__restrict__ perm, int64_t N,
                                                            unsigned long long *__restrict__ mask,
                                                            int *__restrict__ pk_cnt, const int *__restrict__ shared_flag) {
    if (*shared_flag == 0) return;
    const int lane = threadIdx.x & 63;
    const int64_t pk = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pk * 64 >= N) return;
    const int64_t k = pk * 64 + lane;
    const int64_t ri = perm[k < N ? k : N - 1];
    const float dx = rays6[6 * ri + 3], dy = rays6[6 * ri + 4], dz = rays6[6 * ri + 5];
    // cone of this packet: axis = normalised sum of unit directions, cos(theta) = min dot
    const float inv = rsqrtf(dx * dx + dy * dy + dz * dz);
    const float ux = dx * inv, uy = dy * inv, uz = dz * inv;
    float ax = wave_sum_f(ux), ay = wave_sum_f(uy), az = wave_sum_f(uz);
    const float ainv = rsqrtf(ax * ax + ay * ay + az * az);
    ax *= ainv; ay *= ainv; az *= ainv;
    const float ct = wave_min_f(ux * ax + uy * ay + uz * az) - 1e-5f;  // margin: rsqrt + rounding
    // wide or degenerate (NaN) packets do not cull: every comparison below is then false
    const bool can_cull = ct > 0.1f;
    const float st = sqrtf(fmaxf(0.f, 1.0f - ct * ct)) + 1e-5f;
    int cnt = 0;
    // level 1: one test per super-cluster (= one mask word of 64 clusters); lane l takes word
    // sw + l.  level 2: the 64 clusters of every surviving word.
    for (int sw = 0; sw < n_words; sw += 64) {
        const int wl = sw + lane;
        bool live = false;
        if (wl < n_words) {
            const float4 ca = scones[2 * wl];
            const float sp = scones[2 * wl + 1].x;
            const float cosv = ca.x * ax + ca.y * ay + ca.z * az;
            const float lim = ct * ca.w - st * sp - 1e-5f;
            live = !((ca.w > 1.5f) || (can_cull && ca.w > -1.5f && cosv < lim));
            if (!live) mask[(size_t)pk * n_words + wl] = 0ull;
        }
        unsigned long long todo = __builtin_amdgcn_ballot_w64(live);
        while (todo != 0ull) {  // wave-uniform
            const int wi = sw + __builtin_ctzll(todo);
            todo &= todo - 1ull;
            const int c = wi * 64 + lane;
            bool keep = false;
            if (c < n_clusters) {
                const float4 ca = cones[2 * c];
                const float sp = cones[2 * c + 1].x;
                const float cosv = ca.x * ax + ca.y * ay + ca.z * az;
                const float lim = ct * ca.w - st * sp - 1e-5f;  // cos(theta + psi), lowered by a margin
                const bool culled = (ca.w > 1.5f) || (can_cull && ca.w > -1.5f && cosv < lim);
                keep = !culled;
            }
            const unsigned long long m = __builtin_amdgcn_ballot_w64(keep);
            if (lane == 0) mask[(size_t)pk * n_words + wi] = m;
            cnt += __builtin_popcountll(m);
        }
    }
    if (lane == 0) pk_cnt[pk] = cnt;
}

// seg_info[0] = number of segments, seg_info[1] = seg_len
__global__ __launch_bounds__(1024) void ray_segment_kernel(const int *__restrict__ pk_cnt, int n_packets,
                                                           int *__restrict__ seg_pk, int *__restrict__ seg_rank0,
                                                           int *__restrict__ seg_n, int max_segs, int *__restrict__ seg_info,
                                                           const int *__restrict__ shared_flag) {
    if (*shared_flag == 0) { if (threadIdx.x == 0) seg_info[0] = 0; return; }
    __shared__ long long red[16];
    __shared__ int scan[1024];
    __shared__ long long total_s;
    const int tid = threadIdx.x;
    const int per = (n_packets + 1023) / 1024;
    const int b0 = tid * per, b1 = (b0 + per < n_packets) ? b0 + per : n_packets;
    long long v = 0;
    for (int b = b0; b < b1; ++b) v += pk_cnt[b];
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
    long long room = (long long)max_segs - n_packets;
    if (room < 1) room = 1;
    long long sl = (total_s + room - 1) / room;
    if (sl < RSEG_MIN) sl = RSEG_MIN;
    if (sl > RLIST) sl = RLIST;  // the host sizes max_segs so that this cannot bind
    const int seg_len = (int)sl;
    int mine = 0;
    for (int b = b0; b < b1; ++b) mine += (pk_cnt[b] + seg_len - 1) / seg_len;
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
        const int c = pk_cnt[b];
        for (int r0 = 0; r0 < c; r0 += seg_len) {
            if (at < max_segs) { seg_pk[at] = b; seg_rank0[at] = r0; seg_n[at] = (c - r0 < seg_len) ? c - r0 : seg_len; }
            ++at;
        }
    }
    if (tid == 1023) { seg_info[0] = scan[1023] < max_segs ? scan[1023] : max_segs; seg_info[1] = seg_len; }
}

__global__ __launch_bounds__(RPL_BLOCK) void ray_sweep_seg_kernel(
    const f2 *__restrict__ rec, const float *__restrict__ aos, int n_words, const unsigned long long *__restrict__ mask,
    const int *__restrict__ seg_pk, const int *__restrict__ seg_rank0, const int *__restrict__ seg_n,
    const int *__restrict__ seg_info, const float *__restrict__ rays6, const unsigned *__restrict__ perm, int64_t N,
    unsigned long long *__restrict__ keys) {
    __shared__ unsigned surv[RPL_BLOCK / 64][RLIST];
    constexpr int PF = PAIR_SH / 2;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int seg = blockIdx.x * (RPL_BLOCK / 64) + wv;
    if (seg >= seg_info[0]) return;  // wave-uniform
    const int pk = seg_pk[seg], r0 = seg_rank0[seg], n_s = seg_n[seg];
    const int64_t k = (int64_t)pk * 64 + lane;
    const int64_t ri = perm[k < N ? k : N - 1];  // tail lanes re-run the last ray, never store
    Ray r;
    r.ox = rays6[6 * ri + 0]; r.oy = rays6[6 * ri + 1]; r.oz = rays6[6 * ri + 2];
    r.dx = rays6[6 * ri + 3]; r.dy = rays6[6 * ri + 4]; r.dz = rays6[6 * ri + 5];
    // expand ranks [r0, r0 + n_s) of the packet's mask into the LDS cluster list
    unsigned *mine = surv[wv];
    {
        int running = 0;
        const unsigned long long *mw = mask + (size_t)pk * n_words;
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
                const unsigned c0 = (unsigned)(wg + lane) * 64u;
                while (word != 0ull) {
                    const int bit = __builtin_ctzll(word);
                    word &= word - 1ull;
                    if (rank >= r0 && rank < r0 + n_s) mine[rank - r0] = c0 + (unsigned)bit;
                    ++rank;
                }
            }
            running += __shfl(incl, 63, 64);
        }
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): the wave's own LDS writes have landed
    unsigned long long best = KEY_MISS;
    const float dn_seg = fabsf(r.dx) + fabsf(r.dy) + fabsf(r.dz);
    for (int q = 0; q < n_s; ++q) {
        const int cl = (int)__builtin_amdgcn_readfirstlane(mine[q]);  // wave-uniform: scalar record loads below
#pragma unroll 1
        for (int gi = 0; gi < CL_GROUPS; ++gi) {
            const int g = cl * CL_GROUPS + gi;
            const f2 *t = rec + (size_t)g * (RPL_PAIRS * PF);
            f2 sc[RPL_PAIRS];
#pragma unroll
            for (int p = 0; p < RPL_PAIRS; ++p) sc[p] = score_pair_shared(r, dn_seg, t + p * PF);
            const float top = fmaxf(fmaxf(sc[0].x, sc[0].y), fmaxf(sc[1].x, sc[1].y));
            if (__builtin_amdgcn_ballot_w64(top >= 0.0f) != 0) {
                const int f0 = g * (2 * RPL_PAIRS);
#pragma unroll
                for (int e = 0; e < 2 * RPL_PAIRS; ++e) {
                    const float s = (e & 1) ? sc[e >> 1].y : sc[e >> 1].x;
                    if (s >= 0.0f) {
                        MT m = mt_eval(r, aos + (size_t)(f0 + e) * PEDP_TRI_STRIDE);
                        if (mt_accept(m)) {
                            unsigned long long key = mt_key(m, (unsigned)(f0 + e));
                            best = key < best ? key : best;
                        }
                    }
                }
            }
        }
    }
    if (k < N && best != KEY_MISS) atomicMin(&keys[ri], best);
}

}  // namespace
