// The frame-sized host work of FoundationPose's register on the device: what guess_translation (estimater.py:135-147) and
// the gate before it (:182-183) read off a depth frame and a mask with np.where, np.median and a sum.
//
//   stats_kernel    one pass over the pixels: the three counts, the box of mask > 0, and a histogram of the top 12 key bits
//                   of the depths that enter the median
//   refine_kernel   a histogram of the next 10 key bits among the depths whose higher bits equal a chosen prefix; run twice
//   select_kernel   one workgroup between the passes: the bin that holds the wanted rank, the rank left inside it; after
//                   the last pass the median itself and the record
//
// A depth that enters the median is >= 0.001, so its float32 bit pattern orders as an unsigned integer (+inf last; NaN
// and negative values fail the comparison and never enter).  The median is therefore a rank select on those keys, and an
// even count selects two ranks, which may part ways at any of the three levels: every level keeps two prefixes and two
// histograms.  Counts and histograms are integer atomics (LDS per workgroup, then global), so nothing depends on the
// order in which workgroups run.  The launches follow each other on the context's stream; nothing waits inside a kernel.
// DESIGN.md s4.11 is the contract.
#include "pedp_internal.h"
#include <cmath>

namespace {

constexpr int TPB = 256;
constexpr int BITS1 = 12, BITS2 = 10, BITS3 = 10;  // 32 key bits over the three passes
constexpr int NB1 = 1 << BITS1, NB2 = 1 << BITS2;
constexpr unsigned NEVER = 0xFFFFFFFFu;            // a prefix no key has (an empty set: the later passes count nothing)

// Workspace, uint32 words, zeroed by one memset per call.
enum {
    C_NPOS = 0, C_NVALID, C_NMED, C_UMIN_INV, C_UMAX, C_VMIN_INV, C_VMAX,  // minima are kept as maxima of INT_MAX - x
    C_PREFIX = 8,   // [2] key bits chosen so far for the lower and the upper middle rank
    C_RANK = 10,    // [2] their ranks among the keys that share the prefix
    C_RECORD = 16,  // pedp_mask_depth_record (8 words)
    W_HIST1 = 32,
    W_HIST2 = W_HIST1 + NB1,       // [2][NB2]
    W_HIST3 = W_HIST2 + 2 * NB2,   // [2][NB2]
    W_TOTAL = W_HIST3 + 2 * NB2,
};

// numpy's two readings of a mask entry: `mask > 0` and `mask.astype(bool)`
__device__ __forceinline__ bool is_pos(uint8_t m) { return m != 0; }
__device__ __forceinline__ bool is_true(uint8_t m) { return m != 0; }
__device__ __forceinline__ bool is_pos(float m) { return m > 0.0f; }    // false for NaN and negatives
__device__ __forceinline__ bool is_true(float m) { return m != 0.0f; }  // true for NaN and negatives, false for -0.0

__device__ __forceinline__ unsigned wave_max(unsigned v) {
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned o = __shfl_down(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}

__device__ __forceinline__ unsigned wave_sum(unsigned v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

template <typename M>
__global__ __launch_bounds__(TPB) void stats_kernel(const float *__restrict__ depth, const M *__restrict__ mask, unsigned n,
                                                    unsigned W, unsigned *__restrict__ ws) {
    __shared__ unsigned hist[NB1];
    __shared__ unsigned red[7];  // the workgroup's counts and box, in the workspace's order
    for (int k = threadIdx.x; k < NB1; k += TPB) hist[k] = 0;
    if (threadIdx.x < 7) red[threadIdx.x] = 0;
    __syncthreads();
    unsigned npos = 0, nvalid = 0, nmed = 0, umin_inv = 0, umax = 0, imin_inv = 0, imax = 0;
    for (unsigned i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
        const M m = mask[i];
        const float d = depth[i];
        const bool near = d >= 0.001f;
        if (is_pos(m)) {
            const unsigned u = i % W;
            ++npos;
            nvalid += near;
            umin_inv = max(umin_inv, 0x7FFFFFFFu - u);
            umax = max(umax, u);
            imin_inv = max(imin_inv, 0x7FFFFFFFu - i);  // rows grow with the flat index: the row box comes from its extremes
            imax = max(imax, i);
        }
        if (near && is_true(m)) {
            ++nmed;
            atomicAdd(&hist[__float_as_uint(d) >> (32 - BITS1)], 1u);
        }
    }
    npos = wave_sum(npos); nvalid = wave_sum(nvalid); nmed = wave_sum(nmed);
    umin_inv = wave_max(umin_inv); umax = wave_max(umax); imin_inv = wave_max(imin_inv); imax = wave_max(imax);
    if ((threadIdx.x & 63) == 0 && npos) {
        atomicAdd(&red[C_NPOS], npos);
        atomicAdd(&red[C_NVALID], nvalid);
        atomicMax(&red[C_UMIN_INV], umin_inv);
        atomicMax(&red[C_UMAX], umax);
        atomicMax(&red[C_VMIN_INV], 0x7FFFFFFFu - (0x7FFFFFFFu - imin_inv) / W);
        atomicMax(&red[C_VMAX], imax / W);
    }
    if ((threadIdx.x & 63) == 0 && nmed) atomicAdd(&red[C_NMED], nmed);
    __syncthreads();
    if (threadIdx.x < 7 && red[threadIdx.x]) {  // one global atomic per workgroup and field; zero changes neither a sum nor a maximum
        if (threadIdx.x <= C_NMED) atomicAdd(&ws[threadIdx.x], red[threadIdx.x]);
        else atomicMax(&ws[threadIdx.x], red[threadIdx.x]);
    }
    for (int k = threadIdx.x; k < NB1; k += TPB)
        if (hist[k]) atomicAdd(&ws[W_HIST1 + k], hist[k]);
}

// Keys whose bits above `shift + BITS` equal a prefix are counted by their next BITS bits, for each of the two prefixes.
template <typename M>
__global__ __launch_bounds__(TPB) void refine_kernel(const float *__restrict__ depth, const M *__restrict__ mask, unsigned n,
                                                     int shift, const unsigned *__restrict__ state, unsigned *__restrict__ out) {
    __shared__ unsigned hist[2][NB2];
    for (int k = threadIdx.x; k < 2 * NB2; k += TPB) (&hist[0][0])[k] = 0;
    __syncthreads();
    const unsigned p0 = state[C_PREFIX], p1 = state[C_PREFIX + 1];
    for (unsigned i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
        const float d = depth[i];
        if (!(d >= 0.001f) || !is_true(mask[i])) continue;
        const unsigned key = __float_as_uint(d);
        const unsigned hi = key >> (shift + BITS2), bin = (key >> shift) & (NB2 - 1);
        if (hi == p0) atomicAdd(&hist[0][bin], 1u);
        if (hi == p1) atomicAdd(&hist[1][bin], 1u);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < 2 * NB2; k += TPB) {
        const unsigned h = (&hist[0][0])[k];
        if (h) atomicAdd(&out[k], h);
    }
}

// The bin of `hist` that holds the element of rank `rank` (0-based, rank < the histogram's total) and the rank inside that
// bin.  The whole workgroup calls it; every thread gets the answer.
__device__ void find_bin(const unsigned *hist, int nbins, unsigned rank, unsigned *bin, unsigned *left) {
    __shared__ unsigned part[TPB];
    __shared__ unsigned res[2];
    const int t = threadIdx.x, per = nbins / TPB;
    unsigned s = 0;
    for (int k = 0; k < per; ++k) s += hist[t * per + k];
    __syncthreads();  // the previous call's readers are done
    part[t] = s;
    __syncthreads();
    for (int off = 1; off < TPB; off <<= 1) {  // inclusive scan of the threads' sums
        const unsigned v = t >= off ? part[t - off] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    unsigned before = part[t] - s;
    if (before <= rank && rank < part[t]) {  // exactly one thread: its bins hold the rank
        int b = t * per;
        const int last = b + per - 1;
        while (b < last && before + hist[b] <= rank) before += hist[b++];
        res[0] = (unsigned)b;
        res[1] = rank - before;
    }
    __syncthreads();
    *bin = res[0];
    *left = res[1];
}

__device__ void write_record(unsigned *ws, float median) {
    const unsigned npos = ws[C_NPOS];
    int32_t *r = (int32_t *)(ws + C_RECORD);
    r[0] = (int32_t)npos;
    r[1] = (int32_t)ws[C_NVALID];
    r[2] = (int32_t)ws[C_NMED];
    r[3] = npos ? (int32_t)(0x7FFFFFFFu - ws[C_UMIN_INV]) : -1;
    r[4] = npos ? (int32_t)ws[C_UMAX] : -1;
    r[5] = npos ? (int32_t)(0x7FFFFFFFu - ws[C_VMIN_INV]) : -1;
    r[6] = npos ? (int32_t)ws[C_VMAX] : -1;
    ((float *)r)[7] = median;
}

// stage 0: after stats_kernel; 1, 2: after the refining passes.  One workgroup.
__global__ __launch_bounds__(TPB) void select_kernel(unsigned *ws, int stage) {
    const unsigned n = ws[C_NMED];
    if (n == 0) {
        if (threadIdx.x == 0) {
            ws[C_PREFIX] = ws[C_PREFIX + 1] = NEVER;
            if (stage == 2) write_record(ws, __uint_as_float(0x7FC00000u));
        }
        return;
    }
    unsigned bin[2], left[2];
    if (stage == 0) {
        find_bin(ws + W_HIST1, NB1, (n - 1) / 2, &bin[0], &left[0]);  // the lower middle rank (the middle one for odd n)
        find_bin(ws + W_HIST1, NB1, n / 2, &bin[1], &left[1]);
    } else {
        const unsigned *h = ws + (stage == 1 ? W_HIST2 : W_HIST3);
        find_bin(h, NB2, ws[C_RANK], &bin[0], &left[0]);
        find_bin(h + NB2, NB2, ws[C_RANK + 1], &bin[1], &left[1]);
    }
    if (threadIdx.x != 0) return;
    for (int k = 0; k < 2; ++k) {
        const unsigned p = stage == 0 ? bin[k] : ((ws[C_PREFIX + k] << BITS2) | bin[k]);
        ws[C_PREFIX + k] = p;
        ws[C_RANK + k] = left[k];
    }
    if (stage == 2) {
        const float a = __uint_as_float(ws[C_PREFIX]), b = __uint_as_float(ws[C_PREFIX + 1]);
        write_record(ws, (n & 1) ? a : (a + b) / 2.0f);  // numpy: the mean of the two middle elements in float32
    }
}

size_t a256(size_t b) { return (b + 255) & ~(size_t)255; }

template <typename M>
int run(pedp_ctx_s *c, const float *d_depth, const M *d_mask, unsigned n, unsigned W, unsigned *ws) {
    const unsigned per_block = TPB * 8;
    unsigned blocks = (n + per_block - 1) / per_block;
    const unsigned cap = (unsigned)(c->num_cus > 0 ? c->num_cus : 256) * 2;
    blocks = blocks > cap ? cap : (blocks ? blocks : 1);
    PEDP_HIP_CHECK(hipMemsetAsync(ws, 0, sizeof(unsigned) * W_TOTAL, c->stream));
    hipLaunchKernelGGL(stats_kernel<M>, dim3(blocks), dim3(TPB), 0, c->stream, d_depth, d_mask, n, W, ws);
    hipLaunchKernelGGL(select_kernel, dim3(1), dim3(TPB), 0, c->stream, ws, 0);
    hipLaunchKernelGGL(refine_kernel<M>, dim3(blocks), dim3(TPB), 0, c->stream, d_depth, d_mask, n, BITS3, ws, ws + W_HIST2);
    hipLaunchKernelGGL(select_kernel, dim3(1), dim3(TPB), 0, c->stream, ws, 1);
    hipLaunchKernelGGL(refine_kernel<M>, dim3(blocks), dim3(TPB), 0, c->stream, d_depth, d_mask, n, 0, ws, ws + W_HIST3);
    hipLaunchKernelGGL(select_kernel, dim3(1), dim3(TPB), 0, c->stream, ws, 2);
    PEDP_HIP_CHECK(hipGetLastError());
    return PEDP_OK;
}

}  // namespace

extern "C" int pedp_mask_depth_stats(pedp_ctx_t c, const float *depth, const void *mask, int mask_dtype, int H, int W, int mem,
                                     pedp_mask_depth_record *out) {
    const char *who = "pedp_mask_depth_stats";
    static_assert(sizeof(pedp_mask_depth_record) == 32, "the record is eight words");
    PEDP_REQUIRE(c && out, "%s: null context or output", who);
    PEDP_REQUIRE(mem == PEDP_HOST || mem == PEDP_DEVICE, "%s: bad mem flag %d", who, mem);
    PEDP_REQUIRE(mask_dtype == PEDP_U8 || mask_dtype == PEDP_F32, "%s: mask dtype %d", who, mask_dtype);
    PEDP_REQUIRE(H > 0 && W > 0, "%s: %d x %d frame", who, H, W);
    PEDP_REQUIRE((int64_t)H * W <= (int64_t)4096 * 4096, "%s: %d x %d frame (at most 4096 x 4096 pixels)", who, H, W);
    PEDP_REQUIRE(depth && mask, "%s: null depth or mask", who);
    PEDP_HIP_CHECK(hipSetDevice(c->device));
    const unsigned n = (unsigned)H * (unsigned)W;
    const size_t bd = 4 * (size_t)n, bm = (mask_dtype == PEDP_F32 ? 4 : 1) * (size_t)n;
    int rc = c->stats_ws.reserve(sizeof(unsigned) * W_TOTAL);
    if (rc) return rc;
    unsigned *ws = (unsigned *)c->stats_ws.ptr;
    const float *d_depth = depth;
    const void *d_mask = mask;
    if (mem == PEDP_HOST) {
        rc = c->stats_io.reserve(a256(bd) + a256(bm));
        if (rc) return rc;
        char *p = (char *)c->stats_io.ptr;
        d_depth = (const float *)p;
        d_mask = p + a256(bd);
        rc = pedp_upload(c, (void *)d_depth, depth, bd);
        if (!rc) rc = pedp_upload(c, (void *)d_mask, mask, bm);
        if (rc) return rc;
    }
    rc = mask_dtype == PEDP_F32 ? run<float>(c, d_depth, (const float *)d_mask, n, (unsigned)W, ws)
                                : run<uint8_t>(c, d_depth, (const uint8_t *)d_mask, n, (unsigned)W, ws);
    if (rc) return rc;
    const void *view = nullptr;
    rc = pedp_download_view(c, ws + C_RECORD, sizeof(*out), &view);
    if (rc) return rc;
    memcpy(out, view, sizeof(*out));
    return PEDP_OK;
}
