// Point-cloud operations, shared by every stage of pedp_cloudops.hip: rocPRIM's radix-pass configuration and its error
// check, the scratch carver, the squared distance in the oracle's rounding, the 3-vector helpers, the sort's index fill.
#pragma once
#include "../pedp_internal.h"
#include <cmath>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_run_length_encode.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

namespace {

// rocPRIM sorts up to a million items by merging (about twenty launches whatever the key's width); with the limit at
// zero it always takes the radix passes, whose number follows the bits asked for
using RadixPasses = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config, rocprim::default_config, 0>;

inline size_t a256(size_t b) { return (b + 255) & ~(size_t)255; }

struct Carver {
    char *base;
    size_t off = 0;
    template <class T> T *take(size_t n) {
        T *p = (T *)(base + off);
        off = a256(off + sizeof(T) * n);
        return p;
    }
};

__device__ __forceinline__ double dist2(const double *a, const double *b) {
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return (dx * dx + dy * dy) + dz * dz;  // -ffp-contract=off: no FMA, the oracle's rounding
}

__device__ inline void cross3(const double *a, const double *b, double *o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ inline double dot3(const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// the 64-bit key sort's values before the sort: the point indices
__global__ void iota_kernel(int *__restrict__ v, int64_t N) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) v[i] = (int)i;
}

#define PEDP_ROCPRIM(expr)                                                                     \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) {                                                                \
            pedp_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(e_)); \
            return PEDP_ERR_HIP;                                                               \
        }                                                                                      \
    } while (0)

}  // namespace
