// Ray stage, the last kernel of every cast: keys -> t_hit / prim_id / (u, v).  For a grid cast (variant 4) it also
// reports how the cast went, puts the OTHER header back to its start values and, where the grid could not answer,
// completes every ray with the general-origin loop of ray/sweep_packed.h first.
#pragma once
#include "mt.h"
#include "sweep_packed.h"
#include "grid.h"

namespace {

// ------------------------------------------------------------------ finalize
__global__ __launch_bounds__(256) void ray_finalize_kernel(const float *__restrict__ aos, const float *__restrict__ rays6,
                                    int64_t N, unsigned long long *__restrict__ keys,
                                    float *__restrict__ t_hit, uint32_t *__restrict__ prim_id,
                                    float *__restrict__ uv, const RastHdr *__restrict__ rast, RastHdr *__restrict__ rast_next,
                                    int *__restrict__ rast_status, const f2 *__restrict__ pairs, int groups_total, int reset_keys) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0 && rast) {  // variant 4: how the cast went, for the host's choice next time; the other header gets its start values
        rast_status[1] = (int)(N & 0x7FFFFFFF);
        rast_status[0] = rast->ok ? 0 : rast->reason;
        __threadfence_system();
        rast_next->ok = 1; rast_next->n_items = 0; rast_next->reason = 0; rast_next->n_full = 0;
    }
    if (i >= N) return;
    if (rast && rast->ok == 0) {
        // the grid could not answer this cast: every triangle for this ray, the exhaustive sweep's loop
        // (what the grid did find is kept: a minimum over more candidates)
        Ray r;
        r.ox = rays6[6 * i + 0]; r.oy = rays6[6 * i + 1]; r.oz = rays6[6 * i + 2];
        r.dx = rays6[6 * i + 3]; r.dy = rays6[6 * i + 4]; r.dz = rays6[6 * i + 5];
        keys[i] = sweep_groups<false>(r, pairs, aos, 0, groups_total, keys[i]);
    }
    if (i >= N) return;
    unsigned long long key = keys[i];
    if (reset_keys) keys[i] = KEY_MISS;   // a ray set's keys start the next cast clean (nothing else clears them)
    unsigned id = (unsigned)(key & 0xFFFFFFFFull);
    if (key == KEY_MISS) {
        t_hit[i] = __uint_as_float(0x7F800000u);
        prim_id[i] = 0xFFFFFFFFu;
        if (uv) { uv[2 * i] = 0.0f; uv[2 * i + 1] = 0.0f; }
        return;
    }
    t_hit[i] = __uint_as_float((unsigned)(key >> 32));
    prim_id[i] = id;
    if (uv) {
        Ray r;
        r.ox = rays6[6 * i + 0]; r.oy = rays6[6 * i + 1]; r.oz = rays6[6 * i + 2];
        r.dx = rays6[6 * i + 3]; r.dy = rays6[6 * i + 4]; r.dz = rays6[6 * i + 5];
        MT m = mt_eval(r, aos + (size_t)id * PEDP_TRI_STRIDE);
        unsigned sg = __float_as_uint(m.det) & 0x80000000u;
        float U = __uint_as_float(__float_as_uint(m.un) ^ sg);
        float V = __uint_as_float(__float_as_uint(m.vn) ^ sg);
        float ad = fabsf(m.det);
        uv[2 * i] = __fdiv_rn(U, ad);
        uv[2 * i + 1] = __fdiv_rn(V, ad);
    }
}

}  // namespace
