// ICP, the 6x6 solve of a pass's close with a ROW PER LANE (solve6_ldlt_lanes).
//
// solve6_ldlt_reg (fused_close.h) runs the pivoted LDLT on one lane: fifteen column divisions, six more in the
// substitution and about sixty multiply-add pairs, each behind the one before it, at 1/64 of a wave's width, with the
// 36 entries in 72 registers.  Here lane i < 6 of every 16-lane row of a wave holds row i (six doubles), b[i] and later
// y[i]; step k is at most five multiply-add pairs and one division -- on all rows at once.
//
// Every output is computed by solve6_ldlt_reg's sequence of float64 operations (oracle/icp.c's), operation for
// operation: plain * + - / (the build has -ffp-contract=off), each row's sums in ascending j, the backward
// substitution as the one chain it is.
//
// The pivoting is done BEFORE the elimination.  The pivot of step k is the first index i >= k with the largest
// |A[i][i]|, and step k of the elimination writes column k of the rows below it and A[k][k] only -- behind its pivot
// choice -- so every pivot choice reads diagonal entries of the INPUT, moved by the exchanges before it.  The whole
// sequence of exchanges therefore follows from the six input diagonals: it is played through on them first (every lane
// does, in registers), each lane then fetches the row and the columns that END UP at its position, and the elimination
// runs without an exchange.  An entry goes through the same operations on the same values as in the form that exchanges
// as it goes: an exchange only moves entries, and a row's entry in column j is a function of the row's own entries and
// of the rows above position j alone.
//
// What crosses lanes goes through DPP with a constant lane of the row (row_newbcast: plain VALU moves) and, for the six
// results, v_readlane: no LDS, no ds_bpermute -- nothing here counts on lgkmcnt, which would wait behind loads in flight.
#pragma once
#include <hip/hip_runtime.h>

namespace {

// lane K (a constant) of each row of sixteen lanes, in every lane of that row
template <int K>
__device__ __forceinline__ double row_lane(double v) {
    static_assert(K >= 0 && K < 16, "a lane of the row");
    const int hi = __double2hiint(v), lo = __double2loint(v);
    return __hiloint2double(__builtin_amdgcn_update_dpp(hi, hi, 0x150 + K, 0xF, 0xF, false),
                            __builtin_amdgcn_update_dpp(lo, lo, 0x150 + K, 0xF, 0xF, false));
}
__device__ __forceinline__ double row_get(double v, int k) {  // (k is a constant once the caller's loop is unrolled)
    switch (k) {
    case 0: return row_lane<0>(v);
    case 1: return row_lane<1>(v);
    case 2: return row_lane<2>(v);
    case 3: return row_lane<3>(v);
    case 4: return row_lane<4>(v);
    default: return row_lane<5>(v);
    }
}
// NaN or infinite, by the exponent's bits.  pedp_icp.hip is built with -fno-honor-nans: v == v says nothing there, and the
// compiler may read a test of the bits of an arithmetic result as "infinite?" alone -- so the word is made opaque first.
__device__ __forceinline__ bool not_finite64(double v) {
    int hi = __double2hiint(v);
    asm("" : "+v"(hi));
    return (hi & 0x7FF00000) == 0x7FF00000;
}

// All 64 lanes of a wave call this.  A(u, v): entry (u, v) of the matrix, B(u): b[u] -- the same values in every lane.
// x[0..5] and the return value (false: a NaN or infinite solution, and x = 0 -- sign and payload of a NaN depend on
// the instructions the compiler picked, and no caller uses such a solution) are the same in every lane.
template <typename FA, typename FB>
__device__ __forceinline__ bool solve6_ldlt_lanes(FA A, FB B, double *__restrict__ x, const int lane) {
    // 1. the exchanges, played through on the diagonal: id[i] = the input's index that ends up at position i
    double dv[6];
    int id[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) { dv[i] = fabs(A(i, i)); id[i] = i; }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        int p = k;
        double big = dv[k];
#pragma unroll
        for (int i = k + 1; i < 6; ++i)
            if (dv[i] > big) { big = dv[i]; p = i; }
#pragma unroll
        for (int q = k + 1; q < 6; ++q) {  // positions k and p change places (dv[k] is not read again)
            const bool c = p == q;
            dv[q] = c ? dv[k] : dv[q];
            const int t = id[k];
            id[k] = c ? id[q] : id[k];
            id[q] = c ? t : id[q];
        }
    }
    // 2. this lane's position in its row of sixteen (positions 6-15 carry position 5's row again), its row and b
    const int pos = (lane & 15) < 6 ? (lane & 15) : 5;
    int my = id[5];
#pragma unroll
    for (int i = 4; i >= 0; --i) my = pos == i ? id[i] : my;
    double r[6], dd[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) r[j] = A(my, id[j]);
    double y = B(my);
    // 3. the elimination.  Rows above position k write their column k as well (the upper triangle: never read), and the
    // division turns position k's own A[k][k] into 1: the diagonal lives on in dd[], the same in every lane.
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        if (k > 0) {
            double tmp[6];
#pragma unroll
            for (int j = 0; j < k; ++j) tmp[j] = dd[j] * row_get(r[j], k);
            double u = 0.0;
#pragma unroll
            for (int j = 0; j < k; ++j) u += r[j] * tmp[j];
            r[k] = r[k] - u;  // (position k's is the one-lane form's sacc)
        }
        const double akk = row_get(r[k], k);
        dd[k] = akk;
        r[k] = fabs(akk) > 0.0 ? r[k] / akk : r[k];
    }
    // 4. forward substitution by columns (each y[i] sees j ascending), the diagonal, and the backward substitution --
    // one chain by its order (i = 5..0, j ascending) -- in every lane on broadcast entries
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const double yj = row_get(y, j);
        y = pos > j ? y - r[j] * yj : y;
    }
    {
        double dg = dd[5];
#pragma unroll
        for (int i = 4; i >= 0; --i) dg = pos == i ? dd[i] : dg;
        y = fabs(dg) > 2.2250738585072014e-308 ? y / dg : 0.0;
    }
    double yy[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) yy[i] = row_get(y, i);
#pragma unroll
    for (int i = 5; i >= 0; --i)
#pragma unroll
        for (int j = i + 1; j < 6; ++j) yy[i] -= row_get(r[i], j) * yy[j];
    // 5. the exchanges undone: x[id[i]] = yy[i].  Every lane keeps its position's entry; entry m is read from the first
    // lane whose row is m.
    double yl = yy[5];
#pragma unroll
    for (int i = 4; i >= 0; --i) yl = pos == i ? yy[i] : yl;
#pragma unroll
    for (int m = 0; m < 6; ++m) {
        const int src = __builtin_ctzll(__builtin_amdgcn_ballot_w64(my == m));
        x[m] = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(yl), src), __builtin_amdgcn_readlane(__double2loint(yl), src));
    }
    const bool ok = __builtin_amdgcn_ballot_w64(not_finite64(yl)) == 0ull;
#pragma unroll
    for (int m = 0; m < 6; ++m) x[m] = ok ? x[m] : 0.0;
    return ok;
}

}  // namespace
