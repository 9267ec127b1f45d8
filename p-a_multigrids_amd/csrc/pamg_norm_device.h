// The reduction record's device helpers (gfx950), shared by the reduction kernels of pamg_norm.hip
// and the face operator's read-only residual reduction (pamg_face.hip k_face_residual_reduce): one
// definition of the record arithmetic and of the workgroup's fixed tree, so that every reduction
// kernel joins its values in the same order.
#pragma once

#include <hip/hip_runtime.h>

#include "pamg_device.h"
#include "pamg_internal.h"

namespace pamg {
namespace detail {

constexpr int kWaves = kBlock / 64;

__device__ __forceinline__ NormRec rec_identity() {
    NormRec r;
    r.max = -__builtin_huge_val();
    r.maxabs = 0.0;
    r.sumsq = 0.0;
    r.nonfinite = 0ull;
    return r;
}

// one value into a record; the exponent test also catches what fmax would drop (NaN)
__device__ __forceinline__ void rec_add(NormRec &r, double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    r.nonfinite |= (unsigned long long)((b & 0x7ff0000000000000ull) == 0x7ff0000000000000ull);
    r.max = fmax(r.max, v);
    r.maxabs = fmax(r.maxabs, __builtin_fabs(v));
    r.sumsq = r.sumsq + v * v;
}

// What a reduction kernel accumulates into the record's sum word (the record itself is shared with the face
// residual reduction and the ranks' 4-word gather, so it keeps its layout): kAccSq the squares (PAMG_NORM_REF,
// MAXABS, L2 -- rec_add, value by value), kAccAbs the magnitudes (PAMG_NORM_L1), kAccMass one term per
// sub-element, v^T M v with M = M_12 [[2,1,1],[1,2,1],[1,1,2]] = M_12 ((v0 + v1 + v2)^2 + v0^2 + v1^2 + v2^2)
// (PAMG_NORM_L2_MASS). The maxima and the non-finite word are the same in all three.
constexpr int kAccSq = 0, kAccAbs = 1, kAccMass = 2;

// the three values of one sub-element into a record, component order (m12: kAccMass only)
template <int MODE>
__device__ __forceinline__ void rec_add_sub(NormRec &r, const double v[3], double m12) {
    if constexpr (MODE == kAccSq) {
#pragma unroll
        for (int c = 0; c < 3; ++c) rec_add(r, v[c]);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned long long b = (unsigned long long)__double_as_longlong(v[c]);
            r.nonfinite |= (unsigned long long)((b & 0x7ff0000000000000ull) == 0x7ff0000000000000ull);
            r.max = fmax(r.max, v[c]);
            r.maxabs = fmax(r.maxabs, __builtin_fabs(v[c]));
            if constexpr (MODE == kAccAbs) r.sumsq = r.sumsq + __builtin_fabs(v[c]);
        }
        if constexpr (MODE == kAccMass) {
            const double sv = v[0] + v[1] + v[2];
            r.sumsq = r.sumsq + m12 * (sv * sv + v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        }
    }
}

// a (the lower index) combined with b
__device__ __forceinline__ NormRec rec_join(const NormRec &a, const NormRec &b) {
    NormRec r;
    r.max = fmax(a.max, b.max);
    r.maxabs = fmax(a.maxabs, b.maxabs);
    r.sumsq = a.sumsq + b.sumsq;
    r.nonfinite = a.nonfinite | b.nonfinite;
    return r;
}

__device__ __forceinline__ NormRec rec_shfl_down(const NormRec &a, int d) {
    NormRec r;
    r.max = __shfl_down(a.max, d, 64);
    r.maxabs = __shfl_down(a.maxabs, d, 64);
    r.sumsq = __shfl_down(a.sumsq, d, 64);
    r.nonfinite = __shfl_down(a.nonfinite, d, 64);
    return r;
}

// every thread of the workgroup (NW waves) calls it (threads past the tail with the identity); thread 0
// returns the workgroup's record
template <int NW = kWaves>
__device__ __forceinline__ NormRec block_reduce(NormRec r, NormRec *lds) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) r = rec_join(r, rec_shfl_down(r, d));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) lds[wave] = r;
    __syncthreads();
    if (threadIdx.x == 0) {
        r = lds[0];
#pragma unroll
        for (int w = 1; w < NW; ++w) r = rec_join(r, lds[w]);
    }
    return r;
}

}  // namespace detail
}  // namespace pamg
