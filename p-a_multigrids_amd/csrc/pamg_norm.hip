// Device reductions of libpamg (gfx950): one pass over a level produces the record
// {max, maxabs, sumsq, nonfinite} of a state field (k_field_reduce), of level 1's error |tnew - sin(x + y)|
// computed on the fly (k_error_reduce; k_error stores it, get_error :531-540) or of the residual
// A tnew - RHS computed on the fly (k_residual_reduce), which stores no field: the convergence
// monitor of pamg_residual_norm / pamg_solve must leave the state untouched (the reference
// cycle's restrictor reads the residual the previous cycle left, transport_tri_semi.F90:336-338,
// so a stored residual between two cycles changes the next one).
//
// The reduction is deterministic: lanes of a wave are combined with cross-lane shuffles in a
// fixed butterfly, the waves of a workgroup through LDS in wave order, every workgroup writes
// one partial record to a slab, and a second launch of one workgroup combines the slab -- each
// thread its records (every 1024th) in index order, then the same fixed tree. No floating-point
// atomics and no in-launch hand-off between workgroups: the launch boundary is the ordering.
// fmax drops a NaN, so non-finite inputs are carried in a separate word; the combine launch
// writes NaN into the three values when it is set.
#include <hip/hip_runtime.h>

#include <limits>

#include "pamg_device.h"
#include "pamg_internal.h"
#include "pamg_norm_device.h"

namespace pamg {
namespace {

using namespace detail;

// the combine launch: one workgroup of 16 waves, 8 records in flight per thread
constexpr int kCombineBlock = 1024, kCombineWaves = kCombineBlock / 64, kCombineBatch = 8;

// one state field: one thread per pair of sub-elements, 24 B per sub-element in, one record per workgroup out.
// MODE (pamg_norm_device.h): what goes into the record's sum word; kAccMass reads M_12 of the pair's un_ele from
// the level's operator record (a pair never straddles two un_eles: nsub is a power of 4)
template <int MODE>
__global__ __launch_bounds__(kBlock) void k_field_reduce(const double *__restrict__ F, const double *__restrict__ stc,
                                                         int64_t pitch, int64_t npairs, int nsub_log2,
                                                         NormRec *__restrict__ slab) {
    __shared__ NormRec lds[kWaves];
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    NormRec r = rec_identity();
    if (p < npairs) {
        const int64_t s = 2 * p;
        double2 v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = ld2(F + c * pitch + s);
        const double m12 = MODE == kAccMass ? stc[(s >> nsub_log2) * kStcStride + kStcM + 1] : 0.0;
        const double v0[3] = {v[0].x, v[1].x, v[2].x}, v1[3] = {v[0].y, v[1].y, v[2].y};
        rec_add_sub<MODE>(r, v0, m12);
        rec_add_sub<MODE>(r, v1, m12);
    }
    r = block_reduce(r, lds);
    if (threadIdx.x == 0) slab[blockIdx.x] = r;
}

// get_error (transport_tri_semi.F90:531-540): tracer(1)%error = |tnew - sin(x + y)| at the get_splitting nodes,
// the analytical value recomputed from the geometry records (error_one) and never stored; 24 B per sub-element
// in, 24 B out
__global__ __launch_bounds__(kBlock) void k_error(const double *__restrict__ T, double *__restrict__ E,
                                                  const double *__restrict__ geo, const int2 *__restrict__ subinfo,
                                                  int64_t pitch, int64_t npairs, int nsub_log2) {
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= npairs) return;
    const int64_t s = 2 * p, u = s >> nsub_log2;
    const int sub = (int)(s & ((1ll << nsub_log2) - 1));
    double2 tv[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) tv[c] = ld2(T + c * pitch + s);
    const double t0[3] = {tv[0].x, tv[1].x, tv[2].x}, t1[3] = {tv[0].y, tv[1].y, tv[2].y};
    double e0[3], e1[3];
    error_one(geo + u * kGeoStride, subinfo[sub], t0, e0);
    error_one(geo + u * kGeoStride, subinfo[sub + 1], t1, e1);
#pragma unroll
    for (int c = 0; c < 3; ++c) st2(E + c * pitch + s, make_double2(e0[c], e1[c]));
}

// the same values reduced in registers: k_error's loads and its error_one, fed to the workgroup's tree in
// k_field_reduce's order, so every value is bitwise the one k_error would store and every kind equals
// k_error + k_field_reduce on the float; 24 B per sub-element in, no field out
template <int MODE>
__global__ __launch_bounds__(kBlock) void k_error_reduce(const double *__restrict__ T, const double *__restrict__ geo,
                                                         const int2 *__restrict__ subinfo,
                                                         const double *__restrict__ stc, int64_t pitch, int64_t npairs,
                                                         int nsub_log2, NormRec *__restrict__ slab) {
    __shared__ NormRec lds[kWaves];
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    NormRec r = rec_identity();
    if (p < npairs) {
        const int64_t s = 2 * p, u = s >> nsub_log2;
        const int sub = (int)(s & ((1ll << nsub_log2) - 1));
        double2 tv[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) tv[c] = ld2(T + c * pitch + s);
        const double m12 = MODE == kAccMass ? stc[u * kStcStride + kStcM + 1] : 0.0;
        const double t0[3] = {tv[0].x, tv[1].x, tv[2].x}, t1[3] = {tv[0].y, tv[1].y, tv[2].y};
        double e0[3], e1[3];
        error_one(geo + u * kGeoStride, subinfo[sub], t0, e0);
        error_one(geo + u * kGeoStride, subinfo[sub + 1], t1, e1);
        rec_add_sub<MODE>(r, e0, m12);
        rec_add_sub<MODE>(r, e1, m12);
    }
    r = block_reduce(r, lds);
    if (threadIdx.x == 0) slab[blockIdx.x] = r;
}

// get_residual's A tnew - RHS (:725-873) reduced in registers: k_residual's loads and its resid(), so
// every value is bitwise the one k_residual would store; 48 B per sub-element in, no field out
template <class ST>
__global__ __launch_bounds__(kBlock) void k_residual_reduce(const double *__restrict__ T,
                                                            const double *__restrict__ RHS,
                                                            const double *__restrict__ stc, int64_t pitch,
                                                            int64_t npairs, int nsub_log2, double rdt,
                                                            NormRec *__restrict__ slab) {
    __shared__ NormRec lds[kWaves];
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    NormRec r = rec_identity();
    if (p < npairs) {
        const int64_t s = 2 * p;
        double2 xv[3], bv[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            xv[c] = ld2(T + c * pitch + s);
            bv[c] = ld2(RHS + c * pitch + s);
        }
        ST S;
        load_stc(stc + (s >> nsub_log2) * kStcStride, S);
        const double x0[3] = {xv[0].x, xv[1].x, xv[2].x}, x1[3] = {xv[0].y, xv[1].y, xv[2].y};
        const double b0[3] = {bv[0].x, bv[1].x, bv[2].x}, b1[3] = {bv[0].y, bv[1].y, bv[2].y};
        double r0[3], r1[3];
        resid(S, rdt, x0, b0, r0);
        resid(S, rdt, x1, b1, r1);
#pragma unroll
        for (int c = 0; c < 3; ++c) rec_add(r, r0[c]);
#pragma unroll
        for (int c = 0; c < 3; ++c) rec_add(r, r1[c]);
    }
    r = block_reduce(r, lds);
    if (threadIdx.x == 0) slab[blockIdx.x] = r;
}

// the slab's n records into *out, one workgroup of 1024 threads: thread t takes the records t, t + 1024,
// t + 2048, ... in index order, then the workgroup's fixed tree. The loads of a batch of 8 records are
// issued before any is joined: with one load in flight per thread (256 threads, 64 records each, one
// after the other) the launch took 21.6 us for the bench shape's 16,384 records, 64 memory latencies in a row
__global__ __launch_bounds__(kCombineBlock) void k_norm_combine(const NormRec *__restrict__ slab, int n,
                                                                NormRec *__restrict__ out) {
    __shared__ NormRec lds[kCombineWaves];
    NormRec r = rec_identity();
    int i = threadIdx.x;
    for (; i + (kCombineBatch - 1) * kCombineBlock < n; i += kCombineBatch * kCombineBlock) {
        NormRec v[kCombineBatch];
#pragma unroll
        for (int q = 0; q < kCombineBatch; ++q) v[q] = slab[i + q * kCombineBlock];
#pragma unroll
        for (int q = 0; q < kCombineBatch; ++q) r = rec_join(r, v[q]);
    }
    for (; i < n; i += kCombineBlock) r = rec_join(r, slab[i]);
    r = block_reduce<kCombineWaves>(r, lds);
    if (threadIdx.x == 0) {
        if (r.nonfinite) r.max = r.maxabs = r.sumsq = __builtin_nan("");
        *out = r;
    }
}

inline unsigned grid_for(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }
inline int log2i(int v) { int r = 0; while ((1 << r) < v) ++r; return r; }

}  // namespace

hipError_t launch_norm_combine(hipStream_t s, const NormRec *slab, int n, NormRec *out) {
    hipLaunchKernelGGL(k_norm_combine, dim3(1), dim3(kCombineBlock), 0, s, slab, n, out);
    return hipGetLastError();
}

size_t norm_slab_records(const Level &L) { return (size_t)grid_for(L.N / 2); }

hipError_t launch_field_reduce(hipStream_t s, const Level &L, const double *field, int mode, NormRec *slab,
                               NormRec *out) {
    const int64_t npairs = L.N / 2;
    if (npairs == 0) return hipSuccess;   // the caller supplies the identities
    const unsigned g = grid_for(npairs);
    const int lg = log2i(L.nsub);
    if (mode == kAccMass)
        hipLaunchKernelGGL((k_field_reduce<kAccMass>), dim3(g), dim3(kBlock), 0, s, field, L.stc, L.pitch, npairs, lg, slab);
    else if (mode == kAccAbs)
        hipLaunchKernelGGL((k_field_reduce<kAccAbs>), dim3(g), dim3(kBlock), 0, s, field, L.stc, L.pitch, npairs, lg, slab);
    else
        hipLaunchKernelGGL((k_field_reduce<kAccSq>), dim3(g), dim3(kBlock), 0, s, field, L.stc, L.pitch, npairs, lg, slab);
    hipLaunchKernelGGL(k_norm_combine, dim3(1), dim3(kCombineBlock), 0, s, slab, (int)g, out);
    return hipGetLastError();
}

hipError_t launch_error(hipStream_t s, const Level &L, const double *geo1, double *err) {
    const int64_t npairs = L.N / 2;
    if (npairs == 0) return hipSuccess;
    if (!err || !geo1 || !L.subinfo) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_error, dim3(grid_for(npairs)), dim3(kBlock), 0, s, L.T, err, geo1, L.subinfo, L.pitch, npairs,
                       log2i(L.nsub));
    return hipGetLastError();
}

hipError_t launch_error_reduce(hipStream_t s, const Level &L, const double *geo1, int mode, NormRec *slab,
                               NormRec *out) {
    const int64_t npairs = L.N / 2;
    if (npairs == 0) return hipSuccess;
    if (!geo1 || !L.subinfo) return hipErrorInvalidValue;
    const unsigned g = grid_for(npairs);
    const int lg = log2i(L.nsub);
    if (mode == kAccMass)
        hipLaunchKernelGGL((k_error_reduce<kAccMass>), dim3(g), dim3(kBlock), 0, s, L.T, geo1, L.subinfo, L.stc, L.pitch,
                           npairs, lg, slab);
    else if (mode == kAccAbs)
        hipLaunchKernelGGL((k_error_reduce<kAccAbs>), dim3(g), dim3(kBlock), 0, s, L.T, geo1, L.subinfo, L.stc, L.pitch,
                           npairs, lg, slab);
    else
        hipLaunchKernelGGL((k_error_reduce<kAccSq>), dim3(g), dim3(kBlock), 0, s, L.T, geo1, L.subinfo, L.stc, L.pitch,
                           npairs, lg, slab);
    hipLaunchKernelGGL(k_norm_combine, dim3(1), dim3(kCombineBlock), 0, s, slab, (int)g, out);
    return hipGetLastError();
}

hipError_t launch_residual_reduce(hipStream_t s, const Level &L, double rdt, NormRec *slab, NormRec *out) {
    const int64_t npairs = L.N / 2;
    if (npairs == 0) return hipSuccess;
    const unsigned g = grid_for(npairs);
    const int lg = log2i(L.nsub);
    if (L.arith == 1)
        hipLaunchKernelGGL((k_residual_reduce<StcF>), dim3(g), dim3(kBlock), 0, s, L.T, L.RHS, L.stc, L.pitch, npairs,
                           lg, rdt, slab);
    else
        hipLaunchKernelGGL((k_residual_reduce<Stc>), dim3(g), dim3(kBlock), 0, s, L.T, L.RHS, L.stc, L.pitch, npairs,
                           lg, rdt, slab);
    hipLaunchKernelGGL(k_norm_combine, dim3(1), dim3(kCombineBlock), 0, s, slab, (int)g, out);
    return hipGetLastError();
}

}  // namespace pamg
