// ordered_sum.h -- the order in which the library adds what many lanes hold, stated once.  The losses and per-image operators
// (appearance, bilagrid, depth_prior, normal_prior, normal_map, smooth, gaussian_reg, alpha, and reproject.h for correspondence and
// warp) promise: no atomics, no memset, two runs give the same bits, and a view's result is the same bits alone or in a 16-view call.
// The promise is an order of additions, and the order is this file's:
//     lanes -> wave        block_sum: a __shfl_xor butterfly over d = 32, 16, ..., 1; every lane ends with the wave's total
//     waves -> workgroup   ... lane 0 of each wave leaves it in LDS, one barrier; block_total adds the waves in a left fold in wave
//                          order, ((w0 + w1) + w2) + w3
//     rows  -> one total   ordered_rows_sum: thread i of 256 adds rows i, i + 256, ... in that order, then block_sum
// A new loss includes this file and calls these; a kernel that adds in another order says so where it does (alpha_finalize_kernel,
// and sm_mean in smooth.hip).
// Beside them: the quad access of the kernels that take four consecutive floats per thread, and the float-slab sums of the
// per-Gaussian kernels (wave_total_f, slab_column_sum), which K9, antialias, sh_colors and gaussian_normals rely on as they stand.
// Every includer that promises bits is compiled with -ffp-contract=off; nothing here can be contracted anyway (sums and comparisons).
#pragma once
#include "bags_common.h"

namespace osum {

// N doubles per lane -> sh[wave * N + t], the total of column t over the wave; sh: N doubles of LDS per wave of the workgroup, whose
// earlier contents are dead (a caller that reuses sh puts a barrier in front).  Every lane of the workgroup calls it; it ends with
// a barrier.  (WAVES is not used here: it is taken so that a call site names the same pair as its block_total.)
template <int N, int WAVES = 4>
__device__ __forceinline__ void block_sum(const double (&acc)[N], double* __restrict__ sh)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int t = 0; t < N; ++t) {
        double s = acc[t];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
        if (lane == 0) sh[wave * N + t] = s;
    }
    __syncthreads();
}

// ... and column t of a workgroup of WAVES waves, the waves in wave order: the same bits in whichever thread asks
template <int N, int WAVES = 4>
__device__ __forceinline__ double block_total(const double* __restrict__ sh, const int t)
{
    double s = sh[t];
#pragma unroll
    for (int k = 1; k < WAVES; ++k) s += sh[k * N + t];
    return s;
}

// Columns 0..N-1 of `n` rows, `stride` doubles apart, added in row order by a workgroup of 256: thread i takes rows i, i + 256, ...,
// then block_sum.  Every thread ends with the N totals in S.  sh: 4 * N doubles of LDS, as for block_sum.
template <int N>
__device__ __forceinline__ void ordered_rows_sum(const double* __restrict__ rows, const int n, const int stride, double* __restrict__ sh,
                                                 double (&S)[N])
{
    double acc[N];
#pragma unroll
    for (int c = 0; c < N; ++c) acc[c] = 0.0;
#pragma unroll 4
    for (int s = threadIdx.x; s < n; s += 256) {
#pragma unroll
        for (int c = 0; c < N; ++c) acc[c] += rows[(size_t)s * stride + c];
    }
    block_sum<N>(acc, sh);
#pragma unroll
    for (int c = 0; c < N; ++c) S[c] = block_total<N>(sh, c);
}

// ---- a quad: n (1..4) consecutive floats at p.  VEC: a whole quad is one 16-byte access (the caller has checked the alignment); a
// short one is taken element by element in both instances.  load4 leaves 0 in the rest of d.
template <bool VEC> __device__ __forceinline__ void load4(const float* __restrict__ p, const int n, float (&d)[4])
{
    if (VEC && n == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        d[0] = t.x; d[1] = t.y; d[2] = t.z; d[3] = t.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) d[j] = (j < n) ? p[j] : 0.0f;
    }
}
template <bool VEC> __device__ __forceinline__ void store4(float* __restrict__ p, const int n, const float (&d)[4])
{
    if (VEC && n == 4) {
        *reinterpret_cast<float4*>(p) = make_float4(d[0], d[1], d[2], d[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) if (j < n) p[j] = d[j];
    }
}

__device__ __forceinline__ bool finite(const float x) { return x - x == 0.0f; }
__device__ __forceinline__ bool finite(const double x) { return x - x == 0.0; }
__device__ __forceinline__ double sign(const double r) { return (double)((r > 0.0) - (r < 0.0)); }                // sign(0) = 0

}  // namespace osum

// ---- the float slabs of the per-Gaussian kernels ---------------------------------------------------------------------------------
// sum over the 64 lanes on DPP (row_shr 1/2/4/8 inside the 16-lane rows, row_bcast:15 / row_bcast:31 across them: six
// v_add_f32_dpp); the total is valid in lane 63.  Every lane must be active.
__device__ __forceinline__ float wave_total_f(float x)
{
#define DPP_ADD(ctrl, rmask) x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), ctrl, rmask, 0xf, false))
    DPP_ADD(0x111, 0xf); DPP_ADD(0x112, 0xf); DPP_ADD(0x114, 0xf); DPP_ADD(0x118, 0xf); DPP_ADD(0x142, 0xa); DPP_ADD(0x143, 0xc);
#undef DPP_ADD
    return x;
}

// Column t of a slab of nblocks rows (one per workgroup of the kernel that wrote it, `stride` floats apart) summed in fp64 by one
// 256-thread workgroup: thread i adds rows i, i + 256, ... in row order, the 64 partial sums of a wave are added by a fixed shuffle
// tree, the four wave sums in wave order, so the result is deterministic.  The sum is returned in thread 0 (the others' is the same
// and not meant to be used).  Every thread has its 8 loads of a trip in flight at once; rows past the end INSIDE the batch are read
// at a clamped index and dropped afterwards: a remainder loop of single loads -- 1954 rows are 7.6 per thread, so most threads took
// it -- was seven dependent round trips, 6.5 us of a kernel that needs one.  No `in range ? load : 0`: the compiler makes that a
// branch per load with a wait behind each.
__device__ __forceinline__ double slab_column_sum(const float* __restrict__ slab, const int nblocks, const int stride, const int t)
{
    __shared__ double wsum[4];
    double acc = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 8 * 256) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = slab[(size_t)min(b + u * 256, nblocks - 1) * stride + t];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += (b + u * 256 < nblocks) ? (double)v[u] : 0.0;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    return ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}
