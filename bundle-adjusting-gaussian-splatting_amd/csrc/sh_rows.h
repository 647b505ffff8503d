// sh_rows.h -- the write-out of workgroup-staged SH gradient rows, stated once.
//
// dL/dsh[t][c] of a Gaussian is an outer product, basis_t x dL/dcolour_c, so what the thread that stores a piece of ANOTHER thread's
// row needs is 16 + 3 floats, not 48.  Every Gaussian of a workgroup stages those in LDS (shr_stage, SHR_W floats per Gaussian); the
// workgroup's rows of one tensor are one contiguous span of memory (G Gaussians x R floats, 16-byte aligned: G R is a multiple of 4),
// and it leaves as whole 16-byte lines: thread t owns float4 number t, t + 256, ... of the span (a thread writing its own 192-byte
// row 16 bytes at a time puts 64 separate requests per instruction on the L2 channels).  The tensor's very last float4 may be partial
// (P R not a multiple of 4): shr_load / shr_store.
//
// Users: preprocess_bwd_kernel (K9: one view, written or added to the buffer), sh_grad_from_views_kernel (the views' products summed
// in registers, the row written once: shr_product + shr_load + shr_store, G = 128), sh_colors_bwd_kernel (product) and
// sh_colors_views_bwd_kernel (the stage holds the finished rows: packed copy).  The pieces are single fp32 products and single adds:
// no indexing of them can change a bit.  What sharing can change is the generated code: profiles/sh_rows/NOTES.md.
#pragma once
#include "bags_common.h"

#define SHR_W 20         // floats per Gaussian in the product stage: basis[16], dL/dcolour[3], pad

// One Gaussian's row of the product stage: the basis with the entries >= nb (beyond the active degree) as zeros, then the cotangent.
__device__ __forceinline__ void shr_stage(float* __restrict__ row, const float* __restrict__ bs, const int nb, const float d0, const float d1, const float d2)
{
    const float4 q0 = make_float4(bs[0], nb > 1 ? bs[1] : 0.f, nb > 1 ? bs[2] : 0.f, nb > 1 ? bs[3] : 0.f);
    const float4 q1 = make_float4(nb > 4 ? bs[4] : 0.f, nb > 4 ? bs[5] : 0.f, nb > 4 ? bs[6] : 0.f, nb > 4 ? bs[7] : 0.f);
    const float4 q2 = make_float4(nb > 4 ? bs[8] : 0.f, nb > 9 ? bs[9] : 0.f, nb > 9 ? bs[10] : 0.f, nb > 9 ? bs[11] : 0.f);
    const float4 q3 = make_float4(nb > 9 ? bs[12] : 0.f, nb > 9 ? bs[13] : 0.f, nb > 9 ? bs[14] : 0.f, nb > 9 ? bs[15] : 0.f);
    float4* d4 = reinterpret_cast<float4*>(row);
    d4[0] = q0; d4[1] = q1; d4[2] = q2; d4[3] = q3;
    d4[4] = make_float4(d0, d1, d2, 0.f);
}
// ... of a Gaussian whose gradient row is zero
__device__ __forceinline__ void shr_stage_zero(float* row)
{
    float4* d4 = reinterpret_cast<float4*>(row);
#pragma unroll
    for (int t = 0; t < 5; ++t) d4[t] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// First float, in the tensor, of float4 number el of this workgroup's span (G Gaussians per workgroup, R floats per row).
template <u32 G, u32 R>
__device__ __forceinline__ size_t shr_first(const u32 el) { return (size_t)blockIdx.x * G * R + (size_t)el * 4u; }

// Float4 number el of the workgroup's span as products: float f = 4 el + u of the span is row f / R, float r = f - row R of it,
// coefficient T0 + r / 3 (T0: the tensor's first coefficient), channel r % 3.  Plain indexed LDS reads: a three-way select on
// 4j % 3 came out of the compiler with one branch using the wrong operand.
template <u32 R, u32 T0, u32 W>
__device__ __forceinline__ float4 shr_product(const float (*stage)[W], const u32 el)
{
    float o4[4];
#pragma unroll
    for (u32 u = 0; u < 4; ++u) {
        const u32 f = el * 4u + u, row = f / R, r = f - row * R, t = T0 + r / 3u, c = r - 3u * (r / 3u);
        o4[u] = stage[row][t] * stage[row][16u + c];
    }
    return make_float4(o4[0], o4[1], o4[2], o4[3]);
}
// ... from a stage that holds the finished rows, packed: float r of the tensor's row is stage[row][3 T0 + r]
template <u32 R, u32 T0, u32 W>
__device__ __forceinline__ float4 shr_packed(const float (*stage)[W], const u32 el)
{
    float o4[4];
#pragma unroll
    for (u32 u = 0; u < 4; ++u) {
        const u32 f = el * 4u + u, row = f / R, r = f - row * R;
        o4[u] = stage[row][3u * T0 + r];
    }
    return make_float4(o4[0], o4[1], o4[2], o4[3]);
}

// The float4 at float g0 of a tensor of `total` floats: whole when g0 + 3 < total, else the floats that exist (zeros / nothing for the
// others).  WHOLE: the caller knows it is whole (g0 < total and rows of a multiple of 4 floats), which the compiler cannot see.
template <bool WHOLE = false>
__device__ __forceinline__ float4 shr_load(const float* out, const size_t g0, const size_t total)
{
    if (WHOLE || g0 + 3 < total) return *reinterpret_cast<const float4*>(out + g0);
    return make_float4(g0 < total ? out[g0] : 0.f, g0 + 1 < total ? out[g0 + 1] : 0.f, g0 + 2 < total ? out[g0 + 2] : 0.f, 0.f);
}
template <bool WHOLE = false>
__device__ __forceinline__ void shr_store(float* out, const size_t g0, const size_t total, const float4 v)
{
    if (WHOLE || g0 + 3 < total) *reinterpret_cast<float4*>(out + g0) = v;
    else {
        if (g0 < total) out[g0] = v.x;
        if (g0 + 1 < total) out[g0 + 1] = v.y;
        if (g0 + 2 < total) out[g0 + 2] = v.z;
    }
}
// product + what is there, each component one add
__device__ __forceinline__ float4 shr_sum(const float4 o, const float4 a) { return make_float4(o.x + a.x, o.y + a.y, o.z + a.z, o.w + a.w); }

// The single-pass users' driver: the workgroup's G rows of one tensor (P rows of R floats) in one go.  The rounds are unrolled (the
// colour backwards), or, ROLLED, a loop left at the end of the span: K9's 12 rounds of 45-float rows, where unrolling is 1100
// instructions and the guard without the break two registers (profiles/sh_rows/NOTES.md).
enum ShrMode { SHR_PRODUCT, SHR_PRODUCT_ADD, SHR_PACKED };      // the products | the products added to the buffer's content | a packed stage copied
template <u32 G, u32 R, u32 T0, ShrMode MODE, bool ROLLED = false, u32 W>
__device__ __forceinline__ void shr_span(const float (*stage)[W], float* __restrict__ out, const int P)
{
    const size_t total = (size_t)P * R;
#pragma unroll ROLLED ? 1 : 64
    for (u32 k = 0; k < (G * R / 4u + 255u) / 256u; ++k) {
        const u32 el = k * 256u + threadIdx.x;
        const size_t g0 = shr_first<G, R>(el);
        if (ROLLED && el >= G * R / 4u) break;
        if (el < G * R / 4u && g0 < total) {
            float4 o;
            if constexpr (MODE == SHR_PACKED) o = shr_packed<R, T0>(stage, el);
            else o = shr_product<R, T0>(stage, el);
            if constexpr (MODE == SHR_PRODUCT_ADD) o = shr_sum(o, shr_load<R % 4u == 0u>(out, g0, total));
            shr_store<R % 4u == 0u>(out, g0, total, o);
        }
    }
}
