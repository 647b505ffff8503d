// alpha.hip -- the operator's weights map A = sum w_i (the accumulated opacity) held to a silhouette or a sky mask, or pushed to
// solid-or-empty by its entropy.  Per pixel, with an optional target t (constant data) and an optional pixel weight m (NULL: 1):
//     usable = A finite and m > 0 and (entropy: always | target modes: t finite; bce also 0 <= t <= 1)
//     w = m on usable pixels ;  cnt = sum w
//     inside = lo < A < hi  (float32, lo and hi rounded once by the caller) ;  a = A inside, lo where A <= lo, hi where A >= hi
//     bce:      l = -(t log a + (1 - t) log(1 - a))      dl/dA = (a - t) / (a (1 - a))   inside, 0 outside
//     entropy:  l = -(a log a + (1 - a) log(1 - a))      dl/dA = log((1 - a) / a)        inside, 0 outside
//     l1:       l = |A - t|                              dl/dA = sign(A - t), sign(0) = 0
//     l2:       l = (A - t)^2                            dl/dA = 2 (A - t)
//     L = sum w l / cnt                                  cnt <= 0: L = 0 and the gradient all zeros
// The comparisons are float32; everything after the loads is in double, the gradient rounded once.  The clamp and the validity are
// decisions: no gradient through them, and none to t or m.
//
// A map is a flat run of H W floats (no stencil: rows do not matter), taken as quads of four consecutive pixels.  A view has
// BAGS_ALPHA_GROUPS workgroups whatever its size and whatever the number of views (grid dimension y); workgroup g walks the
// contiguous span of quads [g span, (g + 1) span), thread t the quads t, t + ALPHA_BLOCK, ... of it, and leaves one row of 2
// doubles (cnt, sum w l), its lanes added as ordered_sum.h says (eight waves).  A workgroup whose span is empty leaves a zero row,
// so the workspace is never assumed clean.  The finalize kernel adds a view's rows in index order, one after the other.
// A whole quad is one float4 per map where every map of the call is 16-byte aligned, four floats otherwise, instantiated from one
// body (and -ffp-contract=off: the same bits); the last quad of a map whose size is no multiple of four is taken element by
// element in both.  No atomics, no memset: two runs give the same bits, and a view's loss, count and gradient are the same bits in
// a 16-view call and in a call of its own.  The mode is a template parameter: l1 and l2 carry no logarithm.
#include "ordered_sum.h"

#ifndef ALPHA_BLOCK
#define ALPHA_BLOCK 512                              // threads of a sums workgroup (profiles/alpha/NOTES.md: the alternatives timed)
#endif
#define ALPHA_BWD_BLOCK 256
#define ALPHA_ROW BAGS_ALPHA_STATS                   // doubles per partial row (cnt, sum w l) and per stats row (1/cnt or 0, unused)
static_assert(ALPHA_BLOCK % 64 == 0 && ALPHA_BLOCK >= 64 && ALPHA_BLOCK <= 1024, "whole waves");
static_assert(BAGS_ALPHA_GROUPS >= 1 && BAGS_ALPHA_GROUPS <= 256 && (BAGS_ALPHA_GROUPS & (BAGS_ALPHA_GROUPS - 1)) == 0,
              "a power of two of at most 256: the finalize kernel is one workgroup of that many threads");

struct AlphaDev {
    unsigned npix, nquads, span;                     // per view; span: quads per workgroup of the sums kernel
    float lo, hi;
    const float* weights[BAGS_MAX_POSE_ROWS];
    const float* target[BAGS_MAX_POSE_ROWS];         // NULL in the entropy mode
    const float* mask[BAGS_MAX_POSE_ROWS];           // any of them NULL: 1
    float* g_weights[BAGS_MAX_POSE_ROWS];            // backward: any of them NULL
};

// the maps of a quad; a lane past the end of the last quad has m = 0: not usable
template <bool VEC, int MODE> struct AlphaQuad {
    float A[4], t[4], m[4];
    __device__ __forceinline__ void load(const AlphaDev& a, const int v, const size_t at, const int n)
    {
        osum::load4<VEC>(a.weights[v] + at, n, A);
        if (MODE != BAGS_ALPHA_ENTROPY) osum::load4<VEC>(a.target[v] + at, n, t);
        const float* __restrict__ mk = a.mask[v];
        if (mk) osum::load4<VEC>(mk + at, n, m);                                             // uniform
        else {
#pragma unroll
            for (int j = 0; j < 4; ++j) m[j] = (j < n) ? 1.0f : 0.0f;
        }
    }
    __device__ __forceinline__ bool usable(const int j) const
    {
        bool ok = osum::finite(A[j]) && m[j] > 0.0f;
        if (MODE != BAGS_ALPHA_ENTROPY) ok = ok && osum::finite(t[j]);
        if (MODE == BAGS_ALPHA_BCE) ok = ok && t[j] >= 0.0f && t[j] <= 1.0f;
        return ok;
    }
    // the clamped modes: a of pixel j, and whether A is strictly inside (lo, hi)
    __device__ __forceinline__ double clamped(const AlphaDev& a, const int j, bool& inside) const
    {
        const bool low = A[j] <= a.lo, high = A[j] >= a.hi;
        inside = !low && !high;
        return (double)(low ? a.lo : (high ? a.hi : A[j]));
    }
    // l of a usable pixel
    __device__ __forceinline__ double value(const AlphaDev& a, const int j) const
    {
        if (MODE == BAGS_ALPHA_L1) return fabs((double)A[j] - (double)t[j]);
        if (MODE == BAGS_ALPHA_L2) { const double r = (double)A[j] - (double)t[j]; return r * r; }
        bool inside;
        const double x = clamped(a, j, inside);
        const double l0 = log(x), l1 = log(1.0 - x);
        if (MODE == BAGS_ALPHA_BCE) { const double tt = (double)t[j]; return -(tt * l0 + (1.0 - tt) * l1); }
        return -(x * l0 + (1.0 - x) * l1);
    }
    // dl/dA of a usable pixel
    __device__ __forceinline__ double slope(const AlphaDev& a, const int j) const
    {
        if (MODE == BAGS_ALPHA_L1) return osum::sign((double)A[j] - (double)t[j]);
        if (MODE == BAGS_ALPHA_L2) return 2.0 * ((double)A[j] - (double)t[j]);
        bool inside;
        const double x = clamped(a, j, inside);
        if (!inside) return 0.0;
        if (MODE == BAGS_ALPHA_BCE) return (x - (double)t[j]) / (x * (1.0 - x));
        return log((1.0 - x) / x);
    }
};

// Workgroup g of view v walks the quads [g span, (g + 1) span) of the view and leaves one row of partials: cnt, sum w l
template <bool VEC, int MODE>
__global__ void __launch_bounds__(ALPHA_BLOCK) alpha_sums_kernel(const AlphaDev a, double* __restrict__ partials)
{
    __shared__ double sh[ALPHA_BLOCK / 64 * ALPHA_ROW];
    const int v = blockIdx.y;
    double acc[ALPHA_ROW] = {0.0, 0.0};

    const unsigned first = min(blockIdx.x * a.span, a.nquads), last = min(first + a.span, a.nquads);       // first == last: an empty span
    for (unsigned q = first + threadIdx.x; q < last; q += ALPHA_BLOCK) {
        const size_t at = (size_t)q * 4;
        const int n = (int)min(4u, a.npix - 4u * q);
        AlphaQuad<VEC, MODE> Qd;
        Qd.load(a, v, at, n);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (!Qd.usable(j)) continue;
            const double w = (double)Qd.m[j];
            acc[0] += w; acc[1] += w * Qd.value(a, j);
        }
    }
    osum::block_sum<ALPHA_ROW, ALPHA_BLOCK / 64>(acc, sh);                                   // every lane is here
    if (threadIdx.x < ALPHA_ROW)
        partials[((size_t)v * BAGS_ALPHA_GROUPS + blockIdx.x) * ALPHA_ROW + threadIdx.x] = osum::block_total<ALPHA_ROW, ALPHA_BLOCK / 64>(sh, threadIdx.x);
}

// One workgroup per view: its BAGS_ALPHA_GROUPS partial rows, fetched by as many threads, added in index order by one thread per
// column; then loss, count and the stats row.  NOT ordered_sum.h's ordered_rows_sum: one serial chain over the rows, whose bits the
// operator has promised since it was added; a tree over the same rows rounds differently.
__global__ void __launch_bounds__(BAGS_ALPHA_GROUPS) alpha_finalize_kernel(const double* __restrict__ partials, float* __restrict__ loss,
                                                                           float* __restrict__ count, double* __restrict__ stats)
{
    __shared__ double rows[ALPHA_ROW][BAGS_ALPHA_GROUPS];
    __shared__ double total[ALPHA_ROW];
    const int v = blockIdx.x;
    const double* __restrict__ mine = partials + ((size_t)v * BAGS_ALPHA_GROUPS + threadIdx.x) * ALPHA_ROW;
#pragma unroll
    for (int c = 0; c < ALPHA_ROW; ++c) rows[c][threadIdx.x] = mine[c];
    __syncthreads();
    if (threadIdx.x < ALPHA_ROW) {
        double s = 0.0;
        for (int g = 0; g < BAGS_ALPHA_GROUPS; ++g) s += rows[threadIdx.x][g];
        total[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double cnt = total[0], sum = total[1];
    const double inv = cnt > 0.0 ? 1.0 / cnt : 0.0;                                           // (a NaN count: no usable pixel)
    loss[v] = (float)(cnt > 0.0 ? sum * inv : 0.0);
    count[v] = (float)(cnt > 0.0 ? cnt : 0.0);
    stats[(size_t)v * ALPHA_ROW] = inv;
    stats[(size_t)v * ALPHA_ROW + 1] = 0.0;
}

// dL/dA of every pixel (zeros where the pixel is not usable or the view has no usable pixel), each rounded once from double.
// a.g_weights[v] == nullptr: not wanted, nothing is stored.
template <bool VEC, int MODE>
__global__ void __launch_bounds__(ALPHA_BWD_BLOCK) alpha_bwd_kernel(const AlphaDev a, const double* __restrict__ stats,
                                                                    const float* __restrict__ g_loss)
{
    const int v = blockIdx.y;
    float* __restrict__ gA = a.g_weights[v];
    if (!gA) return;                                                                          // uniform
    const unsigned q = blockIdx.x * ALPHA_BWD_BLOCK + threadIdx.x;
    if (q >= a.nquads) return;
    const double inv = stats[(size_t)v * ALPHA_ROW];
    const double g = (double)g_loss[v];
    const size_t at = (size_t)q * 4;
    const int n = (int)min(4u, a.npix - 4u * q);
    AlphaQuad<VEC, MODE> Qd;
    Qd.load(a, v, at, n);
    float d[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        d[j] = 0.0f;
        if (!(inv > 0.0) || !Qd.usable(j)) continue;
        d[j] = (float)((g * ((double)Qd.m[j] * inv)) * Qd.slope(a, j));
    }
    osum::store4<VEC>(gA + at, n, d);
}

static AlphaDev alpha_dev(const BagsAlpha& a, float* const* g_weights)
{
    AlphaDev d{};
    d.npix = (unsigned)((long long)a.H * a.W);                                               // < 2^31: validated by the caller
    d.nquads = (d.npix + 3u) / 4u;
    d.span = (d.nquads + BAGS_ALPHA_GROUPS - 1) / BAGS_ALPHA_GROUPS;
    d.lo = a.lo; d.hi = a.hi;
    for (int k = 0; k < BAGS_MAX_POSE_ROWS; ++k) {
        const bool on = k < a.n_rows;
        d.weights[k] = on ? a.weights[k] : nullptr;
        d.target[k] = (on && a.mode != BAGS_ALPHA_ENTROPY) ? a.target[k] : nullptr;
        d.mask[k] = on ? a.mask[k] : nullptr;
        d.g_weights[k] = (on && g_weights) ? g_weights[k] : nullptr;
    }
    return d;
}

// float4 accesses: every map of every view of the call 16-byte aligned
static bool alpha_vector(const AlphaDev& d, int n_rows)
{
    uintptr_t bits = 0;
    for (int k = 0; k < n_rows; ++k)
        bits |= reinterpret_cast<uintptr_t>(d.weights[k]) | reinterpret_cast<uintptr_t>(d.target[k]) | reinterpret_cast<uintptr_t>(d.mask[k]) |
                reinterpret_cast<uintptr_t>(d.g_weights[k]);
    return (bits & 15) == 0;
}

template <typename F> static hipError_t alpha_with_mode(int mode, F f)
{
    switch (mode) {
    case BAGS_ALPHA_BCE: return f(std::integral_constant<int, BAGS_ALPHA_BCE>{});
    case BAGS_ALPHA_L1: return f(std::integral_constant<int, BAGS_ALPHA_L1>{});
    case BAGS_ALPHA_L2: return f(std::integral_constant<int, BAGS_ALPHA_L2>{});
    default: return f(std::integral_constant<int, BAGS_ALPHA_ENTROPY>{});
    }
}

// the struct is validated by the caller (api.hip); partials: BAGS_MAX_POSE_ROWS * BAGS_ALPHA_GROUPS rows of 2 doubles
hipError_t launch_alpha_fwd(const BagsAlpha& a, double* partials, float* loss, float* count, double* stats, hipStream_t st)
{
    const AlphaDev d = alpha_dev(a, nullptr);
    const hipError_t e = with_bool(alpha_vector(d, a.n_rows), [&](auto VEC) { return alpha_with_mode(a.mode, [&](auto MODE) {
        hipLaunchKernelGGL((alpha_sums_kernel<decltype(VEC)::value, decltype(MODE)::value>), dim3(BAGS_ALPHA_GROUPS, a.n_rows), dim3(ALPHA_BLOCK),
                           0, st, d, partials);
        return hipGetLastError(); }); });
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(alpha_finalize_kernel, dim3(a.n_rows), dim3(BAGS_ALPHA_GROUPS), 0, st, partials, loss, count, stats);
    return hipGetLastError();
}

// g_weights: n_rows pointers of which any may be NULL (at least one is not)
hipError_t launch_alpha_bwd(const BagsAlpha& a, const double* stats, const float* g_loss, float* const* g_weights, hipStream_t st)
{
    const AlphaDev d = alpha_dev(a, g_weights);
    const unsigned blocks = (d.nquads + ALPHA_BWD_BLOCK - 1) / ALPHA_BWD_BLOCK;
    return with_bool(alpha_vector(d, a.n_rows), [&](auto VEC) { return alpha_with_mode(a.mode, [&](auto MODE) {
        hipLaunchKernelGGL((alpha_bwd_kernel<decltype(VEC)::value, decltype(MODE)::value>), dim3(blocks, a.n_rows), dim3(ALPHA_BWD_BLOCK), 0, st,
                           d, stats, g_loss);
        return hipGetLastError(); }); });
}
