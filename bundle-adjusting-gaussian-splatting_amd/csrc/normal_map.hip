// normal_map.hip -- a rendered normal map N = sum w_i n_i (render_normals) held to a target normal map: a monocular prior, or the
// normals of the rendered depth (depth_to_normal), which makes it the normal-consistency term.  Per pixel, with the weights map A,
// target p, pixel weight m (NULL: 1), min_weight and min_norm:
//     valid = A >= min_weight and |N|^2 finite and > min_norm^2 and m > 0 and |p|^2 finite and > 0.25
//     nh = N / |N| ;  ph = p / |p| ;  w = m on valid pixels ;  cnt = sum w
//     cos:  l = 1 - nh . ph        l1:  l = |nh - ph|_1   (sign(0) = 0)
//     L = sum w l / cnt            cnt <= 0: L = 0 and all gradients zero
//     dL/dN = (w / cnt) (u - nh (nh . u)) / |N| ,  u = -ph (cos) or sign(nh - ph) (l1)
// Opposing normals cancel in the blend, so a short N is not a direction: min_norm.  A >= min_weight is a float32 comparison;
// everything after the loads is in double, the gradient rounded once.  There is no gradient to A (a decision), p or m.
//
// The shape is depth_prior.hip's: a thread takes a quad of four consecutive pixels of one image row, as one float4 per plane where
// W % 4 == 0 and every base is 16-byte aligned, element by element otherwise (the same operations, and -ffp-contract=off: the same
// bits).  The views of a call are grid dimension y.  A view has depth_prior_slots(H, W) workgroups whatever the number of views;
// each leaves one row of 2 doubles (cnt, sum w l), and the finalize kernel adds a view's rows in row order (both: ordered_sum.h): a
// view's loss, count and gradients are the same bits in a 16-view call and in a call of its own.  No atomics, no memset.
#include "ordered_sum.h"

#define NM_BLOCK BAGS_DEPTH_PRIOR_BLOCK
#define NM_ROW BAGS_NORMAL_MAP_STATS                 // doubles per partial row (cnt, sum w l) and per stats row (1/cnt or 0, unused)
#define NM_PRIOR_MIN_SQ 0.25

struct NmDev {
    int H, W, Q;                                     // Q: quads per image row
    unsigned nquads, ntiles;                         // per view; a tile is NM_BLOCK quads
    size_t plane;                                    // H * W
    float min_weight;
    double min_norm_sq;
    const float* normal[BAGS_MAX_POSE_ROWS];
    const float* weights[BAGS_MAX_POSE_ROWS];
    const float* prior[BAGS_MAX_POSE_ROWS];
    const float* mask[BAGS_MAX_POSE_ROWS];           // any of them NULL: 1
    float* g_normal[BAGS_MAX_POSE_ROWS];             // backward: any of them NULL
};

// the maps of a quad; a lane past the end of a short quad has A = 0 and N = 0: not valid (min_weight > 0)
template <bool VEC> struct NmQuad {
    float N[3][4], A[4], p[3][4], m[4];
    __device__ __forceinline__ void load(const NmDev& a, const int v, const size_t at, const int n)
    {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            osum::load4<VEC>(a.normal[v] + c * a.plane + at, n, N[c]);
            osum::load4<VEC>(a.prior[v] + c * a.plane + at, n, p[c]);
        }
        osum::load4<VEC>(a.weights[v] + at, n, A);
        const float* __restrict__ mk = a.mask[v];
        if (mk) osum::load4<VEC>(mk + at, n, m);                                             // uniform
        else {
#pragma unroll
            for (int j = 0; j < 4; ++j) m[j] = 1.0f;
        }
    }
    // valid: nh, ph, 1/|N| of pixel j
    __device__ __forceinline__ bool unit(const NmDev& a, const int j, double (&nh)[3], double (&ph)[3], double& inv_len) const
    {
        const double n0 = (double)N[0][j], n1 = (double)N[1][j], n2 = (double)N[2][j];
        const double p0 = (double)p[0][j], p1 = (double)p[1][j], p2 = (double)p[2][j];
        const double nn = n0 * n0 + n1 * n1 + n2 * n2, pp = p0 * p0 + p1 * p1 + p2 * p2;
        const bool ok = A[j] >= a.min_weight && osum::finite(nn) && nn > a.min_norm_sq && m[j] > 0.0f && osum::finite(pp) && pp > NM_PRIOR_MIN_SQ;
        if (!ok) return false;
        const double ln = sqrt(nn), lp = sqrt(pp);
        nh[0] = n0 / ln; nh[1] = n1 / ln; nh[2] = n2 / ln;
        ph[0] = p0 / lp; ph[1] = p1 / lp; ph[2] = p2 / lp;
        inv_len = 1.0 / ln;
        return true;
    }
};

// Workgroup `slot` of view v walks the tiles slot, slot + nslots, ... and leaves one row of partials: cnt, sum w l
template <bool VEC, bool L1>
__global__ void __launch_bounds__(NM_BLOCK) normal_map_sums_kernel(const NmDev a, double* __restrict__ partials)
{
    __shared__ double sh[NM_BLOCK / 64 * NM_ROW];
    const int v = blockIdx.y;
    double acc[NM_ROW] = {0.0, 0.0};

    for (unsigned tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {                   // uniform
        const unsigned q = tile * NM_BLOCK + threadIdx.x;
        if (q >= a.nquads) continue;
        const int y = (int)(q / (unsigned)a.Q), x0 = 4 * (int)(q - (unsigned)y * (unsigned)a.Q);
        const int n = VEC ? 4 : min(4, a.W - x0);                                            // (VEC: W % 4 == 0)
        NmQuad<VEC> Qd;
        Qd.load(a, v, (size_t)y * a.W + x0, n);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double nh[3], ph[3], inv_len;
            if (!Qd.unit(a, j, nh, ph, inv_len)) continue;
            const double w = (double)Qd.m[j];
            double l;
            if (L1) l = fabs(nh[0] - ph[0]) + fabs(nh[1] - ph[1]) + fabs(nh[2] - ph[2]);
            else l = 1.0 - (nh[0] * ph[0] + nh[1] * ph[1] + nh[2] * ph[2]);
            acc[0] += w; acc[1] += w * l;
        }
    }
    osum::block_sum<NM_ROW>(acc, sh);                                                        // every lane is here
    if (threadIdx.x < NM_ROW) partials[((size_t)v * gridDim.x + blockIdx.x) * NM_ROW + threadIdx.x] = osum::block_total<NM_ROW>(sh, threadIdx.x);
}

// One workgroup per view: its nslots partial rows added in slot order (ordered_sum.h), then loss, count and the stats row.
__global__ void __launch_bounds__(256) normal_map_finalize_kernel(const int nslots, const double* __restrict__ partials,
                                                                  float* __restrict__ loss, float* __restrict__ count,
                                                                  double* __restrict__ stats)
{
    __shared__ double sh[4 * NM_ROW];
    const int v = blockIdx.x;
    double S[NM_ROW];
    osum::ordered_rows_sum<NM_ROW>(partials + (size_t)v * nslots * NM_ROW, nslots, NM_ROW, sh, S);
    if (threadIdx.x != 0) return;
    const double cnt = S[0], sum = S[1];
    const double inv = cnt > 0.0 ? 1.0 / cnt : 0.0;                                           // (a NaN count: no valid pixel)
    loss[v] = (float)(cnt > 0.0 ? sum * inv : 0.0);
    count[v] = (float)(cnt > 0.0 ? cnt : 0.0);
    stats[(size_t)v * NM_ROW] = inv;
    stats[(size_t)v * NM_ROW + 1] = 0.0;
}

// dL/dN of every pixel (zeros where the pixel is not valid or the view has no valid pixel), each rounded once from double.
// a.g_normal[v] == nullptr: not wanted, nothing is stored.
template <bool VEC, bool L1>
__global__ void __launch_bounds__(NM_BLOCK) normal_map_bwd_kernel(const NmDev a, const double* __restrict__ stats,
                                                                  const float* __restrict__ g_loss)
{
    const int v = blockIdx.y;
    float* __restrict__ gN = a.g_normal[v];
    if (!gN) return;                                                                          // uniform
    const unsigned q = blockIdx.x * NM_BLOCK + threadIdx.x;
    if (q >= a.nquads) return;
    const double inv = stats[(size_t)v * NM_ROW];
    const double g = (double)g_loss[v];
    const int y = (int)(q / (unsigned)a.Q), x0 = 4 * (int)(q - (unsigned)y * (unsigned)a.Q);
    const int n = VEC ? 4 : min(4, a.W - x0);
    const size_t at = (size_t)y * a.W + x0;
    NmQuad<VEC> Qd;
    Qd.load(a, v, at, n);
    float d[3][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        d[0][j] = 0.0f; d[1][j] = 0.0f; d[2][j] = 0.0f;
        double nh[3], ph[3], inv_len;
        if (!(inv > 0.0) || !Qd.unit(a, j, nh, ph, inv_len)) continue;
        double u[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) u[c] = L1 ? osum::sign(nh[c] - ph[c]) : -ph[c];
        const double nu = nh[0] * u[0] + nh[1] * u[1] + nh[2] * u[2];
        const double k = (g * ((double)Qd.m[j] * inv)) * inv_len;
#pragma unroll
        for (int c = 0; c < 3; ++c) d[c][j] = (float)(k * (u[c] - nh[c] * nu));
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) osum::store4<VEC>(gN + c * a.plane + at, n, d[c]);
}

static NmDev nm_dev(const BagsNormalMap& a, float* const* g_normal)
{
    NmDev d{};
    d.H = a.H; d.W = a.W; d.Q = (a.W + 3) / 4;
    d.nquads = (unsigned)((long long)a.H * d.Q);
    d.ntiles = (d.nquads + NM_BLOCK - 1) / NM_BLOCK;
    d.plane = (size_t)a.H * a.W;
    d.min_weight = a.min_weight;
    d.min_norm_sq = (double)a.min_norm * (double)a.min_norm;
    for (int k = 0; k < BAGS_MAX_POSE_ROWS; ++k) {
        const bool on = k < a.n_rows;
        d.normal[k] = on ? a.normal[k] : nullptr;
        d.weights[k] = on ? a.weights[k] : nullptr;
        d.prior[k] = on ? a.prior[k] : nullptr;
        d.mask[k] = on ? a.mask[k] : nullptr;
        d.g_normal[k] = (on && g_normal) ? g_normal[k] : nullptr;
    }
    return d;
}

// float4 accesses: whole quads (so every plane starts on a quad too) and every map of every view 16-byte aligned
static bool nm_vector(const NmDev& d, int n_rows)
{
    if (d.W % 4 != 0) return false;
    uintptr_t bits = 0;
    for (int k = 0; k < n_rows; ++k)
        bits |= reinterpret_cast<uintptr_t>(d.normal[k]) | reinterpret_cast<uintptr_t>(d.weights[k]) | reinterpret_cast<uintptr_t>(d.prior[k]) |
                reinterpret_cast<uintptr_t>(d.mask[k]) | reinterpret_cast<uintptr_t>(d.g_normal[k]);
    return (bits & 15) == 0;
}

// the struct is validated by the caller (api.hip); partials: n_rows * depth_prior_slots(H, W) rows of 2 doubles
hipError_t launch_normal_map_fwd(const BagsNormalMap& a, double* partials, float* loss, float* count, double* stats, hipStream_t st)
{
    const NmDev d = nm_dev(a, nullptr);
    const int nslots = depth_prior_slots(a.H, a.W);
    const hipError_t e = with_bool(nm_vector(d, a.n_rows), [&](auto VEC) { return with_bool(a.mode == BAGS_NORMAL_PRIOR_L1, [&](auto L1) {
        hipLaunchKernelGGL((normal_map_sums_kernel<decltype(VEC)::value, decltype(L1)::value>), dim3(nslots, a.n_rows), dim3(NM_BLOCK), 0, st,
                           d, partials);
        return hipGetLastError(); }); });
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(normal_map_finalize_kernel, dim3(a.n_rows), dim3(256), 0, st, nslots, partials, loss, count, stats);
    return hipGetLastError();
}

// g_normal: n_rows pointers of which any may be NULL (at least one is not)
hipError_t launch_normal_map_bwd(const BagsNormalMap& a, const double* stats, const float* g_loss, float* const* g_normal, hipStream_t st)
{
    const NmDev d = nm_dev(a, g_normal);
    return with_bool(nm_vector(d, a.n_rows), [&](auto VEC) { return with_bool(a.mode == BAGS_NORMAL_PRIOR_L1, [&](auto L1) {
        hipLaunchKernelGGL((normal_map_bwd_kernel<decltype(VEC)::value, decltype(L1)::value>), dim3(d.ntiles, a.n_rows), dim3(NM_BLOCK), 0, st,
                           d, stats, g_loss);
        return hipGetLastError(); }); });
}
