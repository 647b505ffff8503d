// depth_prior.hip -- a depth prior on the rasterizer's depth map D = sum w_i z_i and weights map A = 1 - T_final: the Pearson
// (scale- and shift-invariant) loss of sparse-view and pose-free splatting, and upstream 3DGS's depth_l1_weight term with its
// per-image depth_params (a, b), one row of an (N,2) table.  Per pixel, with prior p, pixel weight m (NULL: 1) and min_weight:
//     valid = m > 0 and A >= min_weight and D > 0 and p > 0        (a NaN prior fails p > 0)
//     x = D / A  (space depth)   or   x = A / D  (space inverse), ONE float32 division
//     w = m on valid pixels, n = sum w
//     l1:       r = x - (a*p + b) ;  L = sum w|r| / n                                   (sign(0) = 0)
//     pearson:  L = 1 - rho ;  rho = C / sqrt(Vx*Vp) ;  Vx = sum w x^2 / n - (sum w x / n)^2, Vp likewise,
//               C = sum w x p / n - (sum w x / n)(sum w p / n)
//               degenerate (L = 0, zero gradients): n <= 0, Vx <= 1e-12 * sum w x^2 / n, Vp <= 1e-12 * sum w p^2 / n
//     dL/dx = -(w/n) [(p - pbar)/sqrt(Vx*Vp) - rho (x - xbar)/Vx]    (pearson) ;   w sign(r) / n    (l1)
//     dL/da = -sum w sign(r) p / n ;  dL/db = -sum w sign(r) / n
// x is a float32 quantity (the maps are float32).  Everything after it -- every product, r, every sum, the gradient up to its one
// final rounding -- is in double: a product of two float32 values is exact there, so a constant prior has Vp of the order of
// 1e-16 of its mean square and the 1e-12 test catches it (products rounded to float32 would leave 6e-8).
//
// A thread takes a quad: four consecutive pixels of one image row (the last quad of a row may be short), as one float4 per map
// where W % 4 == 0 and every base is 16-byte aligned, element by element otherwise.  Both instances spell the same operations and
// the file is compiled with -ffp-contract=off, so they give the same bits.  The views of a call are grid dimension y; their
// pointers and table rows arrive by value.
//
// The sums of a view: a lane adds its terms in double; after its last tile the workgroup adds its lanes (ordered_sum.h) and leaves
// one row of 8 doubles, the columns it has no sum for written as zeros.  A view has depth_prior_slots(H, W) workgroups whatever the
// number of views, and the finalize kernel adds its rows in row order (ordered_sum.h): a view's loss, count, stats and gradients are
// the same bits in a 16-view call and in a call of its own.  No atomics, no memset.
#include "ordered_sum.h"

#define DP_BLOCK BAGS_DEPTH_PRIOR_BLOCK
#define DP_ROW 8                                     // doubles per partial row and per stats row
// a stats row (the backward reads it): xbar, pbar, 1/sqrt(Vx*Vp), rho/Vx, 1/n, sum w sign(r) p, sum w sign(r), degenerate flag
enum { DP_XBAR = 0, DP_PBAR = 1, DP_K1 = 2, DP_K2 = 3, DP_INV_N = 4, DP_SUM_SP = 5, DP_SUM_S = 6, DP_DEGENERATE = 7 };

struct DpDev {
    int H, W, Q;                                     // Q: quads per image row
    unsigned nquads, ntiles;                         // per view; a tile is DP_BLOCK quads
    int inverse;                                     // x = A / D
    float min_weight;
    const float* table;                              // (N,2) or NULL: a = 1, b = 0
    int N, n_rows;
    int rows[BAGS_MAX_POSE_ROWS];
    const float* depth[BAGS_MAX_POSE_ROWS];
    const float* weights[BAGS_MAX_POSE_ROWS];
    const float* prior[BAGS_MAX_POSE_ROWS];
    const float* mask[BAGS_MAX_POSE_ROWS];           // any of them NULL: 1
    float* g_depth[BAGS_MAX_POSE_ROWS];              // backward: any of them NULL
    float* g_weights[BAGS_MAX_POSE_ROWS];
};

// the four maps of a quad; a lane past the end of a short quad has D = 0: not valid
template <bool VEC> struct DpQuad {
    float D[4], A[4], p[4], m[4];
    __device__ __forceinline__ void load(const DpDev& a, const int v, const size_t at, const int n)
    {
        osum::load4<VEC>(a.depth[v] + at, n, D);
        osum::load4<VEC>(a.weights[v] + at, n, A);
        osum::load4<VEC>(a.prior[v] + at, n, p);
        const float* __restrict__ mk = a.mask[v];
        if (mk) osum::load4<VEC>(mk + at, n, m);                                             // uniform
        else {
#pragma unroll
            for (int j = 0; j < 4; ++j) m[j] = 1.0f;
        }
    }
    __device__ __forceinline__ bool valid(const DpDev& a, const int j) const
    {
        return m[j] > 0.0f && A[j] >= a.min_weight && D[j] > 0.0f && p[j] > 0.0f;
    }
};

__device__ __forceinline__ void dp_ab(const DpDev& a, const int v, double& ca, double& cb)
{
    ca = 1.0; cb = 0.0;
    if (a.table) { ca = (double)a.table[2 * (size_t)a.rows[v]]; cb = (double)a.table[2 * (size_t)a.rows[v] + 1]; }
}

// Workgroup `slot` of view v walks the tiles slot, slot + nslots, ... and leaves one row of partials:
//     n, then  sum wx, sum wp, sum wx^2, sum wp^2, sum wxp  (pearson)   or   sum w|r|, sum w sign(r) p, sum w sign(r)  (L1)
template <bool VEC, bool L1>
__global__ void __launch_bounds__(DP_BLOCK) depth_prior_sums_kernel(const DpDev a, double* __restrict__ partials)
{
    constexpr int NV = L1 ? 4 : 6;
    __shared__ double sh[DP_BLOCK / 64 * DP_ROW];
    const int v = blockIdx.y;
    double ca, cb;
    dp_ab(a, v, ca, cb);
    double acc[NV];
#pragma unroll
    for (int t = 0; t < NV; ++t) acc[t] = 0.0;

    for (unsigned tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {                   // uniform
        const unsigned q = tile * DP_BLOCK + threadIdx.x;
        if (q >= a.nquads) continue;
        const int y = (int)(q / (unsigned)a.Q), x0 = 4 * (int)(q - (unsigned)y * (unsigned)a.Q);
        const int n = VEC ? 4 : min(4, a.W - x0);                                            // (VEC: W % 4 == 0)
        DpQuad<VEC> Qd;
        Qd.load(a, v, (size_t)y * a.W + x0, n);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (!Qd.valid(a, j)) continue;
            const float xf = a.inverse ? Qd.A[j] / Qd.D[j] : Qd.D[j] / Qd.A[j];
            const double x = (double)xf, p = (double)Qd.p[j], w = (double)Qd.m[j];
            acc[0] += w;
            if (L1) {
                const double r = x - (ca * p + cb);
                const double ws = w * osum::sign(r);
                acc[1] += w * fabs(r); acc[2] += ws * p; acc[3] += ws;
            } else {
                const double wx = w * x, wp = w * p;
                acc[1] += wx; acc[2] += wp; acc[3] += wx * x; acc[4] += wp * p; acc[5] += wx * p;
            }
        }
    }
    osum::block_sum<NV>(acc, sh);                                                            // every lane is here
    if (threadIdx.x < DP_ROW)
        partials[((size_t)v * gridDim.x + blockIdx.x) * DP_ROW + threadIdx.x] = ((int)threadIdx.x < NV) ? osum::block_total<NV>(sh, threadIdx.x) : 0.0;
}

// One workgroup per view: its nslots partial rows added in slot order (ordered_sum.h), then loss, count and the stats row.
__global__ void __launch_bounds__(256) depth_prior_finalize_kernel(const int l1, const int nslots, const double* __restrict__ partials,
                                                                   float* __restrict__ loss, float* __restrict__ count,
                                                                   double* __restrict__ stats)
{
    __shared__ double sh[4 * DP_ROW];
    const int v = blockIdx.x;
    double S[6];
    osum::ordered_rows_sum<6>(partials + (size_t)v * nslots * DP_ROW, nslots, DP_ROW, sh, S);
    if (threadIdx.x != 0) return;
    const double n = S[0];
    const double inv_n = n > 0.0 ? 1.0 / n : 0.0;
    double out[DP_ROW] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0};
    double L = 0.0;
    if (l1) {
        if (n > 0.0) {
            L = S[1] * inv_n;
            out[DP_INV_N] = inv_n; out[DP_SUM_SP] = S[2]; out[DP_SUM_S] = S[3]; out[DP_DEGENERATE] = 0.0;
        }
    } else if (n > 0.0) {
        const double mx = S[1] * inv_n, mp = S[2] * inv_n, ex2 = S[3] * inv_n, ep2 = S[4] * inv_n;
        const double Vx = ex2 - mx * mx, Vp = ep2 - mp * mp, C = S[5] * inv_n - mx * mp;
        if (Vx > 1e-12 * ex2 && Vp > 1e-12 * ep2) {                                           // (a NaN sum is degenerate)
            const double k1 = 1.0 / sqrt(Vx * Vp), rho = C * k1;
            L = 1.0 - rho;
            out[DP_XBAR] = mx; out[DP_PBAR] = mp; out[DP_K1] = k1; out[DP_K2] = rho / Vx; out[DP_INV_N] = inv_n; out[DP_DEGENERATE] = 0.0;
        }
    }
    loss[v] = (float)L;
    count[v] = (float)n;
#pragma unroll
    for (int c = 0; c < DP_ROW; ++c) stats[(size_t)v * DP_ROW + c] = out[c];
}

// dL/dD and dL/dA of every pixel (zeros where the pixel is not valid or the view is degenerate), each rounded once from double.
// a.g_depth[v] / a.g_weights[v] == nullptr: not wanted, nothing is stored; what is stored is the same bits whichever is wanted.
template <bool VEC, bool L1>
__global__ void __launch_bounds__(DP_BLOCK) depth_prior_bwd_kernel(const DpDev a, const double* __restrict__ stats,
                                                                   const float* __restrict__ g_loss)
{
    const int v = blockIdx.y;
    const unsigned q = blockIdx.x * DP_BLOCK + threadIdx.x;
    if (q >= a.nquads) return;
    const double* __restrict__ S = stats + (size_t)v * DP_ROW;
    const bool live = S[DP_DEGENERATE] == 0.0;                                                // uniform
    const double g = (double)g_loss[v], inv_n = S[DP_INV_N];
    const double xbar = S[DP_XBAR], pbar = S[DP_PBAR], k1 = S[DP_K1], k2 = S[DP_K2];
    double ca, cb;
    dp_ab(a, v, ca, cb);
    const int y = (int)(q / (unsigned)a.Q), x0 = 4 * (int)(q - (unsigned)y * (unsigned)a.Q);
    const int n = VEC ? 4 : min(4, a.W - x0);
    const size_t at = (size_t)y * a.W + x0;
    DpQuad<VEC> Qd;
    Qd.load(a, v, at, n);
    float dD[4], dA[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        dD[j] = 0.0f; dA[j] = 0.0f;
        if (!live || !Qd.valid(a, j)) continue;
        const float numf = a.inverse ? Qd.A[j] : Qd.D[j], denf = a.inverse ? Qd.D[j] : Qd.A[j];
        const float xf = numf / denf;                                                         // the forward's x
        const double x = (double)xf, p = (double)Qd.p[j], w = (double)Qd.m[j];
        double gx;
        if (L1) gx = (w * osum::sign(x - (ca * p + cb))) * inv_n;
        else gx = -(w * inv_n) * ((p - pbar) * k1 - k2 * (x - xbar));
        gx *= g;
        const double num = (double)numf, den = (double)denf;
        const float gnum = (float)(gx / den), gden = (float)(-(gx * num) / (den * den));      // x = num / den
        dD[j] = a.inverse ? gden : gnum;
        dA[j] = a.inverse ? gnum : gden;
    }
    float* __restrict__ gD = a.g_depth[v];
    float* __restrict__ gA = a.g_weights[v];
    if (gD) osum::store4<VEC>(gD + at, n, dD);                                                // uniform
    if (gA) osum::store4<VEC>(gA + at, n, dA);
}

// The dense (N,2) gradient of the L1 table, every element: row rows[v] gets g_v * (-sum w sign(r) p / n, -sum w sign(r) / n) from
// the view's stats row, every row that is not listed exact zeros.
__global__ void __launch_bounds__(256) depth_prior_table_kernel(const DpDev a, const double* __restrict__ stats, const float* __restrict__ g_loss,
                                                                float* __restrict__ g_table)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= a.N) return;
    float ga = 0.0f, gb = 0.0f;
#pragma unroll
    for (int k = 0; k < BAGS_MAX_POSE_ROWS; ++k)
        if (k < a.n_rows && a.rows[k] == r) {
            const double* __restrict__ S = stats + (size_t)k * DP_ROW;
            const double g = (double)g_loss[k];
            ga = (float)(-(g * S[DP_SUM_SP]) * S[DP_INV_N]);
            gb = (float)(-(g * S[DP_SUM_S]) * S[DP_INV_N]);
        }
    g_table[2 * (size_t)r] = ga;
    g_table[2 * (size_t)r + 1] = gb;
}

static inline unsigned dp_quads(int H, int W) { return (unsigned)((long long)H * ((W + 3) / 4)); }
static inline unsigned dp_tiles(int H, int W) { return (dp_quads(H, W) + DP_BLOCK - 1) / DP_BLOCK; }
// workgroups (= partial rows) per view of the sums kernel: a function of the image size alone
int depth_prior_slots(int H, int W)
{
    const unsigned tiles = dp_tiles(H, W);
    const unsigned want = (tiles + BAGS_DEPTH_PRIOR_TILES_PER_SLOT - 1) / BAGS_DEPTH_PRIOR_TILES_PER_SLOT;
    const unsigned floor_ = BAGS_DEPTH_PRIOR_MIN_SLOTS;
    const unsigned n = want > floor_ ? want : floor_;
    return (int)(tiles < n ? tiles : n);
}

static DpDev dp_dev(const BagsDepthPrior& a, float* const* g_depth, float* const* g_weights)
{
    DpDev d{};
    d.H = a.H; d.W = a.W; d.Q = (a.W + 3) / 4;
    d.nquads = dp_quads(a.H, a.W); d.ntiles = dp_tiles(a.H, a.W);
    d.inverse = a.space == BAGS_DEPTH_PRIOR_INVERSE;
    d.min_weight = a.min_weight;
    d.table = a.table; d.N = a.table ? a.N : 0; d.n_rows = a.n_rows;
    for (int k = 0; k < BAGS_MAX_POSE_ROWS; ++k) {
        const bool on = k < a.n_rows;
        d.rows[k] = (on && a.table) ? a.rows[k] : -1;
        d.depth[k] = on ? a.depth[k] : nullptr;
        d.weights[k] = on ? a.weights[k] : nullptr;
        d.prior[k] = on ? a.prior[k] : nullptr;
        d.mask[k] = on ? a.mask[k] : nullptr;
        d.g_depth[k] = (on && g_depth) ? g_depth[k] : nullptr;
        d.g_weights[k] = (on && g_weights) ? g_weights[k] : nullptr;
    }
    return d;
}

// float4 accesses: whole quads and every map of every view 16-byte aligned
static bool dp_vector(const DpDev& d)
{
    if (d.W % 4 != 0) return false;
    uintptr_t bits = 0;
    for (int k = 0; k < d.n_rows; ++k)
        bits |= reinterpret_cast<uintptr_t>(d.depth[k]) | reinterpret_cast<uintptr_t>(d.weights[k]) | reinterpret_cast<uintptr_t>(d.prior[k]) |
                reinterpret_cast<uintptr_t>(d.mask[k]) | reinterpret_cast<uintptr_t>(d.g_depth[k]) | reinterpret_cast<uintptr_t>(d.g_weights[k]);
    return (bits & 15) == 0;
}

// the struct is validated by the caller (api.hip); partials: n_rows * depth_prior_slots(H, W) rows of 8 doubles
hipError_t launch_depth_prior_fwd(const BagsDepthPrior& a, double* partials, float* loss, float* count, double* stats, hipStream_t st)
{
    const DpDev d = dp_dev(a, nullptr, nullptr);
    const int nslots = depth_prior_slots(a.H, a.W);
    const bool l1 = a.mode == BAGS_DEPTH_PRIOR_L1;
    const hipError_t e = with_bool(dp_vector(d), [&](auto VEC) { return with_bool(l1, [&](auto L1) {
        hipLaunchKernelGGL((depth_prior_sums_kernel<decltype(VEC)::value, decltype(L1)::value>), dim3(nslots, a.n_rows), dim3(DP_BLOCK), 0, st,
                           d, partials);
        return hipGetLastError(); }); });
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(depth_prior_finalize_kernel, dim3(a.n_rows), dim3(256), 0, st, l1 ? 1 : 0, nslots, partials, loss, count, stats);
    return hipGetLastError();
}

// g_depth / g_weights: NULL or n_rows pointers of which any may be NULL; g_table: NULL or (N,2)
hipError_t launch_depth_prior_bwd(const BagsDepthPrior& a, const double* stats, const float* g_loss, float* const* g_depth,
                                  float* const* g_weights, float* g_table, hipStream_t st)
{
    const DpDev d = dp_dev(a, g_depth, g_weights);
    bool pixels = false;
    for (int k = 0; k < d.n_rows; ++k) pixels |= d.g_depth[k] != nullptr || d.g_weights[k] != nullptr;
    if (pixels) {
        const hipError_t e = with_bool(dp_vector(d), [&](auto VEC) { return with_bool(a.mode == BAGS_DEPTH_PRIOR_L1, [&](auto L1) {
            hipLaunchKernelGGL((depth_prior_bwd_kernel<decltype(VEC)::value, decltype(L1)::value>), dim3(d.ntiles, a.n_rows), dim3(DP_BLOCK), 0, st,
                               d, stats, g_loss);
            return hipGetLastError(); }); });
        if (e != hipSuccess) return e;
    }
    if (!g_table) return hipSuccess;
    hipLaunchKernelGGL(depth_prior_table_kernel, dim3((unsigned)((a.N + 255) / 256)), dim3(256), 0, st, d, stats, g_loss, g_table);
    return hipGetLastError();
}
