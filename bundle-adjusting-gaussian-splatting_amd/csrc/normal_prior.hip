// normal_prior.hip -- a normal prior on the rasterizer's depth map D = sum w_i z_i and weights map A = 1 - T_final: the normals of
// the rendered depth by central differences, held to a prior normal map.  Per view: maps D, A (H,W), a pinhole (fx, fy, cx, cy) in
// pixels, prior normals p (3,H,W) in the camera frame of the operator's view space (x right, y down, z forward), an optional pixel
// weight m >= 0 (H,W) (NULL: 1).
//     solid(u,v)  = A >= min_weight  and  D > 0
//     z           = D / A                      one division in the dtype of the maps; everything after it in float64
//     P(u,v)      = z * ((u - cx)/fx, (v - cy)/fy, 1)
//     dx = P(u+1,v) - P(u-1,v) ;  dy = P(u,v+1) - P(u,v-1)          (central differences, as 2DGS's depth_to_normal)
//     N  = dy x dx ;  q = |N|^2 ;  n = N / sqrt(q)                   (faces the camera: n_z < 0 for a fronto-parallel wall)
//     geometric(u,v) = the pixel and its four neighbours are inside the image and solid,
//                      |z(u+1,v) - z(u-1,v)| <= max_jump * z(u,v)  and  |z(u,v+1) - z(u,v-1)| <= max_jump * z(u,v),
//                      q is a positive finite number
//     valid(u,v)  = geometric  and  m > 0  and  |p|^2 is finite and > 0.25      (a zero or NaN prior: "no prior here")
//     ph = p / |p| ;  w = m on valid pixels ;  cnt = sum w
//     mode="cos":  l = 1 - n . ph          mode="l1":  l = |n - ph|_1   (sign(0) = 0)
//     L_v = sum w l / cnt                  cnt <= 0 (also every image with H < 3 or W < 3): L_v = 0, all gradients zero, never NaN
// max_jump = inf switches the guard off.  Validity and the guard are decisions, not differentiated through; invalid pixels get
// exact-zero gradients.  The pinhole is constant data: no gradient to it.  Backward, with s = cot_v * w_c / cnt_v, g = dl/dn (-ph
// for cos, sign(n - ph) for l1) and G = s * (g - n (n . g)) / sqrt(q):
//     dL/ddy = dx x G ;   dL/ddx = G x dy
//     dL/dP(u+1,v) += dL/ddx ;  dL/dP(u-1,v) -= dL/ddx ;  dL/dP(u,v+1) += dL/ddy ;  dL/dP(u,v-1) -= dL/ddy
//     dL/dz = ray . dL/dP ,  ray = ((u-cx)/fx, (v-cy)/fy, 1) ;   dL/dD = dL/dz / A ;   dL/dA = -(z / A) dL/dz
// The centre pixel's own z enters only the guard.
//
// A workgroup of 256 threads takes a tile of NP_TW x NP_TH = 32 x 8 pixels; lane l of a wave is pixel (l % 32, l / 32) of the
// wave's two rows, so a wave reads two 128-byte segments of a map and consecutive LDS words.  z is staged in LDS as a float with
// the halo the kernel needs (one pixel forward, two backward); a pixel that is not solid or not inside the image is staged as -1
// (a solid z is never negative), which is the `solid` flag.  The rays (u - cx)/fx of the tile's columns and (v - cy)/fy of its rows
// are staged beside it, one double division each, and 1/sqrt(q), 1/|p| and 1/A are formed once and multiplied with: the kernels are
// bound by their double arithmetic, and a double division costs some ten multiplies.  The views of a call are grid dimension z;
// their pointers and pinholes arrive by value.  The file is compiled with -ffp-contract=off: only the operations it spells.
//
// The sums of a view: a lane holds w l and w of its one pixel in double, and the workgroup adds its lanes and leaves one row of 2
// doubles.  A view has tiles_x * tiles_y workgroups whatever the number of views, and the finalize kernel adds its rows in row order
// (both: ordered_sum.h): a view's loss, count, stats and gradients are the same bits in a 16-view call and in a call of its own.  No
// atomics, no memset.
#include "ordered_sum.h"

#define NP_TW BAGS_NORMAL_PRIOR_TILE_W
#define NP_TH BAGS_NORMAL_PRIOR_TILE_H
#define NP_BLOCK (NP_TW * NP_TH)
#define NP_ROW BAGS_NORMAL_PRIOR_STATS               // doubles per partial row and per stats row: (sum w l, sum w) / (1/cnt, cnt)
static_assert(NP_BLOCK == 256, "four waves: block_sum's default");

struct NpDev {
    int H, W;
    int l1;
    float min_weight;
    double max_jump;
    int n_rows;
    double pinhole[BAGS_MAX_POSE_ROWS][4];
    const float* depth[BAGS_MAX_POSE_ROWS];
    const float* weights[BAGS_MAX_POSE_ROWS];
    const float* prior[BAGS_MAX_POSE_ROWS];
    const float* mask[BAGS_MAX_POSE_ROWS];           // any of them NULL: 1
    float* g_depth[BAGS_MAX_POSE_ROWS];              // backward: any of them NULL
    float* g_weights[BAGS_MAX_POSE_ROWS];
};

// z of pixel (u, v) as it is staged: D / A in float32 where the pixel is inside the image and solid, -1 elsewhere
__device__ __forceinline__ float np_stage(const float* __restrict__ D, const float* __restrict__ A, const int H, const int W,
                                          const float min_weight, const int u, const int v)
{
    if (u < 0 || v < 0 || u >= W || v >= H) return -1.0f;
    const size_t at = (size_t)v * W + u;
    const float d = D[at], a = A[at];
    return (a >= min_weight && d > 0.0f) ? d / a : -1.0f;
}

// HALO pixels around the tile at (x0, y0) into zs, row stride NP_TW + 2 * HALO, and the rays of those columns and rows:
// rx[i] = (x0 - HALO + i - cx) / fx, ry[j] = (y0 - HALO + j - cy) / fy -- one division per column and per row of a tile, not six
// per pixel (the kernels are bound by their double arithmetic, not by memory)
template <int HALO>
__device__ __forceinline__ void np_stage_tile(float* __restrict__ zs, double* __restrict__ rx, double* __restrict__ ry,
                                              const float* __restrict__ D, const float* __restrict__ A, const int H, const int W,
                                              const float min_weight, const double* __restrict__ pin, const int x0, const int y0)
{
    constexpr int SW = NP_TW + 2 * HALO, SH = NP_TH + 2 * HALO;
    static_assert(SW <= 64 && SH <= 64, "wave 0 takes the columns, wave 1 the rows");
    for (int i = threadIdx.x; i < SW * SH; i += NP_BLOCK) {
        const int ly = i / SW, lx = i - ly * SW;
        zs[i] = np_stage(D, A, H, W, min_weight, x0 - HALO + lx, y0 - HALO + ly);
    }
    const int t = threadIdx.x;
    if (t < SW) rx[t] = ((double)(x0 - HALO + t) - pin[2]) / pin[0];
    else if (t >= 64 && t - 64 < SH) ry[t - 64] = ((double)(y0 - HALO + t - 64) - pin[3]) / pin[1];
}

struct NpGeo {
    double dx[3], dy[3], N[3], q;
};

// The geometric rule for a centre from the staged z of the centre (c) and of its left, right, upper and lower neighbour, and the
// rays of its three columns (rxl, rxc, rxr) and three rows (ryu, ryc, ryd); on true, o holds dx, dy, N = dy x dx and q = |N|^2.
// The one statement of the normal: the loss, its adjoint and depth_to_normal.
__device__ __forceinline__ bool np_geometric(const float zc, const float zl, const float zr, const float zu, const float zd, const double rxl,
                                             const double rxc, const double rxr, const double ryu, const double ryc, const double ryd,
                                             const double max_jump, NpGeo& o)
{
    if (zc < 0.0f || zl < 0.0f || zr < 0.0f || zu < 0.0f || zd < 0.0f) return false;
    const double c = (double)zc, l = (double)zl, r = (double)zr, up = (double)zu, dn = (double)zd;
    const double lim = max_jump * c;                                                          // inf * 0 is NaN: not valid
    if (!(fabs(r - l) <= lim) || !(fabs(dn - up) <= lim)) return false;
    o.dx[0] = r * rxr - l * rxl; o.dx[1] = r * ryc - l * ryc; o.dx[2] = r - l;
    o.dy[0] = dn * rxc - up * rxc; o.dy[1] = dn * ryd - up * ryu; o.dy[2] = dn - up;
    o.N[0] = o.dy[1] * o.dx[2] - o.dy[2] * o.dx[1];
    o.N[1] = o.dy[2] * o.dx[0] - o.dy[0] * o.dx[2];
    o.N[2] = o.dy[0] * o.dx[1] - o.dy[1] * o.dx[0];
    o.q = (o.N[0] * o.N[0] + o.N[1] * o.N[1]) + o.N[2] * o.N[2];
    return o.q > 0.0 && o.q < (double)INFINITY;
}

// The prior and the weight of centre (u, v), which is inside the image: false where m > 0 or the test of |p|^2 fails
__device__ __forceinline__ bool np_prior(const NpDev& a, const int view, const int u, const int v, double (&ph)[3], double& w)
{
    const size_t at = (size_t)v * a.W + u, plane = (size_t)a.H * a.W;
    const float* __restrict__ mk = a.mask[view];
    const float m = mk ? mk[at] : 1.0f;                                                       // uniform
    if (!(m > 0.0f)) return false;
    const float* __restrict__ p = a.prior[view];
    const double p0 = (double)p[at], p1 = (double)p[plane + at], p2 = (double)p[2 * plane + at];
    const double pp = (p0 * p0 + p1 * p1) + p2 * p2;
    if (!(pp > 0.25 && pp < (double)INFINITY)) return false;
    const double inv = 1.0 / sqrt(pp);                                                        // one division, three products
    ph[0] = p0 * inv; ph[1] = p1 * inv; ph[2] = p2 * inv;
    w = (double)m;
    return true;
}

// Workgroup (bx, by) of view bz leaves the row (sum w l, sum w) of its tile.
template <bool L1>
__global__ void __launch_bounds__(NP_BLOCK) normal_prior_sums_kernel(const NpDev a, double* __restrict__ partials)
{
    constexpr int SW = NP_TW + 2;
    __shared__ float zs[SW * (NP_TH + 2)];
    __shared__ double rx[NP_TW + 2], ry[NP_TH + 2];
    __shared__ double sh[NP_BLOCK / 64 * NP_ROW];
    const int view = blockIdx.z;
    const int x0 = blockIdx.x * NP_TW, y0 = blockIdx.y * NP_TH;
    np_stage_tile<1>(zs, rx, ry, a.depth[view], a.weights[view], a.H, a.W, a.min_weight, a.pinhole[view], x0, y0);
    __syncthreads();
    const int lx = threadIdx.x % NP_TW, ly = threadIdx.x / NP_TW;
    const int u = x0 + lx, v = y0 + ly;
    double acc[NP_ROW] = {0.0, 0.0};
    if (u < a.W && v < a.H) {
        const int c = (ly + 1) * SW + lx + 1;
        NpGeo g;
        double ph[3], w;
        if (np_geometric(zs[c], zs[c - 1], zs[c + 1], zs[c - SW], zs[c + SW], rx[lx], rx[lx + 1], rx[lx + 2], ry[ly], ry[ly + 1], ry[ly + 2],
                         a.max_jump, g) &&
            np_prior(a, view, u, v, ph, w)) {
            const double rs = 1.0 / sqrt(g.q);                                                // n = N / sqrt(q): one division
            const double n0 = g.N[0] * rs, n1 = g.N[1] * rs, n2 = g.N[2] * rs;
            double l;
            if (L1) l = (fabs(n0 - ph[0]) + fabs(n1 - ph[1])) + fabs(n2 - ph[2]);
            else l = 1.0 - ((n0 * ph[0] + n1 * ph[1]) + n2 * ph[2]);
            acc[0] = w * l; acc[1] = w;
        }
    }
    osum::block_sum<NP_ROW>(acc, sh);                                                        // every lane is here
    if (threadIdx.x < NP_ROW) {
        const size_t tile = (size_t)blockIdx.y * gridDim.x + blockIdx.x, ntiles = (size_t)gridDim.x * gridDim.y;
        partials[((size_t)view * ntiles + tile) * NP_ROW + threadIdx.x] = osum::block_total<NP_ROW>(sh, threadIdx.x);
    }
}

// One workgroup per view: its ntiles partial rows added in tile order (ordered_sum.h), then loss, count and the stats row.
__global__ void __launch_bounds__(256) normal_prior_finalize_kernel(const int ntiles, const double* __restrict__ partials, float* __restrict__ loss,
                                                                    float* __restrict__ count, double* __restrict__ stats)
{
    __shared__ double sh[4 * NP_ROW];
    const int v = blockIdx.x;
    double S[NP_ROW];
    osum::ordered_rows_sum<NP_ROW>(partials + (size_t)v * ntiles * NP_ROW, ntiles, NP_ROW, sh, S);
    if (threadIdx.x != 0) return;
    const double cnt = S[1];
    const double inv = cnt > 0.0 ? 1.0 / cnt : 0.0;
    loss[v] = (float)(cnt > 0.0 ? S[0] * inv : 0.0);
    count[v] = (float)cnt;
    stats[(size_t)v * NP_ROW] = inv;
    stats[(size_t)v * NP_ROW + 1] = cnt;
}

// dL/dD and dL/dA of every pixel of the tile (zeros where no valid centre reads the pixel), each rounded once from double.
// Phase one: the centres of the tile and of its one-pixel ring leave dL/ddx and dL/ddy in LDS (zeros where the centre is not
// valid or outside the image).  Phase two: a pixel gathers from its left, right, upper and lower centre, in that order.
// a.g_depth[view] / a.g_weights[view] == nullptr: not wanted, nothing is stored; what is stored is the same bits whichever is wanted.
template <bool L1>
__global__ void __launch_bounds__(NP_BLOCK) normal_prior_bwd_kernel(const NpDev a, const double* __restrict__ stats, const float* __restrict__ g_loss)
{
    constexpr int SW = NP_TW + 4, CW = NP_TW + 2, CH = NP_TH + 2, NC = CW * CH;
    __shared__ float zs[SW * (NP_TH + 4)];
    __shared__ double rx[NP_TW + 4], ry[NP_TH + 4];
    __shared__ double gd[6][NC];                     // dL/ddx (0..2) and dL/ddy (3..5) of the centres, component-major
    const int view = blockIdx.z;
    const int x0 = blockIdx.x * NP_TW, y0 = blockIdx.y * NP_TH;
    np_stage_tile<2>(zs, rx, ry, a.depth[view], a.weights[view], a.H, a.W, a.min_weight, a.pinhole[view], x0, y0);
    __syncthreads();
    const double scale = (double)g_loss[view] * stats[(size_t)view * NP_ROW];                 // cot / cnt; 0 where cnt <= 0
    for (int i = threadIdx.x; i < NC; i += NP_BLOCK) {
        const int cy = i / CW, cx = i - cy * CW;
        const int u = x0 - 1 + cx, v = y0 - 1 + cy;
        double out[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (u >= 0 && v >= 0 && u < a.W && v < a.H) {
            const int c = (cy + 1) * SW + cx + 1;
            NpGeo g;
            double ph[3], w;
            // the centre is column cx + 1 and row cy + 1 of the staged halo
            if (np_geometric(zs[c], zs[c - 1], zs[c + 1], zs[c - SW], zs[c + SW], rx[cx], rx[cx + 1], rx[cx + 2], ry[cy], ry[cy + 1], ry[cy + 2],
                             a.max_jump, g) &&
                np_prior(a, view, u, v, ph, w)) {
                const double rs = 1.0 / sqrt(g.q);                                            // the forward's n
                const double n[3] = {g.N[0] * rs, g.N[1] * rs, g.N[2] * rs};
                double gl[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) gl[k] = L1 ? osum::sign(n[k] - ph[k]) : -ph[k];
                const double ng = (n[0] * gl[0] + n[1] * gl[1]) + n[2] * gl[2];
                const double s = w * scale;
                double G[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) G[k] = (s * (gl[k] - n[k] * ng)) * rs;
                // dL/ddx = G x dy ;  dL/ddy = dx x G
                out[0] = G[1] * g.dy[2] - G[2] * g.dy[1];
                out[1] = G[2] * g.dy[0] - G[0] * g.dy[2];
                out[2] = G[0] * g.dy[1] - G[1] * g.dy[0];
                out[3] = g.dx[1] * G[2] - g.dx[2] * G[1];
                out[4] = g.dx[2] * G[0] - g.dx[0] * G[2];
                out[5] = g.dx[0] * G[1] - g.dx[1] * G[0];
            }
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) gd[k][i] = out[k];
    }
    __syncthreads();
    const int lx = threadIdx.x % NP_TW, ly = threadIdx.x / NP_TW;
    const int u = x0 + lx, v = y0 + ly;
    if (u >= a.W || v >= a.H) return;
    float* __restrict__ gD = a.g_depth[view];
    float* __restrict__ gA = a.g_weights[view];
    const size_t at = (size_t)v * a.W + u;
    float dD = 0.0f, dA = 0.0f;
    const float zf = zs[(ly + 2) * SW + lx + 2];
    if (zf >= 0.0f) {                                                                         // not solid: no centre reads it
        const int c = (ly + 1) * CW + lx + 1;                                                 // this pixel as a centre
        const int left = c - 1, right = c + 1, upper = c - CW, lower = c + CW;
        double gP[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) gP[k] = ((gd[k][left] - gd[k][right]) + gd[3 + k][upper]) - gd[3 + k][lower];
        const double gz = (rx[lx + 2] * gP[0] + ry[ly + 2] * gP[1]) + gP[2];
        const double iA = 1.0 / (double)a.weights[view][at], z = (double)zf;
        dD = (float)(gz * iA);
        dA = (float)(-((z * iA) * gz));
    }
    if (gD) gD[at] = dD;                                                                      // uniform
    if (gA) gA[at] = dA;
}

// normal (3,H,W) and valid (H,W) of one view by the geometric rule alone; zeros where not valid
__global__ void __launch_bounds__(NP_BLOCK) depth_to_normal_kernel(const NpDev a, float* __restrict__ normal, uint8_t* __restrict__ valid)
{
    constexpr int SW = NP_TW + 2;
    __shared__ float zs[SW * (NP_TH + 2)];
    __shared__ double rx[NP_TW + 2], ry[NP_TH + 2];
    const int x0 = blockIdx.x * NP_TW, y0 = blockIdx.y * NP_TH;
    np_stage_tile<1>(zs, rx, ry, a.depth[0], a.weights[0], a.H, a.W, a.min_weight, a.pinhole[0], x0, y0);
    __syncthreads();
    const int lx = threadIdx.x % NP_TW, ly = threadIdx.x / NP_TW;
    const int u = x0 + lx, v = y0 + ly;
    if (u >= a.W || v >= a.H) return;
    const int c = (ly + 1) * SW + lx + 1;
    NpGeo g;
    float n[3] = {0.0f, 0.0f, 0.0f};
    const bool ok = np_geometric(zs[c], zs[c - 1], zs[c + 1], zs[c - SW], zs[c + SW], rx[lx], rx[lx + 1], rx[lx + 2], ry[ly], ry[ly + 1], ry[ly + 2],
                                 a.max_jump, g);
    if (ok) {
        const double rs = 1.0 / sqrt(g.q);
#pragma unroll
        for (int k = 0; k < 3; ++k) n[k] = (float)(g.N[k] * rs);
    }
    const size_t at = (size_t)v * a.W + u, plane = (size_t)a.H * a.W;
    normal[at] = n[0]; normal[plane + at] = n[1]; normal[2 * plane + at] = n[2];
    valid[at] = ok ? 1 : 0;
}

static inline int np_tiles_x(int W) { return (W + NP_TW - 1) / NP_TW; }
static inline int np_tiles_y(int H) { return (H + NP_TH - 1) / NP_TH; }
// workgroups (= partial rows) per view: a function of the image size alone
long long normal_prior_tiles(int H, int W) { return (long long)np_tiles_x(W) * np_tiles_y(H); }

static NpDev np_dev(const BagsNormalPrior& a, float* const* g_depth, float* const* g_weights)
{
    NpDev d{};
    d.H = a.H; d.W = a.W;
    d.l1 = a.mode == BAGS_NORMAL_PRIOR_L1;
    d.min_weight = a.min_weight; d.max_jump = (double)a.max_jump;
    d.n_rows = a.n_rows;
    for (int k = 0; k < BAGS_MAX_POSE_ROWS; ++k) {
        const bool on = k < a.n_rows;
        for (int j = 0; j < 4; ++j) d.pinhole[k][j] = on ? a.pinhole[k][j] : 1.0;
        d.depth[k] = on ? a.depth[k] : nullptr;
        d.weights[k] = on ? a.weights[k] : nullptr;
        d.prior[k] = on ? a.prior[k] : nullptr;
        d.mask[k] = on ? a.mask[k] : nullptr;
        d.g_depth[k] = (on && g_depth) ? g_depth[k] : nullptr;
        d.g_weights[k] = (on && g_weights) ? g_weights[k] : nullptr;
    }
    return d;
}

// the struct is validated by the caller (api.hip); partials: n_rows * normal_prior_tiles(H, W) rows of 2 doubles
hipError_t launch_normal_prior_fwd(const BagsNormalPrior& a, double* partials, float* loss, float* count, double* stats, hipStream_t st)
{
    const NpDev d = np_dev(a, nullptr, nullptr);
    const dim3 grid(np_tiles_x(a.W), np_tiles_y(a.H), a.n_rows);
    const hipError_t e = with_bool(d.l1 != 0, [&](auto L1) {
        hipLaunchKernelGGL((normal_prior_sums_kernel<decltype(L1)::value>), grid, dim3(NP_BLOCK), 0, st, d, partials);
        return hipGetLastError(); });
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(normal_prior_finalize_kernel, dim3(a.n_rows), dim3(256), 0, st, (int)normal_prior_tiles(a.H, a.W), partials, loss, count,
                       stats);
    return hipGetLastError();
}

// g_depth / g_weights: NULL or n_rows pointers of which any may be NULL; at least one output is wanted (api.hip)
hipError_t launch_normal_prior_bwd(const BagsNormalPrior& a, const double* stats, const float* g_loss, float* const* g_depth,
                                   float* const* g_weights, hipStream_t st)
{
    const NpDev d = np_dev(a, g_depth, g_weights);
    const dim3 grid(np_tiles_x(a.W), np_tiles_y(a.H), a.n_rows);
    return with_bool(d.l1 != 0, [&](auto L1) {
        hipLaunchKernelGGL((normal_prior_bwd_kernel<decltype(L1)::value>), grid, dim3(NP_BLOCK), 0, st, d, stats, g_loss);
        return hipGetLastError(); });
}

hipError_t launch_depth_to_normal(const float* depth, const float* weights, int H, int W, const double* pinhole, float min_weight, float max_jump,
                                  float* normal, uint8_t* valid, hipStream_t st)
{
    NpDev d{};
    d.H = H; d.W = W; d.min_weight = min_weight; d.max_jump = (double)max_jump; d.n_rows = 1;
    for (int j = 0; j < 4; ++j) d.pinhole[0][j] = pinhole[j];
    d.depth[0] = depth; d.weights[0] = weights;
    hipLaunchKernelGGL(depth_to_normal_kernel, dim3(np_tiles_x(W), np_tiles_y(H)), dim3(NP_BLOCK), 0, st, d, normal, valid);
    return hipGetLastError();
}
