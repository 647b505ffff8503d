// warp.hip -- the photometric reprojection (warping) loss on the rasterizer's depth map D = sum w_i z_i and weights map A = 1 - T_final:
// un-project a pixel of the source view with the rendered depth, carry it into the target view with the two view matrices, sample the
// target view's image there, bilinearly, and hold the sampled colour to the colour of the pixel (CF-3DGS, Nope-NeRF, the
// self-supervised-depth family; the per-pixel core of PGSR-style multi-view consistency).  Conventions, the transform M, c, the point
// x_i / x_j and proj are the correspondence loss's, word for word (correspondence.hip; stated once, in reproject.h).  Per ordered pair:
// source maps D, A (H,W), view matrices Vi, Vj (4,4) on the device, color_src (C,H,W) = the colour each source pixel is held to,
// image_dst (C,Hd,Wd) = the image of view j, an optional confidence conf >= 0 (H,W) (NULL: 1), optional target maps depth_dst,
// weights_dst (Hd,Wd) for the occlusion test (both or neither), host pinholes of both sides.  C is 1 or 3.
//     inside  = 0 <= proj.x <= Wd - 1 and 0 <= proj.y <= Hd - 1                                         (all four taps exist)
//     x0 = floor(proj.x)  y0 = floor(proj.y)  ax = proj.x - x0  ay = proj.y - y0  x1 = min(x0 + 1, Wd - 1)  y1 = min(y0 + 1, Hd - 1)
//     S_c = (1-ay) ((1-ax) T_c[y0,x0] + ax T_c[y0,x1]) + ay ((1-ax) T_c[y1,x0] + ax T_c[y1,x1])          T = image_dst, in float64
//     dS_c/dproj = ((1-ay)(T_c[y0,x1]-T_c[y0,x0]) + ay (T_c[y1,x1]-T_c[y1,x0]),  (1-ax)(T_c[y1,x0]-T_c[y0,x0]) + ax (T_c[y1,x1]-T_c[y0,x1]))
//     visible = no target maps given, or at the nearest target pixel (floor(proj + 0.5)), with z_t = D_t / A_t (one division in the
//               dtype of the maps):  A_t >= min_weight and D_t > 0 and |x_j.z - z_t| <= occlusion * z_t
//     valid   = solid and det(Ai) usable and x_j.z >= min_depth and conf > 0 and inside and visible and every S_c, color_src_c finite
//     r_c = S_c - color_src_c ;  rho = (1/C) sum_c (sqrt(r_c^2 + eps^2) - eps)                          (Charbonnier)
//     w = conf on valid pixels ;  cnt = sum w ;  L_k = sum w rho / cnt
//     dL/dproj = s (w / cnt) (1/C) sum_c r_c / sqrt(r_c^2 + eps^2) * dS_c/dproj                         (s the cotangent)
// From dL/dproj on the backward is the correspondence loss's (reproject.h): dL/dD and dL/dA per pixel, twelve sums per workgroup, the
// chain to dL/dVi and dL/dVj with exact-zero fourth columns.  cnt <= 0, or det(Ai) zero or not finite: L_k = 0 and every gradient an
// exact zero, never NaN.  Validity is a decision, not differentiated through: the bilinear cell and the occlusion test included.  No
// gradient to image_dst, color_src, the target maps, conf or the pinholes: a gradient to the sampled image is a scatter, and this library
// writes no gradient with atomics.
//
// A thread is a source pixel, a workgroup the WP_CHUNK = 256 consecutive pixels of a chunk, the grid (chunk, pair); lane 0 forms M and c
// in double; sums in double, in a fixed order, without atomics and without memset, so a pair has the bits of a call of its own.  The
// four taps times C channels are a gather from image_dst: neighbouring source pixels land on neighbouring target pixels, so the gather
// lives in L2 and nothing is staged in LDS.  Compiled with -ffp-contract=off: only the operations spelled.
#include "reproject.h"

#define WP_CHUNK RP_CHUNK
#define WP_ROW RP_ROW
#define WP_SUMS RP_SUMS

struct WpDev {
    int H, W, Hd, Wd;
    float min_weight;
    double min_depth, eps, occlusion;
    double pin_src[BAGS_MAX_POSE_ROWS][4];
    double pin_dst[BAGS_MAX_POSE_ROWS][4];
    const float* depth[BAGS_MAX_POSE_ROWS];
    const float* weights[BAGS_MAX_POSE_ROWS];
    const float* conf[BAGS_MAX_POSE_ROWS];           // any of them NULL: 1
    const float* view_src[BAGS_MAX_POSE_ROWS];
    const float* view_dst[BAGS_MAX_POSE_ROWS];
    const float* color_src[BAGS_MAX_POSE_ROWS];      // (C,H,W)
    const float* image_dst[BAGS_MAX_POSE_ROWS];      // (C,Hd,Wd)
    const float* depth_dst[BAGS_MAX_POSE_ROWS];      // (Hd,Wd), NULL with weights_dst: no occlusion test
    const float* weights_dst[BAGS_MAX_POSE_ROWS];
    float* g_depth[BAGS_MAX_POSE_ROWS];              // backward: any of them NULL
    float* g_weights[BAGS_MAX_POSE_ROWS];
};

template <int C>
struct WpSample {
    double iz;                                       // 1 / x_j.z
    double ax, ay;
    double t[C][4];                                  // the taps (y0,x0), (y0,x1), (y1,x0), (y1,x1) of every channel
    double S[C];
};

// inside, visible and finite samples for a point rp_point accepted; on true the bilinear cell, its taps and the sampled colour.  Every
// index is formed from proj only after `inside` holds: 0 <= x0 <= x1 <= Wd - 1, 0 <= y0 <= y1 <= Hd - 1, and so for the nearest pixel.
template <int C>
__device__ __forceinline__ bool wp_sample(const WpDev& a, const int pair, const RpPoint& p, WpSample<C>& o)
{
    o.iz = 1.0 / p.xj[2];
    double x, y;
    rp_project(a.pin_dst[pair], p, o.iz, x, y);
    if (!(x >= 0.0 && x <= (double)(a.Wd - 1) && y >= 0.0 && y <= (double)(a.Hd - 1))) return false;      // (a NaN is outside)
    const float* __restrict__ Dt = a.depth_dst[pair];
    if (Dt) {                                                                                 // uniform
        const size_t nearest = (size_t)(int)floor(y + 0.5) * a.Wd + (int)floor(x + 0.5);
        const float dt = Dt[nearest], at = a.weights_dst[pair][nearest];
        if (!(at >= a.min_weight && dt > 0.0f)) return false;
        const double zt = (double)(dt / at);
        if (!(fabs(p.xj[2] - zt) <= a.occlusion * zt)) return false;
    }
    const double fx0 = floor(x), fy0 = floor(y);
    o.ax = x - fx0; o.ay = y - fy0;
    const int x0 = (int)fx0, y0 = (int)fy0;
    const int x1 = min(x0 + 1, a.Wd - 1), y1 = min(y0 + 1, a.Hd - 1);
    const size_t plane = (size_t)a.Hd * a.Wd, r0 = (size_t)y0 * a.Wd, r1 = (size_t)y1 * a.Wd;
    const float* __restrict__ T = a.image_dst[pair];
    bool finite = true;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float* __restrict__ Tc = T + c * plane;
        o.t[c][0] = (double)Tc[r0 + x0]; o.t[c][1] = (double)Tc[r0 + x1];
        o.t[c][2] = (double)Tc[r1 + x0]; o.t[c][3] = (double)Tc[r1 + x1];
        o.S[c] = (1.0 - o.ay) * ((1.0 - o.ax) * o.t[c][0] + o.ax * o.t[c][1]) + o.ay * ((1.0 - o.ax) * o.t[c][2] + o.ax * o.t[c][3]);
        finite = finite && fabs(o.S[c]) < (double)INFINITY;
    }
    return finite;
}

struct WpResidual {
    double w;                                        // conf
    double rho;
    double g[2];                                     // (1/C) sum_c r_c / sqrt(r_c^2 + eps^2) * dS_c/dproj
};

// the rest of `valid` for a pixel rp_point accepted: conf > 0, wp_sample, finite colours; on true the Charbonnier value and -- GRAD --
// its derivative with respect to proj
template <int C, bool GRAD>
__device__ __forceinline__ bool wp_residual(const WpDev& a, const int pair, const size_t at, const RpPoint& p, WpResidual& o, double& iz)
{
    const float* __restrict__ cf = a.conf[pair];
    const float w = cf ? cf[at] : 1.0f;                                                       // uniform
    if (!(w > 0.0f)) return false;
    WpSample<C> s;
    if (!wp_sample<C>(a, pair, p, s)) return false;
    const size_t plane = (size_t)a.H * a.W;
    const float* __restrict__ col = a.color_src[pair];
    float cs[C];
    bool finite = true;
#pragma unroll
    for (int c = 0; c < C; ++c) { cs[c] = col[c * plane + at]; finite = finite && fabsf(cs[c]) < INFINITY; }
    if (!finite) return false;
    o.w = (double)w;
    iz = s.iz;
    double rho = 0.0, gx = 0.0, gy = 0.0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const double r = s.S[c] - (double)cs[c];
        const double q = sqrt(r * r + a.eps * a.eps);
        rho += q - a.eps;
        if (GRAD) {
            const double d = r / q;
            const double sx = (1.0 - s.ay) * (s.t[c][1] - s.t[c][0]) + s.ay * (s.t[c][3] - s.t[c][2]);
            const double sy = (1.0 - s.ax) * (s.t[c][2] - s.t[c][0]) + s.ax * (s.t[c][3] - s.t[c][1]);
            gx += d * sx; gy += d * sy;
        }
    }
    o.rho = rho / (double)C;
    o.g[0] = gx / (double)C; o.g[1] = gy / (double)C;
    return true;
}

// Workgroup bx of pair by leaves the row (sum w rho, sum w) of its chunk.
template <int C>
__global__ void __launch_bounds__(WP_CHUNK) warp_sums_kernel(const WpDev a, double* __restrict__ partials)
{
    __shared__ double Mc[12];
    __shared__ int ok;
    __shared__ double sh[WP_CHUNK / 64 * WP_ROW];
    const int pair = blockIdx.y;
    rp_stage_transform(a, pair, Mc, &ok);
    const long long npix = (long long)a.H * a.W;
    const long long p = (long long)blockIdx.x * WP_CHUNK + threadIdx.x;
    double acc[WP_ROW] = {0.0, 0.0};
    if (ok && p < npix) {
        const int v = (int)(p / a.W), u = (int)(p - (long long)v * a.W);
        RpPoint pt;
        WpResidual rs;
        double iz;
        if (rp_point(a, pair, Mc, (size_t)p, u, v, pt) && wp_residual<C, false>(a, pair, (size_t)p, pt, rs, iz)) {
            acc[0] = rs.w * rs.rho; acc[1] = rs.w;
        }
    }
    osum::block_sum<WP_ROW>(acc, sh);
    if (threadIdx.x < WP_ROW) partials[((size_t)pair * gridDim.x + blockIdx.x) * WP_ROW + threadIdx.x] = osum::block_total<WP_ROW>(sh, threadIdx.x);
}

// One workgroup per pair: its nchunks partial rows added in chunk order, then loss, count and the stats row.
__global__ void __launch_bounds__(256) warp_finalize_kernel(const int nchunks, const double* __restrict__ partials, float* __restrict__ loss,
                                                            float* __restrict__ count, double* __restrict__ stats)
{
    __shared__ double sh[4 * WP_ROW];
    rp_finalize(blockIdx.x, nchunks, partials, loss, count, stats, sh);
}

// dL/dD and dL/dA of every pixel of the chunk (zeros where the pixel is not valid), each rounded once from double, and -- SUMS --
// the chunk's twelve partial sums G_M (9) and g_c (3) into sums[(pair * 12 + t) * nchunks + chunk].
// a.g_depth[pair] / a.g_weights[pair] == nullptr: not wanted, nothing is stored; what is stored is the same bits whichever is wanted.
template <int C, bool SUMS>
__global__ void __launch_bounds__(WP_CHUNK) warp_bwd_kernel(const WpDev a, const double* __restrict__ stats, const float* __restrict__ g_loss,
                                                            double* __restrict__ sums)
{
    __shared__ double Mc[12];
    __shared__ int ok;
    __shared__ double sh[WP_CHUNK / 64 * WP_SUMS];
    const int pair = blockIdx.y;
    rp_stage_transform(a, pair, Mc, &ok);
    const long long npix = (long long)a.H * a.W;
    const long long p = (long long)blockIdx.x * WP_CHUNK + threadIdx.x;
    const double scale = (double)g_loss[pair] * stats[(size_t)pair * WP_ROW];                 // cot / cnt; 0 where cnt <= 0
    double acc[WP_SUMS];
#pragma unroll
    for (int t = 0; t < WP_SUMS; ++t) acc[t] = 0.0;
    if (p < npix) {
        float dD = 0.0f, dA = 0.0f;
        const int v = (int)(p / a.W), u = (int)(p - (long long)v * a.W);
        RpPoint pt;
        WpResidual rs;
        double iz;
        if (ok && rp_point(a, pair, Mc, (size_t)p, u, v, pt) && wp_residual<C, true>(a, pair, (size_t)p, pt, rs, iz)) {
            const double* __restrict__ pin = a.pin_dst[pair];
            const double sw = scale * rs.w;
            const double gx = (sw * rs.g[0]) * pin[0], gy = (sw * rs.g[1]) * pin[1];          // dL/dproj fx_j, dL/dproj fy_j
            rp_pixel_back<SUMS>(pt, Mc, gx, gy, iz, dD, dA, acc);
        }
        float* __restrict__ gD = a.g_depth[pair];
        float* __restrict__ gA = a.g_weights[pair];
        if (gD) gD[p] = dD;                                                                   // uniform
        if (gA) gA[p] = dA;
    }
    if (!SUMS) return;
    rp_store_sums(acc, sh, pair, sums);
}

// One workgroup per pair: the twelve sums of its chunks, then the chain to the two (4,4) gradients (reproject.h)
__global__ void __launch_bounds__(256) warp_views_kernel(const WpDev a, const RpViewGrads g, const int nchunks, const double* __restrict__ sums)
{
    __shared__ double sh[4];
    const int pair = blockIdx.x;
    rp_views_chain(a.view_src[pair], a.view_dst[pair], pair, nchunks, sums, g.src[pair], g.dst[pair], sh);
}

// The warped image (C,H,W) and valid (H,W) of the first pair: S_c where the pixel is solid, x_j.z >= min_depth, inside, visible and
// every S_c finite; zeros elsewhere.  conf and color_src are not read.
template <int C>
__global__ void __launch_bounds__(WP_CHUNK) warp_image_kernel(const WpDev a, float* __restrict__ out, uint8_t* __restrict__ valid)
{
    __shared__ double Mc[12];
    __shared__ int ok;
    rp_stage_transform(a, 0, Mc, &ok);
    const long long npix = (long long)a.H * a.W;
    const long long p = (long long)blockIdx.x * WP_CHUNK + threadIdx.x;
    if (p >= npix) return;
    const int v = (int)(p / a.W), u = (int)(p - (long long)v * a.W);
    RpPoint pt;
    WpSample<C> s;
    const bool in = ok && rp_point(a, 0, Mc, (size_t)p, u, v, pt) && wp_sample<C>(a, 0, pt, s);
#pragma unroll
    for (int c = 0; c < C; ++c) out[c * npix + p] = in ? (float)s.S[c] : 0.0f;
    valid[p] = in ? 1 : 0;
}

static WpDev wp_dev(const BagsWarp& a, float* const* g_depth, float* const* g_weights)
{
    WpDev d{};
    d.H = a.H; d.W = a.W; d.Hd = a.H_dst; d.Wd = a.W_dst;
    d.min_weight = a.min_weight; d.min_depth = a.min_depth; d.eps = a.eps; d.occlusion = a.occlusion;
    for (int k = 0; k < BAGS_MAX_POSE_ROWS; ++k) {
        const bool on = k < a.n_rows;
        for (int j = 0; j < 4; ++j) {
            d.pin_src[k][j] = on ? a.pinhole_src[k][j] : 1.0;
            d.pin_dst[k][j] = on ? a.pinhole_dst[k][j] : 1.0;
        }
        d.depth[k] = on ? a.depth[k] : nullptr;
        d.weights[k] = on ? a.weights[k] : nullptr;
        d.conf[k] = on ? a.conf[k] : nullptr;
        d.view_src[k] = on ? a.view_src[k] : nullptr;
        d.view_dst[k] = on ? a.view_dst[k] : nullptr;
        d.color_src[k] = on ? a.color_src[k] : nullptr;
        d.image_dst[k] = on ? a.image_dst[k] : nullptr;
        d.depth_dst[k] = on ? a.depth_dst[k] : nullptr;
        d.weights_dst[k] = on ? a.weights_dst[k] : nullptr;
        d.g_depth[k] = (on && g_depth) ? g_depth[k] : nullptr;
        d.g_weights[k] = (on && g_weights) ? g_weights[k] : nullptr;
    }
    return d;
}

// C is 1 or 3 (api.hip)
template <typename F> static inline hipError_t wp_with_channels(int C, F f) { return C == 1 ? f(std::integral_constant<int, 1>{}) : f(std::integral_constant<int, 3>{}); }

// the struct is validated by the caller (api.hip); partials: n_rows * correspondence_chunks(H, W) rows of 2 doubles
hipError_t launch_warp_fwd(const BagsWarp& a, double* partials, float* loss, float* count, double* stats, hipStream_t st)
{
    const WpDev d = wp_dev(a, nullptr, nullptr);
    const int nchunks = rp_chunks(a.H, a.W);
    hipError_t e = wp_with_channels(a.C, [&](auto CH) {
        hipLaunchKernelGGL((warp_sums_kernel<decltype(CH)::value>), dim3(nchunks, a.n_rows), dim3(WP_CHUNK), 0, st, d, partials);
        return hipGetLastError(); });
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(warp_finalize_kernel, dim3(a.n_rows), dim3(256), 0, st, nchunks, (const double*)partials, loss, count, stats);
    return hipGetLastError();
}

// g_depth / g_weights / g_view_src / g_view_dst: NULL or n_rows pointers of which any may be NULL; at least one output is wanted, and
// `sums` (n_rows * 12 * correspondence_chunks(H, W) doubles) is given where a matrix gradient is (api.hip)
hipError_t launch_warp_bwd(const BagsWarp& a, const double* stats, const float* g_loss, double* sums, float* const* g_depth, float* const* g_weights,
                           float* const* g_view_src, float* const* g_view_dst, hipStream_t st)
{
    const WpDev d = wp_dev(a, g_depth, g_weights);
    RpViewGrads g{};
    bool views = false;
    for (int k = 0; k < a.n_rows; ++k) {
        g.src[k] = g_view_src ? g_view_src[k] : nullptr;
        g.dst[k] = g_view_dst ? g_view_dst[k] : nullptr;
        views |= g.src[k] || g.dst[k];
    }
    const int nchunks = rp_chunks(a.H, a.W);
    hipError_t e = wp_with_channels(a.C, [&](auto CH) { return with_bool(views, [&](auto SUMS) {
        hipLaunchKernelGGL((warp_bwd_kernel<decltype(CH)::value, decltype(SUMS)::value>), dim3(nchunks, a.n_rows), dim3(WP_CHUNK), 0, st, d, stats, g_loss,
                           sums);
        return hipGetLastError(); }); });
    if (e != hipSuccess || !views) return e;
    hipLaunchKernelGGL(warp_views_kernel, dim3(a.n_rows), dim3(256), 0, st, d, g, nchunks, (const double*)sums);
    return hipGetLastError();
}

hipError_t launch_warp_image(const BagsWarp& a, float* out, uint8_t* valid, hipStream_t st)
{
    const WpDev d = wp_dev(a, nullptr, nullptr);
    return wp_with_channels(a.C, [&](auto CH) {
        hipLaunchKernelGGL((warp_image_kernel<decltype(CH)::value>), dim3(rp_chunks(a.H, a.W)), dim3(WP_CHUNK), 0, st, d, out, valid);
        return hipGetLastError(); });
}
