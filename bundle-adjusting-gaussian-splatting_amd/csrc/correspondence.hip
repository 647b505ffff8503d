// correspondence.hip -- the multi-view correspondence loss on the rasterizer's depth map D = sum w_i z_i and weights map
// A = 1 - T_final: un-project a pixel of the source view with the rendered depth, carry it into the target view with the two view
// matrices and penalise its distance to the pixel a matcher says it corresponds to (SPARF, CoR-GS).  Row vectors,
// x_cam = [X_w, 1] @ viewmatrix; view space x right, y down, z forward; pinholes (fx, fy, cx, cy) in pixels.  Per ordered pair:
// source maps D, A (H,W), view matrices Vi, Vj (4,4) on the device, match (2,H,W) = the target pixel (x, y) of source pixel (u, v),
// an optional confidence conf >= 0 (H,W) (NULL: 1), host pinholes of both sides.
//     solid(u,v) = A >= min_weight and D > 0
//     z          = D / A                      one division in the dtype of the maps; everything after it in float64
//     Ai = Vi[:3,:3]  bi = Vi[3,:3]  Aj = Vj[:3,:3]  bj = Vj[3,:3]
//     M  = inv(Ai) @ Aj ;  c = bj - bi @ M    (the true inverse, adj(Ai) / det(Ai): a global alignment with a scale stays exact)
//     x_i = z * ((u - cx_i)/fx_i, (v - cy_i)/fy_i, 1) ;  x_j = x_i @ M + c
//     valid(u,v) = solid and conf > 0 and match finite (both components) and x_j.z >= min_depth
//     proj = (fx_j x_j.x / x_j.z + cx_j,  fy_j x_j.y / x_j.z + cy_j) ;  r = proj - match ;  e = |r|_2
//     rho  = e^2 / 2 where e <= delta,  delta (e - delta / 2) elsewhere        (delta = inf: half the squared distance)
//     w = conf on valid pixels ;  cnt = sum w ;  L_k = sum w rho / cnt
// cnt <= 0, or det(Ai) zero or not finite: L_k = 0 and every gradient an exact zero, never NaN.  Validity is a decision, not
// differentiated through.  Backward, with s = cot_k / cnt_k and g_r = s w r (e <= delta) or s w delta r / e (elsewhere):
//     g_xj = (g_r.x fx_j / z_j,  g_r.y fy_j / z_j,  -(g_r.x fx_j x_j.x + g_r.y fy_j x_j.y) / z_j^2)
//     g_xi = g_xj @ M^T ;  dL/dz = ray . g_xi ;  dL/dD = dL/dz / A ;  dL/dA = -(z / A) dL/dz
//     G_M = sum x_i^T g_xj ;  g_c = sum g_xj ;  G = G_M - bi^T g_c        (c = bj - bi @ M)
//     dL/dAj = P^T G ;  dL/dAi = -P^T G M^T  (P = inv(Ai), d inv(A) = -inv(A) dA inv(A)) ;  dL/dbj = g_c ;  dL/dbi = -M g_c
// The fourth column of both matrix gradients is zero.  No gradient to match, conf or the pinholes.
//
// A thread is a pixel (in row-major order), a workgroup the CO_CHUNK = 256 consecutive pixels of a chunk, the grid (chunk, pair).
// Lane 0 of a workgroup forms M and c in double from the 24 device floats (about 100 flops) and leaves them in LDS; the host never
// reads the matrices.  The sums: a lane holds its one pixel in double, the workgroup adds its lanes (ordered_sum.h) and leaves its
// partial sums in the workspace.  A pair has ceil(H W / 256) workgroups whatever the number of pairs, and the finishing kernels add
// its partials in chunk order (ordered_sum.h): a pair's results are the same bits in a
// 16-pair launch and in a launch of its own.  No atomics, no memset.  Compiled with -ffp-contract=off: only the operations spelled.
#include "reproject.h"

#define CO_CHUNK RP_CHUNK
#define CO_ROW RP_ROW
#define CO_SUMS RP_SUMS

struct CoDev {
    int H, W;
    float min_weight;
    double min_depth, delta;
    double pin_src[BAGS_MAX_POSE_ROWS][4];
    double pin_dst[BAGS_MAX_POSE_ROWS][4];
    const float* depth[BAGS_MAX_POSE_ROWS];
    const float* weights[BAGS_MAX_POSE_ROWS];
    const float* match[BAGS_MAX_POSE_ROWS];
    const float* conf[BAGS_MAX_POSE_ROWS];           // any of them NULL: 1
    const float* view_src[BAGS_MAX_POSE_ROWS];
    const float* view_dst[BAGS_MAX_POSE_ROWS];
    float* g_depth[BAGS_MAX_POSE_ROWS];              // backward: any of them NULL
    float* g_weights[BAGS_MAX_POSE_ROWS];
};

// The transform and its staging, the pixel's x_i / x_j / proj, the ordered sums, the finalize, the pixel's way back from dL/dproj and
// the chain to the two matrix gradients are stated in reproject.h, which warp.hip shares.
struct CoResidual {
    double w, iz;                                    // conf, 1 / x_j.z
    double r[2], e;
};

// the rest of `valid` for a pixel rp_point accepted: conf > 0 and a finite match; on true the residual
__device__ __forceinline__ bool co_residual(const CoDev& a, const int pair, const size_t at, const RpPoint& p, CoResidual& o)
{
    const float* __restrict__ cf = a.conf[pair];
    const float w = cf ? cf[at] : 1.0f;                                                       // uniform
    if (!(w > 0.0f)) return false;
    const size_t plane = (size_t)a.H * a.W;
    const float mx = a.match[pair][at], my = a.match[pair][plane + at];
    if (!(fabsf(mx) < INFINITY && fabsf(my) < INFINITY)) return false;
    const double* __restrict__ pin = a.pin_dst[pair];
    o.w = (double)w;
    o.iz = 1.0 / p.xj[2];
    double x, y;
    rp_project(pin, p, o.iz, x, y);
    o.r[0] = x - (double)mx;
    o.r[1] = y - (double)my;
    o.e = sqrt(o.r[0] * o.r[0] + o.r[1] * o.r[1]);
    return true;
}

// Workgroup bx of pair by leaves the row (sum w rho, sum w) of its chunk.
__global__ void __launch_bounds__(CO_CHUNK) correspondence_sums_kernel(const CoDev a, double* __restrict__ partials)
{
    __shared__ double Mc[12];
    __shared__ int ok;
    __shared__ double sh[CO_CHUNK / 64 * CO_ROW];
    const int pair = blockIdx.y;
    rp_stage_transform(a, pair, Mc, &ok);
    const long long npix = (long long)a.H * a.W;
    const long long p = (long long)blockIdx.x * CO_CHUNK + threadIdx.x;
    double acc[CO_ROW] = {0.0, 0.0};
    if (ok && p < npix) {
        const int v = (int)(p / a.W), u = (int)(p - (long long)v * a.W);
        RpPoint pt;
        CoResidual rs;
        if (rp_point(a, pair, Mc, (size_t)p, u, v, pt) && co_residual(a, pair, (size_t)p, pt, rs)) {
            const double rho = rs.e <= a.delta ? 0.5 * (rs.e * rs.e) : a.delta * (rs.e - 0.5 * a.delta);
            acc[0] = rs.w * rho; acc[1] = rs.w;
        }
    }
    osum::block_sum<CO_ROW>(acc, sh);
    if (threadIdx.x < CO_ROW) partials[((size_t)pair * gridDim.x + blockIdx.x) * CO_ROW + threadIdx.x] = osum::block_total<CO_ROW>(sh, threadIdx.x);
}

// One workgroup per pair: its nchunks partial rows added in chunk order, then loss, count and the stats row.
__global__ void __launch_bounds__(256) correspondence_finalize_kernel(const int nchunks, const double* __restrict__ partials, float* __restrict__ loss,
                                                                      float* __restrict__ count, double* __restrict__ stats)
{
    __shared__ double sh[4 * CO_ROW];
    rp_finalize(blockIdx.x, nchunks, partials, loss, count, stats, sh);
}

// dL/dD and dL/dA of every pixel of the chunk (zeros where the pixel is not valid), each rounded once from double, and -- SUMS --
// the chunk's twelve partial sums G_M (9) and g_c (3) into sums[(pair * 12 + t) * nchunks + chunk].
// a.g_depth[pair] / a.g_weights[pair] == nullptr: not wanted, nothing is stored; what is stored is the same bits whichever is wanted.
template <bool SUMS>
__global__ void __launch_bounds__(CO_CHUNK) correspondence_bwd_kernel(const CoDev a, const double* __restrict__ stats, const float* __restrict__ g_loss,
                                                                      double* __restrict__ sums)
{
    __shared__ double Mc[12];
    __shared__ int ok;
    __shared__ double sh[CO_CHUNK / 64 * CO_SUMS];
    const int pair = blockIdx.y;
    rp_stage_transform(a, pair, Mc, &ok);
    const long long npix = (long long)a.H * a.W;
    const long long p = (long long)blockIdx.x * CO_CHUNK + threadIdx.x;
    const double scale = (double)g_loss[pair] * stats[(size_t)pair * CO_ROW];                 // cot / cnt; 0 where cnt <= 0
    double acc[CO_SUMS];
#pragma unroll
    for (int t = 0; t < CO_SUMS; ++t) acc[t] = 0.0;
    if (p < npix) {
        float dD = 0.0f, dA = 0.0f;
        const int v = (int)(p / a.W), u = (int)(p - (long long)v * a.W);
        RpPoint pt;
        CoResidual rs;
        if (ok && rp_point(a, pair, Mc, (size_t)p, u, v, pt) && co_residual(a, pair, (size_t)p, pt, rs)) {
            const double* __restrict__ pin = a.pin_dst[pair];
            double sw = scale * rs.w;
            if (!(rs.e <= a.delta)) sw = (sw * a.delta) / rs.e;                               // e > delta > 0
            const double gx = (sw * rs.r[0]) * pin[0], gy = (sw * rs.r[1]) * pin[1];          // g_r fx_j, g_r fy_j
            rp_pixel_back<SUMS>(pt, Mc, gx, gy, rs.iz, dD, dA, acc);
        }
        float* __restrict__ gD = a.g_depth[pair];
        float* __restrict__ gA = a.g_weights[pair];
        if (gD) gD[p] = dD;                                                                   // uniform
        if (gA) gA[p] = dA;
    }
    if (!SUMS) return;
    rp_store_sums(acc, sh, pair, sums);
}

// One workgroup per pair: the twelve sums of its chunks added in a fixed order, then the chain to the two (4,4) gradients in double,
// each element rounded once.  A degenerate pair (det(Ai) zero or not finite) gets exact zeros.  g.src[pair] / g.dst[pair] == nullptr:
// not wanted.
__global__ void __launch_bounds__(256) correspondence_views_kernel(const CoDev a, const RpViewGrads g, const int nchunks, const double* __restrict__ sums)
{
    __shared__ double sh[4];
    const int pair = blockIdx.x;
    rp_views_chain(a.view_src[pair], a.view_dst[pair], pair, nchunks, sums, g.src[pair], g.dst[pair], sh);
}

// proj (2,H,W) and valid (H,W) of one pair: the projection where the pixel is solid and x_j.z >= min_depth, zeros elsewhere; valid
// where the projection also lies inside the W_dst x H_dst image, -0.5 <= x < W_dst - 0.5 and -0.5 <= y < H_dst - 0.5 (pixel centres
// at whole numbers, the pixel rule of pinhole_of)
__global__ void __launch_bounds__(CO_CHUNK) reproject_pixels_kernel(const CoDev a, const int H_dst, const int W_dst, float* __restrict__ proj,
                                                                    uint8_t* __restrict__ valid)
{
    __shared__ double Mc[12];
    __shared__ int ok;
    rp_stage_transform(a, 0, Mc, &ok);
    const long long npix = (long long)a.H * a.W;
    const long long p = (long long)blockIdx.x * CO_CHUNK + threadIdx.x;
    if (p >= npix) return;
    const int v = (int)(p / a.W), u = (int)(p - (long long)v * a.W);
    float px = 0.0f, py = 0.0f;
    bool in = false;
    RpPoint pt;
    if (ok && rp_point(a, 0, Mc, (size_t)p, u, v, pt)) {
        const double* __restrict__ pin = a.pin_dst[0];
        const double iz = 1.0 / pt.xj[2];
        double x, y;
        rp_project(pin, pt, iz, x, y);
        px = (float)x; py = (float)y;
        in = x >= -0.5 && x < (double)W_dst - 0.5 && y >= -0.5 && y < (double)H_dst - 0.5;
    }
    proj[p] = px; proj[npix + p] = py;
    valid[p] = in ? 1 : 0;
}

static inline int co_chunks(int H, int W) { return rp_chunks(H, W); }
// workgroups (= partial rows) per pair: a function of the image size alone
long long correspondence_chunks(int H, int W) { return co_chunks(H, W); }

static CoDev co_dev(const BagsCorrespondence& a, float* const* g_depth, float* const* g_weights)
{
    CoDev d{};
    d.H = a.H; d.W = a.W;
    d.min_weight = a.min_weight; d.min_depth = a.min_depth; d.delta = a.delta;
    for (int k = 0; k < BAGS_MAX_POSE_ROWS; ++k) {
        const bool on = k < a.n_rows;
        for (int j = 0; j < 4; ++j) {
            d.pin_src[k][j] = on ? a.pinhole_src[k][j] : 1.0;
            d.pin_dst[k][j] = on ? a.pinhole_dst[k][j] : 1.0;
        }
        d.depth[k] = on ? a.depth[k] : nullptr;
        d.weights[k] = on ? a.weights[k] : nullptr;
        d.match[k] = on ? a.match[k] : nullptr;
        d.conf[k] = on ? a.conf[k] : nullptr;
        d.view_src[k] = on ? a.view_src[k] : nullptr;
        d.view_dst[k] = on ? a.view_dst[k] : nullptr;
        d.g_depth[k] = (on && g_depth) ? g_depth[k] : nullptr;
        d.g_weights[k] = (on && g_weights) ? g_weights[k] : nullptr;
    }
    return d;
}

// the struct is validated by the caller (api.hip); partials: n_rows * correspondence_chunks(H, W) rows of 2 doubles
hipError_t launch_correspondence_fwd(const BagsCorrespondence& a, double* partials, float* loss, float* count, double* stats, hipStream_t st)
{
    const CoDev d = co_dev(a, nullptr, nullptr);
    const int nchunks = co_chunks(a.H, a.W);
    hipLaunchKernelGGL(correspondence_sums_kernel, dim3(nchunks, a.n_rows), dim3(CO_CHUNK), 0, st, d, partials);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(correspondence_finalize_kernel, dim3(a.n_rows), dim3(256), 0, st, nchunks, partials, loss, count, stats);
    return hipGetLastError();
}

// g_depth / g_weights / g_view_src / g_view_dst: NULL or n_rows pointers of which any may be NULL; at least one output is wanted, and
// `sums` (n_rows * 12 * correspondence_chunks(H, W) doubles) is given where a matrix gradient is (api.hip)
hipError_t launch_correspondence_bwd(const BagsCorrespondence& a, const double* stats, const float* g_loss, double* sums, float* const* g_depth,
                                     float* const* g_weights, float* const* g_view_src, float* const* g_view_dst, hipStream_t st)
{
    const CoDev d = co_dev(a, g_depth, g_weights);
    RpViewGrads g{};
    bool views = false;
    for (int k = 0; k < a.n_rows; ++k) {
        g.src[k] = g_view_src ? g_view_src[k] : nullptr;
        g.dst[k] = g_view_dst ? g_view_dst[k] : nullptr;
        views |= g.src[k] || g.dst[k];
    }
    const int nchunks = co_chunks(a.H, a.W);
    hipError_t e = with_bool(views, [&](auto SUMS) {
        hipLaunchKernelGGL((correspondence_bwd_kernel<decltype(SUMS)::value>), dim3(nchunks, a.n_rows), dim3(CO_CHUNK), 0, st, d, stats, g_loss, sums);
        return hipGetLastError(); });
    if (e != hipSuccess || !views) return e;
    hipLaunchKernelGGL(correspondence_views_kernel, dim3(a.n_rows), dim3(256), 0, st, d, g, nchunks, (const double*)sums);
    return hipGetLastError();
}

hipError_t launch_reproject_pixels(const BagsCorrespondence& a, int H_dst, int W_dst, float* proj, uint8_t* valid, hipStream_t st)
{
    const CoDev d = co_dev(a, nullptr, nullptr);
    hipLaunchKernelGGL(reproject_pixels_kernel, dim3(co_chunks(a.H, a.W)), dim3(CO_CHUNK), 0, st, d, H_dst, W_dst, proj, valid);
    return hipGetLastError();
}
