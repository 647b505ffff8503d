// smooth.hip -- edge-aware smoothness (total variation) of the rasterizer's depth / weights maps and of a splatted normal map: the
// regulariser beside the data terms of depth_prior.hip, normal_prior.hip and normal_map.hip.  Per view: a field F of C channels, a
// weights map A (H,W), an optional guide image I (cg,H,W) with cg = 1 or 3 (NULL: no edge weight), an optional pixel weight m >= 0
// (H,W) (NULL: 1).
//     depth (C = 1):   usable = A >= min_weight and D > 0 and m > 0 and x finite ;  x = A / D (inverse) or D / A (depth), one division
//                      in float32 ;  normalize: mu = sum_usable x / n, F = x / mu (n usable pixels) ;  else F = x
//     normals (C = 3): usable = A >= min_weight and |N|^2 finite and > min_norm^2 and m > 0 ;  F = N / |N| in float64
//     order 1: the stencil anchored at (u,v) has members (u,v), (u+1,v):  d = F(u+1,v) - F(u,v) ;  g = mean_c |I(u+1,v) - I(u,v)|
//     order 2: the stencil centred at (u,v) has members (u-1,v), (u,v), (u+1,v):  d = F(u-1,v) - 2 F(u,v) + F(u+1,v) ;
//              g = mean_c |I(u+1,v) - I(u-1,v)| / 2                                   (and the same along v)
//     a stencil is valid when its members are inside the image and usable and g is finite ;  e = exp(-gamma g) (no guide: 1) ;
//     w = min of m over the members
//     rho(d) = (1/C) sum_c rho1(d_c) ;  l1: rho1(t) = sqrt(t^2 + eps^2) - eps (eps = 0: |t|, sign(0) = 0) ;  l2: rho1(t) = t^2
//     S_dir = sum w e rho(d), cnt_dir = sum w ;  L_v = S_x / cnt_x + S_y / cnt_y (a direction with cnt_dir <= 0 counts 0) ;
//     count = cnt_x + cnt_y
// Validity, e and min are decisions or constant data.  Backward: with q = cot_v w e rho1'(t) / (C cnt_dir) (/ mu where normalised) of
// every stencil, a pixel's dL/dF is the sum of q times its coefficient (-1, +1 or +1, -2, +1) over the stencils that contain it;
// with normalize every usable pixel additionally gets -cot_v T / (mu n), T = sum_dir (1/cnt_dir) sum w e rho'(t) . t.  Then
//     inverse: dL/dA = dL/dx / D, dL/dD = -(x / D) dL/dx ;  depth: dL/dD = dL/dx / A, dL/dA = -(x / A) dL/dx ;
//     normals: dL/dN = (G - n (n . G)) / |N|
// Pixels that are not usable get exact zeros.
//
// A workgroup of 256 threads takes a tile of 32 x 8 pixels, the views of a call are grid dimension z and their pointers arrive by
// value.  The field is staged in LDS in double with the halo the kernel needs (the forward: the stencils of the tile's pixels; the
// backward: the stencils of the tile and of its one-pixel ring), NaN in channel 0 where a pixel is not usable or outside the image:
// a usable value is never NaN, so that is the flag, and a stencil that leaves the image is invalid by it.  The pixel weight and the
// guide are staged beside it as floats.  Every stencil belongs to the workgroup of its anchor (order 1) or centre (order 2).
//
// The sums of a view: a lane holds its two stencils in double, and the workgroup adds its lanes and leaves one row of 6 doubles (S,
// cnt, T per direction; T a zero it writes where not normalised).  The finalize kernel adds a view's rows in row order (both:
// ordered_sum.h).  The mean of `normalize` is one launch in front: smooth_mean_slots(H, W) workgroups per view each leave
// (sum x, n) of a contiguous run of pixels, and every workgroup of the sums kernel (and the finalize kernel) adds those rows with the
// same tree (sm_mean: wave 0 alone, one barrier), so mu is the same bits everywhere.  No atomics, no memset: a view's loss, count, stats and
// gradients are the same bits in a 16-view call and in a call of its own.  exp is evaluated in float32 (expf), everything else after the loads in double.  There is
// one element-by-element instance of each kernel (no float4 twin); the file is compiled with -ffp-contract=off so that the decisions
// (|N|^2 > min_norm^2, finite g) are the statement's and the backward forms the forward's t: only the operations it spells.
#include "ordered_sum.h"

#define SM_TW BAGS_SMOOTH_TILE_W
#define SM_TH BAGS_SMOOTH_TILE_H
#define SM_BLOCK (SM_TW * SM_TH)
#define SM_ROW BAGS_SMOOTH_PARTIALS                  // doubles per partial row: (S, cnt, T) of x, then of y
#define SM_STATS BAGS_SMOOTH_STATS                   // doubles per stats row: 1/cnt_x, 1/cnt_y, 1/mu, n, T, cnt_x, cnt_y, mu
#define SM_SLOTS BAGS_SMOOTH_MEAN_SLOTS
static_assert(SM_BLOCK == 256, "four waves: block_sum's default, and ordered_rows_sum's 256 threads");
static_assert(SM_ROW == 6 && SM_STATS == 8, "the rows are spelled out below");

struct SmDev {
    int H, W;
    int cg;                                          // guide channels: 0 (no guide), 1 or 3
    int inverse, l2, normalize;
    int mean_slots;                                  // workgroups (= rows) per view of the mean kernel
    unsigned mean_chunk;                             // pixels per mean row
    float min_weight;
    double min_norm_sq, eps, gamma;
    double inv_gn;                                   // 1 / (cg * order): the mean over the guide's channels (order 2: and over two pixels)
    const float* field[BAGS_MAX_POSE_ROWS];
    const float* weights[BAGS_MAX_POSE_ROWS];
    const float* guide[BAGS_MAX_POSE_ROWS];          // all NULL where cg == 0
    const float* mask[BAGS_MAX_POSE_ROWS];           // any of them NULL: 1
    float* g_field[BAGS_MAX_POSE_ROWS];              // backward: any of them NULL
    float* g_weights[BAGS_MAX_POSE_ROWS];
};

__device__ __forceinline__ double sm_nan() { return __builtin_nan(""); }

// x of the pixel at `at`, which is inside the image; NaN where it is not usable
__device__ __forceinline__ double sm_depth_x(const SmDev& a, const float* __restrict__ D, const float* __restrict__ A,
                                             const float* __restrict__ mk, const size_t at)
{
    const float d = D[at], w = A[at];
    const float m = mk ? mk[at] : 1.0f;                                                       // uniform
    if (!(w >= a.min_weight && d > 0.0f && m > 0.0f)) return sm_nan();
    const float x = a.inverse ? w / d : d / w;
    return osum::finite(x) ? (double)x : sm_nan();
}

// The tile at (x0, y0) with HL pixels in front and HR behind, row stride SM_TW + HL + HR: the field channel-major in Fs, the pixel
// weight in ms (0 outside the image), the guide channel-major in gs.
template <int C, int HL, int HR>
__device__ __forceinline__ void sm_stage(const SmDev& a, const int view, const int x0, const int y0, double* __restrict__ Fs,
                                         float* __restrict__ ms, float* __restrict__ gs)
{
    constexpr int SW = SM_TW + HL + HR, SH = SM_TH + HL + HR, NP = SW * SH;
    const size_t plane = (size_t)a.H * a.W;
    const float* __restrict__ fp = a.field[view];
    const float* __restrict__ A = a.weights[view];
    const float* __restrict__ G = a.guide[view];
    const float* __restrict__ mk = a.mask[view];
    for (int i = threadIdx.x; i < NP; i += SM_BLOCK) {
        const int ly = i / SW, lx = i - ly * SW;
        const int u = x0 - HL + lx, v = y0 - HL + ly;
        double f[C];
        f[0] = sm_nan();
#pragma unroll
        for (int c = 1; c < C; ++c) f[c] = 0.0;
        float m = 0.0f, g[3] = {0.0f, 0.0f, 0.0f};
        if (u >= 0 && v >= 0 && u < a.W && v < a.H) {
            const size_t at = (size_t)v * a.W + u;
            m = mk ? mk[at] : 1.0f;                                                           // uniform
            if (C == 1) {
                f[0] = sm_depth_x(a, fp, A, mk, at);
            } else {
                const double n0 = (double)fp[at], n1 = (double)fp[plane + at], n2 = (double)fp[2 * plane + at];
                const double nn = n0 * n0 + n1 * n1 + n2 * n2;
                if (A[at] >= a.min_weight && osum::finite(nn) && nn > a.min_norm_sq && m > 0.0f) {
                    const double inv = 1.0 / sqrt(nn);
                    f[0] = n0 * inv; f[C > 1 ? 1 : 0] = n1 * inv; f[C > 2 ? 2 : 0] = n2 * inv;
                }
            }
            for (int c = 0; c < a.cg; ++c) g[c] = G[c * plane + at];                          // uniform
        }
#pragma unroll
        for (int c = 0; c < C; ++c) Fs[c * NP + i] = f[c];
        ms[i] = m;
#pragma unroll
        for (int c = 0; c < 3; ++c) gs[c * NP + i] = g[c];
    }
}

// The stencil along stride s (1: horizontal, the row stride: vertical) whose anchor (order 1) or centre (order 2) is staged at c.
// On true: w, w e and t = d / mu of its channels.  The one statement of a stencil: the sums and the adjoint.
template <int C, int ORDER, int NP>
__device__ __forceinline__ bool sm_stencil(const SmDev& a, const double* __restrict__ Fs, const float* __restrict__ ms,
                                           const float* __restrict__ gs, const int c, const int s, const double inv_mu, double& w, double& we,
                                           double (&t)[C])
{
    const int lo = ORDER == 1 ? c : c - s, hi = c + s;
    if (Fs[lo] != Fs[lo] || Fs[hi] != Fs[hi]) return false;
    if (ORDER == 2 && Fs[c] != Fs[c]) return false;
    double e = 1.0;
    if (a.cg) {                                                                               // uniform
        double g = 0.0;
        for (int k = 0; k < a.cg; ++k) g += fabs((double)gs[k * NP + hi] - (double)gs[k * NP + lo]);
        g = g * a.inv_gn;                                                                     // the mean; order 2: over two pixels
        if (!osum::finite(g)) return false;
        e = (double)expf((float)(-(a.gamma * g)));
    }
    float m = fminf(ms[lo], ms[hi]);
    if (ORDER == 2) m = fminf(m, ms[c]);
    w = (double)m;
    we = w * e;
#pragma unroll
    for (int k = 0; k < C; ++k) {
        const double d = ORDER == 1 ? Fs[k * NP + hi] - Fs[k * NP + lo] : (Fs[k * NP + lo] - 2.0 * Fs[k * NP + c]) + Fs[k * NP + hi];
        t[k] = d * inv_mu;
    }
    return true;
}

// rho1(t); dr = rho1'(t)
__device__ __forceinline__ double sm_rho(const SmDev& a, const double t, double& dr)
{
    if (a.l2) { dr = 2.0 * t; return t * t; }                                                 // uniform
    if (a.eps == 0.0) { dr = osum::sign(t); return fabs(t); }
    const double r = sqrt(t * t + a.eps * a.eps);
    dr = t / r;
    return r - a.eps;
}

// 1 / mu; 0 where the view has no usable pixel or no mean to divide by: every t is 0 then, and so are the loss and the gradients
__device__ __forceinline__ double sm_inv_mu(const double sum, const double n, double& mu)
{
    mu = n > 0.0 ? sum / n : 0.0;
    return (n > 0.0 && osum::finite(mu) && mu != 0.0) ? 1.0 / mu : 0.0;
}

// (1 / mu, mu, n) of a view from its mean rows, the same bits in every workgroup that calls this: lane l of wave 0 adds rows l,
// l + 64, ..., a butterfly leaves the wave's total, and one barrier hands it to the other waves through sh (3 doubles of LDS whose
// earlier contents are dead).  The rows are 16 bytes each and 16-byte aligned (api.hip).  Not ordered_rows_sum, on purpose: every
// workgroup of the sums kernel runs this in front of its tile, and one wave with one barrier is what that costs least; the order
// (64 rows apart, one wave) is this operator's own and its bits are promised.
__device__ __forceinline__ void sm_mean(const SmDev& a, const double* __restrict__ rows, double* __restrict__ sh, double& inv_mu, double& mu, double& n)
{
    if (threadIdx.x < 64) {
        const double2* __restrict__ r2 = reinterpret_cast<const double2*>(rows);
        double acc[2] = {0.0, 0.0};
#pragma unroll 4
        for (int r = threadIdx.x; r < a.mean_slots; r += 64) {
            const double2 t = r2[r];
            acc[0] += t.x; acc[1] += t.y;
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) acc[k] += __shfl_xor(acc[k], d);
        }
        if (threadIdx.x == 0) {                                                               // the two divisions once per workgroup
            double m;
            sh[0] = sm_inv_mu(acc[0], acc[1], m);
            sh[1] = m; sh[2] = acc[1];
        }
    }
    __syncthreads();
    inv_mu = sh[0]; mu = sh[1]; n = sh[2];
}

// Workgroup `slot` of view blockIdx.y leaves (sum x, n) of the usable pixels among its run of mean_chunk pixels.
__global__ void __launch_bounds__(SM_BLOCK) smooth_mean_kernel(const SmDev a, double* __restrict__ mean_rows)
{
    __shared__ double sh[4 * 2];
    const int view = blockIdx.y;
    const size_t HW = (size_t)a.H * a.W;
    const size_t begin = (size_t)blockIdx.x * a.mean_chunk;
    const size_t end = begin + a.mean_chunk < HW ? begin + a.mean_chunk : HW;
    const float* __restrict__ D = a.field[view];
    const float* __restrict__ A = a.weights[view];
    const float* __restrict__ mk = a.mask[view];
    double acc[2] = {0.0, 0.0};
    for (size_t i = begin + threadIdx.x; i < end; i += SM_BLOCK) {
        const double x = sm_depth_x(a, D, A, mk, i);
        if (x == x) { acc[0] += x; acc[1] += 1.0; }
    }
    osum::block_sum<2>(acc, sh);
    if (threadIdx.x < 2) mean_rows[((size_t)view * a.mean_slots + blockIdx.x) * 2 + threadIdx.x] = osum::block_total<2>(sh, threadIdx.x);
}

// Workgroup (bx, by) of view bz leaves the row (S_x, cnt_x, T_x, S_y, cnt_y, T_y) of the stencils its tile's pixels anchor.
template <int C, int ORDER, bool NORM>
__global__ void __launch_bounds__(SM_BLOCK) smooth_sums_kernel(const SmDev a, const double* __restrict__ mean_rows, double* __restrict__ partials)
{
    constexpr int HL = ORDER - 1, HR = 1, SW = SM_TW + HL + HR, SH = SM_TH + HL + HR, NP = SW * SH;
    __shared__ double Fs[C * NP];
    __shared__ float ms[NP], gs[3 * NP];
    __shared__ double sh[4 * SM_ROW];
    const int view = blockIdx.z;
    const int x0 = blockIdx.x * SM_TW, y0 = blockIdx.y * SM_TH;
    sm_stage<C, HL, HR>(a, view, x0, y0, Fs, ms, gs);
    double inv_mu = 1.0;
    if (NORM) {
        double n, mu;
        sm_mean(a, mean_rows + (size_t)view * a.mean_slots * 2, sh, inv_mu, mu, n);
    }
    __syncthreads();
    const int lx = threadIdx.x % SM_TW, ly = threadIdx.x / SM_TW;
    const int c = (ly + HL) * SW + lx + HL;                                                   // a pixel outside the image is staged NaN
    double acc[SM_ROW] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int dir = 0; dir < 2; ++dir) {
        double w, we, t[C];
        if (sm_stencil<C, ORDER, NP>(a, Fs, ms, gs, c, dir ? SW : 1, inv_mu, w, we, t)) {
            double r = 0.0, tt = 0.0;
#pragma unroll
            for (int k = 0; k < C; ++k) {
                double dr;
                r += sm_rho(a, t[k], dr);
                tt += dr * t[k];
            }
            acc[3 * dir] = we * (r * (1.0 / (double)C));
            acc[3 * dir + 1] = w;
            acc[3 * dir + 2] = we * (tt * (1.0 / (double)C));
        }
    }
    // (sh: sm_mean's reads of it are behind the barrier above)
    const int t = threadIdx.x;
    double out;
    if (NORM) {
        osum::block_sum<SM_ROW>(acc, sh);
        out = t < SM_ROW ? osum::block_total<SM_ROW>(sh, t) : 0.0;
    } else {                                                                                  // T is read only where normalised: zeros
        const double four[4] = {acc[0], acc[1], acc[3], acc[4]};
        osum::block_sum<4>(four, sh);
        out = (t < SM_ROW && t % 3 != 2) ? osum::block_total<4>(sh, t - t / 3) : 0.0;         // columns 0, 1, 3, 4
    }
    if (t < SM_ROW) {
        const size_t tile = (size_t)blockIdx.y * gridDim.x + blockIdx.x, ntiles = (size_t)gridDim.x * gridDim.y;
        partials[((size_t)view * ntiles + tile) * SM_ROW + t] = out;
    }
}

// One workgroup per view: its ntiles partial rows added in tile order (ordered_sum.h) and, where normalised, its mean; then loss,
// count and the stats row.
__global__ void __launch_bounds__(SM_BLOCK) smooth_finalize_kernel(const SmDev a, const int ntiles, const int normalised,
                                                                   const double* __restrict__ partials, const double* __restrict__ mean_rows,
                                                                   float* __restrict__ loss, float* __restrict__ count, double* __restrict__ stats)
{
    __shared__ double sh[4 * SM_ROW];
    __shared__ double shm[2 * 4];
    const int v = blockIdx.x;
    double acc[SM_ROW];
    osum::ordered_rows_sum<SM_ROW>(partials + (size_t)v * ntiles * SM_ROW, ntiles, SM_ROW, sh, acc);
    double inv_mu = 1.0, mu = 1.0, n = 0.0;
    if (normalised)                                                                           // uniform
        sm_mean(a, mean_rows + (size_t)v * a.mean_slots * 2, shm, inv_mu, mu, n);
    if (threadIdx.x != 0) return;
    const double cx = acc[1], cy = acc[4];
    const double icx = cx > 0.0 ? 1.0 / cx : 0.0, icy = cy > 0.0 ? 1.0 / cy : 0.0;
    loss[v] = (float)(acc[0] * icx + acc[3] * icy);
    count[v] = (float)(cx + cy);
    double* __restrict__ st = stats + (size_t)v * SM_STATS;
    st[0] = icx; st[1] = icy; st[2] = inv_mu; st[3] = n;
    st[4] = acc[2] * icx + acc[5] * icy;
    st[5] = cx; st[6] = cy; st[7] = mu;
}

// dL/dfield (and dL/dweights of the depth kind) of every pixel of the tile, each rounded once from double.  Phase one: the stencils
// of the tile and of its one-pixel ring leave q = cot w e rho1'(t) / (C cnt_dir mu) per channel and direction in LDS (zeros where the
// stencil is not valid).  Phase two: a pixel gathers from the stencils that contain it, left to right, then top to bottom.
// a.g_field[view] / a.g_weights[view] == nullptr: not wanted, nothing is stored; what is stored is the same bits whichever is wanted.
template <int C, int ORDER>
__global__ void __launch_bounds__(SM_BLOCK) smooth_bwd_kernel(const SmDev a, const double* __restrict__ stats, const float* __restrict__ g_loss)
{
    constexpr int SW = SM_TW + 2 * ORDER, SH = SM_TH + 2 * ORDER, NP = SW * SH;
    constexpr int CW = SM_TW + ORDER, CH = SM_TH + ORDER, NC = CW * CH;                        // stencils: from (x0 - 1, y0 - 1)
    __shared__ double Fs[C * NP];
    __shared__ float ms[NP], gs[3 * NP];
    __shared__ double gd[2][C][NC];
    const int view = blockIdx.z;
    const int x0 = blockIdx.x * SM_TW, y0 = blockIdx.y * SM_TH;
    sm_stage<C, ORDER, ORDER>(a, view, x0, y0, Fs, ms, gs);
    __syncthreads();
    const double* __restrict__ st = stats + (size_t)view * SM_STATS;
    const double cot = (double)g_loss[view], inv_mu = st[2];
    const double kdir[2] = {((cot * st[0]) * inv_mu) * (1.0 / (double)C), ((cot * st[1]) * inv_mu) * (1.0 / (double)C)};
    for (int i = threadIdx.x; i < NC; i += SM_BLOCK) {
        const int cy = i / CW, cx = i - cy * CW;
        const int c = (cy - 1 + ORDER) * SW + (cx - 1 + ORDER);
#pragma unroll
        for (int dir = 0; dir < 2; ++dir) {
            double w, we, t[C], out[C];
#pragma unroll
            for (int k = 0; k < C; ++k) out[k] = 0.0;
            if (sm_stencil<C, ORDER, NP>(a, Fs, ms, gs, c, dir ? SW : 1, inv_mu, w, we, t)) {
#pragma unroll
                for (int k = 0; k < C; ++k) {
                    double dr;
                    sm_rho(a, t[k], dr);
                    out[k] = (we * dr) * kdir[dir];
                }
            }
#pragma unroll
            for (int k = 0; k < C; ++k) gd[dir][k][i] = out[k];
        }
    }
    __syncthreads();
    const int lx = threadIdx.x % SM_TW, ly = threadIdx.x / SM_TW;
    const int u = x0 + lx, v = y0 + ly;
    if (u >= a.W || v >= a.H) return;
    const size_t at = (size_t)v * a.W + u, plane = (size_t)a.H * a.W;
    const int fc = (ly + ORDER) * SW + lx + ORDER;                                            // this pixel in the staged field
    const int sc = (ly + 1) * CW + lx + 1;                                                    // ... and as a stencil
    float gF[C], gA = 0.0f;
#pragma unroll
    for (int k = 0; k < C; ++k) gF[k] = 0.0f;
    if (Fs[fc] == Fs[fc]) {                                                                   // not usable: no stencil reads it
        double G[C];
#pragma unroll
        for (int k = 0; k < C; ++k) {
            const double* __restrict__ qx = gd[0][k];
            const double* __restrict__ qy = gd[1][k];
            if (ORDER == 1) G[k] = ((qx[sc - 1] - qx[sc]) + qy[sc - CW]) - qy[sc];
            else G[k] = ((((qx[sc - 1] - 2.0 * qx[sc]) + qx[sc + 1]) + qy[sc - CW]) - 2.0 * qy[sc]) + qy[sc + CW];
        }
        if (C == 1) {
            const double n = st[3];
            const double shift = (a.normalize && n > 0.0) ? ((cot * st[4]) * inv_mu) / n : 0.0;
            const double gx = G[0] - shift, x = Fs[fc];
            // inverse: x = A / D;  depth: x = D / A -- `den` is the map under the division, `num` the one above it
            const double den = (double)(a.inverse ? a.field[view][at] : a.weights[view][at]);
            const double iden = 1.0 / den;
            const float g_num = (float)(gx * iden), g_den = (float)(-((x * iden) * gx));
            gF[0] = a.inverse ? g_den : g_num;
            gA = a.inverse ? g_num : g_den;
        } else {
            const float* __restrict__ fp = a.field[view];
            const double n0 = (double)fp[at], n1 = (double)fp[plane + at], n2 = (double)fp[2 * plane + at];
            const double inv = 1.0 / sqrt(n0 * n0 + n1 * n1 + n2 * n2);
            double ng = 0.0;
#pragma unroll
            for (int k = 0; k < C; ++k) ng += Fs[k * NP + fc] * G[k];
#pragma unroll
            for (int k = 0; k < C; ++k) gF[k] = (float)((G[k] - Fs[k * NP + fc] * ng) * inv);
        }
    }
    float* __restrict__ gf = a.g_field[view];
    float* __restrict__ gw = a.g_weights[view];
    if (gf) {                                                                                 // uniform
#pragma unroll
        for (int k = 0; k < C; ++k) gf[k * plane + at] = gF[k];
    }
    if (C == 1 && gw) gw[at] = gA;
}

static inline int sm_tiles_x(int W) { return (W + SM_TW - 1) / SM_TW; }
static inline int sm_tiles_y(int H) { return (H + SM_TH - 1) / SM_TH; }
// workgroups (= partial rows) per view of the sums kernel, and of the mean kernel: functions of the image size alone
long long smooth_tiles(int H, int W) { return (long long)sm_tiles_x(W) * sm_tiles_y(H); }
int smooth_mean_slots(int H, int W)
{
    const long long blocks = ((long long)H * W + SM_BLOCK - 1) / SM_BLOCK;
    return (int)(blocks < SM_SLOTS ? blocks : SM_SLOTS);
}

static SmDev sm_dev(const BagsSmooth& a, float* const* g_field, float* const* g_weights)
{
    SmDev d{};
    d.H = a.H; d.W = a.W;
    d.cg = a.guide_channels;
    d.inverse = a.kind == BAGS_SMOOTH_DEPTH && a.space == BAGS_DEPTH_PRIOR_INVERSE;
    d.l2 = a.penalty == BAGS_SMOOTH_L2;
    d.normalize = a.kind == BAGS_SMOOTH_DEPTH && a.normalize != 0;
    d.mean_slots = smooth_mean_slots(a.H, a.W);
    const long long HW = (long long)a.H * a.W;
    d.mean_chunk = (unsigned)((HW + d.mean_slots - 1) / d.mean_slots);
    d.min_weight = a.min_weight;
    d.min_norm_sq = (double)a.min_norm * (double)a.min_norm;
    d.eps = a.eps; d.gamma = a.gamma;
    d.inv_gn = d.cg ? 1.0 / (double)(d.cg * a.order) : 0.0;
    for (int k = 0; k < BAGS_MAX_POSE_ROWS; ++k) {
        const bool on = k < a.n_rows;
        d.field[k] = on ? a.field[k] : nullptr;
        d.weights[k] = on ? a.weights[k] : nullptr;
        d.guide[k] = (on && d.cg) ? a.guide[k] : nullptr;
        d.mask[k] = on ? a.mask[k] : nullptr;
        d.g_field[k] = (on && g_field) ? g_field[k] : nullptr;
        d.g_weights[k] = (on && g_weights && a.kind == BAGS_SMOOTH_DEPTH) ? g_weights[k] : nullptr;
    }
    return d;
}

// f(C, ORDER) with the two as compile-time constants
template <typename F> static inline hipError_t sm_dispatch(const BagsSmooth& a, F f)
{
    return with_bool(a.kind == BAGS_SMOOTH_DEPTH, [&](auto DEPTH) {
        return with_bool(a.order == 1, [&](auto FIRST) {
            return f(std::integral_constant<int, decltype(DEPTH)::value ? 1 : 3>{}, std::integral_constant<int, decltype(FIRST)::value ? 1 : 2>{});
        });
    });
}

// the struct is validated by the caller (api.hip); partials: n_rows * smooth_tiles(H, W) rows of 6 doubles; mean_rows: n_rows *
// smooth_mean_slots(H, W) rows of 2 doubles (read and written only where the depth kind is normalised)
hipError_t launch_smooth_fwd(const BagsSmooth& a, double* partials, double* mean_rows, float* loss, float* count, double* stats, hipStream_t st)
{
    const SmDev d = sm_dev(a, nullptr, nullptr);
    if (d.normalize) {
        hipLaunchKernelGGL(smooth_mean_kernel, dim3(d.mean_slots, a.n_rows), dim3(SM_BLOCK), 0, st, d, mean_rows);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const dim3 grid(sm_tiles_x(a.W), sm_tiles_y(a.H), a.n_rows);
    const hipError_t e = sm_dispatch(a, [&](auto C, auto ORDER) {
        return with_bool(d.normalize != 0, [&](auto NORM) {
            // (the normal kind is never normalised: that instance is not reached)
            hipLaunchKernelGGL((smooth_sums_kernel<decltype(C)::value, decltype(ORDER)::value, decltype(NORM)::value>), grid, dim3(SM_BLOCK), 0, st,
                               d, mean_rows, partials);
            return hipGetLastError(); }); });
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(smooth_finalize_kernel, dim3(a.n_rows), dim3(SM_BLOCK), 0, st, d, (int)smooth_tiles(a.H, a.W), d.normalize, partials, mean_rows,
                       loss, count, stats);
    return hipGetLastError();
}

// g_field / g_weights: NULL or n_rows pointers of which any may be NULL; at least one output is wanted (api.hip)
hipError_t launch_smooth_bwd(const BagsSmooth& a, const double* stats, const float* g_loss, float* const* g_field, float* const* g_weights,
                             hipStream_t st)
{
    const SmDev d = sm_dev(a, g_field, g_weights);
    const dim3 grid(sm_tiles_x(a.W), sm_tiles_y(a.H), a.n_rows);
    return sm_dispatch(a, [&](auto C, auto ORDER) {
        hipLaunchKernelGGL((smooth_bwd_kernel<decltype(C)::value, decltype(ORDER)::value>), grid, dim3(SM_BLOCK), 0, st, d, stats, g_loss);
        return hipGetLastError(); });
}
