// bilagrid.hip -- per-image bilateral-grid colour on the rendered image (gsplat's lib_bilagrid), behind the AppearanceBank step and in
// front of the loss, and the total variation of the grids.  A view's grid G is (12, L, Gy, Gx): coefficient k = 4*c + j is entry
// [c][j] of a 3x4 affine matrix.  Per pixel (x, y) of a (3,H,W) image with channels p_0..p_2:
//     u = (x + 0.5) / W * (Gx - 1) ;  x0 = min(floor(u), Gx-1) ;  x1 = min(x0+1, Gx-1) ;  tx = u - x0        (y likewise)
//     luma = 0.299 p_0 + 0.587 p_1 + 0.114 p_2 ;  s = luma * (L-1) ;  w = clamp(s, 0, L-1)
//     z0 = min(floor(w), L-1) ;  z1 = min(z0+1, L-1) ;  tz = w - z0 ;  lerp(a, b, t) = a + t * (b - a)
//     plane(z) = lerp(lerp(G[k,z,y0,x0], G[k,z,y0,x1], tx), lerp(G[k,z,y1,x0], G[k,z,y1,x1], tx), ty)
//     A[k] = lerp(plane(z0), plane(z1), tz) ;  out_c = A[4c] p_0 + A[4c+1] p_1 + A[4c+2] p_2 + A[4c+3]
// and for a cotangent g, with dA[4c+j] = g_c p_j, dA[4c+3] = g_c:
//     dL/dp_j = sum_c g_c A[4c+j] + (0 < s < L-1 ? dtz * (L-1) * (0.299, 0.587, 0.114)_j : 0) ,  dtz = sum_k dA[k] * (plane(z1)[k] - plane(z0)[k])
//     dL/dG through the lerps:  d lerp / db = t * d ,  d lerp / da = d - t * d
//
// Slice kernels (forward, dL/dimage): a thread is a pixel, a workgroup a tile of BG_TILE_W x BG_TILE_H pixels, the views of a call
// grid dimension y; pointers and rows arrive by value.  A tile whose pixels reach at most BG_STAGE_VERTS xy-vertices stages those
// vertices' L x 12 coefficients in LDS (k innermost: a corner's 12 coefficients are three 16-byte reads); any other tile -- an image
// smaller than its grid -- reads the grid directly.  Both spell the same operations on the same values and the file is compiled with
// -ffp-contract=off: the same bits.
//
// dL/dgrid: one workgroup per (xy-vertex, output channel c, view).  It walks the vertex's support rectangle (about 2W/(Gx-1) x
// 2H/(Gy-1) pixels; the rectangle is a conservative bound, membership is decided per pixel by the forward's own x0, x1, y0, y1), a
// lane adds a pixel's terms into L x 4 double accumulators with predicated adds for its two live z-bins; the workgroup adds its
// lanes (ordered_sum.h), and every one of the vertex's L x 4 elements is rounded once and written -- zeros where no pixel reaches.
// The workgroups behind them write zeros into the rows that are not listed.  No atomics, no memset, no workspace; a view's gradient
// is its own workgroups' alone.
//
// Total variation: a partials kernel with a workgroup count decided by the element count alone and a one-workgroup finalize; the
// backward is a gather.
#include "ordered_sum.h"

#define BG_TILE_W BAGS_BILAGRID_TILE_W
#define BG_TILE_H BAGS_BILAGRID_TILE_H
#define BG_BLOCK (BG_TILE_W * BG_TILE_H)
#define BG_STAGE_VERTS BAGS_BILAGRID_STAGE_VERTS
#define BG_MAX_L BAGS_BILAGRID_MAX_L
#define BG_TV_BLOCK BAGS_BILAGRID_TV_BLOCK
static_assert(BG_BLOCK == 256 && BG_TV_BLOCK == 256, "four waves: block_sum's default, and ordered_rows_sum's 256 threads");

struct BgDev {
    const float* grids;                              // (N,12,L,Gy,Gx)
    int H, W, Gx, Gy, L;
    int tiles_x, tiles_y;
    int direct;                                      // path == BAGS_BILAGRID_PATH_DIRECT: no tile stages
    int N, n_rows;
    int rows[BAGS_MAX_POSE_ROWS];
    const float* image[BAGS_MAX_POSE_ROWS];
    float* out[BAGS_MAX_POSE_ROWS];                  // forward: the outputs; backward: dL/dimage, any of them NULL
    const float* g[BAGS_MAX_POSE_ROWS];              // backward: the cotangents
};

__device__ __forceinline__ float bg_lerp(const float a, const float b, const float t) { return a + t * (b - a); }

// pixel index i of n along an axis with G vertices
__device__ __forceinline__ void bg_axis(const int i, const int n, const int G, int& i0, int& i1, float& t)
{
    const float u = ((float)i + 0.5f) / (float)n * (float)(G - 1);
    i0 = min((int)floorf(u), G - 1);
    i1 = min(i0 + 1, G - 1);
    t = u - (float)i0;
}

// the guidance axis; live: 0 < s < L-1, where tz follows the pixel
__device__ __forceinline__ void bg_guide(const float p0, const float p1, const float p2, const int L, int& z0, int& z1, float& tz, bool& live)
{
    const float luma = 0.299f * p0 + 0.587f * p1 + 0.114f * p2;
    const float top = (float)(L - 1);
    const float s = luma * top;
    const float w = fminf(fmaxf(s, 0.0f), top);      // (a NaN luma lands on 0: every index stays inside the grid)
    z0 = min((int)floorf(w), L - 1);
    z1 = min(z0 + 1, L - 1);
    tz = w - (float)z0;
    live = s > 0.0f && s < top;
}

struct BgPixel { int x0, x1, y0, y1, z0, z1; float tx, ty, tz; bool live; };

// plane(z0)[k] and plane(z1)[k] for k = 0..11 through `at(k, z, y, x)`
template <typename At>
__device__ __forceinline__ void bg_planes(const BgPixel& q, const At at, float (&P0)[12], float (&P1)[12])
{
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        P0[k] = bg_lerp(bg_lerp(at(k, q.z0, q.y0, q.x0), at(k, q.z0, q.y0, q.x1), q.tx),
                        bg_lerp(at(k, q.z0, q.y1, q.x0), at(k, q.z0, q.y1, q.x1), q.tx), q.ty);
        P1[k] = bg_lerp(bg_lerp(at(k, q.z1, q.y0, q.x0), at(k, q.z1, q.y0, q.x1), q.tx),
                        bg_lerp(at(k, q.z1, q.y1, q.x0), at(k, q.z1, q.y1, q.x1), q.tx), q.ty);
    }
}

// BWD == false: out = A p.  BWD == true: dL/dimage from the cotangent.  One tile per workgroup.
template <bool BWD>
__global__ void __launch_bounds__(BG_BLOCK) bilagrid_slice_kernel(const BgDev a)
{
    __shared__ __attribute__((aligned(16))) float lds[BG_STAGE_VERTS * BG_MAX_L * 12];
    const int v = blockIdx.y;
    float* __restrict__ out = a.out[v];
    if (BWD && !out) return;                                                               // uniform: this view's dL/dimage is not wanted
    const int ty_ = (int)blockIdx.x / a.tiles_x, tx_ = (int)blockIdx.x - ty_ * a.tiles_x;
    const int px0 = tx_ * BG_TILE_W, py0 = ty_ * BG_TILE_H;
    const int px1 = min(px0 + BG_TILE_W, a.W) - 1, py1 = min(py0 + BG_TILE_H, a.H) - 1;   // the tile's last pixel, inside the image
    const float* __restrict__ G = a.grids + (size_t)a.rows[v] * 12 * a.L * a.Gy * a.Gx;
    const int L = a.L, Gx = a.Gx, Gy = a.Gy;

    // the xy-vertices the tile reaches: x0 of its first pixel .. x1 of its last (u does not decrease with the pixel index)
    int vx_lo, vx_hi, vy_lo, vy_hi, unused;
    float tunused;
    bg_axis(px0, a.W, Gx, vx_lo, unused, tunused);
    bg_axis(px1, a.W, Gx, unused, vx_hi, tunused);
    bg_axis(py0, a.H, Gy, vy_lo, unused, tunused);
    bg_axis(py1, a.H, Gy, unused, vy_hi, tunused);
    const int nvx = vx_hi - vx_lo + 1, nvy = vy_hi - vy_lo + 1;
    const bool staged = !a.direct && nvx * nvy <= BG_STAGE_VERTS;                          // uniform
    if (staged) {
        const int n = nvx * nvy * L * 12;                                                  // <= BG_STAGE_VERTS * BG_MAX_L * 12
        for (int i = threadIdx.x; i < n; i += BG_BLOCK) {
            const int lx = i % nvx, r1 = i / nvx, ly = r1 % nvy, r2 = r1 / nvy, z = r2 % L, k = r2 / L;
            lds[((ly * nvx + lx) * L + z) * 12 + k] = G[(((size_t)k * L + z) * Gy + (vy_lo + ly)) * Gx + (vx_lo + lx)];
        }
        __syncthreads();
    }
    const int x = px0 + (int)(threadIdx.x % BG_TILE_W), y = py0 + (int)(threadIdx.x / BG_TILE_W);
    if (x >= a.W || y >= a.H) return;
    const size_t plane = (size_t)a.H * a.W, at = (size_t)y * a.W + x;
    const float* __restrict__ img = a.image[v];
    const float p0 = img[at], p1 = img[plane + at], p2 = img[2 * plane + at];
    BgPixel q;
    bg_axis(x, a.W, Gx, q.x0, q.x1, q.tx);
    bg_axis(y, a.H, Gy, q.y0, q.y1, q.ty);
    bg_guide(p0, p1, p2, L, q.z0, q.z1, q.tz, q.live);
    float P0[12], P1[12], A[12];
    if (staged) {
        // a corner's 12 coefficients are contiguous and 16-byte aligned: the compiler reads them as three b128
        bg_planes(q, [&](int k, int z, int yy, int xx) { return lds[(((yy - vy_lo) * nvx + (xx - vx_lo)) * L + z) * 12 + k]; }, P0, P1);
    } else {
        bg_planes(q, [&](int k, int z, int yy, int xx) { return G[(((size_t)k * L + z) * Gy + yy) * Gx + xx]; }, P0, P1);
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) A[k] = bg_lerp(P0[k], P1[k], q.tz);
    if (!BWD) {
#pragma unroll
        for (int c = 0; c < 3; ++c) out[c * plane + at] = A[4 * c] * p0 + A[4 * c + 1] * p1 + A[4 * c + 2] * p2 + A[4 * c + 3];
    } else {
        const float* __restrict__ gout = a.g[v];
        const float g[3] = {gout[at], gout[plane + at], gout[2 * plane + at]};
        const float p[3] = {p0, p1, p2};
        float dtz = 0.0f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
            for (int j = 0; j < 3; ++j) dtz += (g[c] * p[j]) * (P1[4 * c + j] - P0[4 * c + j]);
            dtz += g[c] * (P1[4 * c + 3] - P0[4 * c + 3]);
        }
        const float guide = q.live ? dtz * (float)(L - 1) : 0.0f;
        const float coef[3] = {0.299f, 0.587f, 0.114f};
#pragma unroll
        for (int j = 0; j < 3; ++j) out[j * plane + at] = (g[0] * A[j] + g[1] * A[4 + j] + g[2] * A[8 + j]) + guide * coef[j];
    }
}

// what d (the cotangent of a row's lerp result) leaves at vertex vx of the row's two corners x0, x1
__device__ __forceinline__ float bg_to_x(const float d, const BgPixel& q, const int vx)
{
    const float db = q.tx * d, da = d - db;
    return (q.x0 == vx ? da : 0.0f) + (q.x1 == vx ? db : 0.0f);
}
// ... and d (the cotangent of plane(z)) at xy-vertex (vx, vy)
__device__ __forceinline__ float bg_to_xy(const float d, const BgPixel& q, const int vx, const int vy)
{
    const float db = q.ty * d, da = d - db;
    return (q.y0 == vy ? bg_to_x(da, q, vx) : 0.0f) + (q.y1 == vy ? bg_to_x(db, q, vx) : 0.0f);
}

// Workgroup b < n_rows * Gx * Gy * 3: view b / (Gx Gy 3), vertex (b / 3) % (Gx Gy), channel c = b % 3 -- the elements
// g_grids[rows[v]][4c + j][z][vy][vx], j < 4, z < L, every one of them.  The workgroups behind: zeros into every row not listed.
template <int LMAX>
__global__ void __launch_bounds__(BG_BLOCK) bilagrid_grid_bwd_kernel(const BgDev a, float* __restrict__ g_grids)
{
    const int L = a.L, Gx = a.Gx, Gy = a.Gy;
    const unsigned per_view = (unsigned)(Gx * Gy * 3), sums = per_view * (unsigned)a.n_rows;
    const size_t row_elems = (size_t)12 * L * Gy * Gx;
    if (blockIdx.x >= sums) {                                                              // uniform
        const size_t e = (size_t)(blockIdx.x - sums) * BG_BLOCK + threadIdx.x;
        if (e >= (size_t)a.N * row_elems) return;
        const int r = (int)(e / row_elems);
        bool listed = false;
#pragma unroll
        for (int k = 0; k < BAGS_MAX_POSE_ROWS; ++k) listed |= (k < a.n_rows && a.rows[k] == r);
        if (!listed) g_grids[e] = 0.0f;
        return;
    }
    __shared__ double sh[BG_BLOCK / 64 * LMAX * 4];
    const int v = (int)(blockIdx.x / per_view), rest = (int)(blockIdx.x - (unsigned)v * per_view);
    const int c = rest % 3, vert = rest / 3, vy = vert / Gx, vx = vert - vy * Gx;
    // a bound of the pixels with x0 == vx or x1 == vx: u in [vx-1, vx+1), widened by two pixels against the rounding of u
    int xlo = 0, xhi = a.W - 1, ylo = 0, yhi = a.H - 1;
    if (Gx > 1) {
        xlo = max(0, (int)(((long long)(vx - 1) * a.W) / (Gx - 1)) - 2);
        xhi = min(a.W - 1, (int)(((long long)(vx + 1) * a.W + (Gx - 2)) / (Gx - 1)) + 2);
    }
    if (Gy > 1) {
        ylo = max(0, (int)(((long long)(vy - 1) * a.H) / (Gy - 1)) - 2);
        yhi = min(a.H - 1, (int)(((long long)(vy + 1) * a.H + (Gy - 2)) / (Gy - 1)) + 2);
    }
    const int rw = xhi - xlo + 1, rh = yhi - ylo + 1;                                      // (vx = 0 with Gx > 1: xlo = 0 after the clamp)
    const unsigned npix = (rw > 0 && rh > 0) ? (unsigned)rw * (unsigned)rh : 0u;           // below 2^31: the rectangle is inside the image
    const size_t plane = (size_t)a.H * a.W;
    const float* __restrict__ img = a.image[v];
    const float* __restrict__ gc = a.g[v] + (size_t)c * plane;
    double acc[LMAX * 4];                                                                  // [z][j]
#pragma unroll
    for (int t = 0; t < LMAX * 4; ++t) acc[t] = 0.0;

    for (unsigned i = threadIdx.x; i < npix; i += BG_BLOCK) {
        const int yy = (int)(i / (unsigned)rw), y = ylo + yy, x = xlo + (int)(i - (unsigned)yy * (unsigned)rw);
        BgPixel q;
        bg_axis(x, a.W, Gx, q.x0, q.x1, q.tx);
        bg_axis(y, a.H, Gy, q.y0, q.y1, q.ty);
        if ((q.x0 != vx && q.x1 != vx) || (q.y0 != vy && q.y1 != vy)) continue;
        const size_t at = (size_t)y * a.W + x;
        const float p0 = img[at], p1 = img[plane + at], p2 = img[2 * plane + at], g = gc[at];
        bg_guide(p0, p1, p2, L, q.z0, q.z1, q.tz, q.live);
        const float dA[4] = {g * p0, g * p1, g * p2, g};
        float t0[4], t1[4];                                                                // what the pixel leaves in bins z0 and z1
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float d1 = q.tz * dA[j], d0 = dA[j] - d1;
            t0[j] = bg_to_xy(d0, q, vx, vy);
            t1[j] = bg_to_xy(d1, q, vx, vy);
        }
#pragma unroll
        for (int z = 0; z < LMAX; ++z)
#pragma unroll
            for (int j = 0; j < 4; ++j)                                                    // (z1 == z0 only where tz == 0: t1 is zero there)
                acc[z * 4 + j] += (double)((z == q.z0) ? t0[j] : ((z == q.z1) ? t1[j] : 0.0f));
    }
    osum::block_sum<LMAX * 4>(acc, sh);                                                    // every lane is here
    if ((int)threadIdx.x < L * 4) {
        const int z = threadIdx.x >> 2, j = threadIdx.x & 3;
        g_grids[(size_t)a.rows[v] * row_elems + (((size_t)(4 * c + j) * L + z) * Gy + vy) * Gx + vx] = (float)osum::block_total<LMAX * 4>(sh, threadIdx.x);
    }
}

// ---- total variation ------------------------------------------------------------------------------------------------------------
// the sums of the squared forward differences along x, y, z over the workgroup's elements (e, e + stride, ...), as a row of 4 doubles
__global__ void __launch_bounds__(BG_TV_BLOCK) bilagrid_tv_partials_kernel(const float* __restrict__ X, const size_t E, const int Gx, const int Gy,
                                                                           const int L, double* __restrict__ partials)
{
    __shared__ double sh[BG_TV_BLOCK / 64 * 3];
    double acc[3] = {0.0, 0.0, 0.0};
    const size_t sy = (size_t)Gx, sz = (size_t)Gx * Gy;
    for (size_t e = (size_t)blockIdx.x * BG_TV_BLOCK + threadIdx.x; e < E; e += (size_t)gridDim.x * BG_TV_BLOCK) {
        const int ix = (int)(e % Gx), iy = (int)((e / sy) % Gy), iz = (int)((e / sz) % L);
        const float x = X[e];
        if (ix + 1 < Gx) { const double d = (double)(X[e + 1] - x); acc[0] += d * d; }
        if (iy + 1 < Gy) { const double d = (double)(X[e + sy] - x); acc[1] += d * d; }
        if (iz + 1 < L) { const double d = (double)(X[e + sz] - x); acc[2] += d * d; }
    }
    osum::block_sum<3>(acc, sh);
    if (threadIdx.x < 4) partials[(size_t)blockIdx.x * 4 + threadIdx.x] = threadIdx.x < 3 ? osum::block_total<3>(sh, threadIdx.x) : 0.0;
}

// 1 / (12 * (n_d - 1) * the other two sizes), 0 for an axis of one vertex
__host__ __device__ static inline double bg_tv_scale(const int n, const int o1, const int o2)
{
    return n >= 2 ? 1.0 / (12.0 * (double)(n - 1) * (double)o1 * (double)o2) : 0.0;
}

// one workgroup: the nblk rows added in row order (ordered_sum.h), then the one scalar
__global__ void __launch_bounds__(BG_TV_BLOCK) bilagrid_tv_finalize_kernel(const double* __restrict__ partials, const int nblk, const int N, const int Gx,
                                                                           const int Gy, const int L, float* __restrict__ loss)
{
    __shared__ double sh[BG_TV_BLOCK / 64 * 3];
    double tot[3];
    osum::ordered_rows_sum<3>(partials, nblk, 4, sh, tot);
    if (threadIdx.x == 0) {
        const double sum = (tot[0] * bg_tv_scale(Gx, Gy, L) + tot[1] * bg_tv_scale(Gy, Gx, L)) + tot[2] * bg_tv_scale(L, Gx, Gy);
        loss[0] = (float)(sum / (double)N);
    }
}

// every element: g * 2 / (N count_d) * ((x_i - x_{i-1}) - (x_{i+1} - x_i)) over the axes, a difference that does not exist counting 0
__global__ void __launch_bounds__(BG_TV_BLOCK) bilagrid_tv_bwd_kernel(const float* __restrict__ X, const size_t E, const int N, const int Gx, const int Gy,
                                                                      const int L, const float* __restrict__ g_loss, float* __restrict__ g_grids)
{
    const size_t e = (size_t)blockIdx.x * BG_TV_BLOCK + threadIdx.x;
    if (e >= E) return;
    const size_t sy = (size_t)Gx, sz = (size_t)Gx * Gy;
    const int ix = (int)(e % Gx), iy = (int)((e / sy) % Gy), iz = (int)((e / sz) % L);
    const float x = X[e];
    const double lo[3] = {ix > 0 ? (double)(x - X[e - 1]) : 0.0, iy > 0 ? (double)(x - X[e - sy]) : 0.0, iz > 0 ? (double)(x - X[e - sz]) : 0.0};
    const double hi[3] = {ix + 1 < Gx ? (double)(X[e + 1] - x) : 0.0, iy + 1 < Gy ? (double)(X[e + sy] - x) : 0.0,
                          iz + 1 < L ? (double)(X[e + sz] - x) : 0.0};
    const double sum = ((lo[0] - hi[0]) * bg_tv_scale(Gx, Gy, L) + (lo[1] - hi[1]) * bg_tv_scale(Gy, Gx, L)) + (lo[2] - hi[2]) * bg_tv_scale(L, Gx, Gy);
    g_grids[e] = (float)((double)g_loss[0] * 2.0 / (double)N * sum);
}

// workgroups (= partial rows) of the TV forward: a function of the element count alone
int bilagrid_tv_blocks(long long elems)
{
    const long long want = (elems + BG_TV_BLOCK - 1) / BG_TV_BLOCK;
    return (int)(want < 1 ? 1 : (want > BAGS_BILAGRID_TV_MAX_BLOCKS ? BAGS_BILAGRID_TV_MAX_BLOCKS : want));
}

static BgDev bg_dev(const BagsBilagrid& a, const float* const* g_out, float* const* outs)
{
    BgDev d{};
    d.grids = a.grids; d.H = a.H; d.W = a.W; d.Gx = a.Gx; d.Gy = a.Gy; d.L = a.L;
    d.tiles_x = (a.W + BG_TILE_W - 1) / BG_TILE_W; d.tiles_y = (a.H + BG_TILE_H - 1) / BG_TILE_H;
    d.direct = a.path == BAGS_BILAGRID_PATH_DIRECT;
    d.N = a.N; d.n_rows = a.n_rows;
    for (int k = 0; k < BAGS_MAX_POSE_ROWS; ++k) {
        const bool on = k < a.n_rows;
        d.rows[k] = on ? a.rows[k] : -1;
        d.image[k] = on ? a.image[k] : nullptr;
        d.out[k] = (on && outs) ? outs[k] : nullptr;
        d.g[k] = (on && g_out) ? g_out[k] : nullptr;
    }
    return d;
}

// the struct is validated by the caller (api.hip): rows distinct and in range, sizes in range, H * W below 2^31, pointers given
hipError_t launch_bilagrid_fwd(const BagsBilagrid& a, hipStream_t st)
{
    const BgDev d = bg_dev(a, nullptr, a.out);
    hipLaunchKernelGGL((bilagrid_slice_kernel<false>), dim3((unsigned)d.tiles_x * (unsigned)d.tiles_y, a.n_rows), dim3(BG_BLOCK), 0, st, d);
    return hipGetLastError();
}

// g_image: NULL or n_rows pointers, any of them NULL; g_grids: NULL or (N,12,L,Gy,Gx).  At most two launches.
hipError_t launch_bilagrid_bwd(const BagsBilagrid& a, const float* const* g_out, float* const* g_image, float* g_grids, hipStream_t st)
{
    const BgDev d = bg_dev(a, g_out, g_image);
    if (g_image) {
        hipLaunchKernelGGL((bilagrid_slice_kernel<true>), dim3((unsigned)d.tiles_x * (unsigned)d.tiles_y, a.n_rows), dim3(BG_BLOCK), 0, st, d);
        if (const hipError_t e = hipGetLastError()) return e;
    }
    if (!g_grids) return hipSuccess;
    const size_t elems = (size_t)a.N * 12 * a.L * a.Gy * a.Gx;
    const size_t blocks = (size_t)a.n_rows * a.Gx * a.Gy * 3 + (elems + BG_BLOCK - 1) / BG_BLOCK;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    return with_bool(a.L > 8, [&](auto DEEP) {
        hipLaunchKernelGGL((bilagrid_grid_bwd_kernel<decltype(DEEP)::value ? BG_MAX_L : 8>), dim3((unsigned)blocks), dim3(BG_BLOCK), 0, st, d, g_grids);
        return hipGetLastError(); });
}

// partials: bilagrid_tv_blocks(elems) rows of 4 doubles
hipError_t launch_bilagrid_tv_fwd(const float* grids, int N, int Gx, int Gy, int L, double* partials, float* loss, hipStream_t st)
{
    const size_t E = (size_t)N * 12 * L * Gy * Gx;
    const int nblk = bilagrid_tv_blocks((long long)E);
    hipLaunchKernelGGL(bilagrid_tv_partials_kernel, dim3(nblk), dim3(BG_TV_BLOCK), 0, st, grids, E, Gx, Gy, L, partials);
    if (const hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(bilagrid_tv_finalize_kernel, dim3(1), dim3(BG_TV_BLOCK), 0, st, partials, nblk, N, Gx, Gy, L, loss);
    return hipGetLastError();
}

hipError_t launch_bilagrid_tv_bwd(const float* grids, int N, int Gx, int Gy, int L, const float* g_loss, float* g_grids, hipStream_t st)
{
    const size_t E = (size_t)N * 12 * L * Gy * Gx;
    const size_t blocks = (E + BG_TV_BLOCK - 1) / BG_TV_BLOCK;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bilagrid_tv_bwd_kernel, dim3((unsigned)blocks), dim3(BG_TV_BLOCK), 0, st, grids, E, N, Gx, Gy, L, g_loss, g_grids);
    return hipGetLastError();
}
