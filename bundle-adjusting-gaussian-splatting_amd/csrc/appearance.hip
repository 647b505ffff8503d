// appearance.hip -- per-camera appearance on the rendered image, between the resample and the loss: an even radial vignetting
// polynomial, then upstream 3DGS's 3x4 exposure matrix.  Row r of the (N,16) table is E (3,4) row-major | k1 k2 k3 | unused.
// Per pixel (x, y) with channels p_0..p_2, centre (cx, cy) and s2 = (W*W + H*H) / 4:
//     dx = x + 0.5 - cx ; dy = y + 0.5 - cy ; r2 = (dx*dx + dy*dy) / s2
//     f  = 1 + r2*(k1 + r2*(k2 + r2*k3))
//     q_k = f * p_k
//     out_c = q_0*E[0][c] + q_1*E[1][c] + q_2*E[2][c] + E[c][3]
// and for a cotangent g, with t_k = g_0*E[k][0] + g_1*E[k][1] + g_2*E[k][2]:
//     dL/dp_k = f * t_k ;  dL/dE[k][c] = sum g_c*q_k ;  dL/dE[c][3] = sum g_c ;  dL/dk_j = sum r2^(j+1) * (p_0*t_0 + p_1*t_1 + p_2*t_2)
//
// A thread takes a quad: four consecutive pixels of one image row (the last quad of a row may be short), as one float4 per
// channel where W % 4 == 0 and every base is 16-byte aligned, element by element otherwise.  Both instances spell the same
// operations and the file is compiled with -ffp-contract=off, so they give the same bits.  The views of a call are grid
// dimension y; their pointers and table rows arrive by value, and a view's row is read through wave-uniform addresses.
//
// The 15 sums of a view: a lane adds its terms in double; after its last tile the workgroup adds its lanes (ordered_sum.h) and
// leaves one row of 16 doubles, the 16th a zero it writes.  A view has appearance_slots(H, W) workgroups whatever the number of
// views, so its rows -- and the table kernel's sum of them in row order (ordered_sum.h) -- are the same in a 16-view call and in a
// call of its own.  No atomics, no memset.
#include "ordered_sum.h"

#define APP_BLOCK BAGS_APPEARANCE_BLOCK
#define APP_VALS 15                                  // sums per view; the 16th column of a row is unused

struct AppDev {
    const float* table;
    int H, W, Q;                                     // Q: quads per image row
    unsigned nquads, ntiles;                         // per view; a tile is APP_BLOCK quads
    float cx, cy, s2;
    int N, n_rows;
    int rows[BAGS_MAX_POSE_ROWS];
    const float* image[BAGS_MAX_POSE_ROWS];
    float* out[BAGS_MAX_POSE_ROWS];                  // forward: the outputs; backward: dL/dimage, any of them NULL
    const float* g[BAGS_MAX_POSE_ROWS];              // backward: the cotangents
};

struct AppRow { float e[3][4]; float k1, k2, k3; };
__device__ __forceinline__ AppRow app_row(const float* __restrict__ t)
{
    AppRow r;
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int c = 0; c < 4; ++c) r.e[k][c] = t[4 * k + c];
    r.k1 = t[12]; r.k2 = t[13]; r.k3 = t[14];
    return r;
}

__device__ __forceinline__ float app_r2(const AppDev& a, const int x, const int y)
{
    const float dx = ((float)x + 0.5f) - a.cx, dy = ((float)y + 0.5f) - a.cy;
    return (dx * dx + dy * dy) / a.s2;
}
__device__ __forceinline__ float app_falloff(const AppRow& R, const float r2) { return 1.0f + r2 * (R.k1 + r2 * (R.k2 + r2 * R.k3)); }

template <bool VEC>
__global__ void __launch_bounds__(APP_BLOCK) appearance_fwd_kernel(const AppDev a)
{
    const int v = blockIdx.y;
    const AppRow R = app_row(a.table + (size_t)a.rows[v] * 16);
    const unsigned q = blockIdx.x * APP_BLOCK + threadIdx.x;
    if (q >= a.nquads) return;
    const int y = (int)(q / (unsigned)a.Q), x0 = 4 * (int)(q - (unsigned)y * (unsigned)a.Q);
    const int n = VEC ? 4 : min(4, a.W - x0);                                                // (VEC: W % 4 == 0)
    const size_t plane = (size_t)a.H * a.W, at = (size_t)y * a.W + x0;
    const float* __restrict__ img = a.image[v];
    float* __restrict__ out = a.out[v];
    float p[3][4], o[3][4];
#pragma unroll
    for (int k = 0; k < 3; ++k) osum::load4<VEC>(img + k * plane + at, n, p[k]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float f = app_falloff(R, app_r2(a, x0 + j, y));
        const float q0 = f * p[0][j], q1 = f * p[1][j], q2 = f * p[2][j];
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c][j] = q0 * R.e[0][c] + q1 * R.e[1][c] + q2 * R.e[2][c] + R.e[c][3];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) osum::store4<VEC>(out + c * plane + at, n, o[c]);
}

// Workgroup `slot` of view v walks the tiles slot, slot + nslots, ...  SUMS == false: the table gradient is not wanted, the image
// is not read and nothing is summed (an instance of its own, not a branch: behind a run-time test the compiler sinks a part of the
// image loads into the branch, a second round trip per tile); a.out[v] == nullptr: dL/dimage of that view is not wanted and
// nothing is stored.  What a pixel contributes to either is formed by the same operations whichever is wanted.
template <bool VEC, bool SUMS>
__global__ void __launch_bounds__(APP_BLOCK) appearance_bwd_kernel(const AppDev a, double* __restrict__ partials)
{
    __shared__ double sh[APP_BLOCK / 64 * 16];
    const int v = blockIdx.y;
    const AppRow R = app_row(a.table + (size_t)a.rows[v] * 16);
    const size_t plane = (size_t)a.H * a.W;
    const float* __restrict__ img = a.image[v];
    const float* __restrict__ gout = a.g[v];
    float* __restrict__ gimg = a.out[v];
    double acc[APP_VALS];
#pragma unroll
    for (int t = 0; t < APP_VALS; ++t) acc[t] = 0.0;

    for (unsigned tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {                // uniform
        const unsigned q = tile * APP_BLOCK + threadIdx.x;
        if (q >= a.nquads) continue;
        const int y = (int)(q / (unsigned)a.Q), x0 = 4 * (int)(q - (unsigned)y * (unsigned)a.Q);
        const int n = VEC ? 4 : min(4, a.W - x0);
        const size_t at = (size_t)y * a.W + x0;
        float p[3][4], g[3][4], d[3][4];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            osum::load4<VEC>(gout + k * plane + at, n, g[k]);
            if (SUMS) osum::load4<VEC>(img + k * plane + at, n, p[k]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float r2 = app_r2(a, x0 + j, y);
            const float f = app_falloff(R, r2);
            float t[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                t[k] = g[0][j] * R.e[k][0] + g[1][j] * R.e[k][1] + g[2][j] * R.e[k][2];
                d[k][j] = f * t[k];
            }
            if (SUMS) {
                // (a lane past the end of a short quad has p = g = 0: every term below is 0)
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float qk = f * p[k][j];
#pragma unroll
                    for (int c = 0; c < 3; ++c) acc[4 * k + c] += (double)(g[c][j] * qk);
                    acc[4 * k + 3] += (double)g[k][j];
                }
                const float df = p[0][j] * t[0] + p[1][j] * t[1] + p[2][j] * t[2];
                const float w1 = r2 * df, w2 = r2 * w1, w3 = r2 * w2;
                acc[12] += (double)w1; acc[13] += (double)w2; acc[14] += (double)w3;
            }
        }
        if (gimg) {                                                                        // uniform
#pragma unroll
            for (int k = 0; k < 3; ++k) osum::store4<VEC>(gimg + k * plane + at, n, d[k]);
        }
    }
    if (!SUMS) return;
    osum::block_sum<APP_VALS>(acc, sh);                                                    // every lane is here
    if (threadIdx.x < 16)
        partials[((size_t)v * gridDim.x + blockIdx.x) * 16 + threadIdx.x] = (threadIdx.x < APP_VALS) ? osum::block_total<APP_VALS>(sh, threadIdx.x) : 0.0;
}

// The (N,16) gradient, every element.  Workgroup (c, v) of the first n_rows * 16: column c of listed row rows[v], the view's
// nslots partial rows added in slot order (ordered_sum.h) and rounded once (column 15: no rows, zero).  The workgroups after them:
// zeros into every row that is not listed.
__global__ void __launch_bounds__(256) appearance_table_kernel(const AppDev a, const double* __restrict__ partials, const int nslots,
                                                               float* __restrict__ g_table)
{
    const int sums = a.n_rows * 16;
    if ((int)blockIdx.x < sums) {                                                          // uniform
        __shared__ double sh[4];
        const int v = blockIdx.x >> 4, c = blockIdx.x & 15;
        double S[1];
        osum::ordered_rows_sum<1>(partials + (size_t)v * nslots * 16 + c, c < APP_VALS ? nslots : 0, 16, sh, S);
        if (threadIdx.x == 0) g_table[(size_t)a.rows[v] * 16 + c] = (float)S[0];
        return;
    }
    const size_t e = (size_t)(blockIdx.x - sums) * 256 + threadIdx.x;
    if (e >= (size_t)a.N * 16) return;
    const int r = (int)(e >> 4);
    bool listed = false;
#pragma unroll
    for (int k = 0; k < BAGS_MAX_POSE_ROWS; ++k) listed |= (k < a.n_rows && a.rows[k] == r);
    if (!listed) g_table[e] = 0.0f;
}

static inline unsigned app_quads(int H, int W) { return (unsigned)((long long)H * ((W + 3) / 4)); }
static inline unsigned app_tiles(int H, int W) { return (app_quads(H, W) + APP_BLOCK - 1) / APP_BLOCK; }
// workgroups (= partial rows) per view of the backward: a function of the image size alone
int appearance_slots(int H, int W)
{
    const unsigned tiles = app_tiles(H, W);
    const unsigned want = (tiles + BAGS_APPEARANCE_TILES_PER_SLOT - 1) / BAGS_APPEARANCE_TILES_PER_SLOT;
    const unsigned floor_ = BAGS_APPEARANCE_MIN_SLOTS;
    const unsigned n = want > floor_ ? want : floor_;
    return (int)(tiles < n ? tiles : n);
}

static AppDev app_dev(const BagsAppearance& a, const float* const* g_out, float* const* outs)
{
    AppDev d{};
    d.table = a.table; d.H = a.H; d.W = a.W; d.Q = (a.W + 3) / 4;
    d.nquads = app_quads(a.H, a.W); d.ntiles = app_tiles(a.H, a.W);
    d.cx = a.cx; d.cy = a.cy;
    d.s2 = (float)(((double)a.W * a.W + (double)a.H * a.H) / 4.0);
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

// float4 accesses: whole quads and every plane of every tensor 16-byte aligned
static bool app_vector(const AppDev& d)
{
    if (d.W % 4 != 0) return false;
    uintptr_t bits = 0;
    for (int k = 0; k < d.n_rows; ++k)
        bits |= reinterpret_cast<uintptr_t>(d.image[k]) | reinterpret_cast<uintptr_t>(d.out[k]) | reinterpret_cast<uintptr_t>(d.g[k]);
    return (bits & 15) == 0;
}

// the struct is validated by the caller (api.hip): rows distinct and in range, H * W below 2^31, pointers given
hipError_t launch_appearance_fwd(const BagsAppearance& a, hipStream_t st)
{
    const AppDev d = app_dev(a, nullptr, a.out);
    return with_bool(app_vector(d), [&](auto VEC) {
        hipLaunchKernelGGL((appearance_fwd_kernel<decltype(VEC)::value>), dim3(d.ntiles, a.n_rows), dim3(APP_BLOCK), 0, st, d);
        return hipGetLastError(); });
}

// partials: n_rows * appearance_slots(H, W) rows of 16 doubles, needed when g_table is wanted; g_image: NULL or n_rows pointers
hipError_t launch_appearance_bwd(const BagsAppearance& a, const float* const* g_out, double* partials, float* const* g_image, float* g_table,
                                 hipStream_t st)
{
    const AppDev d = app_dev(a, g_out, g_image);
    const int nslots = appearance_slots(a.H, a.W);
    const hipError_t e = with_bool(app_vector(d), [&](auto VEC) { return with_bool(g_table != nullptr, [&](auto SUMS) {
        hipLaunchKernelGGL((appearance_bwd_kernel<decltype(VEC)::value, decltype(SUMS)::value>), dim3(nslots, a.n_rows), dim3(APP_BLOCK), 0, st,
                           d, partials);
        return hipGetLastError(); }); });
    if (e != hipSuccess || !g_table) return e;
    const unsigned fill = (unsigned)(((size_t)a.N * 16 + 255) / 256);
    hipLaunchKernelGGL(appearance_table_kernel, dim3(a.n_rows * 16 + fill), dim3(256), 0, st, d, partials, nslots, g_table);
    return hipGetLastError();
}
