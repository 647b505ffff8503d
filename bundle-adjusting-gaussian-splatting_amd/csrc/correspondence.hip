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
// reads the matrices.  The sums: a lane adds its one pixel in double; the lanes of a wave are added by a shuffle butterfly, the four
// waves in wave order in LDS, and the workgroup leaves its partial sums in the workspace.  A pair has ceil(H W / 256) workgroups
// whatever the number of pairs, and the finishing kernels add its partials in a fixed order: a pair's results are the same bits in a
// 16-pair launch and in a launch of its own.  No atomics, no memset.  Compiled with -ffp-contract=off: only the operations spelled.
#include "bags_common.h"

#define CO_CHUNK BAGS_CORRESPONDENCE_CHUNK
#define CO_ROW BAGS_CORRESPONDENCE_STATS             // doubles per forward partial row and per stats row: (sum w rho, sum w) / (1/cnt, cnt)
#define CO_SUMS 12                                   // backward partial sums per workgroup: G_M (9, row-major), g_c (3)
static_assert(CO_CHUNK == 256, "four waves: the wave-order sums below name them");

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

struct CoViewGrads {
    float* src[BAGS_MAX_POSE_ROWS];                  // (4,4) each, any of them NULL
    float* dst[BAGS_MAX_POSE_ROWS];
};

struct CoTransform {
    double P[3][3];                                  // inv(Ai)
    double M[3][3], c[3];
    double Aj[3][3], bi[3];
};

// M = inv(Ai) @ Aj and c = bj - bi @ M in double from the two (4,4) row-major float matrices; false where det(Ai) is zero or not
// finite (the pair is degenerate and nothing of `t` may be used).  The one statement of the transform: every kernel of this file.
__device__ __forceinline__ bool co_transform(const float* __restrict__ Vi, const float* __restrict__ Vj, CoTransform& t)
{
    double A[3][3], bj[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { A[r][k] = (double)Vi[4 * r + k]; t.Aj[r][k] = (double)Vj[4 * r + k]; }
        t.bi[r] = (double)Vi[12 + r]; bj[r] = (double)Vj[12 + r];
    }
    // cofactors C[r][k] of Ai; adj = C^T
    double Cf[3][3];
    Cf[0][0] = A[1][1] * A[2][2] - A[1][2] * A[2][1];
    Cf[0][1] = A[1][2] * A[2][0] - A[1][0] * A[2][2];
    Cf[0][2] = A[1][0] * A[2][1] - A[1][1] * A[2][0];
    Cf[1][0] = A[0][2] * A[2][1] - A[0][1] * A[2][2];
    Cf[1][1] = A[0][0] * A[2][2] - A[0][2] * A[2][0];
    Cf[1][2] = A[0][1] * A[2][0] - A[0][0] * A[2][1];
    Cf[2][0] = A[0][1] * A[1][2] - A[0][2] * A[1][1];
    Cf[2][1] = A[0][2] * A[1][0] - A[0][0] * A[1][2];
    Cf[2][2] = A[0][0] * A[1][1] - A[0][1] * A[1][0];
    const double det = (A[0][0] * Cf[0][0] + A[0][1] * Cf[0][1]) + A[0][2] * Cf[0][2];
    if (!(det != 0.0 && fabs(det) < (double)INFINITY)) return false;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k) t.P[r][k] = Cf[k][r] / det;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k) t.M[r][k] = (t.P[r][0] * t.Aj[0][k] + t.P[r][1] * t.Aj[1][k]) + t.P[r][2] * t.Aj[2][k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t.c[k] = bj[k] - ((t.bi[0] * t.M[0][k] + t.bi[1] * t.M[1][k]) + t.bi[2] * t.M[2][k]);
    return true;
}

// The workgroup's prologue: lane 0 forms the transform of pair `pair` and leaves M (row-major, 0..8), c (9..11) and the flag in LDS.
__device__ __forceinline__ void co_stage_transform(const CoDev& a, const int pair, double* __restrict__ Mc, int* __restrict__ ok)
{
    if (threadIdx.x == 0) {
        CoTransform t;
        const bool good = co_transform(a.view_src[pair], a.view_dst[pair], t);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int k = 0; k < 3; ++k) Mc[3 * r + k] = good ? t.M[r][k] : 0.0;
            Mc[9 + r] = good ? t.c[r] : 0.0;
        }
        *ok = good ? 1 : 0;
    }
    __syncthreads();
}

struct CoPoint {
    double ray[2];                                   // ((u - cx_i)/fx_i, (v - cy_i)/fy_i)
    double z, xi[3], xj[3];
    float a;                                         // A of the pixel
};

// solid and x_j.z >= min_depth for pixel (u, v) at offset `at` of pair `pair`; on true, o holds the point in both views
__device__ __forceinline__ bool co_point(const CoDev& a, const int pair, const double* __restrict__ Mc, const size_t at, const int u, const int v,
                                         CoPoint& o)
{
    const float d = a.depth[pair][at];
    o.a = a.weights[pair][at];
    if (!(o.a >= a.min_weight && d > 0.0f)) return false;
    o.z = (double)(d / o.a);
    const double* __restrict__ pin = a.pin_src[pair];
    o.ray[0] = ((double)u - pin[2]) / pin[0];
    o.ray[1] = ((double)v - pin[3]) / pin[1];
    o.xi[0] = o.z * o.ray[0]; o.xi[1] = o.z * o.ray[1]; o.xi[2] = o.z;
#pragma unroll
    for (int k = 0; k < 3; ++k) o.xj[k] = ((o.xi[0] * Mc[k] + o.xi[1] * Mc[3 + k]) + o.xi[2] * Mc[6 + k]) + Mc[9 + k];
    return o.xj[2] >= a.min_depth;
}

struct CoResidual {
    double w, iz;                                    // conf, 1 / x_j.z
    double r[2], e;
};

// the rest of `valid` for a pixel co_point accepted: conf > 0 and a finite match; on true the residual
__device__ __forceinline__ bool co_residual(const CoDev& a, const int pair, const size_t at, const CoPoint& p, CoResidual& o)
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
    o.r[0] = ((pin[0] * p.xj[0]) * o.iz + pin[2]) - (double)mx;
    o.r[1] = ((pin[1] * p.xj[1]) * o.iz + pin[3]) - (double)my;
    o.e = sqrt(o.r[0] * o.r[0] + o.r[1] * o.r[1]);
    return true;
}

// N doubles per lane -> N doubles per workgroup in out[0..N) of the first N threads' registers: lanes by a butterfly (the same total in
// every lane), waves in wave order through LDS.  Every lane of the workgroup calls it.
template <int N>
__device__ __forceinline__ void co_block_sum(double (&acc)[N], double (*wsum)[N])
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int t = 0; t < N; ++t) {
        double s = acc[t];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
        if (lane == 0) wsum[wave][t] = s;
    }
    __syncthreads();
}

// Workgroup bx of pair by leaves the row (sum w rho, sum w) of its chunk.
__global__ void __launch_bounds__(CO_CHUNK) correspondence_sums_kernel(const CoDev a, double* __restrict__ partials)
{
    __shared__ double Mc[12];
    __shared__ int ok;
    __shared__ double wsum[CO_CHUNK / 64][CO_ROW];
    const int pair = blockIdx.y;
    co_stage_transform(a, pair, Mc, &ok);
    const long long npix = (long long)a.H * a.W;
    const long long p = (long long)blockIdx.x * CO_CHUNK + threadIdx.x;
    double acc[CO_ROW] = {0.0, 0.0};
    if (ok && p < npix) {
        const int v = (int)(p / a.W), u = (int)(p - (long long)v * a.W);
        CoPoint pt;
        CoResidual rs;
        if (co_point(a, pair, Mc, (size_t)p, u, v, pt) && co_residual(a, pair, (size_t)p, pt, rs)) {
            const double rho = rs.e <= a.delta ? 0.5 * (rs.e * rs.e) : a.delta * (rs.e - 0.5 * a.delta);
            acc[0] = rs.w * rho; acc[1] = rs.w;
        }
    }
    co_block_sum<CO_ROW>(acc, wsum);
    if (threadIdx.x < CO_ROW)
        partials[((size_t)pair * gridDim.x + blockIdx.x) * CO_ROW + threadIdx.x] =
            ((wsum[0][threadIdx.x] + wsum[1][threadIdx.x]) + wsum[2][threadIdx.x]) + wsum[3][threadIdx.x];
}

// `n` doubles at `rows` with stride 1 added in a fixed order by a workgroup of 256: thread i takes i, i + 256, ..., a fixed shuffle
// tree, the waves in wave order; the total is returned to thread 0 (other threads: unspecified).  wsum: 4 doubles of LDS.
__device__ __forceinline__ double co_ordered_sum(const double* __restrict__ rows, const int n, double* __restrict__ wsum)
{
    double acc = 0.0;
#pragma unroll 4
    for (int s = threadIdx.x; s < n; s += 256) acc += rows[s];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
    __syncthreads();                                                                          // wsum of the call before is read
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    return ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// One workgroup per pair: its nchunks partial rows added in chunk order, then loss, count and the stats row.
__global__ void __launch_bounds__(256) correspondence_finalize_kernel(const int nchunks, const double* __restrict__ partials, float* __restrict__ loss,
                                                                      float* __restrict__ count, double* __restrict__ stats)
{
    __shared__ double wsum[CO_ROW][4];
    const int k = blockIdx.x;
    static_assert(CO_ROW == 2, "a partial row is one 16-byte load");
    const double2* __restrict__ rows = reinterpret_cast<const double2*>(partials) + (size_t)k * nchunks;       // 16-byte aligned (api.hip)
    double acc[CO_ROW] = {0.0, 0.0};
#pragma unroll 4
    for (int s = threadIdx.x; s < nchunks; s += 256) {
        const double2 r = rows[s];
        acc[0] += r.x; acc[1] += r.y;
    }
#pragma unroll
    for (int c = 0; c < CO_ROW; ++c) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) acc[c] += __shfl_xor(acc[c], d);
        if ((threadIdx.x & 63) == 0) wsum[c][threadIdx.x >> 6] = acc[c];
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double S[CO_ROW];
#pragma unroll
    for (int c = 0; c < CO_ROW; ++c) S[c] = ((wsum[c][0] + wsum[c][1]) + wsum[c][2]) + wsum[c][3];
    const double cnt = S[1];
    const double inv = cnt > 0.0 ? 1.0 / cnt : 0.0;
    loss[k] = (float)(cnt > 0.0 ? S[0] * inv : 0.0);
    count[k] = (float)cnt;
    stats[(size_t)k * CO_ROW] = inv;
    stats[(size_t)k * CO_ROW + 1] = cnt;
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
    __shared__ double wsum[CO_CHUNK / 64][CO_SUMS];
    const int pair = blockIdx.y;
    co_stage_transform(a, pair, Mc, &ok);
    const long long npix = (long long)a.H * a.W;
    const long long p = (long long)blockIdx.x * CO_CHUNK + threadIdx.x;
    const double scale = (double)g_loss[pair] * stats[(size_t)pair * CO_ROW];                 // cot / cnt; 0 where cnt <= 0
    double acc[CO_SUMS];
#pragma unroll
    for (int t = 0; t < CO_SUMS; ++t) acc[t] = 0.0;
    if (p < npix) {
        float dD = 0.0f, dA = 0.0f;
        const int v = (int)(p / a.W), u = (int)(p - (long long)v * a.W);
        CoPoint pt;
        CoResidual rs;
        if (ok && co_point(a, pair, Mc, (size_t)p, u, v, pt) && co_residual(a, pair, (size_t)p, pt, rs)) {
            const double* __restrict__ pin = a.pin_dst[pair];
            double sw = scale * rs.w;
            if (!(rs.e <= a.delta)) sw = (sw * a.delta) / rs.e;                               // e > delta > 0
            const double gx = (sw * rs.r[0]) * pin[0], gy = (sw * rs.r[1]) * pin[1];          // g_r fx_j, g_r fy_j
            double gj[3];
            gj[0] = gx * rs.iz; gj[1] = gy * rs.iz;
            gj[2] = -(((gx * pt.xj[0] + gy * pt.xj[1]) * rs.iz) * rs.iz);
            double gi[3];
#pragma unroll
            for (int m = 0; m < 3; ++m) gi[m] = (Mc[3 * m] * gj[0] + Mc[3 * m + 1] * gj[1]) + Mc[3 * m + 2] * gj[2];
            const double gz = (pt.ray[0] * gi[0] + pt.ray[1] * gi[1]) + gi[2];
            const double iA = 1.0 / (double)pt.a;
            dD = (float)(gz * iA);
            dA = (float)(-((pt.z * iA) * gz));
            if (SUMS) {
#pragma unroll
                for (int m = 0; m < 3; ++m)
#pragma unroll
                    for (int n = 0; n < 3; ++n) acc[3 * m + n] = pt.xi[m] * gj[n];
#pragma unroll
                for (int n = 0; n < 3; ++n) acc[9 + n] = gj[n];
            }
        }
        float* __restrict__ gD = a.g_depth[pair];
        float* __restrict__ gA = a.g_weights[pair];
        if (gD) gD[p] = dD;                                                                   // uniform
        if (gA) gA[p] = dA;
    }
    if (!SUMS) return;
    co_block_sum<CO_SUMS>(acc, wsum);
    if (threadIdx.x < CO_SUMS)
        sums[((size_t)pair * CO_SUMS + threadIdx.x) * gridDim.x + blockIdx.x] =
            ((wsum[0][threadIdx.x] + wsum[1][threadIdx.x]) + wsum[2][threadIdx.x]) + wsum[3][threadIdx.x];
}

// One workgroup per pair: the twelve sums of its chunks added in a fixed order, then the chain to the two (4,4) gradients in double,
// each element rounded once.  A degenerate pair (det(Ai) zero or not finite) gets exact zeros.  g.src[pair] / g.dst[pair] == nullptr:
// not wanted.
__global__ void __launch_bounds__(256) correspondence_views_kernel(const CoDev a, const CoViewGrads g, const int nchunks, const double* __restrict__ sums)
{
    __shared__ double wsum[4];
    const int pair = blockIdx.x;
    double S[CO_SUMS];
#pragma unroll
    for (int t = 0; t < CO_SUMS; ++t) S[t] = co_ordered_sum(sums + ((size_t)pair * CO_SUMS + t) * nchunks, nchunks, wsum);
    if (threadIdx.x != 0) return;
    double gVi[4][4], gVj[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int k = 0; k < 4; ++k) gVi[r][k] = gVj[r][k] = 0.0;
    CoTransform t;
    if (co_transform(a.view_src[pair], a.view_dst[pair], t)) {
        double G[3][3], T[3][3];
#pragma unroll
        for (int m = 0; m < 3; ++m)
#pragma unroll
            for (int n = 0; n < 3; ++n) G[m][n] = S[3 * m + n] - t.bi[m] * S[9 + n];          // through c = bj - bi @ M
#pragma unroll
        for (int m = 0; m < 3; ++m)
#pragma unroll
            for (int k = 0; k < 3; ++k) T[m][k] = (G[m][0] * t.M[k][0] + G[m][1] * t.M[k][1]) + G[m][2] * t.M[k][2];      // G M^T
#pragma unroll
        for (int k = 0; k < 3; ++k) {
#pragma unroll
            for (int n = 0; n < 3; ++n) {
                gVj[k][n] = (t.P[0][k] * G[0][n] + t.P[1][k] * G[1][n]) + t.P[2][k] * G[2][n];                          // P^T G
                gVi[k][n] = -((t.P[0][k] * T[0][n] + t.P[1][k] * T[1][n]) + t.P[2][k] * T[2][n]);                       // -P^T G M^T
            }
            gVj[3][k] = S[9 + k];
            gVi[3][k] = -((t.M[k][0] * S[9] + t.M[k][1] * S[10]) + t.M[k][2] * S[11]);
        }
    }
    float* __restrict__ oi = g.src[pair];
    float* __restrict__ oj = g.dst[pair];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (oi) oi[4 * r + k] = (float)gVi[r][k];
            if (oj) oj[4 * r + k] = (float)gVj[r][k];
        }
}

// proj (2,H,W) and valid (H,W) of one pair: the projection where the pixel is solid and x_j.z >= min_depth, zeros elsewhere; valid
// where the projection also lies inside the W_dst x H_dst image, -0.5 <= x < W_dst - 0.5 and -0.5 <= y < H_dst - 0.5 (pixel centres
// at whole numbers, the pixel rule of pinhole_of)
__global__ void __launch_bounds__(CO_CHUNK) reproject_pixels_kernel(const CoDev a, const int H_dst, const int W_dst, float* __restrict__ proj,
                                                                    uint8_t* __restrict__ valid)
{
    __shared__ double Mc[12];
    __shared__ int ok;
    co_stage_transform(a, 0, Mc, &ok);
    const long long npix = (long long)a.H * a.W;
    const long long p = (long long)blockIdx.x * CO_CHUNK + threadIdx.x;
    if (p >= npix) return;
    const int v = (int)(p / a.W), u = (int)(p - (long long)v * a.W);
    float px = 0.0f, py = 0.0f;
    bool in = false;
    CoPoint pt;
    if (ok && co_point(a, 0, Mc, (size_t)p, u, v, pt)) {
        const double* __restrict__ pin = a.pin_dst[0];
        const double iz = 1.0 / pt.xj[2];
        const double x = (pin[0] * pt.xj[0]) * iz + pin[2], y = (pin[1] * pt.xj[1]) * iz + pin[3];
        px = (float)x; py = (float)y;
        in = x >= -0.5 && x < (double)W_dst - 0.5 && y >= -0.5 && y < (double)H_dst - 0.5;
    }
    proj[p] = px; proj[npix + p] = py;
    valid[p] = in ? 1 : 0;
}

static inline int co_chunks(int H, int W) { return (int)(((long long)H * W + CO_CHUNK - 1) / CO_CHUNK); }
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
    CoViewGrads g{};
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
