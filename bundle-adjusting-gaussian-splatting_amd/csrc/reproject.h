// reproject.h -- what the two losses that carry a pixel of one view into another share (correspondence.hip, warp.hip): the relative
// transform of an ordered pair and its staging in LDS, the pixel's x_i / x_j / proj, the forward's finalize and the store of a
// workgroup's twelve sums (the order of every sum: ordered_sum.h), the pixel's way back from dL/dproj to dL/dD, dL/dA and the twelve sums, and the chain from those sums to the two
// matrix gradients.  One statement each, so that the two losses round every one of them the same way; the formulas are in the header
// comment of correspondence.hip.  A `Dev` is a kernel's by-value argument struct: H, W, min_weight, min_depth, pin_src, pin_dst, depth,
// weights, view_src, view_dst (CoDev, WpDev).  Both files are compiled with -ffp-contract=off: only the operations spelled here and
// in ordered_sum.h.
#pragma once
#include "ordered_sum.h"

#define RP_CHUNK BAGS_CORRESPONDENCE_CHUNK
#define RP_ROW BAGS_CORRESPONDENCE_STATS             // doubles per forward partial row and per stats row: (sum w rho, sum w) / (1/cnt, cnt)
#define RP_SUMS BAGS_CORRESPONDENCE_SUMS             // backward partial sums per workgroup: G_M (9, row-major), g_c (3)
static_assert(RP_CHUNK == 256, "four waves: block_sum's default, and ordered_rows_sum's 256 threads");
static_assert(RP_SUMS == 12, "G_M and g_c");

struct RpViewGrads {
    float* src[BAGS_MAX_POSE_ROWS];                  // (4,4) each, any of them NULL
    float* dst[BAGS_MAX_POSE_ROWS];
};

struct RpTransform {
    double P[3][3];                                  // inv(Ai)
    double M[3][3], c[3];
    double Aj[3][3], bi[3];
};

// M = inv(Ai) @ Aj and c = bj - bi @ M in double from the two (4,4) row-major float matrices; false where det(Ai) is zero or not
// finite (the pair is degenerate and nothing of `t` may be used).  The one statement of the transform: every kernel of both files.
__device__ __forceinline__ bool rp_transform(const float* __restrict__ Vi, const float* __restrict__ Vj, RpTransform& t)
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
template <class Dev>
__device__ __forceinline__ void rp_stage_transform(const Dev& a, const int pair, double* __restrict__ Mc, int* __restrict__ ok)
{
    if (threadIdx.x == 0) {
        RpTransform t;
        const bool good = rp_transform(a.view_src[pair], a.view_dst[pair], t);
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

struct RpPoint {
    double ray[2];                                   // ((u - cx_i)/fx_i, (v - cy_i)/fy_i)
    double z, xi[3], xj[3];
    float a;                                         // A of the pixel
};

// solid and x_j.z >= min_depth for pixel (u, v) at offset `at` of pair `pair`; on true, o holds the point in both views
template <class Dev>
__device__ __forceinline__ bool rp_point(const Dev& a, const int pair, const double* __restrict__ Mc, const size_t at, const int u, const int v,
                                         RpPoint& o)
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

// proj = (fx_j x_j.x / x_j.z + cx_j, fy_j x_j.y / x_j.z + cy_j) of a point rp_point accepted, with iz = 1 / x_j.z
__device__ __forceinline__ void rp_project(const double* __restrict__ pin, const RpPoint& p, const double iz, double& x, double& y)
{
    x = (pin[0] * p.xj[0]) * iz + pin[2];
    y = (pin[1] * p.xj[1]) * iz + pin[3];
}

// The forward's second kernel, a workgroup of 256 per pair k: its nchunks partial rows (sum w rho, sum w) added in chunk order, then
// loss, count and the stats row (1/cnt, cnt).  sh: 4 * RP_ROW doubles of LDS.
__device__ __forceinline__ void rp_finalize(const int k, const int nchunks, const double* __restrict__ partials, float* __restrict__ loss,
                                            float* __restrict__ count, double* __restrict__ stats, double* __restrict__ sh)
{
    double S[RP_ROW];
    osum::ordered_rows_sum<RP_ROW>(partials + (size_t)k * nchunks * RP_ROW, nchunks, RP_ROW, sh, S);
    if (threadIdx.x != 0) return;
    const double cnt = S[1];
    const double inv = cnt > 0.0 ? 1.0 / cnt : 0.0;
    loss[k] = (float)(cnt > 0.0 ? S[0] * inv : 0.0);
    count[k] = (float)cnt;
    stats[(size_t)k * RP_ROW] = inv;
    stats[(size_t)k * RP_ROW + 1] = cnt;
}

// A valid pixel's way back from (gx, gy) = (dL/dproj.x fx_j, dL/dproj.y fy_j): dL/dD and dL/dA, each rounded once from double, and --
// SUMS -- the pixel's twelve terms of G_M = sum x_i^T g_xj and g_c = sum g_xj into acc.  iz = 1 / x_j.z.
template <bool SUMS>
__device__ __forceinline__ void rp_pixel_back(const RpPoint& pt, const double* __restrict__ Mc, const double gx, const double gy, const double iz,
                                              float& dD, float& dA, double (&acc)[RP_SUMS])
{
    double gj[3];
    gj[0] = gx * iz; gj[1] = gy * iz;
    gj[2] = -(((gx * pt.xj[0] + gy * pt.xj[1]) * iz) * iz);
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

// The workgroup's twelve sums into sums[(pair * 12 + t) * nchunks + chunk].  Every lane of the workgroup calls it.  sh: 4 * RP_SUMS
// doubles of LDS.
__device__ __forceinline__ void rp_store_sums(const double (&acc)[RP_SUMS], double* __restrict__ sh, const int pair, double* __restrict__ sums)
{
    osum::block_sum<RP_SUMS>(acc, sh);
    if (threadIdx.x < RP_SUMS) sums[((size_t)pair * RP_SUMS + threadIdx.x) * gridDim.x + blockIdx.x] = osum::block_total<RP_SUMS>(sh, threadIdx.x);
}

// The backward's second kernel, a workgroup of 256 per pair: the twelve sums of its chunks added in a fixed order, then the chain to
// the two (4,4) gradients in double, each element rounded once.  A degenerate pair (det(Ai) zero or not finite) gets exact zeros.
// oi / oj == nullptr: not wanted.  sh: 4 doubles of LDS, used for one sum after the other.
__device__ __forceinline__ void rp_views_chain(const float* __restrict__ Vi, const float* __restrict__ Vj, const int pair, const int nchunks,
                                               const double* __restrict__ sums, float* __restrict__ oi, float* __restrict__ oj, double* __restrict__ sh)
{
    double S[RP_SUMS];
#pragma unroll
    for (int t = 0; t < RP_SUMS; ++t) {
        double one[1];
        __syncthreads();                                                                      // sh of the sum before is read
        osum::ordered_rows_sum<1>(sums + ((size_t)pair * RP_SUMS + t) * nchunks, nchunks, 1, sh, one);
        S[t] = one[0];
    }
    if (threadIdx.x != 0) return;
    double gVi[4][4], gVj[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int k = 0; k < 4; ++k) gVi[r][k] = gVj[r][k] = 0.0;
    RpTransform t;
    if (rp_transform(Vi, Vj, t)) {
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
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (oi) oi[4 * r + k] = (float)gVi[r][k];
            if (oj) oj[4 * r + k] = (float)gVj[r][k];
        }
}

// workgroups (= partial rows) per pair: a function of the source image's size alone
static inline int rp_chunks(int H, int W) { return (int)(((long long)H * W + RP_CHUNK - 1) / RP_CHUNK); }
