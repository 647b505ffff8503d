// gaussian_normals.hip -- the normal of every Gaussian in the camera frame of up to BAGS_MAX_SH_VIEWS views: its shortest axis,
// turned towards the camera (DN-Splatter, GaussianShader, the PGSR / GOF / RaDe-GS family splat it through override_color).  Per
// Gaussian and view, with q = (w,x,y,z) as given (not normalised), scales s, mean x and the row-vector view matrix V:
//     k      = first minimum of (s0, s1, s2)                              (a decision; NaN compares false)
//     c      = column k of Q(q) = |q|^2 R(q/|q|), written without a division
//     m_j    = sum_i c_i V[i,j] ;  t = x @ V[:3,:3] + V[3,:3]
//     sigma  = -1 if m . t > 0 else +1                                    (a decision: the normal faces the camera)
//     l2     = |m|^2 ;  live = l2 is finite and > 0
//     out    = sigma * m / sqrt(l2) where live, (0,0,0) elsewhere
// It lives IN FRONT of the operator, like antialias.hip: its output is the operator's colors_precomp.  Gradients go to the quaternion
// (through Q and the normalisation, summed over the views of the call) and to the 3x3 block of every view matrix; k and sigma are
// decisions, so scales and means get none.  A dead row has a zero output and takes part in no sum: selects, never 0 * inf.
//
// One lane per Gaussian both ways; q, s and x are read once whatever V is, and the 12 floats of every view are staged in LDS once per
// workgroup.  The file is compiled with -ffp-contract=off: the two decisions are those of the float32 statement
// (bags_raster/gaussian_normals.py), which spells the same operations in the same order.  The backward recomputes the forward
// (nothing is saved), holds dL/dc summed over the views in registers and writes dL/dq once; the 9 V view-matrix terms are reduced
// wave -> workgroup -> one slab row per workgroup, and a second small launch adds the rows in double in a fixed order
// (ordered_sum.h: slab_column_sum) and writes the zeros of the fourth row and column.  No atomics: two runs give the same bits, and
// a view's sums are formed from its own terms alone, so they do not depend on its neighbours in the call.
#include "ordered_sum.h"

#define GN_BLOCK 256
#define GN_VIEW 12               // staged floats per view: V[i,j], i = 0..3, j = 0..2, at 3 i + j
#define GN_TERMS GN_SLAB_PER_VIEW // slab columns per view: dL/dV[i,j], i, j = 0..2, at 3 i + j

struct GnViews { const float* v[BAGS_MAX_SH_VIEWS]; };
struct GnOuts { float* p[BAGS_MAX_SH_VIEWS]; };
struct GnGrads { const float* p[BAGS_MAX_SH_VIEWS]; };

// every thread of the workgroup calls it; sv is valid after the barrier
__device__ __forceinline__ void gn_stage(const GnViews& views, const int V, float (*sv)[GN_VIEW])
{
    for (int e = threadIdx.x; e < V * GN_VIEW; e += GN_BLOCK) {
        const int v = e / GN_VIEW, r = e - v * GN_VIEW;
        sv[v][r] = views.v[v][4 * (r / 3) + r % 3];
    }
    __syncthreads();
}

struct GnRow { float w, x, y, z, px, py, pz; int k; float c0, c1, c2; };
__device__ __forceinline__ GnRow gn_load(const size_t i, const float* __restrict__ rotations, const float* __restrict__ scales,
                                         const float* __restrict__ means3D)
{
    GnRow r;
    r.w = rotations[4 * i]; r.x = rotations[4 * i + 1]; r.y = rotations[4 * i + 2]; r.z = rotations[4 * i + 3];
    const float s0 = scales[3 * i], s1 = scales[3 * i + 1], s2 = scales[3 * i + 2];
    r.px = means3D[3 * i]; r.py = means3D[3 * i + 1]; r.pz = means3D[3 * i + 2];
    int k = 0;
    float sk = s0;
    if (s1 < sk) { k = 1; sk = s1; }
    if (s2 < sk) { k = 2; }
    r.k = k;
    const float w = r.w, x = r.x, y = r.y, z = r.z;
    const float ww = w * w, xx = x * x, yy = y * y, zz = z * z;
    if (k == 0) { r.c0 = ww + xx - yy - zz; r.c1 = 2.0f * (x * y + w * z); r.c2 = 2.0f * (x * z - w * y); }
    else if (k == 1) { r.c0 = 2.0f * (x * y - w * z); r.c1 = ww - xx + yy - zz; r.c2 = 2.0f * (y * z + w * x); }
    else { r.c0 = 2.0f * (x * z + w * y); r.c1 = 2.0f * (y * z - w * x); r.c2 = ww - xx - yy + zz; }
    return r;
}

// one view of one Gaussian
struct GnView { float m0, m1, m2, sigma, l2; bool live; };
__device__ __forceinline__ GnView gn_view(const GnRow& r, const float* sv)
{
    GnView f;
    f.m0 = r.c0 * sv[0] + r.c1 * sv[3] + r.c2 * sv[6];
    f.m1 = r.c0 * sv[1] + r.c1 * sv[4] + r.c2 * sv[7];
    f.m2 = r.c0 * sv[2] + r.c1 * sv[5] + r.c2 * sv[8];
    const float t0 = r.px * sv[0] + r.py * sv[3] + r.pz * sv[6] + sv[9];
    const float t1 = r.px * sv[1] + r.py * sv[4] + r.pz * sv[7] + sv[10];
    const float t2 = r.px * sv[2] + r.py * sv[5] + r.pz * sv[8] + sv[11];
    const float d = f.m0 * t0 + f.m1 * t1 + f.m2 * t2;
    f.sigma = (d > 0.0f) ? -1.0f : 1.0f;
    f.l2 = f.m0 * f.m0 + f.m1 * f.m1 + f.m2 * f.m2;
    f.live = (f.l2 > 0.0f) && (f.l2 < __builtin_huge_valf());         // finite and positive; NaN fails both
    return f;
}

__global__ void __launch_bounds__(GN_BLOCK)
gaussian_normals_fwd_kernel(const int P, const int V, const float* __restrict__ rotations, const float* __restrict__ scales,
                            const float* __restrict__ means3D, const GnViews views, const GnOuts outs)
{
    __shared__ float sv[BAGS_MAX_SH_VIEWS][GN_VIEW];
    gn_stage(views, V, sv);
    const int i = blockIdx.x * GN_BLOCK + threadIdx.x;
    if (i >= P) return;
    const GnRow r = gn_load((size_t)i, rotations, scales, means3D);
    for (int v = 0; v < V; ++v) {                                      // uniform
        const GnView f = gn_view(r, sv[v]);
        const float len = sqrtf(f.l2);
        float* __restrict__ o = outs.p[v] + 3 * (size_t)i;
        o[0] = f.live ? (f.sigma * f.m0) / len : 0.0f;
        o[1] = f.live ? (f.sigma * f.m1) / len : 0.0f;
        o[2] = f.live ? (f.sigma * f.m2) / len : 0.0f;
    }
}

// slab == nullptr: no view-matrix gradient is wanted and nothing is reduced; g_rot == nullptr: not stored.  Every per-Gaussian value is
// formed whether or not it is stored, so the bits of a wanted output do not depend on which others are wanted.
__global__ void __launch_bounds__(GN_BLOCK)
gaussian_normals_bwd_kernel(const int P, const int V, const float* __restrict__ rotations, const float* __restrict__ scales,
                            const float* __restrict__ means3D, const GnViews views, const GnGrads grads, float* __restrict__ slab,
                            float* __restrict__ g_rot)
{
    __shared__ float sv[BAGS_MAX_SH_VIEWS][GN_VIEW];
    __shared__ float wsum[GN_BLOCK / 64][BAGS_MAX_SH_VIEWS * GN_TERMS];
    gn_stage(views, V, sv);
    const int i = blockIdx.x * GN_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // every lane runs the chain (index clamped: P > 0 here), so that the DPP rows of the reduction are complete; what a lane without a
    // Gaussian or a dead row computes is replaced by 0 in the selects below and never reaches a sum
    const size_t ic = (size_t)(i < P ? i : P - 1);
    const GnRow r = gn_load(ic, rotations, scales, means3D);
    float gc0 = 0.0f, gc1 = 0.0f, gc2 = 0.0f;                          // dL/dc, summed over the views in view order
    bool any = false;
    for (int v = 0; v < V; ++v) {                                      // uniform
        const float* s = sv[v];
        const GnView f = gn_view(r, s);
        const bool on = (i < P) && f.live;
        const float* __restrict__ go = grads.p[v];                    // NULL: no loss uses this view, a zero cotangent (uniform)
        const float g0 = go ? go[3 * ic] : 0.0f, g1 = go ? go[3 * ic + 1] : 0.0f, g2 = go ? go[3 * ic + 2] : 0.0f;
        // out = sigma m / |m|:  dL/dm = sigma (g - mh (mh . g)) / |m|,  mh = m / |m|
        const float len = sqrtf(f.l2);
        const float h0 = f.m0 / len, h1 = f.m1 / len, h2 = f.m2 / len;
        const float hg = h0 * g0 + h1 * g1 + h2 * g2;
        const float a0 = on ? (f.sigma * (g0 - h0 * hg)) / len : 0.0f;
        const float a1 = on ? (f.sigma * (g1 - h1 * hg)) / len : 0.0f;
        const float a2 = on ? (f.sigma * (g2 - h2 * hg)) / len : 0.0f;
        // m_j = sum_i c_i V[i,j]
        const float d0 = a0 * s[0] + a1 * s[1] + a2 * s[2];
        const float d1 = a0 * s[3] + a1 * s[4] + a2 * s[5];
        const float d2 = a0 * s[6] + a1 * s[7] + a2 * s[8];
        gc0 += on ? d0 : 0.0f; gc1 += on ? d1 : 0.0f; gc2 += on ? d2 : 0.0f;
        any = any || on;
        if (slab) {                                                    // uniform
            const float cs[3] = {r.c0, r.c1, r.c2}, as[3] = {a0, a1, a2};
#pragma unroll
            for (int e = 0; e < GN_TERMS; ++e) {
                const float tot = wave_total_f(on ? cs[e / 3] * as[e % 3] : 0.0f);
                if (lane == 63) wsum[wave][v * GN_TERMS + e] = tot;
            }
        }
    }
    // c = column k of Q(q)
    const float w = r.w, x = r.x, y = r.y, z = r.z;
    float gw, gx, gy, gz;
    if (r.k == 0) {
        gw = 2.0f * (w * gc0 + z * gc1 - y * gc2); gx = 2.0f * (x * gc0 + y * gc1 + z * gc2);
        gy = 2.0f * (-y * gc0 + x * gc1 - w * gc2); gz = 2.0f * (-z * gc0 + w * gc1 + x * gc2);
    } else if (r.k == 1) {
        gw = 2.0f * (-z * gc0 + w * gc1 + x * gc2); gx = 2.0f * (y * gc0 - x * gc1 + w * gc2);
        gy = 2.0f * (x * gc0 + y * gc1 + z * gc2); gz = 2.0f * (-w * gc0 - z * gc1 + y * gc2);
    } else {
        gw = 2.0f * (y * gc0 - x * gc1 + w * gc2); gx = 2.0f * (z * gc0 - w * gc1 - x * gc2);
        gy = 2.0f * (w * gc0 + z * gc1 - y * gc2); gz = 2.0f * (x * gc0 + y * gc1 + z * gc2);
    }
    if (g_rot && i < P) {
        float* __restrict__ o = g_rot + 4 * (size_t)i;
        o[0] = any ? gw : 0.0f; o[1] = any ? gx : 0.0f; o[2] = any ? gy : 0.0f; o[3] = any ? gz : 0.0f;
    }
    // ---- wave rows -> the workgroup's slab row, the four waves in wave order
    if (slab) {                                                        // uniform
        __syncthreads();
        for (int e = threadIdx.x; e < V * GN_TERMS; e += GN_BLOCK)
            slab[(size_t)blockIdx.x * (V * GN_TERMS) + e] = (wsum[0][e] + wsum[1][e]) + (wsum[2][e] + wsum[3][e]);
    }
}

// slab rows -> the (4,4) gradients, one workgroup per (view, term), summed in double in a fixed order.  The fourth column is written
// as zeros by the term next to it, the fourth row by the view's first term.
__global__ void __launch_bounds__(256)
gaussian_normals_reduce_kernel(const float* __restrict__ slab, const int nblocks, const int V, const GnOuts g_view)
{
    const int t = blockIdx.x, v = t / GN_TERMS, e = t - v * GN_TERMS;
    const double sum = slab_column_sum(slab, nblocks, V * GN_TERMS, t);
    if (threadIdx.x != 0) return;
    float* __restrict__ g = g_view.p[v];
    if (!g) return;
    g[(e / 3) * 4 + e % 3] = (float)sum;
    if (e % 3 == 2) g[(e / 3) * 4 + 3] = 0.0f;
    if (e == 0) { g[12] = 0.0f; g[13] = 0.0f; g[14] = 0.0f; g[15] = 0.0f; }
}

int gaussian_normals_blocks(int P) { return cdiv(P > 0 ? P : 1, GN_BLOCK); }

static GnViews gn_views(const BagsGaussianNormals& a)
{
    GnViews w{};
    for (int v = 0; v < BAGS_MAX_SH_VIEWS; ++v) w.v[v] = v < a.V ? a.viewmatrix[v] : nullptr;
    return w;
}

// the struct and the tables are validated by the caller (api.hip)
hipError_t launch_gaussian_normals_fwd(const BagsGaussianNormals& a, float* const* out, hipStream_t st)
{
    if (a.P == 0) return hipSuccess;
    GnOuts o{};
    for (int v = 0; v < a.V; ++v) o.p[v] = out[v];
    hipLaunchKernelGGL(gaussian_normals_fwd_kernel, dim3(cdiv(a.P, GN_BLOCK)), dim3(GN_BLOCK), 0, st, a.P, a.V, a.rotations, a.scales, a.means3D,
                       gn_views(a), o);
    return hipGetLastError();
}

// grad_out: V pointers of which any may be NULL (a zero cotangent); slab: gaussian_normals_blocks(P) rows of 9 V floats, or nullptr
// when no view-matrix gradient is wanted; g_view: V pointers of which any may be NULL (only read with a slab)
hipError_t launch_gaussian_normals_bwd(const BagsGaussianNormals& a, const float* const* grad_out, float* slab, float* g_rot,
                                       float* const* g_view, hipStream_t st)
{
    if (a.P == 0) return hipSuccess;
    const int nblocks = cdiv(a.P, GN_BLOCK);
    GnGrads g{};
    for (int v = 0; v < a.V; ++v) g.p[v] = grad_out[v];
    hipLaunchKernelGGL(gaussian_normals_bwd_kernel, dim3(nblocks), dim3(GN_BLOCK), 0, st, a.P, a.V, a.rotations, a.scales, a.means3D, gn_views(a),
                       g, slab, g_rot);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || !slab) return e;
    GnOuts o{};
    for (int v = 0; v < a.V; ++v) o.p[v] = g_view[v];
    hipLaunchKernelGGL(gaussian_normals_reduce_kernel, dim3(a.V * GN_TERMS), dim3(256), 0, st, slab, nblocks, a.V, o);
    return hipGetLastError();
}
