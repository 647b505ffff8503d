// sh_colors.hip -- SH -> RGB as a stand-alone operator with its own backward: the colour path render() takes by default
// (hybrid=True: gaussian_renderer/__init__.py:90-95, the rasterizer then gets colors_precomp).
//
//   d = xyz - campos,  u = d / |d|,  raw_c = sum_{t < (deg+1)^2} basis_t(u) * sh[t][c] + 0.5,  rgb_c = raw_c < 0 ? 0 : raw_c
//
// In PyTorch that is a cat, a transposed copy, ~30 elementwise launches for the basis, a broadcast product and a sum, and all of
// it again backwards; here one kernel each way plus a three-workgroup reduction for dL/dcampos.  One thread per Gaussian, the
// coefficient row in registers (K = 16: twelve dwordx4 loads requested before the first use, as in K1); the coefficients come
// packed, shs (P,K,3), or split, shs (P,1,3) + shs_rest (P,K-1,3), whose rows are only 4-byte aligned.
//
// COMPILED WITH -ffp-contract=off: the backward saves nothing, it recomputes raw_c with the forward's operations to get the
// forward's clamp decision, and the packed and the split instance must give the same bits.  Nothing here is bound by arithmetic.
//
// Backward, per Gaussian (m_c = raw_c < 0 ? 0 : dL/drgb_c; raw_c == 0 passes, as clamp_min does):
//   dL/dsh[t][c] = basis_t * m_c  (t < (deg+1)^2; exactly zero for the stored rows beyond)
//   dL/du        = sum_t grad basis_t * (sum_c sh[t][c] m_c),   dL/dxyz = (dL/du - u (u . dL/du)) / |d|,   dL/dcampos = -sum_P dL/dxyz
// A Gaussian whose three cotangents are zero (everything the rasterizer culled) reads neither its position nor its row and writes
// zeros.  The SH gradient rows leave as whole lines through LDS (sh_rows.h: the write-out K9 uses); the campos sums go wave (DPP) ->
// workgroup -> one slab row, and sh_campos_reduce_kernel adds the rows in fp64 in a fixed order (a last-workgroup tail inside the kernel is the
// fold that lost twice for pose_reduce).  No atomics: every gradient is bitwise reproducible.
//
// Multi-view form (sh_colors_views_*_kernel): the V <= BAGS_MAX_SH_VIEWS views of one step over the same Gaussians.
// The row is read once each way; the forward stores 12 bytes per view, the backward adds the views' gradient rows in registers, in
// view order, each product and each add rounded once -- the bits of the fp32 fold ((g_0 + g_1) + g_2) ... of the single-view
// kernel's gradients -- and writes the row once.  The camera centres, the outputs and the cotangents travel as pointer tables by
// value in the kernel arguments (adam.hip's group table): nothing is uploaded.
//
// The four colour kernels are built from the same statements, spelled once where that leaves the generated code as it is:
// shc_load_row (the coefficient row) and shc_eval (a view's direction, basis and raw colour); the SH gradient rows leave through
// sh_rows.h (shr_stage, shr_span), which preprocess_bwd.hip shares.  The direction gradient is spelled in each backward kernel: as a function of its own it compiles to other code
// (profiles/sh_colors/NOTES.md), so a change to it is made in both.  They share statements, not kernels: the views backward stages
// 51200 bytes of LDS and needs twice the registers of the single-view one, which is render()'s default path.
#include "ordered_sum.h"
#include "sh_basis.h"
#include "sh_rows.h"

struct ShcIn { int P, deg; const float *shs, *shs_rest, *xyz, *campos; };

// the first 3 * nb floats of a Gaussian's coefficients into c[]; K == 16 loads the whole 192-byte row with wide loads
template <int K, bool SPLIT>
__device__ __forceinline__ void shc_load_row(const float* shs, const float* shs_rest, const size_t i, const int nb, float* __restrict__ c)
{
    const float* __restrict__ dcp = SPLIT ? shs + 3 * i : shs + i * (size_t)(K * 3);
    const float* __restrict__ rsp = SPLIT ? shs_rest + i * (size_t)((K - 1) * 3) : dcp + 3;
    if (K == 16) {
        if (SPLIT) {                      // 12 + 180 bytes, the second row only 4-byte aligned (dwordx4 loads at any dword)
            struct __attribute__((packed, aligned(4))) UF4 { float x, y, z, w; };
            c[0] = dcp[0]; c[1] = dcp[1]; c[2] = dcp[2];
            const UF4* u4 = reinterpret_cast<const UF4*>(rsp);
#pragma unroll
            for (int t = 0; t < 11; ++t) {
                const UF4 w = u4[t];
                c[3 + 4 * t] = w.x; c[4 + 4 * t] = w.y; c[5 + 4 * t] = w.z; c[6 + 4 * t] = w.w;
            }
            c[47] = rsp[44];
        } else {
            const float4* s4 = reinterpret_cast<const float4*>(dcp);
#pragma unroll
            for (int t = 0; t < 12; ++t) {
                const float4 w = s4[t];
                c[4 * t] = w.x; c[4 * t + 1] = w.y; c[4 * t + 2] = w.z; c[4 * t + 3] = w.w;
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < 3 * K; ++k) c[k] = (k < 3 * nb) ? (k < 3 ? dcp[k] : rsp[k - 3]) : 0.f;
    }
}

// One view of one Gaussian: the distance dl and the direction u from the camera centre cp, the basis b[16] and the raw colour.
// The ONE spelling of the direction and of the sum, shared by both forwards and by the backwards' clamp masks.  (c and b carry no
// __restrict__, and sh_basis gets the direction from locals, not through the references: either changes what the compiler makes
// of the kernels, profiles/sh_colors/NOTES.md.)
template <int K>
__device__ __forceinline__ void shc_eval(const float x, const float y, const float z, const float* cp, const int deg, const int nb,
                                         const float* c, float& dl, float& ux, float& uy, float& uz, float* b,
                                         float& r, float& g, float& bl)
{
    const float dx = x - cp[0], dy = y - cp[1], dz = z - cp[2];
    dl = sqrtf(dx * dx + dy * dy + dz * dz);
    const float vx = dx / dl, vy = dy / dl, vz = dz / dl;
    ux = vx; uy = vy; uz = vz;
    sh_basis(deg, vx, vy, vz, b);
    r = 0.f; g = 0.f; bl = 0.f;
#pragma unroll
    for (int t = 0; t < K; ++t)
        if (t < nb) { r += b[t] * c[3 * t]; g += b[t] * c[3 * t + 1]; bl += b[t] * c[3 * t + 2]; }
    r += 0.5f; g += 0.5f; bl += 0.5f;
}

template <int K, bool SPLIT>
__global__ void __launch_bounds__(256)
sh_colors_fwd_kernel(const ShcIn A, float* __restrict__ rgb)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= A.P) return;
    const int nb = (A.deg + 1) * (A.deg + 1);
    const float x = A.xyz[3 * (size_t)i], y = A.xyz[3 * (size_t)i + 1], z = A.xyz[3 * (size_t)i + 2];
    float c[48];
    shc_load_row<K, SPLIT>(A.shs, A.shs_rest, (size_t)i, nb, c);
    float dl, ux, uy, uz, b[16], r, g, bl;
    shc_eval<K>(x, y, z, A.campos, A.deg, nb, c, dl, ux, uy, uz, b, r, g, bl);
    rgb[3 * (size_t)i] = r < 0.f ? 0.f : r; rgb[3 * (size_t)i + 1] = g < 0.f ? 0.f : g; rgb[3 * (size_t)i + 2] = bl < 0.f ? 0.f : bl;
}

#define SHC_ROW 49       // floats per Gaussian in the views backward's LDS stage: 48 + 1, so that the 64 lanes' own rows fall on distinct banks

// need_dir: the direction gradient is wanted (deg > 0 and g_xyz or slab given); without it g_xyz, if given, receives zeros
template <int K, bool SPLIT>
__global__ void __launch_bounds__(256)
sh_colors_bwd_kernel(const ShcIn A, const float* __restrict__ g_rgb, float* __restrict__ g_shs, float* __restrict__ g_shs_rest,
                     float* __restrict__ g_xyz, float* __restrict__ slab, const int need_dir)
{
    __shared__ float srow[256][SHR_W];
    __shared__ float wsum[4][4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool on = i < A.P;
    const size_t ic = (size_t)(on ? i : A.P - 1);
    const int nb = (A.deg + 1) * (A.deg + 1);
    const float g0 = g_rgb[3 * ic], g1 = g_rgb[3 * ic + 1], g2 = g_rgb[3 * ic + 2];
    const bool any = on && (g0 != 0.f || g1 != 0.f || g2 != 0.f);
    float bs[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) bs[t] = 0.f;
    float m0 = 0.f, m1 = 0.f, m2 = 0.f, gx = 0.f, gy = 0.f, gz = 0.f;
    if (any) {
        const float x = A.xyz[3 * ic], y = A.xyz[3 * ic + 1], z = A.xyz[3 * ic + 2];
        float c[48];
        shc_load_row<K, SPLIT>(A.shs, A.shs_rest, ic, nb, c);
        float dl, ux, uy, uz, b[16], r, g, bl;
        shc_eval<K>(x, y, z, A.campos, A.deg, nb, c, dl, ux, uy, uz, b, r, g, bl);   // the forward's bits, hence its clamp decision
        m0 = r < 0.f ? 0.f : g0; m1 = g < 0.f ? 0.f : g1; m2 = bl < 0.f ? 0.f : g2;
#pragma unroll
        for (int t = 0; t < K; ++t) bs[t] = b[t];
        if (need_dir && (m0 != 0.f || m1 != 0.f || m2 != 0.f)) {
            float bx[16], by[16], bz[16];
            sh_basis_grad(A.deg, ux, uy, uz, bx, by, bz);
            float dux = 0.f, duy = 0.f, duz = 0.f;
#pragma unroll
            for (int t = 1; t < K; ++t)
                if (t < nb) {
                    const float s = c[3 * t] * m0 + c[3 * t + 1] * m1 + c[3 * t + 2] * m2;
                    dux += bx[t] * s; duy += by[t] * s; duz += bz[t] * s;
                }
            const float dot = ux * dux + uy * duy + uz * duz;          // d(d / |d|): the component along u drops out
            gx = (dux - ux * dot) / dl; gy = (duy - uy * dot) / dl; gz = (duz - uz * dot) / dl;
        }
    }
    if (g_xyz && on) { g_xyz[3 * ic] = gx; g_xyz[3 * ic + 1] = gy; g_xyz[3 * ic + 2] = gz; }

    if (g_shs || g_shs_rest) {                           // (kernel arguments: the whole workgroup takes the same side)
        shr_stage(&srow[threadIdx.x][0], bs, nb, m0, m1, m2);      // (bs is zero beyond the active degree already, and for a Gaussian that writes zeros)
        __syncthreads();
        if constexpr (SPLIT) {
            if (g_shs) shr_span<256u, 3u, 0u, SHR_PRODUCT>(srow, g_shs, A.P);
            if (g_shs_rest) shr_span<256u, 3u * (K - 1), 1u, SHR_PRODUCT>(srow, g_shs_rest, A.P);
        } else if (g_shs) {
            shr_span<256u, 3u * K, 0u, SHR_PRODUCT>(srow, g_shs, A.P);
        }
    }

    if (slab) {                                          // dL/dcampos = -sum dL/dxyz: wave, workgroup, one slab row
        const float r0 = wave_total_f(-gx), r1 = wave_total_f(-gy), r2 = wave_total_f(-gz);
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        if (lane == 63) { wsum[wave][0] = r0; wsum[wave][1] = r1; wsum[wave][2] = r2; wsum[wave][3] = 0.f; }
        __syncthreads();
        if (threadIdx.x < 4) {
            const int t = threadIdx.x;
            slab[(size_t)blockIdx.x * 4 + t] = (wsum[0][t] + wsum[1][t]) + (wsum[2][t] + wsum[3][t]);
        }
    }
}

// slab rows -> dL/dcampos in fp64, one workgroup per component (ordered_sum.h: slab_column_sum, pose_reduce_kernel's sum)
__device__ __forceinline__ void shc_campos_reduce(const float* __restrict__ slab, const int nblocks, const int t, float* __restrict__ g_campos)
{
    const double sum = slab_column_sum(slab, nblocks, SH_SLAB, t);
    if (threadIdx.x == 0) g_campos[t] = (float)sum;
}

__global__ void __launch_bounds__(256)
sh_campos_reduce_kernel(const float* __restrict__ slab, const int nblocks, float* __restrict__ g_campos)
{
    shc_campos_reduce(slab, nblocks, blockIdx.x, g_campos);
}

// ---------------------------------------------------------------------------------------------- the views of one step
struct ShcViewsIn { int P, deg, V; const float *shs, *shs_rest, *xyz; const float* campos[BAGS_MAX_SH_VIEWS]; };
struct ShcViewsOut { float* p[BAGS_MAX_SH_VIEWS]; };            // rgb (forward), dL/dcampos (reduction); an entry may be null
struct ShcViewsCot { const float* p[BAGS_MAX_SH_VIEWS]; };      // dL/drgb per view; null = no loss depends on that view

template <int K, bool SPLIT>
__global__ void __launch_bounds__(256)
sh_colors_views_fwd_kernel(const ShcViewsIn A, const ShcViewsOut O)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= A.P) return;
    const int nb = (A.deg + 1) * (A.deg + 1);
    const float x = A.xyz[3 * (size_t)i], y = A.xyz[3 * (size_t)i + 1], z = A.xyz[3 * (size_t)i + 2];
    float c[48];
    shc_load_row<K, SPLIT>(A.shs, A.shs_rest, (size_t)i, nb, c);
    for (int v = 0; v < A.V; ++v) {                      // per view: the single-view kernel's operations on campos_v
        const float* __restrict__ cp = A.campos[v];
        float dl, ux, uy, uz, b[16], r, g, bl;
        shc_eval<K>(x, y, z, cp, A.deg, nb, c, dl, ux, uy, uz, b, r, g, bl);
        float* __restrict__ rgb = O.p[v];
        rgb[3 * (size_t)i] = r < 0.f ? 0.f : r; rgb[3 * (size_t)i + 1] = g < 0.f ? 0.f : g; rgb[3 * (size_t)i + 2] = bl < 0.f ? 0.f : bl;
    }
}

// One thread per Gaussian.  A thread's LDS row first holds its V cotangent triples (zeros for a view that contributes nothing: a
// null pointer or an all-zero triple), so the view loop indexes them without a register array; after the loop it holds the summed
// gradient row for the store pass.  slab: V x gridDim.x rows of 4 floats, view-major.
template <int K, bool SPLIT>
__global__ void __launch_bounds__(256)
sh_colors_views_bwd_kernel(const ShcViewsIn A, const ShcViewsCot G, float* __restrict__ g_shs, float* __restrict__ g_shs_rest,
                           float* __restrict__ g_xyz, float* __restrict__ slab, const int need_dir)
{
    __shared__ float sacc[256][SHC_ROW];
    __shared__ float wsum[BAGS_MAX_SH_VIEWS][4][4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool on = i < A.P;
    const size_t ic = (size_t)(on ? i : A.P - 1);
    const int nb = (A.deg + 1) * (A.deg + 1);
    float* __restrict__ mine = &sacc[threadIdx.x][0];

    // the cotangents first, four views' loads in flight together (a view without one reads the position instead: any valid triple)
    u32 live = 0;
#pragma unroll
    for (int q = 0; q < BAGS_MAX_SH_VIEWS / 4; ++q)
        if (4 * q < A.V) {
            float t[4][3];
            bool have[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float* p = (4 * q + u < A.V) ? G.p[4 * q + u] : nullptr;
                have[u] = p != nullptr;
                const float* __restrict__ src = (have[u] ? p : A.xyz) + 3 * ic;
                t[u][0] = src[0]; t[u][1] = src[1]; t[u][2] = src[2];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bool ok = on && have[u] && (t[u][0] != 0.f || t[u][1] != 0.f || t[u][2] != 0.f);
                mine[3 * (4 * q + u)] = ok ? t[u][0] : 0.f; mine[3 * (4 * q + u) + 1] = ok ? t[u][1] : 0.f; mine[3 * (4 * q + u) + 2] = ok ? t[u][2] : 0.f;
                live |= ok ? (1u << (4 * q + u)) : 0u;
            }
        }

    float acc[48];
#pragma unroll
    for (int k = 0; k < 48; ++k) acc[k] = 0.f;
    float gx = 0.f, gy = 0.f, gz = 0.f, x = 0.f, y = 0.f, z = 0.f;
    float c[48];
#pragma unroll
    for (int k = 0; k < 48; ++k) c[k] = 0.f;
    if (live) {                                          // a Gaussian no view contributes to reads nothing else and writes zeros
        x = A.xyz[3 * ic]; y = A.xyz[3 * ic + 1]; z = A.xyz[3 * ic + 2];
        shc_load_row<K, SPLIT>(A.shs, A.shs_rest, ic, nb, c);
    }
    for (int v = 0; v < A.V; ++v) {
        float nx = 0.f, ny = 0.f, nz = 0.f;              // this view's dL/dd, for its dL/dcampos
        if ((live >> v) & 1u) {
            const float* __restrict__ cp = A.campos[v];
            const float g0 = mine[3 * v], g1 = mine[3 * v + 1], g2 = mine[3 * v + 2];
            float dl, ux, uy, uz, b[16], r, g, bl;
            shc_eval<K>(x, y, z, cp, A.deg, nb, c, dl, ux, uy, uz, b, r, g, bl);   // the forward's bits, hence its clamp decision for this view
            const float m0 = r < 0.f ? 0.f : g0, m1 = g < 0.f ? 0.f : g1, m2 = bl < 0.f ? 0.f : g2;
#pragma unroll
            for (int t = 0; t < K; ++t)
                if (t < nb) { acc[3 * t] += b[t] * m0; acc[3 * t + 1] += b[t] * m1; acc[3 * t + 2] += b[t] * m2; }
            if (need_dir && (m0 != 0.f || m1 != 0.f || m2 != 0.f)) {
                float bx[16], by[16], bz[16];
                sh_basis_grad(A.deg, ux, uy, uz, bx, by, bz);
                float dux = 0.f, duy = 0.f, duz = 0.f;
#pragma unroll
                for (int t = 1; t < K; ++t)
                    if (t < nb) {
                        const float s = c[3 * t] * m0 + c[3 * t + 1] * m1 + c[3 * t + 2] * m2;
                        dux += bx[t] * s; duy += by[t] * s; duz += bz[t] * s;
                    }
                const float dot = ux * dux + uy * duy + uz * duz;
                nx = (dux - ux * dot) / dl; ny = (duy - uy * dot) / dl; nz = (duz - uz * dot) / dl;
                gx += nx; gy += ny; gz += nz;
            }
        }
        if (slab) {                                      // (a kernel argument inside a uniform loop: every lane is here)
            const float r0 = wave_total_f(-nx), r1 = wave_total_f(-ny), r2 = wave_total_f(-nz);
            const int wave = threadIdx.x >> 6;
            if ((threadIdx.x & 63) == 63) { wsum[v][wave][0] = r0; wsum[v][wave][1] = r1; wsum[v][wave][2] = r2; wsum[v][wave][3] = 0.f; }
        }
    }
    if (g_xyz && on) { g_xyz[3 * ic] = gx; g_xyz[3 * ic + 1] = gy; g_xyz[3 * ic + 2] = gz; }

    if (g_shs || g_shs_rest) {                           // the row's own thread was the only reader of its cotangents
#pragma unroll
        for (int k = 0; k < 3 * K; ++k) mine[k] = acc[k];
    }
    __syncthreads();
    if constexpr (SPLIT) {
        if (g_shs) shr_span<256u, 3u, 0u, SHR_PACKED>(sacc, g_shs, A.P);
        if (g_shs_rest) shr_span<256u, 3u * (K - 1), 1u, SHR_PACKED>(sacc, g_shs_rest, A.P);
    } else if (g_shs) {
        shr_span<256u, 3u * K, 0u, SHR_PACKED>(sacc, g_shs, A.P);
    }
    if (slab && threadIdx.x < 4 * A.V) {                 // one slab row per (view, workgroup), the single-view kernel's sum of the waves
        const int v = threadIdx.x >> 2, t = threadIdx.x & 3;
        slab[((size_t)v * gridDim.x + blockIdx.x) * 4 + t] = (wsum[v][0][t] + wsum[v][1][t]) + (wsum[v][2][t] + wsum[v][3][t]);
    }
}

// grid (3, V): view v's slab rows -> its dL/dcampos; nblocks == 0 writes zeros (degree 0, P == 0: no direction gradient)
__global__ void __launch_bounds__(256)
sh_campos_views_reduce_kernel(const float* __restrict__ slab, const int nblocks, const ShcViewsOut O)
{
    float* out = O.p[blockIdx.y];
    if (!out) return;
    shc_campos_reduce(slab + (size_t)blockIdx.y * nblocks * 4, nblocks, blockIdx.x, out);
}

// ---------------------------------------------------------------------------------------------- launchers
// CALL(K, SPLIT) for the instance that fits the operands `a`: the stored coefficients and the layout (shs_rest given = split)
#define SHC_DISPATCH(a, CALL)                                                               \
    if ((a).shs_rest) {                                                                     \
        if ((a).K == 16) { CALL(16, true) } else if ((a).K == 9) { CALL(9, true) } else { CALL(4, true) } \
    } else {                                                                                \
        if ((a).K == 16) { CALL(16, false) } else if ((a).K == 9) { CALL(9, false) } else if ((a).K == 4) { CALL(4, false) } else { CALL(1, false) } \
    }

// What a backward enqueues, from what it was asked for: need_dir as the kernels take it; rows = the slab if the campos sums are to
// be written, else null (degree 0, P <= 0: no direction gradient, dL/dcampos is zero); main = does the colour kernel run at all
struct ShcBwdPlan { int nb, need_dir; float* rows; bool main; };
static ShcBwdPlan shc_bwd_plan(const int P, const int deg, const bool want_sh, const bool want_xyz, const bool want_campos, float* slab)
{
    ShcBwdPlan p;                                       // (the P > 0 guards serve the views launcher: the single-view one has returned by then)
    p.nb = cdiv(P > 0 ? P : 1, 256);
    p.need_dir = (P > 0 && deg > 0 && (want_xyz || want_campos)) ? 1 : 0;
    p.rows = (p.need_dir && want_campos) ? slab : nullptr;
    p.main = P > 0 && (want_sh || want_xyz || p.rows);
    return p;
}

hipError_t launch_sh_colors_fwd(const BagsShColors& a, float* rgb, hipStream_t st)
{
    if (a.P <= 0) return hipSuccess;
    const ShcIn A{a.P, a.sh_degree, a.shs, a.shs_rest, a.xyz, a.campos};
    const dim3 grid((unsigned)cdiv(a.P, 256));
#define SHC_FWD(K_, S_) hipLaunchKernelGGL((sh_colors_fwd_kernel<K_, S_>), grid, dim3(256), 0, st, A, rgb);
    SHC_DISPATCH(a, SHC_FWD)
#undef SHC_FWD
    return hipGetLastError();
}

hipError_t launch_sh_colors_bwd(const BagsShColors& a, const float* g_rgb, float* slab, float* g_shs, float* g_shs_rest, float* g_xyz,
                                float* g_campos, hipStream_t st)
{
    if (a.P <= 0) return g_campos ? hipMemsetAsync(g_campos, 0, 3 * sizeof(float), st) : hipSuccess;
    const ShcIn A{a.P, a.sh_degree, a.shs, a.shs_rest, a.xyz, a.campos};
    const ShcBwdPlan p = shc_bwd_plan(A.P, A.deg, g_shs || g_shs_rest, g_xyz != nullptr, g_campos != nullptr, slab);
    if (p.main) {
#define SHC_BWD(K_, S_) hipLaunchKernelGGL((sh_colors_bwd_kernel<K_, S_>), dim3(p.nb), dim3(256), 0, st, A, g_rgb, g_shs, g_shs_rest, g_xyz, p.rows, p.need_dir);
        SHC_DISPATCH(a, SHC_BWD)
#undef SHC_BWD
    }
    if (g_campos) {
        if (p.rows) hipLaunchKernelGGL(sh_campos_reduce_kernel, dim3(3), dim3(256), 0, st, p.rows, p.nb, g_campos);
        else { const hipError_t e = hipMemsetAsync(g_campos, 0, 3 * sizeof(float), st); if (e != hipSuccess) return e; }   // degree 0: no direction
    }
    return hipGetLastError();
}

hipError_t launch_sh_colors_views_fwd(const BagsShColorsViews& a, float* const* rgb, hipStream_t st)
{
    if (a.P <= 0) return hipSuccess;
    ShcViewsIn A{a.P, a.sh_degree, a.V, a.shs, a.shs_rest, a.xyz, {}};
    ShcViewsOut O{};
    for (int v = 0; v < a.V; ++v) { A.campos[v] = a.campos[v]; O.p[v] = rgb[v]; }
    const dim3 grid((unsigned)cdiv(a.P, 256));
#define SHC_FWD(K_, S_) hipLaunchKernelGGL((sh_colors_views_fwd_kernel<K_, S_>), grid, dim3(256), 0, st, A, O);
    SHC_DISPATCH(a, SHC_FWD)
#undef SHC_FWD
    return hipGetLastError();
}

hipError_t launch_sh_colors_views_bwd(const BagsShColorsViews& a, const float* const* g_rgb, float* slab, float* g_shs, float* g_shs_rest,
                                      float* g_xyz, float* const* g_campos, hipStream_t st)
{
    ShcViewsIn A{a.P, a.sh_degree, a.V, a.shs, a.shs_rest, a.xyz, {}};
    ShcViewsCot G{};
    ShcViewsOut C{};
    bool any_campos = false;
    for (int v = 0; v < a.V; ++v) {
        A.campos[v] = a.campos[v]; G.p[v] = g_rgb ? g_rgb[v] : nullptr; C.p[v] = g_campos ? g_campos[v] : nullptr;
        any_campos = any_campos || C.p[v] != nullptr;
    }
    const ShcBwdPlan p = shc_bwd_plan(A.P, A.deg, g_shs || g_shs_rest, g_xyz != nullptr, any_campos, slab);
    if (p.main) {
#define SHC_BWD(K_, S_) hipLaunchKernelGGL((sh_colors_views_bwd_kernel<K_, S_>), dim3(p.nb), dim3(256), 0, st, A, G, g_shs, g_shs_rest, g_xyz, p.rows, p.need_dir);
        SHC_DISPATCH(a, SHC_BWD)
#undef SHC_BWD
    }
    if (any_campos) hipLaunchKernelGGL(sh_campos_views_reduce_kernel, dim3(3, a.V), dim3(256), 0, st, p.rows, p.rows ? p.nb : 0, C);
    return hipGetLastError();
}
