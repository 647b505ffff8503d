// mcmc.hip -- the 3DGS-MCMC densification strategy (bags_compute_relocation / bags_mcmc_relocate / bags_mcmc_add_new /
// bags_mcmc_noise, include/bags_raster.h).
//
// The reference runs relocate_gs / add_new_gs as boolean-mask indexing, bincount, compute_relocation and torch.cat over six parameters
// and their two Adam moments, and the per-iteration noise step as about twenty small launches that build a (P,3,3) covariance.  Here:
//
//   count     one thread per listed source row -> c[s], how often row s is listed (integer atomics: the sums do not depend on order)
//   stage     one thread per row with c[s] > 0 -> its new opacity and scaling (logit / log applied), 16 bytes in the workspace, computed
//             from the OLD row: nothing of the set has been written yet
//   relocate  one thread per (dead row, element): the dead row takes its source's parameters, the source its staged values, the
//             source's moments are zeroed; nothing else is touched
//   add_new   one pass over the OUTPUT elements of every (group, array), as densify_apply: coalesced float4 stores, gathered reads
//   noise     one thread per row: gate, covariance and the matrix-vector product in registers; only the new xyz is written
//
// compute_relocation's alternating sum is ill-conditioned, and the relocated values pass through logit / log; both, and the noise step,
// are evaluated in double from the fp32 inputs and rounded to fp32 once.  Built with -ffp-contract=off.  No floating-point atomics:
// two runs give the same bits.  add_new's walk over the output elements is the one of csrc/row_rebuild.h, which densify_apply_kernel shares.
#include "bags_common.h"
#include "philox_normal.h"
#include "row_rebuild.h"
#include <float.h>

#define MCMC_BLOCK 256
#define MCMC_TABLE (BAGS_MCMC_MAX_BINOMS * BAGS_MCMC_MAX_BINOMS)

enum { MSEG_OPACITY = 1, MSEG_SCALING = 2 };               // beside ROWSEG_COPY / MOMENT / ZERO

struct McmcWorkspace { u32* count; float4* stage; };

static inline int mcmc_blocks(size_t n) { return (int)((n + MCMC_BLOCK - 1) / MCMC_BLOCK); }

// workspace (base rounded up here): [count P: times a row is listed | stage P: (opacity, scaling x 3) of a listed row, as stored]
static size_t carve_mcmc(void* base, int P, McmcWorkspace* out)
{
    Carver c(base);
    const int n = P > 0 ? P : 1;
    McmcWorkspace w;
    w.count = c.take<u32>((size_t)n); w.stage = c.take<float4>((size_t)n);
    if (out) *out = w;
    return c.used();
}
size_t mcmc_workspace_bytes(int P) { return carve_mcmc(nullptr, P, nullptr) + BASE_SLACK; }

// ------------------------------------------------------------------------------------------------ compute_relocation
__device__ __forceinline__ void load_binoms(float* s_b, const float* __restrict__ binoms, const int n_max)
{
    for (int i = threadIdx.x; i < n_max * n_max; i += MCMC_BLOCK) s_b[i] = binoms[i];
    __syncthreads();
}

// o_new = 1 - (1 - o_old)^(1/n) and coeff = o_old / sum_{i=1..n} sum_{k<i} b[i-1][k] (-1)^k o_new^(k+1) / sqrt(k+1), summed by column:
// the inner sums are sums of integers below 2^53, exact in double whatever the order.  n in 1..n_max-1.
__device__ __forceinline__ void relocation(const float* b, const int n_max, const double o_old, const int n, double& o_new, double& coeff)
{
    o_new = 1.0 - pow(1.0 - o_old, 1.0 / (double)n);
    double acc = 0.0, pw = 1.0;
    for (int k = 0; k < n; ++k) {
        double col = 0.0;
        for (int i = k; i < n; ++i) col += (double)b[i * n_max + k];
        pw *= o_new;
        const double t = col * (1.0 / sqrt((double)(k + 1))) * pw;
        acc += (k & 1) ? -t : t;
    }
    coeff = o_old / acc;
}

__global__ void __launch_bounds__(MCMC_BLOCK) compute_relocation_kernel(const float* __restrict__ o_old, const float* __restrict__ sc_old,
                                                                        const int32_t* __restrict__ N, const float* __restrict__ binoms, const int n_max,
                                                                        const int P, float* __restrict__ o_out, float* __restrict__ sc_out)
{
    __shared__ float s_b[MCMC_TABLE];
    load_binoms(s_b, binoms, n_max);
    const size_t r = (size_t)blockIdx.x * MCMC_BLOCK + threadIdx.x;
    if (r >= (size_t)P) return;
    const int n = min(max(N[r], 1), n_max - 1);
    double on, coeff;
    relocation(s_b, n_max, (double)o_old[r], n, on, coeff);
    o_out[r] = (float)on;
#pragma unroll
    for (int c = 0; c < 3; ++c) sc_out[3 * r + c] = (float)(coeff * (double)sc_old[3 * r + c]);
}

// ------------------------------------------------------------------------------------------------ count, stage
__global__ void __launch_bounds__(MCMC_BLOCK) mcmc_count_kernel(const int32_t* __restrict__ sampled, const int n_sampled, const int P, u32* __restrict__ count)
{
    const size_t j = (size_t)blockIdx.x * MCMC_BLOCK + threadIdx.x;
    if (j >= (size_t)n_sampled) return;
    const int s = sampled[j];
    if ((u32)s < (u32)P) atomicAdd(&count[s], 1u);                       // a row outside the set is listed by no valid caller: it is skipped everywhere
}

__global__ void __launch_bounds__(MCMC_BLOCK) mcmc_stage_kernel(const float* __restrict__ opacity, const float* __restrict__ scaling,
                                                                const u32* __restrict__ count, const float* __restrict__ binoms, const int n_max, const int P,
                                                                const double min_opacity, float4* __restrict__ stage)
{
    const size_t r = (size_t)blockIdx.x * MCMC_BLOCK + threadIdx.x;
    if (r >= (size_t)P) return;
    const u32 c = count[r];
    if (c == 0) return;
    const int n = (int)min(max(c + 1u, 1u), (u32)(n_max - 1));
    const double o = 1.0 / (1.0 + exp(-(double)opacity[r]));
    double on, coeff;
    relocation(binoms, n_max, o, n, on, coeff);                          // few rows are listed, with small counts: the table is read through the
                                                                         // cache here, not staged in LDS by every workgroup
    on = fmin(fmax(on, min_opacity), 1.0 - (double)FLT_EPSILON);
    float4 out;
    out.x = (float)log(on / (1.0 - on));
    out.y = (float)log(coeff * exp((double)scaling[3 * r]));
    out.z = (float)log(coeff * exp((double)scaling[3 * r + 1]));
    out.w = (float)log(coeff * exp((double)scaling[3 * r + 2]));
    stage[r] = out;
}

__device__ __forceinline__ float staged(const float4 v, const u32 mode, const u32 c)
{
    return mode == MSEG_OPACITY ? v.x : (c == 0 ? v.y : c == 1 ? v.z : v.w);
}

// ------------------------------------------------------------------------------------------------ relocate
struct RelocSeg {
    float* param; float* m; float* v;
    u32 first_block;               // of this segment in the grid; 0xFFFFFFFF for an unused slot
    u32 width, mode, pad;
};
struct RelocParams {
    RelocSeg seg[BAGS_DENSIFY_MAX_GROUPS];
    const int32_t* dead; const int32_t* sampled; const float4* stage;
    int P, D;
};

__global__ void __launch_bounds__(MCMC_BLOCK) mcmc_relocate_kernel(const RelocParams a)
{
    const u32 b = blockIdx.x;
    RelocSeg G = a.seg[0];                                               // rowseg_find (row_rebuild.h) costs this kernel 16 SGPRs: spelled here
#pragma unroll
    for (int k = 1; k < BAGS_DENSIFY_MAX_GROUPS; ++k)
        if (b >= a.seg[k].first_block) G = a.seg[k];
    const u32 w = G.width;
    const size_t e = (size_t)(b - G.first_block) * MCMC_BLOCK + threadIdx.x;
    if (e >= (size_t)a.D * w) return;
    const size_t j = e / w;
    const u32 c = (u32)(e - j * w);
    const int s = a.sampled[j], d = a.dead[j];
    if ((u32)s >= (u32)a.P || (u32)d >= (u32)a.P) return;                 // rows outside the set: nothing is read or written
    const size_t se = (size_t)s * w + c, de = (size_t)d * w + c;
    if (G.mode == ROWSEG_COPY) G.param[de] = G.param[se];
    else {                                                               // every j that lists s stores the same bits to it
        const float val = staged(a.stage[s], G.mode, c);
        G.param[de] = val; G.param[se] = val;
    }
    if (G.m) { G.m[se] = 0.0f; G.v[se] = 0.0f; }
}

// ------------------------------------------------------------------------------------------------ add_new
struct AddParams {
    RowSeg seg[ROWSEG_MAX_SEGS];
    const int32_t* sampled; const u32* count; const float4* stage;
    long long P_new;
    int P;
};
struct AddRow { size_t s; bool valid, source; };

__device__ __forceinline__ AddRow add_row(const AddParams& a, const size_t row)
{
    AddRow r;
    if (row < (size_t)a.P) { r.s = row; r.valid = true; r.source = a.count[row] != 0u; }
    else { const int s = a.sampled[row - (size_t)a.P]; r.valid = (u32)s < (u32)a.P; r.s = r.valid ? (size_t)s : 0; r.source = true; }
    return r;
}

__device__ __forceinline__ float add_value(const AddParams& a, const RowSeg& G, const AddRow r, const u32 c)
{
    if (!r.valid) return 0.0f;
    if (G.mode == ROWSEG_MOMENT) return r.source ? 0.0f : G.src[r.s * G.width + c];
    if (r.source && G.mode != ROWSEG_COPY) return staged(a.stage[r.s], G.mode, c);
    return G.src[r.s * G.width + c];
}

__global__ void __launch_bounds__(ROWSEG_BLOCK) mcmc_add_new_kernel(const AddParams a)
{
    RowSeg G;                                                            // found here, not in the walker: see row_rebuild.h
    rowseg_find(G, a.seg, blockIdx.x);
    rowseg_walk(G, a.P_new, [&](const size_t row) { return add_row(a, row); }, [&](const AddRow r, const u32 c) { return add_value(a, G, r, c); });
}

// ------------------------------------------------------------------------------------------------ noise
__global__ void __launch_bounds__(MCMC_BLOCK) mcmc_noise_kernel(float* __restrict__ xyz, const float* __restrict__ opacity, const float* __restrict__ scaling,
                                                                const float* __restrict__ rotation, const int P, const float* __restrict__ noise,
                                                                const u32 seed_lo, const u32 seed_hi, const double scale, const double k, const double x0,
                                                                const double modifier)
{
    const size_t r = (size_t)blockIdx.x * MCMC_BLOCK + threadIdx.x;
    if (r >= (size_t)P) return;
    float zf[3];
    if (noise) { zf[0] = noise[3 * r]; zf[1] = noise[3 * r + 1]; zf[2] = noise[3 * r + 2]; }
    else normal3(seed_lo, seed_hi, (u32)r, 0u, zf);
    const double o = 1.0 / (1.0 + exp(-(double)opacity[r]));
    const double g = 1.0 / (1.0 + exp(-k * ((1.0 - o) - x0)));
    const double v0 = (double)zf[0] * g * scale, v1 = (double)zf[1] * g * scale, v2 = (double)zf[2] * g * scale;
    const double r0 = rotation[4 * r], r1 = rotation[4 * r + 1], r2 = rotation[4 * r + 2], r3 = rotation[4 * r + 3];
    const double nq = sqrt(r0 * r0 + r1 * r1 + r2 * r2 + r3 * r3);
    const double w = r0 / nq, x = r1 / nq, y = r2 / nq, z = r3 / nq;
    const double s0 = modifier * exp((double)scaling[3 * r]), s1 = modifier * exp((double)scaling[3 * r + 1]), s2 = modifier * exp((double)scaling[3 * r + 2]);
    // L = R diag(s), Sigma = L L^T
    const double L[3][3] = {{(1.0 - 2.0 * (y * y + z * z)) * s0, (2.0 * (x * y - w * z)) * s1, (2.0 * (x * z + w * y)) * s2},
                            {(2.0 * (x * y + w * z)) * s0, (1.0 - 2.0 * (x * x + z * z)) * s1, (2.0 * (y * z - w * x)) * s2},
                            {(2.0 * (x * z - w * y)) * s0, (2.0 * (y * z + w * x)) * s1, (1.0 - 2.0 * (x * x + y * y)) * s2}};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double c0 = L[i][0] * L[0][0] + L[i][1] * L[0][1] + L[i][2] * L[0][2];
        const double c1 = L[i][0] * L[1][0] + L[i][1] * L[1][1] + L[i][2] * L[1][2];
        const double c2 = L[i][0] * L[2][0] + L[i][1] * L[2][1] + L[i][2] * L[2][2];
        xyz[3 * r + i] = (float)((double)xyz[3 * r + i] + (c0 * v0 + c1 * v1 + c2 * v2));
    }
}

// ------------------------------------------------------------------------------------------------ launchers (arguments validated by api.hip)
hipError_t launch_compute_relocation(const float* opacity_old, const float* scale_old, const int32_t* N, const float* binoms, int n_max, int P,
                                     float* opacity_new, float* scale_new, hipStream_t st)
{
    hipLaunchKernelGGL(compute_relocation_kernel, dim3((unsigned)mcmc_blocks((size_t)P)), dim3(MCMC_BLOCK), 0, st, opacity_old, scale_old, N, binoms, n_max, P,
                       opacity_new, scale_new);
    return hipGetLastError();
}

// count + stage: what relocate and add_new share.  opacity / scaling: the OLD arrays of the groups with those roles.
static hipError_t launch_mcmc_stage(const BagsMcmcGroup* groups, int n_groups, int P, const int32_t* sampled, int n_sampled, const float* binoms, int n_max,
                                    double min_opacity, const McmcWorkspace& w, hipStream_t st)
{
    const float* opacity = nullptr; const float* scaling = nullptr;
    for (int k = 0; k < n_groups; ++k) {
        if (groups[k].role == BAGS_ROLE_OPACITY) opacity = groups[k].param;
        if (groups[k].role == BAGS_ROLE_SCALING) scaling = groups[k].param;
    }
    hipError_t e = hipMemsetAsync(w.count, 0, (size_t)P * sizeof(u32), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mcmc_count_kernel, dim3((unsigned)mcmc_blocks((size_t)n_sampled)), dim3(MCMC_BLOCK), 0, st, sampled, n_sampled, P, w.count);
    hipLaunchKernelGGL(mcmc_stage_kernel, dim3((unsigned)mcmc_blocks((size_t)P)), dim3(MCMC_BLOCK), 0, st, opacity, scaling, w.count, binoms, n_max, P,
                       min_opacity, w.stage);
    return hipGetLastError();
}

static inline u32 mcmc_mode(int role) { return role == BAGS_ROLE_OPACITY ? MSEG_OPACITY : role == BAGS_ROLE_SCALING ? MSEG_SCALING : ROWSEG_COPY; }

hipError_t launch_mcmc_relocate(const BagsMcmcGroup* groups, int n_groups, int P, const int32_t* dead, const int32_t* sampled, int n_sampled,
                                const float* binoms, int n_max, double min_opacity, void* workspace, hipStream_t st)
{
    McmcWorkspace w; carve_mcmc(workspace, P, &w);
    hipError_t e = launch_mcmc_stage(groups, n_groups, P, sampled, n_sampled, binoms, n_max, min_opacity, w, st);
    if (e != hipSuccess) return e;
    RelocParams a;
    size_t blocks = 0;
    for (int k = 0; k < n_groups; ++k) {
        const BagsMcmcGroup& g = groups[k];
        a.seg[k] = RelocSeg{g.param, g.exp_avg, g.exp_avg_sq, (u32)blocks, (u32)g.width, mcmc_mode(g.role), 0};
        blocks += ((size_t)n_sampled * (size_t)g.width + MCMC_BLOCK - 1) / MCMC_BLOCK;
    }
    for (int k = n_groups; k < BAGS_DENSIFY_MAX_GROUPS; ++k) a.seg[k] = RelocSeg{nullptr, nullptr, nullptr, 0xFFFFFFFFu, 1, ROWSEG_COPY, 0};
    if (blocks >= 0x7FFFFFFFull) return hipErrorInvalidValue;
    a.dead = dead; a.sampled = sampled; a.stage = w.stage; a.P = P; a.D = n_sampled;
    hipLaunchKernelGGL(mcmc_relocate_kernel, dim3((unsigned)blocks), dim3(MCMC_BLOCK), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_mcmc_add_new(const BagsMcmcGroup* groups, int n_groups, int P, const int32_t* sampled, int n_sampled, const float* binoms,
                               int n_max, double min_opacity, void* workspace, float* accum_out, float* denom_out, float* radii_out, hipStream_t st)
{
    McmcWorkspace w; carve_mcmc(workspace, P, &w);
    hipError_t e = launch_mcmc_stage(groups, n_groups, P, sampled, n_sampled, binoms, n_max, min_opacity, w, st);
    if (e != hipSuccess) return e;
    const long long P_new = (long long)P + n_sampled;
    AddParams a;
    const unsigned blocks = rowseg_table(a.seg, groups, n_groups, P_new, mcmc_mode, accum_out, denom_out, radii_out);
    if (!blocks) return hipErrorInvalidValue;
    a.sampled = sampled; a.count = w.count; a.stage = w.stage; a.P_new = P_new; a.P = P;
    hipLaunchKernelGGL(mcmc_add_new_kernel, dim3(blocks), dim3(ROWSEG_BLOCK), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_mcmc_noise(float* xyz, const float* opacity, const float* scaling, const float* rotation, int P, const float* noise, uint64_t seed,
                             double scale, double k, double x0, double scaling_modifier, hipStream_t st)
{
    hipLaunchKernelGGL(mcmc_noise_kernel, dim3((unsigned)mcmc_blocks((size_t)P)), dim3(MCMC_BLOCK), 0, st, xyz, opacity, scaling, rotation, P, noise,
                       (u32)seed, (u32)(seed >> 32), scale, k, x0, scaling_modifier);
    return hipGetLastError();
}
