// densify.hip -- densify-and-prune of the Gaussian set and the opacity reset (bags_densify_plan / bags_densify_apply /
// bags_reset_opacity, include/bags_raster.h).
//
// The reference runs GaussianModel.densify_and_prune (scene/gaussian_model.py:393-447) as clone, split, prune: three rounds of
// boolean-mask indexing and torch.cat over six parameters and their two Adam moments.  Everything a row's fate depends on is a
// function of that source row alone (a clone has its source's opacity and scale, the N children of a split row share theirs), so a
// source row yields 0, 1, 2 or N output rows and three exclusive scans place them:
//
//   decide   one thread per source row -> a flag word (kept / clone / children in the output) and per-workgroup counts
//   scan     one workgroup: exclusive scan of the per-workgroup counts, totals for the host (the one synchronisation of the call)
//   map      one thread per source row -> (source row, kind) of every output row: the provenance map, which is the gather index
//   apply    one pass over the OUTPUT elements of every (group, array): coalesced float4 stores, gathered reads; children's xyz
//            and scaling computed, moments of new rows and the three statistics arrays zero
//
// Output order (what the reference's cat / mask sequence produces): kept originals in source order, clones in source order, then
// the children block with child k of the j-th surviving split row at k * S + j.
// Fixed order, no atomics: bitwise reproducible.  Built with -ffp-contract=off: the children's values are the operations spelled
// here, each rounded once.  apply's walk over the output elements is the one of csrc/row_rebuild.h, which mcmc_add_new_kernel shares.
#include "bags_common.h"
#include "binning_common.h"
#include "philox_normal.h"
#include "row_rebuild.h"

#define DENS_BLOCK 256
#define DENS_COUNTS 5                                       // kept, clones out, split rows out, clone-selected, split-selected

enum { F_KEPT = 1, F_CLONE = 2, F_CHILD = 4, F_CLONE_SEL = 8, F_SPLIT_SEL = 16 };
enum { SEG_XYZ = 1, SEG_SCALING = 2 };                      // beside ROWSEG_COPY / MOMENT / ZERO

struct DensWorkspace { u32* cls; u32* sums; u32* totals; int nb; };

static inline int dens_blocks(int P) { return (int)(((size_t)P + DENS_BLOCK - 1) / DENS_BLOCK); }

// workspace (base rounded up here): [cls P: a row's flag word | sums nb * DENS_COUNTS: per-workgroup counts | totals DENS_COUNTS]
static size_t carve_densify(void* base, int P, DensWorkspace* out)
{
    Carver c(base);
    const int n = P > 0 ? P : 1;
    DensWorkspace w;
    w.nb = dens_blocks(n);
    w.cls = c.take<u32>((size_t)n); w.sums = c.take<u32>((size_t)w.nb * DENS_COUNTS); w.totals = c.take<u32>(DENS_COUNTS);
    if (out) *out = w;
    return c.used();
}
size_t densify_workspace_bytes(int P) { return carve_densify(nullptr, P, nullptr) + BASE_SLACK; }

// ------------------------------------------------------------------------------------------------ decide
struct DecideParams {
    const float* accum; const float* denom; const float* radii; const float* scaling; const float* opacity;
    float max_grad, min_opacity, dense_thr, world_thr, max_screen, child_div;
    int use_screen, pre_densify, P;
};

__device__ __forceinline__ u32 decide_row(const DecideParams& a, const size_t r)
{
    float g = a.accum[r] / a.denom[r];
    if (g != g) g = 0.0f;
    const float e0 = expf(a.scaling[3 * r]), e1 = expf(a.scaling[3 * r + 1]), e2 = expf(a.scaling[3 * r + 2]);
    const float s = fmaxf(e0, fmaxf(e1, e2));
    const float x = a.opacity[r];
    const float o = 1.0f / (1.0f + expf(-x));
    const bool sel = fabsf(g) >= a.max_grad;
    const bool clone = sel && s <= a.dense_thr;
    const bool split = sel && s > a.dense_thr;
    const bool low = o < a.min_opacity;
    // the rows the clone and split steps append carry max_radii2D = 0; so does every row under the published order
    const bool screen_new = a.use_screen && 0.0f > a.max_screen;
    const bool screen_old = a.use_screen && (a.pre_densify ? a.radii[r] > a.max_screen : 0.0f > a.max_screen);
    const bool world = a.use_screen && s > a.world_thr;
    u32 f = 0;
    if (!split && !(low || screen_old || world)) f |= F_KEPT;
    if (clone) { f |= F_CLONE_SEL; if (!(low || screen_new || world)) f |= F_CLONE; }
    if (split) {
        f |= F_SPLIT_SEL;
        // a child is tested with its own shrunk scale, through the log / exp round trip its stored value makes
        const float c0 = expf(logf(e0 / a.child_div)), c1 = expf(logf(e1 / a.child_div)), c2 = expf(logf(e2 / a.child_div));
        const float sc = fmaxf(c0, fmaxf(c1, c2));
        if (!(low || screen_new || (a.use_screen && sc > a.world_thr))) f |= F_CHILD;
    }
    return f;
}

__global__ void __launch_bounds__(DENS_BLOCK) densify_decide_kernel(const DecideParams a, u32* __restrict__ cls, u32* __restrict__ sums, const int nb)
{
    __shared__ u32 s_cnt[DENS_BLOCK / 64][DENS_COUNTS];
    const size_t r = (size_t)blockIdx.x * DENS_BLOCK + threadIdx.x;
    u32 f = 0;
    if (r < (size_t)a.P) { f = decide_row(a, r); cls[r] = f; }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < DENS_COUNTS; ++k) {
        const u64 m = __ballot((f >> k) & 1u);
        if (lane == 0) s_cnt[wave][k] = (u32)__popcll(m);
    }
    __syncthreads();
    if (threadIdx.x < DENS_COUNTS) {
        u32 t = 0;
#pragma unroll
        for (int w = 0; w < DENS_BLOCK / 64; ++w) t += s_cnt[w][threadIdx.x];
        sums[(size_t)threadIdx.x * nb + blockIdx.x] = t;
    }
}

// ------------------------------------------------------------------------------------------------ scan
// One workgroup of 1024: sums[k][0..nb) becomes its exclusive scan for the three placed counts, totals[k] the five sums.
__global__ void __launch_bounds__(1024) densify_scan_kernel(u32* __restrict__ sums, const int nb, u32* __restrict__ totals)
{
    __shared__ u32 s_wave[17];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = 0; k < DENS_COUNTS; ++k) {
        u32* row = sums + (size_t)k * nb;
        u32 carry = 0;
        for (int base = 0; base < nb; base += 1024) {
            const int i = base + (int)threadIdx.x;
            const u32 v = i < nb ? row[i] : 0u;
            const u32 incl = wave_incl_scan(v);
            __syncthreads();                                 // s_wave free again
            if (lane == 63) s_wave[wave] = incl;
            __syncthreads();
            u32 before = 0, all = 0;
#pragma unroll
            for (int w = 0; w < 16; ++w) { before += (w < wave) ? s_wave[w] : 0u; all += s_wave[w]; }
            if (i < nb && k < 3) row[i] = carry + before + incl - v;
            carry += all;
        }
        if (threadIdx.x == 0) totals[k] = carry;
    }
}

// ------------------------------------------------------------------------------------------------ map
__global__ void __launch_bounds__(DENS_BLOCK) densify_map_kernel(const u32* __restrict__ cls, const u32* __restrict__ sums, const u32* __restrict__ totals,
                                                                 const int nb, const int P, const int N, const long long P_new, int2* __restrict__ prov)
{
    __shared__ u32 s_cnt[DENS_BLOCK / 64][3];
    const size_t r = (size_t)blockIdx.x * DENS_BLOCK + threadIdx.x;
    const u32 f = r < (size_t)P ? cls[r] : 0u;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    u32 pre[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const u64 m = __ballot((f >> k) & 1u);
        pre[k] = (u32)__popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) s_cnt[wave][k] = (u32)__popcll(m);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        for (int w = 0; w < DENS_BLOCK / 64; ++w) pre[k] += (w < wave) ? s_cnt[w][k] : 0u;
        pre[k] += sums[(size_t)k * nb + blockIdx.x];
    }
    const long long K = totals[0], C = totals[1], S = totals[2];
    // the bound repeats what the host derived from the same totals: a caller that passes another P_new gets no write outside its map
    if (f & F_KEPT)  { const long long d = pre[0];     if (d < P_new) prov[d] = make_int2((int)r, 0); }
    if (f & F_CLONE) { const long long d = K + pre[1]; if (d < P_new) prov[d] = make_int2((int)r, 1); }
    if (f & F_CHILD)
        for (int c = 0; c < N; ++c) { const long long d = K + C + (long long)c * S + pre[2]; if (d < P_new) prov[d] = make_int2((int)r, 2 + c); }
}

// ------------------------------------------------------------------------------------------------ apply
struct ApplyParams {
    RowSeg seg[ROWSEG_MAX_SEGS];
    const int2* prov;
    const float* xyz; const float* scaling; const float* rotation; const float* noise;
    long long P_new;
    u32 seed_lo, seed_hi;
    int P, N;
    float child_div;
};

// normal3: three standard normals for (seed, source row, child), philox_normal.h

// component c of a child's position: R(normalize(q)) (exp(scaling) * z) + xyz of its source row
__device__ __forceinline__ float child_xyz(const ApplyParams& a, const size_t s, const u32 child, const u32 c)
{
    const float r0 = a.rotation[4 * s], r1 = a.rotation[4 * s + 1], r2 = a.rotation[4 * s + 2], r3 = a.rotation[4 * s + 3];
    const float n = sqrtf(r0 * r0 + r1 * r1 + r2 * r2 + r3 * r3);
    const float w = r0 / n, x = r1 / n, y = r2 / n, zq = r3 / n;
    float z[3];
    if (a.noise) { const float* p = a.noise + ((size_t)s * a.N + child) * 3; z[0] = p[0]; z[1] = p[1]; z[2] = p[2]; }
    else normal3(a.seed_lo, a.seed_hi, (u32)s, child, z);
    const float v0 = expf(a.scaling[3 * s]) * z[0], v1 = expf(a.scaling[3 * s + 1]) * z[1], v2 = expf(a.scaling[3 * s + 2]) * z[2];
    float m0, m1, m2;
    if (c == 0)      { m0 = 1.0f - 2.0f * (y * y + zq * zq); m1 = 2.0f * (x * y - w * zq); m2 = 2.0f * (x * zq + w * y); }
    else if (c == 1) { m0 = 2.0f * (x * y + w * zq); m1 = 1.0f - 2.0f * (x * x + zq * zq); m2 = 2.0f * (y * zq - w * x); }
    else             { m0 = 2.0f * (x * zq - w * y); m1 = 2.0f * (y * zq + w * x); m2 = 1.0f - 2.0f * (x * x + y * y); }
    return (m0 * v0 + m1 * v1 + m2 * v2) + a.xyz[3 * s + c];
}

__device__ __forceinline__ float dens_value(const ApplyParams& a, const RowSeg& G, const int2 ent, const u32 c)
{
    if ((u32)ent.x >= (u32)a.P || ent.y >= 2 + a.N) return 0.0f;      // a map the plan did not write (mismatched calls): nothing is read
    const size_t s = (size_t)ent.x;
    const int kind = ent.y;
    if (G.mode == ROWSEG_MOMENT) return kind == 0 ? G.src[s * G.width + c] : 0.0f;
    if (kind >= 2) {
        if (G.mode == SEG_XYZ) return child_xyz(a, s, (u32)(kind - 2), c);
        if (G.mode == SEG_SCALING) return logf(expf(G.src[s * G.width + c]) / a.child_div);
    }
    return G.src[s * G.width + c];
}

__global__ void __launch_bounds__(ROWSEG_BLOCK) densify_apply_kernel(const ApplyParams a)
{
    RowSeg G;                                                            // found here, not in the walker: see row_rebuild.h
    rowseg_find(G, a.seg, blockIdx.x);
    rowseg_walk(G, a.P_new, [&](const size_t row) { return a.prov[row]; }, [&](const int2 ent, const u32 c) { return dens_value(a, G, ent, c); });
}

// ------------------------------------------------------------------------------------------------ reset_opacity
__global__ void __launch_bounds__(DENS_BLOCK) reset_opacity_kernel(float* __restrict__ opacity, float* __restrict__ m, float* __restrict__ v, const int P,
                                                                   const float cap)
{
    const size_t r = (size_t)blockIdx.x * DENS_BLOCK + threadIdx.x;
    if (r >= (size_t)P) return;
    const float o = fminf(1.0f / (1.0f + expf(-opacity[r])), cap);
    opacity[r] = logf(o / (1.0f - o));
    if (m) m[r] = 0.0f;
    if (v) v[r] = 0.0f;
}

// ------------------------------------------------------------------------------------------------ launchers (arguments validated by api.hip)
hipError_t launch_densify_plan(const BagsDensifyRule& r, void* workspace, u32 host_totals[DENS_COUNTS], hipStream_t st)
{
    DensWorkspace w; carve_densify(workspace, r.P, &w);
    DecideParams d;
    d.accum = r.xyz_gradient_accum; d.denom = r.denom; d.radii = r.max_radii2D; d.scaling = r.scaling; d.opacity = r.opacity;
    d.max_grad = r.max_grad; d.min_opacity = r.min_opacity; d.dense_thr = r.dense_threshold; d.world_thr = r.world_threshold;
    d.max_screen = r.max_screen_size; d.child_div = (float)(0.8 * r.N);
    d.use_screen = r.use_screen_size; d.pre_densify = r.screen_size_mode == BAGS_SCREEN_PRE_DENSIFY; d.P = r.P;
    hipLaunchKernelGGL(densify_decide_kernel, dim3((unsigned)w.nb), dim3(DENS_BLOCK), 0, st, d, w.cls, w.sums, w.nb);
    hipLaunchKernelGGL(densify_scan_kernel, dim3(1), dim3(1024), 0, st, w.sums, w.nb, w.totals);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = hipMemcpyAsync(host_totals, w.totals, DENS_COUNTS * sizeof(u32), hipMemcpyDeviceToHost, st);
    if (e != hipSuccess) return e;
    return hipStreamSynchronize(st);
}

hipError_t launch_densify_apply(const BagsDensifyRule& r, const BagsDensifyGroup* groups, int n_groups, void* workspace, long long P_new,
                                float* accum_out, float* denom_out, float* radii_out, int32_t* provenance, hipStream_t st)
{
    DensWorkspace w; carve_densify(workspace, r.P, &w);
    hipLaunchKernelGGL(densify_map_kernel, dim3((unsigned)w.nb), dim3(DENS_BLOCK), 0, st, w.cls, w.sums, w.totals, w.nb, r.P, r.N, P_new,
                       reinterpret_cast<int2*>(provenance));
    ApplyParams a;
    a.xyz = a.scaling = a.rotation = nullptr;
    for (int k = 0; k < n_groups; ++k) {
        if (groups[k].role == BAGS_ROLE_XYZ) a.xyz = groups[k].param;
        if (groups[k].role == BAGS_ROLE_SCALING) a.scaling = groups[k].param;
        if (groups[k].role == BAGS_ROLE_ROTATION) a.rotation = groups[k].param;
    }
    const unsigned blocks = rowseg_table(a.seg, groups, n_groups, P_new,
                                         [](int role) -> u32 { return role == BAGS_ROLE_XYZ ? SEG_XYZ : role == BAGS_ROLE_SCALING ? SEG_SCALING : ROWSEG_COPY; },
                                         accum_out, denom_out, radii_out);
    if (!blocks) return hipErrorInvalidValue;
    a.prov = reinterpret_cast<const int2*>(provenance);
    a.noise = r.noise;
    a.P_new = P_new; a.P = r.P; a.N = r.N;
    a.seed_lo = (u32)r.seed; a.seed_hi = (u32)(r.seed >> 32);
    a.child_div = (float)(0.8 * r.N);
    hipLaunchKernelGGL(densify_apply_kernel, dim3(blocks), dim3(ROWSEG_BLOCK), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_reset_opacity(float* opacity, float* exp_avg, float* exp_avg_sq, int P, float cap, hipStream_t st)
{
    hipLaunchKernelGGL(reset_opacity_kernel, dim3((unsigned)dens_blocks(P)), dim3(DENS_BLOCK), 0, st, opacity, exp_avg, exp_avg_sq, P, cap);
    return hipGetLastError();
}
