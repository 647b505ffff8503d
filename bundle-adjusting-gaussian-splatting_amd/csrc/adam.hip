// adam.hip -- the optimizer step of the Gaussian parameters in one launch (bags_adam_step, include/bags_raster.h).
//
// The reference steps torch.optim.Adam(l, lr=0.0, eps=1e-15) over six parameter groups once per iteration
// (scene/gaussian_model.py:192-210, train.py:420-421): xyz, f_dc, f_rest, opacity, scaling, rotation, 59 floats per Gaussian.
// Here one pass reads param, grad, exp_avg, exp_avg_sq and writes param, exp_avg, exp_avg_sq: 28 bytes per element, each once.
//
// Layout.  Every group is a flat array of n = P * width floats.  A workgroup owns ADAM_CHUNK consecutive elements of ONE group
// (the group table arrives by value in the kernel arguments; first_block is its prefix sum), a thread ADAM_UNROLL float4s that
// are a workgroup's width apart, so that a wave's accesses are 1 KiB contiguous per instruction.  A group whose four base
// pointers are 16-byte aligned goes through float4 accesses with a scalar tail of n % 4 elements in its last workgroup; any
// other group through coalesced scalar accesses.  The densification statistics are one thread per Gaussian in extra
// workgroups at the end of the same grid.
//
// Visible-only mode (adam_kernel<true>) keeps that element-to-thread map: a thread finds the rows its four elements belong to
// (one 32-bit division by the group's width; the 64-bit one of the chunk's first element is wave-uniform), loads their flags,
// does nothing when none is set, stores float4s when all are, and single floats when only some are.  A row's update does
// not depend on which instance computes it: this file is built with -ffp-contract=off and no fast-math flag, so adam_element
// is exactly the seven IEEE operations it spells (two of them explicit fmaf), correctly rounded division and square root
// included, in both instances.  The dense instance never divides and never reads a flag.
#include "bags_common.h"

#define ADAM_BLOCK 256
#ifndef ADAM_UNROLL
#define ADAM_UNROLL 4
#endif
#define ADAM_CHUNK (ADAM_BLOCK * ADAM_UNROLL * 4)          // elements per workgroup

struct AdamGroupDev {
    float* p; const float* g; float* m; float* v;
    size_t n;                      // P * width
    u32 first_block;               // of this group in the grid; 0xFFFFFFFF for an unused slot
    u32 width;
    float neg_step, bc2;
    u32 vec;                       // all four pointers 16-byte aligned
    u32 pad;
};
struct AdamParams {
    AdamGroupDev grp[BAGS_ADAM_MAX_GROUPS];
    float w1, b2, w2, eps;         // 1 - beta1, beta2, 1 - beta2, eps
    const int32_t* visible;
    BagsDensifyStats stats;
    u32 stats_first_block;         // 0xFFFFFFFF: no statistics
    int P;
};

struct AdamConst { float w1, b2, w2, eps, neg_step, bc2; };

// torch.optim.Adam's single update, in the operation order of its GPU kernels (lerp_, mul_ + addcmul_, sqrt / div / add, addcdiv_)
__device__ __forceinline__ void adam_element(float& p, const float g, float& m, float& v, const AdamConst& c)
{
    m = fmaf(c.w1, g - m, m);
    v = fmaf(c.w2, g * g, v * c.b2);
    const float d = sqrtf(v) / c.bc2 + c.eps;
    p = fmaf(c.neg_step, m / d, p);
}

__device__ __forceinline__ void adam_scalar(const AdamGroupDev& G, const size_t e, const AdamConst& c)
{
    float p = G.p[e], m = G.m[e], v = G.v[e];
    adam_element(p, G.g[e], m, v, c);
    G.p[e] = p; G.m[e] = m; G.v[e] = v;
}

__device__ __forceinline__ void adam_vec4(float4& p, const float4& g, float4& m, float4& v, const AdamConst& c)
{
    adam_element(p.x, g.x, m.x, v.x, c); adam_element(p.y, g.y, m.y, v.y, c);
    adam_element(p.z, g.z, m.z, v.z, c); adam_element(p.w, g.w, m.w, v.w, c);
}

// FULL: every float4 of the chunk exists (all workgroups of a group but its last)
template <bool FULL>
__device__ __forceinline__ void adam_chunk_dense(const AdamGroupDev& G, const size_t i0, const size_t n4, const AdamConst& c)
{
    float4 p[ADAM_UNROLL], g[ADAM_UNROLL], m[ADAM_UNROLL], v[ADAM_UNROLL];
#pragma unroll
    for (int j = 0; j < ADAM_UNROLL; ++j) {
        const size_t i = i0 + (size_t)j * ADAM_BLOCK;
        if (FULL || i < n4) {
            p[j] = reinterpret_cast<const float4*>(G.p)[i]; g[j] = reinterpret_cast<const float4*>(G.g)[i];
            m[j] = reinterpret_cast<const float4*>(G.m)[i]; v[j] = reinterpret_cast<const float4*>(G.v)[i];
        }
    }
#pragma unroll
    for (int j = 0; j < ADAM_UNROLL; ++j) {
        const size_t i = i0 + (size_t)j * ADAM_BLOCK;
        if (FULL || i < n4) {
            adam_vec4(p[j], g[j], m[j], v[j], c);
            reinterpret_cast<float4*>(G.p)[i] = p[j]; reinterpret_cast<float4*>(G.m)[i] = m[j];
            reinterpret_cast<float4*>(G.v)[i] = v[j];
        }
    }
}

__device__ __forceinline__ void stats_rows(const BagsDensifyStats& s, const int P, const u32 block)
{
    const size_t r = (size_t)block * ADAM_BLOCK + threadIdx.x;
    if (r >= (size_t)P) return;
    const int rad = s.radii[r];
    if (rad <= 0) return;
    const float gx = s.grad_means2D[r * (size_t)s.grad_stride], gy = s.grad_means2D[r * (size_t)s.grad_stride + 1];
    s.xyz_gradient_accum[r] += sqrtf(fmaf(gx, gx, gy * gy));
    s.denom[r] += 1.0f;
    s.max_radii2D[r] = fmaxf(s.max_radii2D[r], (float)rad);
}

template <bool MASKED>
__global__ void __launch_bounds__(ADAM_BLOCK) adam_kernel(const AdamParams a)
{
    const u32 b = blockIdx.x;
    if (b >= a.stats_first_block) { stats_rows(a.stats, a.P, b - a.stats_first_block); return; }
    // the group this workgroup belongs to: wave-uniform selects over the by-value table (unused slots start at 0xFFFFFFFF)
    AdamGroupDev G = a.grp[0];
#pragma unroll
    for (int k = 1; k < BAGS_ADAM_MAX_GROUPS; ++k)
        if (b >= a.grp[k].first_block) G = a.grp[k];
    const AdamConst c{a.w1, a.b2, a.w2, a.eps, G.neg_step, G.bc2};
    const size_t e0 = (size_t)(b - G.first_block) * ADAM_CHUNK;          // first element of the chunk, < n
    const size_t n4 = G.vec ? (G.n >> 2) : 0;
    const bool last = e0 + ADAM_CHUNK >= G.n;

    if (!MASKED) {
        if (G.vec) {
            const size_t i0 = (e0 >> 2) + threadIdx.x;
            if (e0 + ADAM_CHUNK <= (n4 << 2)) adam_chunk_dense<true>(G, i0, n4, c);
            else adam_chunk_dense<false>(G, i0, n4, c);
            if (last) {
                const size_t t = (n4 << 2) + threadIdx.x;
                if (t < G.n) adam_scalar(G, t, c);
            }
        } else {
#pragma unroll 4
            for (int j = 0; j < ADAM_UNROLL * 4; ++j) {
                const size_t e = e0 + (size_t)j * ADAM_BLOCK + threadIdx.x;
                if (e < G.n) adam_scalar(G, e, c);
            }
        }
        return;
    }

    // ---- visible-only
    const int32_t* __restrict__ vis = a.visible;
    const u32 w = G.width;
    const size_t row_base = e0 / w;                                      // wave-uniform
    const u32 rem_base = (u32)(e0 - row_base * w);                       // < w
    const u64 w2 = 2ull * w, w3 = 3ull * w;
    if (G.vec) {
#pragma unroll
        for (int j = 0; j < ADAM_UNROLL; ++j) {
            const u32 li = (u32)j * ADAM_BLOCK + threadIdx.x;            // float4 within the chunk
            const size_t i = (e0 >> 2) + li;
            if (i >= n4) continue;
            const u32 t = rem_base + 4u * li;                            // < w + ADAM_CHUNK
            const u32 q = t / w, r = t - q * w;
            const size_t r0 = row_base + q;
            // element k of the float4 sits r + k floats into row r0, r < w: at most rows r0 .. r0 + 3 (w = 1)
            const size_t r1 = r0 + (r + 1 >= w);
            const size_t r2 = r0 + (r + 2 >= w) + (r + 2 >= w2);
            const size_t r3 = r0 + (r + 3 >= w) + (r + 3 >= w2) + (r + 3 >= w3);
            const bool u0 = vis[r0] > 0;
            const bool u3 = (r3 == r0) ? u0 : vis[r3] > 0;
            const bool u1 = (r1 == r0) ? u0 : (r1 == r3) ? u3 : vis[r1] > 0;
            const bool u2 = (r2 == r1) ? u1 : (r2 == r3) ? u3 : vis[r2] > 0;
            if (!(u0 || u1 || u2 || u3)) continue;
            float4 p = reinterpret_cast<const float4*>(G.p)[i], m = reinterpret_cast<const float4*>(G.m)[i];
            float4 v = reinterpret_cast<const float4*>(G.v)[i];
            const float4 g = reinterpret_cast<const float4*>(G.g)[i];
            adam_vec4(p, g, m, v, c);
            if (u0 && u1 && u2 && u3) {
                reinterpret_cast<float4*>(G.p)[i] = p; reinterpret_cast<float4*>(G.m)[i] = m; reinterpret_cast<float4*>(G.v)[i] = v;
            } else {
                const size_t e = i << 2;
                if (u0) { G.p[e] = p.x; G.m[e] = m.x; G.v[e] = v.x; }
                if (u1) { G.p[e + 1] = p.y; G.m[e + 1] = m.y; G.v[e + 1] = v.y; }
                if (u2) { G.p[e + 2] = p.z; G.m[e + 2] = m.z; G.v[e + 2] = v.z; }
                if (u3) { G.p[e + 3] = p.w; G.m[e + 3] = m.w; G.v[e + 3] = v.w; }
            }
        }
        if (last) {
            const size_t t = (n4 << 2) + threadIdx.x;
            if (t < G.n && vis[t / w] > 0) adam_scalar(G, t, c);
        }
    } else {
#pragma unroll 4
        for (int j = 0; j < ADAM_UNROLL * 4; ++j) {
            const u32 le = (u32)j * ADAM_BLOCK + threadIdx.x;
            const size_t e = e0 + le;
            if (e < G.n && vis[row_base + (rem_base + le) / w] > 0) adam_scalar(G, e, c);
        }
    }
}

static inline bool aligned16(const void* p) { return (reinterpret_cast<size_t>(p) & 15u) == 0; }

// args and stats are validated by the caller (api.hip); stats == nullptr or all-NULL: no statistics
hipError_t launch_adam(const BagsAdamArgs& args, const BagsDensifyStats* stats, hipStream_t st)
{
    AdamParams a;
    size_t blocks = 0;
    for (int k = 0; k < BAGS_ADAM_MAX_GROUPS; ++k) {
        AdamGroupDev& G = a.grp[k];
        G = AdamGroupDev{nullptr, nullptr, nullptr, nullptr, 0, 0xFFFFFFFFu, 1, 0.0f, 1.0f, 0, 0};
        if (k >= args.n_groups || !args.groups[k].grad) continue;
        const BagsAdamGroup& s = args.groups[k];
        G.p = s.param; G.g = s.grad; G.m = s.exp_avg; G.v = s.exp_avg_sq;
        G.n = (size_t)args.P * (size_t)s.width;
        G.width = (u32)s.width;
        G.neg_step = -s.step_size; G.bc2 = s.bias_correction2_sqrt;
        G.vec = aligned16(G.p) && aligned16(G.g) && aligned16(G.m) && aligned16(G.v);
        G.first_block = (u32)blocks;
        blocks += (G.n + ADAM_CHUNK - 1) / ADAM_CHUNK;
        if (blocks >= 0x7FFFFFFFull) return hipErrorInvalidValue;
    }
    a.w1 = (float)(1.0 - args.beta1); a.b2 = (float)args.beta2; a.w2 = (float)(1.0 - args.beta2); a.eps = (float)args.eps;
    a.visible = args.visible;
    a.P = args.P;
    a.stats_first_block = 0xFFFFFFFFu;
    a.stats = BagsDensifyStats{};
    if (stats && stats->radii) {
        a.stats = *stats;
        a.stats_first_block = (u32)blocks;
        blocks += ((size_t)args.P + ADAM_BLOCK - 1) / ADAM_BLOCK;
        if (blocks >= 0x7FFFFFFFull) return hipErrorInvalidValue;
    }
    if (blocks == 0) return hipSuccess;
    if (args.visible) hipLaunchKernelGGL(adam_kernel<true>, dim3((unsigned)blocks), dim3(ADAM_BLOCK), 0, st, a);
    else hipLaunchKernelGGL(adam_kernel<false>, dim3((unsigned)blocks), dim3(ADAM_BLOCK), 0, st, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- the camera bank's Adam (bags_pose_adam_step)
// One thread per (listed row, column) of the (N,9) pose tables, 16 x 9 at most: one workgroup.  Camera rows[v] has three groups
// (columns 0..3, 4..6, 7..8), each with its own step count, so the constants of adam_element arrive per (row, group) by value.
// A thread whose group is not enabled returns before it reads anything; rows that are not listed have no thread.
#define POSE_ADAM_BLOCK 192
struct PoseAdamDev {
    float* p; const float* g; float* m; float* v;
    float w1, b2, w2, eps;
    int n_rows;
    int rows[BAGS_MAX_POSE_ROWS];
    BagsPoseAdamGroup grp[BAGS_MAX_POSE_ROWS][3];
};

__global__ void __launch_bounds__(POSE_ADAM_BLOCK) pose_adam_kernel(const PoseAdamDev a)
{
    const int t = threadIdx.x;
    if (blockIdx.x != 0 || t >= a.n_rows * 9) return;
    const int v = t / 9, c = t - 9 * v, grp = c < 4 ? 0 : (c < 7 ? 1 : 2);
    // selects over the by-value tables (v is not uniform over a wave)
    int r = a.rows[0];
    BagsPoseAdamGroup G{0, 0.f, 1.f};
#pragma unroll
    for (int k = 0; k < BAGS_MAX_POSE_ROWS; ++k) {
        if (v == k) {
            r = a.rows[k];
            G = grp == 0 ? a.grp[k][0] : (grp == 1 ? a.grp[k][1] : a.grp[k][2]);
        }
    }
    if (!G.enabled) return;
    const AdamConst k{a.w1, a.b2, a.w2, a.eps, -G.step_size, G.bias_correction2_sqrt};
    const size_t e = (size_t)r * 9 + c;
    float p = a.p[e], m = a.m[e], s = a.v[e];
    adam_element(p, a.g[e], m, s, k);
    a.p[e] = p; a.m[e] = m; a.v[e] = s;
}

// validated by the caller (api.hip)
hipError_t launch_pose_adam(const BagsPoseAdamArgs& args, hipStream_t st)
{
    PoseAdamDev a;
    a.p = args.leaves; a.g = args.grad; a.m = args.exp_avg; a.v = args.exp_avg_sq;
    a.w1 = (float)(1.0 - args.beta1); a.b2 = (float)args.beta2; a.w2 = (float)(1.0 - args.beta2); a.eps = (float)args.eps;
    a.n_rows = args.n_rows;
    for (int k = 0; k < BAGS_MAX_POSE_ROWS; ++k) {
        a.rows[k] = k < args.n_rows ? args.rows[k] : 0;
        for (int g = 0; g < 3; ++g) a.grp[k][g] = k < args.n_rows ? args.groups[k][g] : BagsPoseAdamGroup{0, 0.f, 1.f};
    }
    hipLaunchKernelGGL(pose_adam_kernel, dim3(1), dim3(POSE_ADAM_BLOCK), 0, st, a);
    return hipGetLastError();
}
