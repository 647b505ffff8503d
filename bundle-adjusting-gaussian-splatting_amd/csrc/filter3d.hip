// filter3d.hip -- Mip-Splatting's 3D smoothing filter (compute_3D_filter of its GaussianModel): per Gaussian the size of the low-pass
// kernel that the highest sampling rate of any training camera allows,
//     f = (dist / focal) * sqrt(variance),   dist = the smallest view-space depth over the cameras that see the Gaussian,
// with `focal` the largest focal length in pixels of the camera table and, for a Gaussian no camera sees, dist = the largest dist
// of the others.  Upstream loops over the cameras in Python, ~20 elementwise kernels on (P, ...) tensors per camera; here xyz is
// read once and every lane walks the camera table, whose rows come in through wave-uniform indices (scalar loads).
//
// Two launches, no atomics, nothing allocated, no host synchronisation:
//   1  one lane per Gaussian: dist into the workspace (F3_NONE where no camera is valid), and the workgroup's maximum of the valid
//      dists -- wave reduce, LDS across the four waves -- as one partial per workgroup;
//   2  every workgroup reduces the partials (ceil(P / 256) floats, L2-resident) to dmax and the camera table to focal, then writes
//      its rows of `out`.
// min and max are exact, so the result repeats bit for bit and does not depend on the workgroup count or on the order of rows or
// cameras.  The view-space point is projection.h's pj_view and the focal length is formed as pj_cov2d forms it; the file is compiled
// with -ffp-contract=off, because the five validity tests are discontinuous in fp32: each expression below is the sequence of
// individually rounded operations that bags_raster/filter3d.py states.
//
// The filtered activations (scales' = sqrt(s^2 + f^2), opacity' = sigmoid * sqrt(prod s^2 / prod (s^2 + f^2))) are an instance of
// the activation kernels: activations.hip.
#include "bags_common.h"
#include "projection.h"

#define F3_BLOCK 256
#define F3_NONE (-1.0f)          // "no camera valid" in the workspace: a valid dist is above 0.2, so max() skips the sentinel by itself
#define F3_FAR 100000.0f         // upstream's initial distance; the dmax of a set no camera sees

// maximum over the workgroup, valid in every thread; `slots` is F3_BLOCK / 64 floats of LDS (not reused before the next barrier)
__device__ __forceinline__ float f3_block_max(float x, float* slots)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x = fmaxf(x, __shfl_xor(x, d));
    if ((threadIdx.x & 63) == 0) slots[threadIdx.x >> 6] = x;
    __syncthreads();
    return fmaxf(fmaxf(slots[0], slots[1]), fmaxf(slots[2], slots[3]));
}

__global__ void __launch_bounds__(F3_BLOCK)
filter3d_dist_kernel(int P, int N, const float* __restrict__ xyz, const float* __restrict__ viewmatrices,
                     const float* __restrict__ intrinsics, const int32_t* __restrict__ sizes, float* __restrict__ dist,
                     float* __restrict__ partials)
{
    __shared__ float slots[F3_BLOCK / 64];
    const size_t i = (size_t)blockIdx.x * F3_BLOCK + threadIdx.x;
    const bool row = i < (size_t)P;
    const size_t ic = row ? i : (size_t)P - 1;                 // every lane runs the loop (P > 0 here): the wave reduce is complete
    const float x = xyz[3 * ic], y = xyz[3 * ic + 1], z = xyz[3 * ic + 2];
    float best = F3_FAR;
    bool any = false;
    for (int c = 0; c < N; ++c) {                              // c is uniform: the camera's rows are scalar loads
        const float* v = viewmatrices + 16 * (size_t)c;
        const float k0 = intrinsics[16 * (size_t)c], k5 = intrinsics[16 * (size_t)c + 5];
        const float W = (float)sizes[2 * (size_t)c], H = (float)sizes[2 * (size_t)c + 1];
        const PjView t = pj_view(v, x, y, z);
        const float hw = 0.5f * W, hh = 0.5f * H;
        const float fx = k0 * hw, fy = k5 * hh;
        const float px = t.tx / t.tz * fx + hw;
        const float py = t.ty / t.tz * fy + hh;
        const bool valid = (t.tz > 0.2f) && (px >= -0.15f * W) && (px <= 1.15f * W) && (py >= -0.15f * H) && (py <= 1.15f * H);
        if (valid) { best = fminf(best, t.tz); any = true; }
    }
    const float d = (row && any) ? best : F3_NONE;
    if (row) dist[i] = d;
    const float m = f3_block_max(d, slots);
    if (threadIdx.x == 0) partials[blockIdx.x] = m;
}

__global__ void __launch_bounds__(F3_BLOCK)
filter3d_apply_kernel(int P, int N, int nblocks, const float* __restrict__ intrinsics, const int32_t* __restrict__ sizes,
                      const float* __restrict__ dist, const float* __restrict__ partials, float sqrt_variance, float* __restrict__ out)
{
    __shared__ float slots_d[F3_BLOCK / 64], slots_f[F3_BLOCK / 64];
    float m = F3_NONE;
    for (int b = threadIdx.x; b < nblocks; b += F3_BLOCK) m = fmaxf(m, partials[b]);
    float focal = -INFINITY;
    for (int c = threadIdx.x; c < N; c += F3_BLOCK) focal = fmaxf(focal, intrinsics[16 * (size_t)c] * (0.5f * (float)sizes[2 * (size_t)c]));
    m = f3_block_max(m, slots_d);
    focal = f3_block_max(focal, slots_f);
    const float dmax = (m > 0.0f) ? m : F3_FAR;                // no row of the set has a valid camera
    const size_t i = (size_t)blockIdx.x * F3_BLOCK + threadIdx.x;
    if (i < (size_t)P) {
        const float d = dist[i];
        out[i] = ((d > 0.0f ? d : dmax) / focal) * sqrt_variance;
    }
}

int filter3d_blocks(int P) { return cdiv(P > 0 ? P : 1, F3_BLOCK); }

// dist: P floats, partials: filter3d_blocks(P) floats (carve_filter3d in api.hip)
hipError_t launch_filter3d(const float* xyz, int P, const float* viewmatrices, const float* intrinsics, const int32_t* sizes, int N,
                           float variance, float* dist, float* partials, float* out, hipStream_t st)
{
    if (P <= 0) return hipSuccess;
    const int nblocks = cdiv(P, F3_BLOCK);
    hipLaunchKernelGGL(filter3d_dist_kernel, dim3(nblocks), dim3(F3_BLOCK), 0, st, P, N, xyz, viewmatrices, intrinsics, sizes, dist, partials);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(filter3d_apply_kernel, dim3(nblocks), dim3(F3_BLOCK), 0, st, P, N, nblocks, intrinsics, sizes, dist, partials,
                       sqrtf(variance), out);
    return hipGetLastError();
}
