// lens_field.hip -- the lens network of the distortion route (bags_lens_field_*, include/bags_raster.h): an invertible ResNet on
// M points of R^2, B residual blocks x <- x + g_b(x), g_b = Linear(2,H), ELU, n x (Linear(H,H), ELU), Linear(H,2).
//
// In PyTorch that is about six launches per block forward and twice as many backward, every iteration, on a few thousand to a
// few tens of thousands of points: launch-bound.  Here the forward is one launch, the backward two.
//
// Layout of the work.  A tile is LF_TILE = 64 points, and a lane is a point: every per-point operation is the same instruction
// sequence whatever the point's position in the call, so a row of the output does not depend on the rows around it (no build
// flag is needed for that).  A workgroup is 8 waves; wave w owns rows [8w, 8w + 8) of every hidden vector.  The weights of ONE
// block are staged in LDS, (out, in) row-major as they arrive, rows and columns zero-padded to HP = H rounded up to 8, so that
// no loop has a tail: a padded unit has weight 0 and bias 0, its activation is ELU(0) = 0 and its cotangent 0 * 1.  Hidden
// vectors live in LDS as [unit][point] with a pitch of LF_PS = 68 floats: a wave reading one unit for its 64 points touches 64
// consecutive banks, and a wave whose lanes are UNITS (the weight-gradient products) reads float4s 68 floats apart, which the
// four 16-lane groups of ds_read_b128 serve without a conflict.  A weight row is read as float4s that every lane shares
// (broadcast).
//
// Forward / inverse: one tile per workgroup, the block loop inside; two activation buffers alternate.
// Backward: min(tiles, LF_MAX_GROUPS) workgroups, each walking its tiles INSIDE the block loop, so a block is staged once per
// sweep and its parameter-gradient sums stay in registers across the tiles.  A first sweep recomputes the block inputs
// x_1 .. x_{B-1} into the workspace (8 bytes per point and block boundary, written and read back by the same thread); the
// reverse sweep recomputes a block's activations h_0 .. h_n into n + 1 LDS buffers and walks back through them, turning h_i
// into dL/da_i IN PLACE (ELU'(a) is 1 for h > 0 and h + 1 otherwise, h = expm1(a)), and overwrites the slot of x_b with
// dL/dx_b for the block below.  Each workgroup writes its sums as one row of partials; lens_field_reduce_kernel adds the rows in
// workgroup order.  No atomics, and the number of workgroups depends on M alone: the bits do not depend on the device or stream.
#include "bags_common.h"

#define LF_BLOCK 512
#define LF_WAVES (LF_BLOCK / BAGS_WAVE)
#define LF_TILE 64
#define LF_PS 68
#define LF_ROWS 8                              // rows of a hidden vector per wave: LF_WAVES * LF_ROWS = BAGS_LENS_MAX_HIDDEN
#define LF_MAX_GROUPS 256
#define LF_REDUCE_BLOCK 256
#define LF_STAGE_TRIPS ((BAGS_LENS_MAX_HIDDEN * BAGS_LENS_MAX_HIDDEN + BAGS_LENS_MAX_HIDDEN + LF_BLOCK - 1) / LF_BLOCK)   // of a thread staging W_i, b_i
static_assert(LF_WAVES * LF_ROWS == BAGS_LENS_MAX_HIDDEN, "a workgroup's waves cover the widest hidden vector");
static_assert(BAGS_LENS_MAX_INTERNAL_LAYERS == 4, "the backward unrolls its layer loop and names four accumulator sets");

struct LfNet { int B, H, n, HP; const float* params; };

static inline int lf_pad(int H) { return (H + 7) / 8 * 8; }
// a block in LDS: W_0 [HP][2] | b_0 [HP] | n x (W_i [HP][HP] | b_i [HP]) | W_out [2][HP] | b_out [4]
__host__ __device__ static inline int lf_lds_hidden(int HP, int i) { return 3 * HP + (i - 1) * (HP * HP + HP); }   // W_i, i = 1..n (n + 1: W_out)
__host__ __device__ static inline int lf_lds_floats(int HP, int n) { return lf_lds_hidden(HP, n + 1) + 2 * HP + 4; }

__device__ __forceinline__ float lf_elu(const float a) { return a > 0.0f ? a : expm1f(a); }
__device__ __forceinline__ float lf_elu_slope(const float h) { return h > 0.0f ? 1.0f : h + 1.0f; }     // from h = ELU(a)

// 64-point sums over two LDS rows (16-byte aligned), p ascending, continuing `acc`
__device__ __forceinline__ float lf_dot(const float* a, const float* b, float acc)
{
#pragma unroll 4
    for (int p = 0; p < LF_TILE; p += 4) {
        const float4 u = *reinterpret_cast<const float4*>(a + p), v = *reinterpret_cast<const float4*>(b + p);
        acc = fmaf(u.x, v.x, acc); acc = fmaf(u.y, v.y, acc); acc = fmaf(u.z, v.z, acc); acc = fmaf(u.w, v.w, acc);
    }
    return acc;
}
__device__ __forceinline__ float lf_sum(const float* a, float acc)
{
#pragma unroll 4
    for (int p = 0; p < LF_TILE; p += 4) {
        const float4 u = *reinterpret_cast<const float4*>(a + p);
        acc += u.x; acc += u.y; acc += u.z; acc += u.w;
    }
    return acc;
}

// One block's parameters from the flat vector into LDS, zero-padded.  The caller synchronises before (nobody still reads the
// block staged before) and after.
__device__ void lf_stage(float* sw, const float* __restrict__ gp, const int H, const int HP, const int n)
{
    const int t = threadIdx.x;
    for (int e = t; e < 3 * HP; e += LF_BLOCK) {
        float v = 0.0f;
        if (e < 2 * HP) { if ((e >> 1) < H) v = gp[e]; }
        else if (e - 2 * HP < H) v = gp[2 * H + (e - 2 * HP)];
        sw[e] = v;
    }
    for (int i = 1; i <= n; ++i) {
        const float* g = gp + 3 * H + (i - 1) * (H * H + H);
        float* s = sw + lf_lds_hidden(HP, i);
        // every load of the thread in flight at once: unconditional, at a clamped index, dropped afterwards (a load behind a
        // branch is waited for before the next is issued, and a block is staged 2B - 1 times in the backward)
        float v[LF_STAGE_TRIPS];
#pragma unroll
        for (int u = 0; u < LF_STAGE_TRIPS; ++u) {
            const int e = t + u * LF_BLOCK;
            const int j = e / HP, k = e - j * HP, r = e - HP * HP;
            const bool weight = e < HP * HP && j < H && k < H, bias = r >= 0 && r < H;
            v[u] = g[weight ? j * H + k : bias ? H * H + r : 0];
            if (!weight && !bias) v[u] = 0.0f;
        }
#pragma unroll
        for (int u = 0; u < LF_STAGE_TRIPS; ++u)
            if (t + u * LF_BLOCK < HP * HP + HP) s[t + u * LF_BLOCK] = v[u];
    }
    const float* g = gp + 3 * H + n * (H * H + H);
    float* s = sw + lf_lds_hidden(HP, n + 1);
    for (int e = t; e < 2 * HP + 4; e += LF_BLOCK) {
        float v = 0.0f;
        if (e < 2 * HP) { const int c = e >= HP ? 1 : 0, k = e - c * HP; if (k < H) v = g[c * H + k]; }
        else if (e - 2 * HP < 2) v = g[2 * H + (e - 2 * HP)];
        s[e] = v;
    }
}

// g_b of the staged block for the tile's 64 points.  xs: the block's input, [2][LF_PS].  KEEP: activation h_i goes to buffer i of
// `act` (the backward reads them all); otherwise two buffers alternate.  OUT: the last layer is evaluated into gs [2][LF_PS].
// Ends with a barrier; the caller has synchronised since xs was written.
template <bool KEEP, bool OUT>
__device__ __forceinline__ void lf_block_g(const float* sw, const float* xs, float* act, float* gs, const int HP, const int n)
{
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63, j0 = w * LF_ROWS;
    const bool on = j0 < HP;
    const int AS = HP * LF_PS;
    if (on) {
        const float x0 = xs[l], x1 = xs[LF_PS + l];
#pragma unroll
        for (int q = 0; q < LF_ROWS; ++q) {
            const int j = j0 + q;
            act[j * LF_PS + l] = lf_elu(fmaf(sw[2 * j + 1], x1, fmaf(sw[2 * j], x0, sw[2 * HP + j])));
        }
    }
    __syncthreads();
    for (int i = 1; i <= n; ++i) {
        const float* in = act + (KEEP ? i - 1 : (i - 1) & 1) * AS;
        float* out = act + (KEEP ? i : i & 1) * AS;
        if (on) {
            const float* W = sw + lf_lds_hidden(HP, i);
            const float* b = W + HP * HP;
            float acc[LF_ROWS];
#pragma unroll
            for (int q = 0; q < LF_ROWS; ++q) acc[q] = b[j0 + q];
            for (int k = 0; k < HP; k += 4) {
                const float h0 = in[k * LF_PS + l], h1 = in[(k + 1) * LF_PS + l], h2 = in[(k + 2) * LF_PS + l], h3 = in[(k + 3) * LF_PS + l];
#pragma unroll
                for (int q = 0; q < LF_ROWS; ++q) {
                    const float4 wv = *reinterpret_cast<const float4*>(W + (j0 + q) * HP + k);
                    acc[q] = fmaf(wv.x, h0, acc[q]); acc[q] = fmaf(wv.y, h1, acc[q]);
                    acc[q] = fmaf(wv.z, h2, acc[q]); acc[q] = fmaf(wv.w, h3, acc[q]);
                }
            }
#pragma unroll
            for (int q = 0; q < LF_ROWS; ++q) out[(j0 + q) * LF_PS + l] = lf_elu(acc[q]);
        }
        __syncthreads();
    }
    if (OUT) {
        if (w < 2) {
            const float* in = act + (KEEP ? n : n & 1) * AS;
            const float* Wo = sw + lf_lds_hidden(HP, n + 1) + w * HP;
            float acc = sw[lf_lds_hidden(HP, n + 1) + 2 * HP + w];
            for (int k = 0; k < HP; k += 4) {
                const float4 wv = *reinterpret_cast<const float4*>(Wo + k);
                acc = fmaf(wv.x, in[k * LF_PS + l], acc); acc = fmaf(wv.y, in[(k + 1) * LF_PS + l], acc);
                acc = fmaf(wv.z, in[(k + 2) * LF_PS + l], acc); acc = fmaf(wv.w, in[(k + 3) * LF_PS + l], acc);
            }
            gs[w * LF_PS + l] = acc;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------- forward, inverse
// One tile per workgroup.  Thread (c, l), c = t / 64 < 2, keeps coordinate c of point l in a register and in xs.
template <bool INVERSE>
__global__ void __launch_bounds__(LF_BLOCK) lens_field_fwd_kernel(const LfNet net, const float* src, const long long M, float* dst,
                                                                  const int iterations)
{
    extern __shared__ float4 lf_lds4[];
    float* sw = reinterpret_cast<float*>(lf_lds4);
    float* act = sw + lf_lds_floats(net.HP, net.n);
    float* xs = act + 2 * net.HP * LF_PS;
    float* gs = xs + 2 * LF_PS;
    const int t = threadIdx.x, c = t >> 6, l = t & 63;
    const long long p = (long long)blockIdx.x * LF_TILE + l;
    const bool mine = t < 2 * LF_TILE, valid = mine && p < M;
    const int BF = lens_block_floats(net.H, net.n);
    float v = valid ? src[p * 2 + c] : 0.0f;
    if (mine) xs[c * LF_PS + l] = v;
    for (int s = 0; s < net.B; ++s) {
        const int b = INVERSE ? net.B - 1 - s : s;
        lf_stage(sw, net.params + (size_t)b * BF, net.H, net.HP, net.n);
        __syncthreads();
        if (!INVERSE) {
            lf_block_g<false, true>(sw, xs, act, gs, net.HP, net.n);
            if (mine) { v += gs[c * LF_PS + l]; xs[c * LF_PS + l] = v; }
            __syncthreads();
        } else {
            const float y = v;                               // x <- y - g_b(x), from x = y (xs holds it)
            for (int it = 0; it < iterations; ++it) {
                lf_block_g<false, true>(sw, xs, act, gs, net.HP, net.n);
                if (mine) { v = y - gs[c * LF_PS + l]; xs[c * LF_PS + l] = v; }
                __syncthreads();
            }
        }
    }
    if (valid) dst[p * 2 + c] = v;
}

// ---------------------------------------------------------------------------------------------- backward
// rows j0 .. j0 + 7 of dL/dW += D h^T over the tile's points for column k = lane: D [HP][LF_PS] cotangents, hrow = h[k]
__device__ __forceinline__ void lf_wgrad(float (&acc)[LF_ROWS], const float* D, const float* hrow, const int j0)
{
    for (int p = 0; p < LF_TILE; p += 4) {
        const float4 h4 = *reinterpret_cast<const float4*>(hrow + p);
#pragma unroll
        for (int q = 0; q < LF_ROWS; ++q) {
            const float4 d4 = *reinterpret_cast<const float4*>(D + (j0 + q) * LF_PS + p);
            acc[q] = fmaf(d4.x, h4.x, acc[q]); acc[q] = fmaf(d4.y, h4.y, acc[q]);
            acc[q] = fmaf(d4.z, h4.z, acc[q]); acc[q] = fmaf(d4.w, h4.w, acc[q]);
        }
    }
}

// slots: x_s, later dL/dx_s, for s = 1 .. B-1 at slots + (s - 1) * 2M.  part: one row of B * BF sums per workgroup (want_params).
__global__ void __launch_bounds__(LF_BLOCK) lens_field_bwd_kernel(const LfNet net, const float* __restrict__ x, const long long M,
                                                                  const float* __restrict__ grad_y, float* slots, float* __restrict__ part,
                                                                  float* __restrict__ grad_x, const int want_params)
{
    extern __shared__ float4 lf_lds4[];
    const int H = net.H, HP = net.HP, n = net.n, B = net.B;
    const int AS = HP * LF_PS;
    float* sw = reinterpret_cast<float*>(lf_lds4);
    float* act = sw + lf_lds_floats(HP, n);
    float* xs = act + (n + 1) * AS;
    float* ds = xs + 2 * LF_PS;
    float* gs = ds + 2 * LF_PS;
    const int t = threadIdx.x, w = t >> 6, c = w, l = t & 63, j0 = w * LF_ROWS;
    const bool on = j0 < HP, mine = t < 2 * LF_TILE;
    const long long tiles = (M + LF_TILE - 1) / LF_TILE;
    const int BF = lens_block_floats(H, n);
    const size_t slot = (size_t)M * 2;

    // x_1 .. x_{B-1}
    for (int b = 0; b + 1 < B; ++b) {
        __syncthreads();
        lf_stage(sw, net.params + (size_t)b * BF, H, HP, n);
        __syncthreads();
        const float* in = b == 0 ? x : slots + (size_t)(b - 1) * slot;
        float* out = slots + (size_t)b * slot;
        for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
            const long long p = tile * LF_TILE + l;
            const bool valid = mine && p < M;
            const float v = valid ? in[p * 2 + c] : 0.0f;
            if (mine) xs[c * LF_PS + l] = v;
            __syncthreads();
            lf_block_g<false, true>(sw, xs, act, gs, HP, n);
            if (valid) out[p * 2 + c] = v + gs[c * LF_PS + l];
        }
    }

    for (int b = B - 1; b >= 0; --b) {
        __syncthreads();
        lf_stage(sw, net.params + (size_t)b * BF, H, HP, n);
        __syncthreads();
        const float* in = b == 0 ? x : slots + (size_t)(b - 1) * slot;
        const float* cot = b == B - 1 ? grad_y : slots + (size_t)b * slot;
        float* gin = b == 0 ? grad_x : slots + (size_t)(b - 1) * slot;          // NULL: block 0 without grad_x
        const float* Wo = sw + lf_lds_hidden(HP, n + 1);
        float aW1[LF_ROWS], aW2[LF_ROWS], aW3[LF_ROWS], aW4[LF_ROWS];
#pragma unroll
        for (int q = 0; q < LF_ROWS; ++q) aW1[q] = aW2[q] = aW3[q] = aW4[q] = 0.0f;
        float ab1 = 0.0f, ab2 = 0.0f, ab3 = 0.0f, ab4 = 0.0f;      // b_i: lanes 0..7 of a wave, row j0 + lane
        float a0 = 0.0f;                                           // lanes 0..15: W_0[j0 + lane / 2][lane % 2]; lanes 16..23: b_0[j0 + lane - 16]
        float ao = 0.0f;                                           // waves 0, 1: W_out[w][lane]; wave 2, lanes 0, 1: b_out[lane]

        for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
            const long long p = tile * LF_TILE + l;
            const bool valid = mine && p < M;
            if (mine) {
                xs[c * LF_PS + l] = valid ? in[p * 2 + c] : 0.0f;
                ds[c * LF_PS + l] = valid ? cot[p * 2 + c] : 0.0f;       // a point past M contributes exact zeros to every sum
            }
            __syncthreads();
            lf_block_g<true, false>(sw, xs, act, gs, HP, n);

            // the output layer: y = x + W_out h_n + b_out
            float* hn = act + n * AS;
            if (want_params) {
                if (w < 2) { if (l < HP) ao = lf_dot(ds + w * LF_PS, hn + l * LF_PS, ao); }
                else if (w == 2 && l < 2) ao = lf_sum(ds + l * LF_PS, ao);
            }
            __syncthreads();
            if (on) {
                const float d0 = ds[l], d1 = ds[LF_PS + l];
#pragma unroll
                for (int q = 0; q < LF_ROWS; ++q) {
                    const int k = j0 + q;
                    const float dh = fmaf(Wo[HP + k], d1, Wo[k] * d0);
                    hn[k * LF_PS + l] = dh * lf_elu_slope(hn[k * LF_PS + l]);
                }
            }
            __syncthreads();

            // the hidden layers, last first: D = act[i] holds dL/da_i, act[i - 1] holds h_{i-1} and receives dL/da_{i-1}
#pragma unroll
            for (int i = BAGS_LENS_MAX_INTERNAL_LAYERS; i >= 1; --i) {
                if (i > n) continue;
                const float* D = act + i * AS;
                float* hin = act + (i - 1) * AS;
                const float* W = sw + lf_lds_hidden(HP, i);
                if (want_params && on) {
                    if (l < HP) lf_wgrad(i == 1 ? aW1 : i == 2 ? aW2 : i == 3 ? aW3 : aW4, D, hin + l * LF_PS, j0);
                    if (l < LF_ROWS) {
                        float& ab = i == 1 ? ab1 : i == 2 ? ab2 : i == 3 ? ab3 : ab4;
                        ab = lf_sum(D + (j0 + l) * LF_PS, ab);
                    }
                }
                __syncthreads();
                if (on) {
                    float dh[LF_ROWS];
#pragma unroll
                    for (int q = 0; q < LF_ROWS; ++q) dh[q] = 0.0f;
                    for (int j = 0; j < HP; ++j) {
                        const float d = D[j * LF_PS + l];
                        const float4 wa = *reinterpret_cast<const float4*>(W + j * HP + j0), wb = *reinterpret_cast<const float4*>(W + j * HP + j0 + 4);
                        dh[0] = fmaf(wa.x, d, dh[0]); dh[1] = fmaf(wa.y, d, dh[1]); dh[2] = fmaf(wa.z, d, dh[2]); dh[3] = fmaf(wa.w, d, dh[3]);
                        dh[4] = fmaf(wb.x, d, dh[4]); dh[5] = fmaf(wb.y, d, dh[5]); dh[6] = fmaf(wb.z, d, dh[6]); dh[7] = fmaf(wb.w, d, dh[7]);
                    }
#pragma unroll
                    for (int q = 0; q < LF_ROWS; ++q) hin[(j0 + q) * LF_PS + l] = dh[q] * lf_elu_slope(hin[(j0 + q) * LF_PS + l]);
                }
                __syncthreads();
            }

            // the first layer: D = act[0] holds dL/da_0
            if (want_params && on) {
                if (l < 2 * LF_ROWS) a0 = lf_dot(act + (j0 + (l >> 1)) * LF_PS, xs + (l & 1) * LF_PS, a0);
                else if (l < 3 * LF_ROWS) a0 = lf_sum(act + (j0 + l - 2 * LF_ROWS) * LF_PS, a0);
            }
            if (mine && gin) {
                float dg = 0.0f;                                   // summed on its own: HP small terms rounded into ds one by one cost sqrt(HP) ulps of ds
                for (int j = 0; j < HP; ++j) dg = fmaf(sw[2 * j + c], act[j * LF_PS + l], dg);
                if (valid) gin[p * 2 + c] = ds[c * LF_PS + l] + dg;
            }
            __syncthreads();
        }

        if (want_params) {
            float* dst = part + (size_t)blockIdx.x * ((size_t)B * BF) + (size_t)b * BF;
            if (on) {
                if (l < 2 * LF_ROWS) { if (j0 + (l >> 1) < H) dst[(j0 + (l >> 1)) * 2 + (l & 1)] = a0; }
                else if (l < 3 * LF_ROWS) { if (j0 + l - 2 * LF_ROWS < H) dst[2 * H + j0 + l - 2 * LF_ROWS] = a0; }
#pragma unroll
                for (int i = 1; i <= BAGS_LENS_MAX_INTERNAL_LAYERS; ++i) {
                    if (i > n) continue;
                    float* gW = dst + 3 * H + (i - 1) * (H * H + H);
                    const float (&aW)[LF_ROWS] = i == 1 ? aW1 : i == 2 ? aW2 : i == 3 ? aW3 : aW4;
                    if (l < H) {
#pragma unroll
                        for (int q = 0; q < LF_ROWS; ++q) if (j0 + q < H) gW[(j0 + q) * H + l] = aW[q];
                    }
                    if (l < LF_ROWS && j0 + l < H) gW[H * H + j0 + l] = i == 1 ? ab1 : i == 2 ? ab2 : i == 3 ? ab3 : ab4;
                }
            }
            float* gO = dst + 3 * H + n * (H * H + H);
            if (w < 2) { if (l < H) gO[w * H + l] = ao; }
            else if (w == 2 && l < 2) gO[2 * H + l] = ao;
        }
    }
}

// grad_params[e] = the sum of the workgroups' rows, in workgroup order
__global__ void __launch_bounds__(LF_REDUCE_BLOCK) lens_field_reduce_kernel(const float* __restrict__ part, const int groups, const int np,
                                                                            float* __restrict__ grad_params)
{
    const int e = blockIdx.x * LF_REDUCE_BLOCK + threadIdx.x;
    if (e >= np) return;
    float acc = 0.0f;
    int g = 0;
    for (; g + 8 <= groups; g += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = part[(size_t)(g + u) * np + e];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += v[u];
    }
    for (; g < groups; ++g) acc += part[(size_t)g * np + e];
    grad_params[e] = acc;
}

// ---------------------------------------------------------------------------------------------- host side
static inline long long lf_tiles(long long M) { return (M + LF_TILE - 1) / LF_TILE; }
static inline int lf_groups(long long M) { const long long t = lf_tiles(M); return (int)(t < LF_MAX_GROUPS ? t : LF_MAX_GROUPS); }

struct LfWork { float* slots; float* part; };

// workspace (base rounded up here): [x_1 .. x_{B-1}, (B - 1) x (M,2) | partial sums, groups x (B * block floats)]
static size_t lf_carve(void* base, int B, int H, int n, long long M, LfWork* w)
{
    Carver c(base);
    const size_t m = (size_t)(M > 0 ? M : 0);
    LfWork k;
    k.slots = c.take<float>((size_t)(B > 1 ? B - 1 : 0) * m * 2);
    k.part = c.take<float>((size_t)lf_groups((long long)m) * (size_t)(B > 0 ? B : 0) * (size_t)lens_block_floats(H, n));
    if (w) *w = k;
    return c.used();
}

size_t lens_field_workspace_bytes(int B, int H, int n, long long M) { return lf_carve(nullptr, B, H, n, M, nullptr) + BASE_SLACK; }

template <typename K>
static hipError_t lf_big_lds(K kernel, size_t bytes)          // more than 64 KB of dynamic LDS has to be asked for
{
    if (bytes <= 65536) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

static LfNet lf_net(const BagsLensField& a) { return LfNet{a.blocks, a.hidden, a.internal_layers, lf_pad(a.hidden), a.params}; }

// validated by the caller (api.hip); M > 0.  inverse: src is y, dst is x
hipError_t launch_lens_field_fwd(const BagsLensField& a, const float* src, long long M, float* dst, bool inverse, int iterations, hipStream_t st)
{
    const LfNet net = lf_net(a);
    const size_t lds = ((size_t)lf_lds_floats(net.HP, net.n) + 2 * (size_t)net.HP * LF_PS + 4 * LF_PS) * sizeof(float);
    const dim3 grid((unsigned)lf_tiles(M));
    hipError_t e;
    if (inverse) {
        if ((e = lf_big_lds(lens_field_fwd_kernel<true>, lds)) != hipSuccess) return e;
        hipLaunchKernelGGL(lens_field_fwd_kernel<true>, grid, dim3(LF_BLOCK), lds, st, net, src, M, dst, iterations);
    } else {
        if ((e = lf_big_lds(lens_field_fwd_kernel<false>, lds)) != hipSuccess) return e;
        hipLaunchKernelGGL(lens_field_fwd_kernel<false>, grid, dim3(LF_BLOCK), lds, st, net, src, M, dst, 0);
    }
    return hipGetLastError();
}

hipError_t launch_lens_field_bwd(const BagsLensField& a, const float* x, long long M, const float* grad_y, void* workspace, float* grad_x,
                                 float* grad_params, hipStream_t st)
{
    const LfNet net = lf_net(a);
    LfWork wk; lf_carve(workspace, net.B, net.H, net.n, M, &wk);
    const size_t lds = ((size_t)lf_lds_floats(net.HP, net.n) + (size_t)(net.n + 1) * net.HP * LF_PS + 6 * LF_PS) * sizeof(float);
    const int groups = lf_groups(M), np = net.B * lens_block_floats(net.H, net.n);
    hipError_t e;
    if ((e = lf_big_lds(lens_field_bwd_kernel, lds)) != hipSuccess) return e;
    hipLaunchKernelGGL(lens_field_bwd_kernel, dim3(groups), dim3(LF_BLOCK), lds, st, net, x, M, grad_y, wk.slots, wk.part, grad_x,
                       grad_params ? 1 : 0);
    if (grad_params)
        hipLaunchKernelGGL(lens_field_reduce_kernel, dim3(cdiv(np, LF_REDUCE_BLOCK)), dim3(LF_REDUCE_BLOCK), 0, st, (const float*)wk.part, groups, np,
                           grad_params);
    return hipGetLastError();
}
