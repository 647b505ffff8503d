// resample_faces.hip -- the cubemap stitch (utils/cubemap_utils.py:181-186,219-288).
//
// The reference's large-FoV mode renders F perspective faces of the same Gaussians, warps each into the distorted output image with
// F.grid_sample and sums the masked results.  Here one kernel each way does that per OUTPUT pixel: the lens flow (smooth) is
// upsampled at the pixel with resample.hip's own taps, projected onto every face plane THERE -- not on the coarse control grid,
// where the projection is singular along the line a ray turns parallel to the face plane and upsampling across that line gives
// in-range garbage at every face boundary -- and the first face it lands in is sampled once.
//     (a, b, c) = M_f (gx, gy, 1)^T,  u = a / c,  v = b / c,  valid iff c > 0 && |u| <= 1 && |v| <= 1     (a NaN: not valid)
// The choice is a discrete decision: the forward writes it (face_index, -1 = no face), the backward REPLAYS it and never decides.
// Backward: resample.hip's scheme with (face, 16x16 tile) pairs as source tiles.  No global float atomics, bitwise reproducible,
// every element of every wanted face gradient written (no memset).
#include "resample_taps.h"

struct FacesArg {                 // by value in the kernel arguments, as adam.hip's group table
    ResampleGeom g;               // C, H, W: one face
    int F;
    const float* img[BAGS_MAX_FACES];
    float m[BAGS_MAX_FACES][9];
};
struct FacesGrad { float* g[BAGS_MAX_FACES]; };

struct FaceUV { float u, v, c; };
// the upsampled flow at a cropped pixel
__device__ __forceinline__ float2 flow_at(const ResampleGeom& g, const float* __restrict__ ctrl, int yc, int xc)
{
    const FlowTap f = flow_taps(g, g.y0 + yc, g.x0 + xc);
    const float2* c2 = reinterpret_cast<const float2*>(ctrl);
    const float2 a = c2[f.i00], b = c2[f.i01], c = c2[f.i10], d = c2[f.i11];
    // w00 a + w01 b + w10 c + w11 d with the roundings resample_fwd_kernel's build gives that sum (one product, three fused
    // multiply-adds, in this order), spelled out: left to the compiler, the contraction came out in another order here, and with
    // one face and the identity matrix the image is resample_image's bit for bit (tests/test_resample_faces_gpu.py holds it to that)
    return make_float2(fmaf(f.w11, d.x, fmaf(f.w10, c.x, fmaf(f.w00, a.x, f.w01 * b.x))),
                       fmaf(f.w11, d.y, fmaf(f.w10, c.y, fmaf(f.w00, a.y, f.w01 * b.y))));
}
__device__ __forceinline__ FaceUV face_uv(const float* m, float gx, float gy)
{
    const float a = m[0] * gx + m[1] * gy + m[2], b = m[3] * gx + m[4] * gy + m[5], c = m[6] * gx + m[7] * gy + m[8];
    FaceUV r; r.u = a / c; r.v = b / c; r.c = c;
    return r;
}

__global__ void __launch_bounds__(256)
faces_fwd_kernel(FacesArg A, const float* __restrict__ ctrl, float* __restrict__ out, int8_t* __restrict__ face_index)
{
    const ResampleGeom& g = A.g;
    const int xc = blockIdx.x * RS_TILE + (threadIdx.x & 15), yc = blockIdx.y * RS_TILE + (threadIdx.x >> 4);
    if (xc >= g.Wc || yc >= g.Hc) return;
    const float2 fl = flow_at(g, ctrl, yc, xc);
    const size_t plane = (size_t)g.H * g.W, oplane = (size_t)g.Hc * g.Wc, px = (size_t)yc * g.Wc + xc;
    int face = -1;
    float val[4] = {0.f, 0.f, 0.f, 0.f};
    // f is uniform: the matrix and the image pointer of a face are scalar loads
#pragma unroll 1
    for (int f = 0; f < A.F; ++f) {
        if (face >= 0) continue;
        const FaceUV p = face_uv(A.m[f], fl.x, fl.y);
        if (!(p.c > 0.f && fabsf(p.u) <= 1.f && fabsf(p.v) <= 1.f)) continue;          // written so that a NaN is "not valid"
        face = f;
        const ImgTap t = img_taps(g, p.u, p.v);            // integer positions only from coordinates known to be in [-1, 1]
        const float w00 = (1.f - t.fx) * (1.f - t.fy), w01 = t.fx * (1.f - t.fy), w10 = (1.f - t.fx) * t.fy, w11 = t.fx * t.fy;
        const size_t base = (size_t)t.y0 * g.W + t.x0;
        const float* img = A.img[f];
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
            if (ch >= g.C) break;
            const float* im = img + ch * plane;
            float v = 0.f;
            if (t.in00) v += w00 * im[base];
            if (t.in01) v += w01 * im[base + 1];
            if (t.in10) v += w10 * im[base + g.W];
            if (t.in11) v += w11 * im[base + g.W + 1];
            val[ch] = v;
        }
    }
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) if (ch < g.C) out[ch * oplane + px] = val[ch];
    face_index[px] = (int8_t)face;
}

// ---------------------------------------------------------------------------------------------------- backward
// resample.hip's two kernels with a face beside every tile:
//   1. faces_bwd_pixels_kernel, one workgroup per 16x16 OUTPUT tile.  Per pixel: its face (from face_index), its four taps and face
//      (left for the gather), dL/dflow through u = a/c, v = b/c (zero where no face).  Per tile and FACE: the bounding box of the
//      in-bounds taps in that face -- a tile at a cube corner holds three faces, so there is a box per face, and the tile is
//      appended to the list of every (face, 16x16 source tile) a box overlaps.
//   2. faces_gather_kernel, one workgroup per (face, source tile): the listed output tiles' taps that carry this face and land in
//      this tile, summed in LDS as 64-bit fixed-point integers; a list longer than RS_CAP is ignored and the boxes of all output
//      tiles are tested instead (slow, exact).  Every element is written.
struct FcWork { float2* gflow; int4* bbox; float* tmax; u32* count; u32* list; float4* taps; };

__global__ void __launch_bounds__(256)
faces_bwd_pixels_kernel(FacesArg A, const float* __restrict__ ctrl, const int8_t* __restrict__ face_index, const float* __restrict__ grad_out,
                        float2* __restrict__ gflow /* (Hc,Wc) or NULL */, int4* __restrict__ bbox /* NULL: no face gradient wanted */,
                        float* __restrict__ tmax, u32* __restrict__ count, u32* __restrict__ list, float4* __restrict__ taps,
                        int src_tiles_x, int src_tiles)
{
    __shared__ int s_box[BAGS_MAX_FACES][4];
    __shared__ int s_max;                                     // bits of a non-negative float: integer order is float order
    const ResampleGeom& g = A.g;
    const int otx = blockIdx.x, oty = blockIdx.y, ot = oty * gridDim.x + otx;
    const int xc = otx * RS_TILE + (threadIdx.x & 15), yc = oty * RS_TILE + (threadIdx.x >> 4);
    if (threadIdx.x < BAGS_MAX_FACES) {
        s_box[threadIdx.x][0] = 0x7FFFFFFF; s_box[threadIdx.x][1] = 0x7FFFFFFF; s_box[threadIdx.x][2] = -1; s_box[threadIdx.x][3] = -1;
    }
    if (threadIdx.x == 0) s_max = 0;
    __syncthreads();
    float amax = 0.f;
    int face = -1, bx0 = 0x7FFFFFFF, by0 = 0x7FFFFFFF, bx1 = -1, by1 = -1;      // this pixel's face and the box of its in-bounds taps
    if (xc < g.Wc && yc < g.Hc) {
        const size_t plane = (size_t)g.H * g.W, oplane = (size_t)g.Hc * g.Wc, px = (size_t)yc * g.Wc + xc;
        face = face_index[px];
        if (face >= A.F) face = -1;                           // not this call's map: no face rather than a wild pointer
        float go[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) if (ch < g.C) { go[ch] = grad_out[ch * oplane + px]; amax = fmaxf(amax, fabsf(go[ch])); }
        float2 gf = make_float2(0.f, 0.f);
        float4 rec = make_float4(__uint_as_float(0xFFFEFFFEu), 0.f, 0.f, __int_as_float(-1));       // taps at (-2, -2), no face
        if (face >= 0) {
            const float2 fl = flow_at(g, ctrl, yc, xc);
#pragma unroll 1
            for (int f = 0; f < A.F; ++f) {                   // uniform f, one pass per face present in the wave
                if (f != face) continue;
                const float* m = A.m[f];
                const FaceUV p = face_uv(m, fl.x, fl.y);
                const ImgTap t = img_taps(g, p.u, p.v);
                const bool any_in = t.in00 || t.in01 || t.in10 || t.in11;
                const u32 xy = ((u32)t.x0 & 0xFFFFu) | ((u32)t.y0 << 16);              // x0, y0 in [-2, 32000]: int16 pairs
                rec = make_float4(__uint_as_float(xy), any_in ? t.fx : 0.f, t.fy, __int_as_float(f));
                if (gflow) {
                    const size_t base = (size_t)t.y0 * g.W + t.x0;
                    const float* img = A.img[f];
                    float dix = 0.f, diy = 0.f;
#pragma unroll
                    for (int ch = 0; ch < 4; ++ch) {
                        if (ch >= g.C) break;
                        const float* im = img + ch * plane;
                        const float v00 = t.in00 ? im[base] : 0.f, v01 = t.in01 ? im[base + 1] : 0.f;
                        const float v10 = t.in10 ? im[base + g.W] : 0.f, v11 = t.in11 ? im[base + g.W + 1] : 0.f;
                        dix += go[ch] * ((v01 - v00) * (1.f - t.fy) + (v11 - v10) * t.fy);
                        diy += go[ch] * ((v10 - v00) * (1.f - t.fx) + (v11 - v01) * t.fx);
                    }
                    const float du = dix * 0.5f * (float)(g.W - 1), dv = diy * 0.5f * (float)(g.H - 1);     // dL/du, dL/dv
                    // u = a / c: du/dgx = (m0 - u m6) / c, du/dgy = (m1 - u m7) / c; v = b / c alike
                    gf.x = (du * (m[0] - p.u * m[6]) + dv * (m[3] - p.v * m[6])) / p.c;
                    gf.y = (du * (m[1] - p.u * m[7]) + dv * (m[4] - p.v * m[7])) / p.c;
                }
                if (any_in) {
                    bx0 = (t.in00 || t.in10) ? t.x0 : t.x0 + 1; bx1 = (t.in01 || t.in11) ? t.x0 + 1 : t.x0;
                    by0 = (t.in00 || t.in01) ? t.y0 : t.y0 + 1; by1 = (t.in10 || t.in11) ? t.y0 + 1 : t.y0;
                }
            }
        }
        if (gflow) gflow[px] = gf;
        if (bbox) taps[px] = rec;
    }
    if (!bbox) return;                                        // no face gradient wanted
    // the largest |dL/dout| of the tile (a NaN is dropped by fmaxf, an inf is kept): every lane takes part, one LDS atomic per wave
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) amax = fmaxf(amax, __shfl_xor(amax, d));
    if ((threadIdx.x & 63) == 0) atomicMax(&s_max, __float_as_int(amax));
    // the box of every face the wave holds (mostly one): reduced over the wave, then four LDS atomics by one lane.  (One LDS atomic
    // per pixel and bound serialised 64 lanes on one address four times per wave.)
    for (int f = 0; f < A.F; ++f) {
        const bool mine = face == f && bx1 >= 0;
        if (__ballot(mine) == 0ull) continue;                 // uniform over the wave: every lane takes part in the shuffles
        int x0 = mine ? bx0 : 0x7FFFFFFF, y0 = mine ? by0 : 0x7FFFFFFF, x1 = mine ? bx1 : -1, y1 = mine ? by1 : -1;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            x0 = min(x0, __shfl_xor(x0, d)); y0 = min(y0, __shfl_xor(y0, d));
            x1 = max(x1, __shfl_xor(x1, d)); y1 = max(y1, __shfl_xor(y1, d));
        }
        if ((threadIdx.x & 63) == 0) {
            atomicMin(&s_box[f][0], x0); atomicMin(&s_box[f][1], y0); atomicMax(&s_box[f][2], x1); atomicMax(&s_box[f][3], y1);
        }
    }
    __syncthreads();
    amax = __int_as_float(s_max);
    if (threadIdx.x < A.F)
        bbox[(size_t)ot * A.F + threadIdx.x] = make_int4(s_box[threadIdx.x][0], s_box[threadIdx.x][1], s_box[threadIdx.x][2], s_box[threadIdx.x][3]);
    if (threadIdx.x == 0) tmax[ot] = amax;
    if (!(amax > 0.f)) return;                                // a zero cotangent: on no list
    for (int f = 0; f < A.F; ++f) {
        const int tx0 = s_box[f][0], ty0 = s_box[f][1], tx1 = s_box[f][2], ty1 = s_box[f][3];
        if (tx1 < tx0 || ty1 < ty0) continue;                 // nothing of this tile lands in face f
        const int sx0 = tx0 / RS_TILE, sx1 = tx1 / RS_TILE, sy0 = ty0 / RS_TILE, sy1 = ty1 / RS_TILE;
        const int nsx = sx1 - sx0 + 1, n = nsx * (sy1 - sy0 + 1);
        for (int k = threadIdx.x; k < n; k += 256) {
            const int st = f * src_tiles + (sy0 + k / nsx) * src_tiles_x + sx0 + k % nsx;
            const u32 slot = atomicAdd(&count[st], 1u);
            if (slot < RS_CAP) list[(size_t)st * RS_CAP + slot] = (u32)ot;
        }
    }
}

__global__ void __launch_bounds__(256)
faces_gather_kernel(ResampleGeom g, int F, const float* __restrict__ grad_out, const int4* __restrict__ bbox, const float* __restrict__ tmax,
                    const u32* __restrict__ count, const u32* __restrict__ list, const float4* __restrict__ taps, FacesGrad G,
                    int out_tiles_x, int out_tiles)
{
    __shared__ unsigned long long acc[4 * 256];              // [C][256] fixed-point sums
    __shared__ u32 s_list[RS_CAP];
    __shared__ float s_red[4];
    const int face = blockIdx.z;
    float* __restrict__ grad_image = G.g[face];
    if (!grad_image) return;                                  // this face's gradient is not wanted (uniform)
    const int stx = blockIdx.x, sty = blockIdx.y, st = (face * gridDim.y + sty) * gridDim.x + stx;
    const int X0 = stx * RS_TILE, Y0 = sty * RS_TILE;
    const u32 n_all = count[st];
    const bool listed = n_all <= RS_CAP;
    const u32 n = listed ? n_all : (u32)out_tiles;
    auto overlaps = [&](int ot) {
        const int4 bb = bbox[(size_t)ot * F + face];
        return bb.x <= X0 + RS_TILE - 1 && bb.z >= X0 && bb.y <= Y0 + RS_TILE - 1 && bb.w >= Y0;
    };
    for (int i = threadIdx.x; i < g.C * 256; i += 256) acc[i] = 0ull;
    if (listed && threadIdx.x < n_all) s_list[threadIdx.x] = list[(size_t)st * RS_CAP + threadIdx.x];
    // largest |dL/dout| among the contributing tiles (order-independent) -> the power-of-two quantum, as resample_gather_kernel
    float m = 0.f;
    if (listed) { if (threadIdx.x < n_all) m = tmax[list[(size_t)st * RS_CAP + threadIdx.x]]; }
    else for (int ot = threadIdx.x; ot < out_tiles; ot += 256) if (overlaps(ot)) m = fmaxf(m, tmax[ot]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d));
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
    // quantum = 2^(e - bits), m < 2^e, bits = 62 - ceil(log2(n * 1024)): at most n * 1024 terms of at most m meet in one accumulator
    int e = 0; (void)frexpf(m, &e);
    if (e < -100) e = -100;
    int lg = 10; { u32 v = (n > 1 ? n : 1u) - 1u; while (v) { ++lg; v >>= 1; } }
    const int bits = 62 - lg;
    const float up = ldexpf(1.0f, 24 - e);
    const int shift = bits - 24;
    const size_t oplane = (size_t)g.Hc * g.Wc;
    if (m > 0.f && isfinite(m)) {
        auto add_taps = [&](const float4 rec, const float* go) {
            if (__float_as_int(rec.w) != face) return;        // the pixel belongs to another face (or to none)
            const u32 xy = __float_as_uint(rec.x);
            const int tx0 = (int)(short)(xy & 0xFFFFu), ty0 = (int)(short)(xy >> 16);
            const float fxw = rec.y, fyw = rec.z;
            const float w[4] = {(1.f - fxw) * (1.f - fyw), fxw * (1.f - fyw), (1.f - fxw) * fyw, fxw * fyw};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int sx = tx0 + (q & 1), sy = ty0 + (q >> 1);
                const int lx = sx - X0, ly = sy - Y0;
                // in this source tile (and hence inside the face: every source tile is clipped by the write-out below)?
                if (lx < 0 || lx >= RS_TILE || ly < 0 || ly >= RS_TILE || sx >= g.W || sy >= g.H) continue;
#pragma unroll
                for (int ch = 0; ch < 4; ++ch)
                    if (ch < g.C) atomicAdd(&acc[ch * 256 + ly * RS_TILE + lx], rs_fixed(w[q] * go[ch], up, shift));
            }
        };
        auto load = [&](int ot, float4& rec, float* go) {    // thread = one pixel of output tile ot; false outside the crop
            const int xc = (ot % out_tiles_x) * RS_TILE + (threadIdx.x & 15), yc = (ot / out_tiles_x) * RS_TILE + (threadIdx.x >> 4);
            if (xc >= g.Wc || yc >= g.Hc) return false;
            const size_t px = (size_t)yc * g.Wc + xc;
            rec = taps[px];
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) if (ch < g.C) go[ch] = grad_out[ch * oplane + px];
            return true;
        };
        constexpr int RS_BATCH = 4;                           // list entries requested together: one round trip per batch
        if (listed) {
            for (u32 k0 = 0; k0 < n; k0 += RS_BATCH) {
                float4 rec[RS_BATCH]; float go[RS_BATCH][4]; bool on[RS_BATCH];
#pragma unroll
                for (int j = 0; j < RS_BATCH; ++j) {
                    rec[j] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                    for (int ch = 0; ch < 4; ++ch) go[j][ch] = 0.f;
                    on[j] = k0 + j < n && load((int)s_list[k0 + j], rec[j], go[j]);
                }
#pragma unroll
                for (int j = 0; j < RS_BATCH; ++j) if (on[j]) add_taps(rec[j], go[j]);
            }
        } else {
            for (int ot = 0; ot < out_tiles; ++ot) {
                if (!overlaps(ot)) continue;                  // uniform
                float4 rec; float go[4] = {0.f, 0.f, 0.f, 0.f};
                if (load(ot, rec, go)) add_taps(rec, go);
            }
        }
    }
    __syncthreads();
    const int x = X0 + (threadIdx.x & 15), y = Y0 + (threadIdx.x >> 4);
    if (x < g.W && y < g.H) {
        const double q = ldexp(1.0, e - 24 - 24 - (shift - 24));            // value of one fixed-point unit
        // a non-finite cotangent anywhere on this source tile's list poisons the tile, as PyTorch's scatter would the taps it hits
        const bool bad = !isfinite(m);
        for (int ch = 0; ch < g.C; ++ch)
            grad_image[(size_t)ch * g.H * g.W + (size_t)y * g.W + x] =
                bad ? __builtin_nanf("") : (float)((double)(long long)acc[ch * 256 + threadIdx.x] * q);
    }
}

static FacesArg make_arg(const BagsFaces& f, int h, int w, int Hf, int Wf, int Hc, int Wc)
{
    FacesArg A;
    A.g = make_geom(f.C, f.H, f.W, h, w, Hf, Wf, Hc, Wc);
    A.F = f.n_faces;
    for (int i = 0; i < BAGS_MAX_FACES; ++i) {
        A.img[i] = i < f.n_faces ? f.image[i] : nullptr;
        for (int k = 0; k < 9; ++k) A.m[i][k] = i < f.n_faces ? f.mats[i][k] : 0.f;
    }
    return A;
}

hipError_t launch_resample_faces_fwd(const BagsFaces& f, const float* ctrl, int h, int w, int Hf, int Wf, int Hc, int Wc, float* out,
                                     int8_t* face_index, hipStream_t st)
{
    const FacesArg A = make_arg(f, h, w, Hf, Wf, Hc, Wc);
    hipLaunchKernelGGL(faces_fwd_kernel, dim3(cdiv(Wc, RS_TILE), cdiv(Hc, RS_TILE)), dim3(256), 0, st, A, ctrl, out, face_index);
    return hipGetLastError();
}

static size_t fc_carve(void* base, int F, int H, int W, int Hc, int Wc, FcWork* w)
{
    Carver c(base);
    const size_t To = (size_t)cdiv(Wc, RS_TILE) * cdiv(Hc, RS_TILE), Ts = (size_t)F * cdiv(W, RS_TILE) * cdiv(H, RS_TILE);
    FcWork r;
    r.gflow = c.take<float2>((size_t)Hc * Wc); r.bbox = c.take<int4>(To * F); r.tmax = c.take<float>(To);
    r.count = c.take<u32>(Ts); r.list = c.take<u32>(Ts * RS_CAP); r.taps = c.take<float4>((size_t)Hc * Wc);
    if (w) *w = r;
    return c.used();
}
size_t resample_faces_workspace_bytes(int F, int H, int W, int Hc, int Wc) { return fc_carve(nullptr, F, H, W, Hc, Wc, nullptr) + BASE_SLACK; }

hipError_t launch_resample_faces_bwd(const BagsFaces& f, const float* ctrl, int h, int w, int Hf, int Wf, int Hc, int Wc,
                                     const int8_t* face_index, const float* grad_out, void* workspace, float* const* grad_faces,
                                     float* grad_ctrl, hipStream_t st)
{
    const FacesArg A = make_arg(f, h, w, Hf, Wf, Hc, Wc);
    FcWork wk; fc_carve(workspace, f.n_faces, f.H, f.W, Hc, Wc, &wk);
    FacesGrad G; bool any = false;
    for (int i = 0; i < BAGS_MAX_FACES; ++i) { G.g[i] = (grad_faces && i < f.n_faces) ? grad_faces[i] : nullptr; any |= G.g[i] != nullptr; }
    const int otx = cdiv(Wc, RS_TILE), oty = cdiv(Hc, RS_TILE), stx = cdiv(f.W, RS_TILE), sty = cdiv(f.H, RS_TILE);
    hipError_t e;
    if (any && (e = hipMemsetAsync(wk.count, 0, (size_t)f.n_faces * stx * sty * sizeof(u32), st)) != hipSuccess) return e;
    hipLaunchKernelGGL(faces_bwd_pixels_kernel, dim3(otx, oty), dim3(256), 0, st, A, ctrl, face_index, grad_out,
                       grad_ctrl ? wk.gflow : (float2*)nullptr, any ? wk.bbox : (int4*)nullptr, wk.tmax, wk.count, wk.list, wk.taps, stx, stx * sty);
    if (any)
        hipLaunchKernelGGL(faces_gather_kernel, dim3(stx, sty, f.n_faces), dim3(256), 0, st, A.g, f.n_faces, grad_out, (const int4*)wk.bbox,
                           (const float*)wk.tmax, (const u32*)wk.count, (const u32*)wk.list, (const float4*)wk.taps, G, otx, otx * oty);
    if (grad_ctrl && (e = launch_resample_ctrl_gather(h, w, Hf, Wf, Hc, Wc, (const float2*)wk.gflow, grad_ctrl, st)) != hipSuccess) return e;
    return hipGetLastError();
}
