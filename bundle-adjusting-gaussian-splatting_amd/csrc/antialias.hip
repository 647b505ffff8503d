// antialias.hip -- the mip filter's opacity scale (upstream diff_gaussian_rasterization's `antialiasing`, Mip-Splatting's 2D filter):
//     out = opacity * h,   h = sqrt(max(0.000025, det(cov2D) / det(cov2D + 0.3 I)))
// the factor that makes the dilated Gaussian K1 rasterizes carry the energy of the undilated one.  It lives IN FRONT of the
// operator: upstream applies it in exactly one place, conic_opacity.w, so a function on the operator's `opacities`
// input, chained with the operator's dL/dopacities, is upstream's antialiased forward and backward; BagsSettings, K1 and K9 do
// not change.
//
// One lane per Gaussian both ways.  The forward chain is projection.h's, included and not restated, and this file is compiled
// with -ffp-contract=off like K1 and K9: d1 below is K1's det bit for bit, so `d1 != 0` is K1's cull.  The backward recomputes
// the forward from the inputs (nothing is saved, as K9) and states the backward of the covariance chain a SECOND time -- K9's
// lines in K9's order (preprocess_bwd.hip step 3 and the shift polynomial), to be folded later (DESIGN.md open items).  The 17
// non-zero pose terms (viewmatrix 4x3, k[0], k[5], shift_factors) are reduced wave -> workgroup -> one slab row per workgroup;
// a second small launch adds the rows in double in a fixed order (ordered_sum.h: slab_column_sum).  No atomics: two runs give
// the same bits.
#include "ordered_sum.h"
#include "projection.h"

#define AA_BLOCK 256
#define AA_VALS 17               // slab columns used: [0..11] viewmatrix rows 0..3 x cols 0..2, [12] k[0], [13] k[5], [14..16] shift_factors
#define AA_FLOOR 0.000025f       // upstream's floor of the ratio: h >= 0.005

// The forward of one Gaussian: everything the backward needs stays in the struct (the forward kernel uses h alone).
struct AaForward {
    PjView t; PjShift sh; PjCov3d S; PjCov2d c;
    float s0, s1, s2;            // the modified scales
    float uxx, uxy, uyy;         // cov2D BEFORE the + 0.3
    float d0, d1, ratio, h;
    bool live;
};
template <bool COV3D>
__device__ __forceinline__ AaForward aa_forward(const float* v, const float* k, const int W, const int H, const float tanfovx, const float tanfovy,
                                                const float mod, const float sf0, const float sf1, const float sf2, const float x, const float y,
                                                const float z, const float in_s0, const float in_s1, const float in_s2, const float qr,
                                                const float qx, const float qy, const float qz, const float* in_c)
{
    AaForward f;
    f.t = pj_view(v, x, y, z);
    f.sh = pj_shift(f.t.tx, f.t.ty, f.t.tz, sf0, sf1, sf2);
    float c0, c1, c2, c3, c4, c5;
    if (COV3D) {
        c0 = in_c[0]; c1 = in_c[1]; c2 = in_c[2]; c3 = in_c[3]; c4 = in_c[4]; c5 = in_c[5];
        f.s0 = f.s1 = f.s2 = 0.f;
    } else {
        f.s0 = in_s0 * mod; f.s1 = in_s1 * mod; f.s2 = in_s2 * mod;
        f.S = pj_cov3d(f.s0, f.s1, f.s2, qr, qx, qy, qz);
        c0 = f.S.c0; c1 = f.S.c1; c2 = f.S.c2; c3 = f.S.c3; c4 = f.S.c4; c5 = f.S.c5;
    }
    f.c = pj_cov2d(v, k[0], k[5], W, H, tanfovx, tanfovy, f.t.tx, f.t.ty, f.sh.tzs, c0, c1, c2, c3, c4, c5);
    // (not cxx - 0.3: these are the sums the + 0.3 was added to, so c.cxx == uxx + 0.3f and c.cyy == uyy + 0.3f exactly)
    f.uxx = f.c.b00 * f.c.a00 + f.c.b01 * f.c.a01 + f.c.b02 * f.c.a02;
    f.uxy = f.c.cxy;
    f.uyy = f.c.b10 * f.c.a10 + f.c.b11 * f.c.a11 + f.c.b12 * f.c.a12;
    f.d0 = f.uxx * f.uyy - f.uxy * f.uxy;
    f.d1 = pj_conic(f.c.cxx, f.c.cxy, f.c.cyy).det;
    f.live = (f.t.tz > 0.2f) && (f.d1 != 0.0f);       // K1's two culls; a Gaussian K1 drops keeps its opacity (nobody reads it)
    f.ratio = f.d0 / f.d1;
    f.h = f.live ? sqrtf(fmaxf(AA_FLOOR, f.ratio)) : 1.0f;
    return f;
}

// a Gaussian's input rows (index clamped by the caller)
struct AaRows { float x, y, z, s0, s1, s2, qr, qx, qy, qz, c[6]; };
template <bool COV3D>
__device__ __forceinline__ AaRows aa_load(const size_t ic, const float* __restrict__ means3D, const float* __restrict__ scales,
                                          const float* __restrict__ rotations, const float* __restrict__ cov3D_precomp)
{
    AaRows r;
    r.x = means3D[3 * ic]; r.y = means3D[3 * ic + 1]; r.z = means3D[3 * ic + 2];
    r.s0 = r.s1 = r.s2 = r.qr = r.qx = r.qy = r.qz = 0.f;
#pragma unroll
    for (int t = 0; t < 6; ++t) r.c[t] = 0.f;
    if (COV3D) {
#pragma unroll
        for (int t = 0; t < 6; ++t) r.c[t] = cov3D_precomp[6 * ic + t];
    } else {
        r.s0 = scales[3 * ic]; r.s1 = scales[3 * ic + 1]; r.s2 = scales[3 * ic + 2];
        r.qr = rotations[4 * ic]; r.qx = rotations[4 * ic + 1]; r.qy = rotations[4 * ic + 2]; r.qz = rotations[4 * ic + 3];
    }
    return r;
}

template <bool COV3D>
__global__ void __launch_bounds__(AA_BLOCK)
antialias_fwd_kernel(int P, int W, int H, float tanfovx, float tanfovy, float mod, const float* __restrict__ means3D,
                     const float* __restrict__ scales, const float* __restrict__ rotations, const float* __restrict__ cov3D_precomp,
                     const float* __restrict__ opacities, const float* __restrict__ shift_factors, const float* __restrict__ viewmatrix,
                     const float* __restrict__ intrinsic, float* __restrict__ out)
{
    const int i = blockIdx.x * AA_BLOCK + threadIdx.x;
    if (i >= P) return;
    // the camera through wave-uniform indices of the kernel's own pointers: scalar loads, as K9
    const float sf0 = shift_factors ? shift_factors[0] : 0.0f, sf1 = shift_factors ? shift_factors[1] : 0.0f,
                sf2 = shift_factors ? shift_factors[2] : 0.0f;
    const AaRows r = aa_load<COV3D>((size_t)i, means3D, scales, rotations, cov3D_precomp);
    const float opac = opacities[i];
    const AaForward f = aa_forward<COV3D>(viewmatrix, intrinsic, W, H, tanfovx, tanfovy, mod, sf0, sf1, sf2, r.x, r.y, r.z, r.s0, r.s1, r.s2,
                                          r.qr, r.qx, r.qy, r.qz, r.c);
    out[i] = opac * f.h;
}

// slab == nullptr: no pose output is wanted and nothing is reduced.  Every per-Gaussian value is formed whether or not it is
// stored, so the bits of a wanted output do not depend on which others are wanted.
template <bool COV3D>
__global__ void __launch_bounds__(AA_BLOCK)
antialias_bwd_kernel(int P, int W, int H, float tanfovx, float tanfovy, float mod, int clamp_stock, const float* __restrict__ means3D,
                     const float* __restrict__ scales, const float* __restrict__ rotations, const float* __restrict__ cov3D_precomp,
                     const float* __restrict__ opacities, const float* __restrict__ shift_factors, const float* __restrict__ viewmatrix,
                     const float* __restrict__ intrinsic, const float* __restrict__ grad_out, float* __restrict__ slab,
                     float* __restrict__ g_opac, float* __restrict__ g_means3D, float* __restrict__ g_scales, float* __restrict__ g_rot,
                     float* __restrict__ g_cov3D)
{
    __shared__ float wpose[AA_BLOCK / 64][AA_VALS];
    const int i = blockIdx.x * AA_BLOCK + threadIdx.x;
    const float* v = viewmatrix;
    const float sf0 = shift_factors ? shift_factors[0] : 0.0f, sf1 = shift_factors ? shift_factors[1] : 0.0f,
                sf2 = shift_factors ? shift_factors[2] : 0.0f;
    // every lane runs the chain (index clamped: P > 0 here), so that the DPP rows of the pose reduction are complete; what a lane
    // without a Gaussian, a culled Gaussian or one on the floor computes -- Inf, NaN -- is replaced by 0 in the selects below and
    // never reaches a sum: no 0 * inf in the pose terms
    const size_t ic = (size_t)(i < P ? i : P - 1);
    const AaRows r = aa_load<COV3D>(ic, means3D, scales, rotations, cov3D_precomp);
    const float opac = opacities[ic], g = grad_out[ic];
    const float x = r.x, y = r.y, z = r.z;
    const AaForward f = aa_forward<COV3D>(v, intrinsic, W, H, tanfovx, tanfovy, mod, sf0, sf1, sf2, x, y, z, r.s0, r.s1, r.s2, r.qr, r.qx, r.qy,
                                          r.qz, r.c);
    // the gradient runs through h only for a Gaussian K1 keeps whose ratio is above the floor
    const bool through = (i < P) && f.live && (f.ratio > AA_FLOOR);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    auto red = [&](const int t, const float val) {
        if (slab) {                                                           // uniform
            const float tot = wave_total_f(through ? val : 0.f);
            if (lane == 63) wpose[wave][t] = tot;
        }
    };

    // ---- h -> cov2D.  With g_d0 = g_ratio / d1 and g_d1 = -g_ratio d0 / d1^2 the three sums
    //     g_uxx = g_d0 uyy + g_d1 (uyy + 0.3),   g_uyy = g_d0 uxx + g_d1 (uxx + 0.3),   g_uxy = -2 uxy (g_d0 + g_d1)
    // are differences of nearly equal terms once a splat is larger than a pixel (ratio -> 1).  Over the common denominator d1^2 the
    // numerators are uyy d1 - d0 cyy = 0.3 (uyy cyy + uxy^2), likewise for uxx, and d1 - d0 = 0.3 (uxx + uyy) + 0.09: the same
    // sums with nothing left to cancel, which is what is evaluated here.
    const PjCov2d& C = f.c;
    const float uxx = f.uxx, uxy = f.uxy, uyy = f.uyy, d1 = f.d1;
    const float g_ratio = g * opac / (2.0f * f.h);
    const float w = g_ratio / (d1 * d1);
    const float dcxx = w * (0.3f * (uyy * C.cyy + uxy * uxy));
    const float dcyy = w * (0.3f * (uxx * C.cxx + uxy * uxy));
    const float dcxy = -2.0f * uxy * (w * (0.3f * (uxx + uyy) + 0.09f));

    // ---- cov2D -> (J, Wc, Sigma): preprocess_bwd.hip's lines from "cov2D -> Sigma" on, in its order
    const float a00 = C.a00, a01 = C.a01, a02 = C.a02, a10 = C.a10, a11 = C.a11, a12 = C.a12;
    const float b00 = C.b00, b01 = C.b01, b02 = C.b02, b10 = C.b10, b11 = C.b11, b12 = C.b12;
    const float j00 = C.j00, j02 = C.j02, j11 = C.j11, j12 = C.j12;
    const float fx = C.fx, fy = C.fy, itz = C.itz, ux = C.ux, uy = C.uy;
    const float tx = f.t.tx, ty = f.t.ty, tz = f.t.tz, tzs = f.sh.tzs;
    const bool clx = (C.txtz < -C.limx) || (C.txtz > C.limx), cly = (C.tytz < -C.limy) || (C.tytz > C.limy);
    float gc[6];
    gc[0] = dcxx * a00 * a00 + dcxy * a00 * a10 + dcyy * a10 * a10;
    gc[3] = dcxx * a01 * a01 + dcxy * a01 * a11 + dcyy * a11 * a11;
    gc[5] = dcxx * a02 * a02 + dcxy * a02 * a12 + dcyy * a12 * a12;
    gc[1] = 2.f * dcxx * a00 * a01 + dcxy * (a00 * a11 + a01 * a10) + 2.f * dcyy * a10 * a11;
    gc[2] = 2.f * dcxx * a00 * a02 + dcxy * (a00 * a12 + a02 * a10) + 2.f * dcyy * a10 * a12;
    gc[4] = 2.f * dcxx * a01 * a02 + dcxy * (a01 * a12 + a02 * a11) + 2.f * dcyy * a11 * a12;
    // cov2D -> A = J Wc
    const float dA00 = 2.f * dcxx * b00 + dcxy * b10, dA01 = 2.f * dcxx * b01 + dcxy * b11, dA02 = 2.f * dcxx * b02 + dcxy * b12;
    const float dA10 = 2.f * dcyy * b10 + dcxy * b00, dA11 = 2.f * dcyy * b11 + dcxy * b01, dA12 = 2.f * dcyy * b12 + dcxy * b02;
    // A -> J
    const float dj00 = dA00 * v[0] + dA01 * v[4] + dA02 * v[8];
    const float dj02 = dA00 * v[2] + dA01 * v[6] + dA02 * v[10];
    const float dj11 = dA10 * v[1] + dA11 * v[5] + dA12 * v[9];
    const float dj12 = dA10 * v[2] + dA11 * v[6] + dA12 * v[10];
    // J -> focal lengths, view-space point
    const float dfx = dj00 * itz - dj02 * ux * itz;
    const float dfy = dj11 * itz - dj12 * uy * itz;
    const float dux = -dj02 * fx * itz, duy = -dj12 * fy * itz;
    const float ditz = dj00 * fx - dj02 * fx * ux + dj11 * fy - dj12 * fy * uy;
    float dtx = 0.f, dty = 0.f;
    float dtzs = -ditz * itz * itz;
    // the 1.3 x field-of-view clamp (BagsAntialias.clamp_grad, as BagsSettings.clamp_grad in K9): stock holds a clamped t.x = ux tzs
    // constant inside dL/dt.z, exact differentiates the clamped expression (nothing more for a clamped axis)
    if (!clx) { dtx += dux * itz; dtzs -= dux * tx * itz * itz; }
    else if (clamp_stock) dtzs -= dux * (ux * tzs) * itz * itz;
    if (!cly) { dty += duy * itz; dtzs -= duy * ty * itz * itz; }
    else if (clamp_stock) dtzs -= duy * (uy * tzs) * itz * itz;
    // tzs = tz + shift, the shift polynomial in theta = atan2(rho, tz)
    float dtz = dtzs;
    const float dshift = dtzs;
    const float rho = f.sh.rho, th2 = f.sh.th2, th3 = f.sh.th3;
    const float dtheta = dshift * (3.f * sf0 * th2 + 5.f * sf1 * th2 * th2 + 7.f * sf2 * th2 * th2 * th2);
    const float ir2 = 1.0f / (rho * rho + tz * tz);
    const float drho = dtheta * tz * ir2;
    dtz -= dtheta * rho * ir2;
    dtx += drho * tx / rho; dty += drho * ty / rho;
    // view-space point -> world point
    float dmx = dtx * v[0] + dty * v[1] + dtz * v[2];
    float dmy = dtx * v[4] + dty * v[5] + dtz * v[6];
    float dmz = dtx * v[8] + dty * v[9] + dtz * v[10];
    // ---- the camera side of those products: viewmatrix's rotation block through Wc and through t, its translation row through t
    red(0, dA00 * j00 + dtx * x); red(1, dA10 * j11 + dty * x); red(2, (dA00 * j02 + dA10 * j12) + dtz * x);       // v[0], v[1], v[2]
    red(3, dA01 * j00 + dtx * y); red(4, dA11 * j11 + dty * y); red(5, (dA01 * j02 + dA11 * j12) + dtz * y);       // v[4], v[5], v[6]
    red(6, dA02 * j00 + dtx * z); red(7, dA12 * j11 + dty * z); red(8, (dA02 * j02 + dA12 * j12) + dtz * z);       // v[8], v[9], v[10]
    red(9, dtx); red(10, dty); red(11, dtz);                                                                          // v[12], v[13], v[14]
    red(12, dfx * (0.5f * (float)W));
    red(13, dfy * (0.5f * (float)H));
    red(14, dshift * th3); red(15, dshift * th3 * th2); red(16, dshift * th3 * th2 * th2);

    // ---- Sigma -> scales, rotation (the quaternion as given)
    float gs0 = 0.f, gs1 = 0.f, gs2 = 0.f, gqr = 0.f, gqx = 0.f, gqy = 0.f, gqz = 0.f;
    if (!COV3D) {
        const PjCov3d& S = f.S;
        const float s0 = f.s0, s1 = f.s1, s2 = f.s2, qr = r.qr, qx = r.qx, qy = r.qy, qz = r.qz;
        const float S00 = 2.f * gc[0], S01 = gc[1], S02 = gc[2], S11 = 2.f * gc[3], S12 = gc[4], S22 = 2.f * gc[5];
        const float l00 = S.r00 * s0, l01 = S.r01 * s1, l02 = S.r02 * s2;
        const float l10 = S.r10 * s0, l11 = S.r11 * s1, l12 = S.r12 * s2;
        const float l20 = S.r20 * s0, l21 = S.r21 * s1, l22 = S.r22 * s2;
        const float dl00 = S00 * l00 + S01 * l10 + S02 * l20, dl01 = S00 * l01 + S01 * l11 + S02 * l21, dl02 = S00 * l02 + S01 * l12 + S02 * l22;
        const float dl10 = S01 * l00 + S11 * l10 + S12 * l20, dl11 = S01 * l01 + S11 * l11 + S12 * l21, dl12 = S01 * l02 + S11 * l12 + S12 * l22;
        const float dl20 = S02 * l00 + S12 * l10 + S22 * l20, dl21 = S02 * l01 + S12 * l11 + S22 * l21, dl22 = S02 * l02 + S12 * l12 + S22 * l22;
        gs0 = mod * (dl00 * S.r00 + dl10 * S.r10 + dl20 * S.r20);
        gs1 = mod * (dl01 * S.r01 + dl11 * S.r11 + dl21 * S.r21);
        gs2 = mod * (dl02 * S.r02 + dl12 * S.r12 + dl22 * S.r22);
        const float d00 = dl00 * s0, d01 = dl01 * s1, d02 = dl02 * s2;
        const float d10 = dl10 * s0, d11 = dl11 * s1, d12 = dl12 * s2;
        const float d20 = dl20 * s0, d21 = dl21 * s1, d22 = dl22 * s2;
        gqr = 2.f * (-qz * d01 + qy * d02 + qz * d10 - qx * d12 - qy * d20 + qx * d21);
        gqx = 2.f * (qy * d01 + qz * d02 + qy * d10 - 2.f * qx * d11 - qr * d12 + qz * d20 + qr * d21 - 2.f * qx * d22);
        gqy = 2.f * (-2.f * qy * d00 + qx * d01 + qr * d02 + qx * d10 + qz * d12 - qr * d20 + qz * d21 - 2.f * qy * d22);
        gqz = 2.f * (-2.f * qz * d00 - qr * d01 + qx * d02 + qr * d10 - 2.f * qz * d11 + qy * d12 + qx * d20 + qy * d21);
    }
    // a culled Gaussian or one on the floor: g h to its opacity and exactly nothing to anything else
    if (!through) {
        dmx = dmy = dmz = 0.f; gs0 = gs1 = gs2 = gqr = gqx = gqy = gqz = 0.f;
#pragma unroll
        for (int t = 0; t < 6; ++t) gc[t] = 0.f;
    }
    if (i < P) {
        if (g_opac) g_opac[i] = g * f.h;
        if (g_means3D) { g_means3D[3 * (size_t)i] = dmx; g_means3D[3 * (size_t)i + 1] = dmy; g_means3D[3 * (size_t)i + 2] = dmz; }
        if (!COV3D) {
            if (g_scales) { g_scales[3 * (size_t)i] = gs0; g_scales[3 * (size_t)i + 1] = gs1; g_scales[3 * (size_t)i + 2] = gs2; }
            if (g_rot) { g_rot[4 * (size_t)i] = gqr; g_rot[4 * (size_t)i + 1] = gqx; g_rot[4 * (size_t)i + 2] = gqy; g_rot[4 * (size_t)i + 3] = gqz; }
        } else if (g_cov3D) {
#pragma unroll
            for (int t = 0; t < 6; ++t) g_cov3D[6 * (size_t)i + t] = gc[t];
        }
    }
    // ---- wave rows -> the workgroup's slab row, the four waves in wave order
    if (slab) {                                                               // uniform
        __syncthreads();
        if (threadIdx.x < AA_SLAB)
            slab[(size_t)blockIdx.x * AA_SLAB + threadIdx.x] =
                (threadIdx.x < AA_VALS) ? (wpose[0][threadIdx.x] + wpose[1][threadIdx.x]) + (wpose[2][threadIdx.x] + wpose[3][threadIdx.x]) : 0.f;
    }
}

// slab rows -> the three pose tensors, one workgroup per column, summed in double in a fixed order.  The entries of the 4x4
// outputs no Gaussian contributes to (viewmatrix's fourth column, all of intrinsic but k[0] and k[5]) are written as zeros by the
// column next to them.
__global__ void __launch_bounds__(256)
antialias_pose_reduce_kernel(const float* __restrict__ slab, int nblocks, float* __restrict__ g_view, float* __restrict__ g_intr,
                             float* __restrict__ g_shift)
{
    const int t = blockIdx.x;
    const double sum = slab_column_sum(slab, nblocks, AA_SLAB, t);
    if (threadIdx.x != 0) return;
    const float val = (float)sum;
    if (t < 12) {
        if (g_view) { g_view[(t / 3) * 4 + t % 3] = val; if (t % 3 == 2) g_view[(t / 3) * 4 + 3] = 0.f; }
    } else if (t < 14) {
        if (g_intr) {
            g_intr[t == 12 ? 0 : 5] = val;
            if (t == 12) {
#pragma unroll
                for (int e = 0; e < 16; ++e) if (e != 0 && e != 5) g_intr[e] = 0.f;
            }
        }
    } else if (g_shift) g_shift[t - 14] = val;
}

int antialias_blocks(int P) { return cdiv(P > 0 ? P : 1, AA_BLOCK); }

hipError_t launch_antialias_fwd(const BagsAntialias& a, float* out, hipStream_t st)
{
    if (a.P == 0) return hipSuccess;
    return with_bool(a.cov3D_precomp != nullptr, [&](auto COV) {
        hipLaunchKernelGGL((antialias_fwd_kernel<decltype(COV)::value>), dim3(cdiv(a.P, AA_BLOCK)), dim3(AA_BLOCK), 0, st, a.P, a.image_width,
                           a.image_height, a.tanfovx, a.tanfovy, a.scale_modifier, a.means3D, a.scales, a.rotations, a.cov3D_precomp, a.opacities,
                           a.shift_factors, a.viewmatrix, a.intrinsic, out);
        return hipGetLastError(); });
}

// slab: antialias_blocks(P) rows of AA_SLAB floats, or nullptr when none of the three pose outputs is wanted
hipError_t launch_antialias_bwd(const BagsAntialias& a, const float* grad_out, float* slab, float* g_opac, float* g_means3D, float* g_scales,
                                float* g_rot, float* g_cov3D, float* g_view, float* g_intr, float* g_shift, hipStream_t st)
{
    if (a.P == 0) return hipSuccess;
    const int nblocks = cdiv(a.P, AA_BLOCK);
    const hipError_t e = with_bool(a.cov3D_precomp != nullptr, [&](auto COV) {
        hipLaunchKernelGGL((antialias_bwd_kernel<decltype(COV)::value>), dim3(nblocks), dim3(AA_BLOCK), 0, st, a.P, a.image_width, a.image_height,
                           a.tanfovx, a.tanfovy, a.scale_modifier, (a.clamp_grad == BAGS_CLAMP_GRAD_EXACT) ? 0 : 1, a.means3D, a.scales, a.rotations,
                           a.cov3D_precomp, a.opacities, a.shift_factors, a.viewmatrix, a.intrinsic, grad_out, slab, g_opac, g_means3D, g_scales,
                           g_rot, g_cov3D);
        return hipGetLastError(); });
    if (e != hipSuccess || !slab) return e;
    hipLaunchKernelGGL(antialias_pose_reduce_kernel, dim3(AA_VALS), dim3(256), 0, st, slab, nblocks, g_view, g_intr, g_shift);
    return hipGetLastError();
}
