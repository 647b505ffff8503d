// projection.h -- the per-Gaussian chain world point -> view space -> entrance-pupil shift -> clip space, and
// quaternion + scales -> Sigma -> cov2D -> conic, stated ONCE for K1 (preprocess_fwd.hip: k1_project) and K9
// (preprocess_bwd.hip: preprocess_bwd_kernel).  K9 re-derives K1's det, Jacobian and conic bit for bit: both files include
// these statements and both are compiled with -ffp-contract=off, so every expression below is the same sequence of
// individually rounded IEEE fp32 mul/add/div/sqrt, left to right, in both kernels.  Do not re-associate, merge or "simplify"
// one: radius, rectangle, tile mask and depth key must also stay bit-identical to the fp32 oracle, the independent second
// statement of this chain (oracle/raster_oracle.py: preprocess).
// Plain floats in, plain floats out: each caller keeps its own way of loading a Gaussian's rows (K1 from global memory with the
// camera in LDS, K9 from rows prefetched into registers with the camera on scalar loads); v, m are the camera's 4x4 row-vector
// matrices, wherever the caller keeps them.  Conventions: utils/graphics_utils.py:26-33 (row-vector transforms),
// utils/general_utils.py:130-163 (quaternion order, R.S).
#pragma once
#include "bags_common.h"

// view-space point (K1 culls on tz > 0.2f between this and the rest; K9 does not cull)
struct PjView { float tx, ty, tz; };
__device__ __forceinline__ PjView pj_view(const float* v, const float x, const float y, const float z)
{
    PjView r;
    r.tx = x * v[0] + y * v[4] + z * v[8] + v[12];
    r.ty = x * v[1] + y * v[5] + z * v[9] + v[13];
    r.tz = x * v[2] + y * v[6] + z * v[10] + v[14];
    return r;
}

// D2: entrance-pupil shift, a polynomial in theta = atan2(rho, tz) (zero factors => exact identity).  K9's backward of the
// polynomial needs every member.
struct PjShift { float rho, theta, th2, th3, shift, tzs; };
__device__ __forceinline__ PjShift pj_shift(const float tx, const float ty, const float tz, const float sf0, const float sf1, const float sf2)
{
    PjShift r;
    r.rho = sqrtf(tx * tx + ty * ty + 1e-20f);
    r.theta = det_atan2_pos(r.rho, tz);
    r.th2 = r.theta * r.theta;
    r.th3 = r.th2 * r.theta;
    r.shift = sf0 * r.th3 + sf1 * (r.th3 * r.th2) + sf2 * (r.th3 * r.th2 * r.th2);
    r.tzs = tz + r.shift;
    return r;
}

// homogeneous point (the shift enters through the intrinsic's third row: k8 = k[8], k9 = k[9], k11 = k[11]) and 1 / w
struct PjClip { float hx, hy, hw, pw; };
__device__ __forceinline__ PjClip pj_clip(const float* m, const float k8, const float k9, const float k11, const float x, const float y,
                                          const float z, const float shift)
{
    PjClip r;
    r.hx = x * m[0] + y * m[4] + z * m[8] + m[12] + shift * k8;
    r.hy = x * m[1] + y * m[5] + z * m[9] + m[13] + shift * k9;
    r.hw = x * m[3] + y * m[7] + z * m[11] + m[15] + shift * k11;
    r.pw = 1.0f / (r.hw + 1e-7f);
    return r;
}

// quaternion (qr, qx, qy, qz) -> R, L = R S with the already-modified scales, Sigma = L L^T (unique entries c0..c5).  K9's scale
// and quaternion backward needs R.  A precomputed 3D covariance replaces this piece in the callers.
struct PjCov3d { float r00, r01, r02, r10, r11, r12, r20, r21, r22, c0, c1, c2, c3, c4, c5; };
__device__ __forceinline__ PjCov3d pj_cov3d(const float s0, const float s1, const float s2, const float qr, const float qx, const float qy,
                                            const float qz)
{
    PjCov3d r;
    r.r00 = 1.0f - 2.0f * (qy * qy + qz * qz);
    r.r01 = 2.0f * (qx * qy - qr * qz);
    r.r02 = 2.0f * (qx * qz + qr * qy);
    r.r10 = 2.0f * (qx * qy + qr * qz);
    r.r11 = 1.0f - 2.0f * (qx * qx + qz * qz);
    r.r12 = 2.0f * (qy * qz - qr * qx);
    r.r20 = 2.0f * (qx * qz - qr * qy);
    r.r21 = 2.0f * (qy * qz + qr * qx);
    r.r22 = 1.0f - 2.0f * (qx * qx + qy * qy);
    const float l00 = r.r00 * s0, l01 = r.r01 * s1, l02 = r.r02 * s2;
    const float l10 = r.r10 * s0, l11 = r.r11 * s1, l12 = r.r12 * s2;
    const float l20 = r.r20 * s0, l21 = r.r21 * s1, l22 = r.r22 * s2;
    r.c0 = l00 * l00 + l01 * l01 + l02 * l02;
    r.c1 = l00 * l10 + l01 * l11 + l02 * l12;
    r.c2 = l00 * l20 + l01 * l21 + l02 * l22;
    r.c3 = l10 * l10 + l11 * l11 + l12 * l12;
    r.c4 = l10 * l20 + l11 * l21 + l12 * l22;
    r.c5 = l20 * l20 + l21 * l21 + l22 * l22;
    return r;
}

// D1 focal lengths from the intrinsic (k0 = k[0], k5 = k[5]), D8 the 1.3 x field-of-view clamp of t.x / t.z, the EWA Jacobian J,
// A = J W (W = the view matrix's rotation block), B = A Sigma, cov2D = B A^T + 0.3 I.  ux, uy are the CLAMPED ratios: J's third
// column uses t.x = ux tzs; a caller that needs to know whether an axis was clamped compares txtz / tytz with limx / limy.
struct PjCov2d {
    float fx, fy, limx, limy, txtz, tytz, ux, uy, itz, itz2;
    float j00, j02, j11, j12;
    float a00, a01, a02, a10, a11, a12;
    float b00, b01, b02, b10, b11, b12;
    float cxx, cxy, cyy;
};
__device__ __forceinline__ PjCov2d pj_cov2d(const float* v, const float k0, const float k5, const int W, const int H, const float tanfovx,
                                            const float tanfovy, const float tx, const float ty, const float tzs, const float c0,
                                            const float c1, const float c2, const float c3, const float c4, const float c5)
{
    PjCov2d r;
    r.fx = k0 * (0.5f * (float)W);
    r.fy = k5 * (0.5f * (float)H);
    r.limx = 1.3f * tanfovx; r.limy = 1.3f * tanfovy;
    r.txtz = tx / tzs; r.tytz = ty / tzs;
    r.ux = fminf(r.limx, fmaxf(-r.limx, r.txtz));
    r.uy = fminf(r.limy, fmaxf(-r.limy, r.tytz));
    r.itz = 1.0f / tzs;
    r.itz2 = r.itz * r.itz;
    r.j00 = r.fx * r.itz;
    r.j02 = -(r.fx * (r.ux * tzs)) * r.itz2;
    r.j11 = r.fy * r.itz;
    r.j12 = -(r.fy * (r.uy * tzs)) * r.itz2;
    r.a00 = r.j00 * v[0] + r.j02 * v[2];
    r.a01 = r.j00 * v[4] + r.j02 * v[6];
    r.a02 = r.j00 * v[8] + r.j02 * v[10];
    r.a10 = r.j11 * v[1] + r.j12 * v[2];
    r.a11 = r.j11 * v[5] + r.j12 * v[6];
    r.a12 = r.j11 * v[9] + r.j12 * v[10];
    r.b00 = r.a00 * c0 + r.a01 * c1 + r.a02 * c2;
    r.b01 = r.a00 * c1 + r.a01 * c3 + r.a02 * c4;
    r.b02 = r.a00 * c2 + r.a01 * c4 + r.a02 * c5;
    r.b10 = r.a10 * c0 + r.a11 * c1 + r.a12 * c2;
    r.b11 = r.a10 * c1 + r.a11 * c3 + r.a12 * c4;
    r.b12 = r.a10 * c2 + r.a11 * c4 + r.a12 * c5;
    r.cxx = r.b00 * r.a00 + r.b01 * r.a01 + r.b02 * r.a02 + 0.3f;
    r.cxy = r.b00 * r.a10 + r.b01 * r.a11 + r.b02 * r.a12;
    r.cyy = r.b10 * r.a10 + r.b11 * r.a11 + r.b12 * r.a12 + 0.3f;
    return r;
}

// det of cov2D, its reciprocal and the conic (cyy, -cxy, cxx) / det.  K1 culls on det != 0 (and stores nothing of a culled
// Gaussian); K9's choice between the stock and the exact derivative of the inverse stays in K9.
struct PjConic { float det, det_inv, con_a, con_b, con_c; };
__device__ __forceinline__ PjConic pj_conic(const float cxx, const float cxy, const float cyy)
{
    PjConic r;
    r.det = cxx * cyy - cxy * cxy;
    r.det_inv = 1.0f / r.det;
    r.con_a = cyy * r.det_inv; r.con_b = -cxy * r.det_inv; r.con_c = cxx * r.det_inv;
    return r;
}
