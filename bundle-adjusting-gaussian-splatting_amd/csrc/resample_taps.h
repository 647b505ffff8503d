// resample_taps.h -- what resample.hip (one image) and resample_faces.hip (a cubemap's faces) state once: the geometry of a warp,
// the upsampling taps of the control flow, the sampling taps of an image, and the tile constants of the backward's lists.
#pragma once
#include "bags_common.h"

struct ResampleGeom {
    int C, H, W;          // image
    int h, w;             // control grid of the flow
    int Hf, Wf;           // size the flow is upsampled to (= size of the warped image before the crop)
    int Hc, Wc;           // centre crop
    int y0, x0;           // crop origin inside (Hf, Wf)
};

static inline ResampleGeom make_geom(int C, int H, int W, int h, int w, int Hf, int Wf, int Hc, int Wc)
{
    ResampleGeom g{C, H, W, h, w, Hf, Wf, Hc, Wc, (Hf - Hc) / 2, (Wf - Wc) / 2};
    return g;
}

struct FlowTap { int i00, i01, i10, i11; float w00, w01, w10, w11; };

// bilinear upsampling source taps of F.interpolate(align_corners=False) at destination (Y, X)
__device__ __forceinline__ FlowTap flow_taps(const ResampleGeom& g, int Y, int X)
{
    const float sy = fmaxf(((float)Y + 0.5f) * ((float)g.h / (float)g.Hf) - 0.5f, 0.f);
    const float sx = fmaxf(((float)X + 0.5f) * ((float)g.w / (float)g.Wf) - 0.5f, 0.f);
    const int y0 = min((int)sy, g.h - 1), x0 = min((int)sx, g.w - 1);
    const int y1 = y0 + (y0 < g.h - 1), x1 = x0 + (x0 < g.w - 1);
    const float ly = sy - (float)y0, lx = sx - (float)x0;
    FlowTap t;
    t.i00 = y0 * g.w + x0; t.i01 = y0 * g.w + x1; t.i10 = y1 * g.w + x0; t.i11 = y1 * g.w + x1;
    t.w00 = (1.f - ly) * (1.f - lx); t.w01 = (1.f - ly) * lx; t.w10 = ly * (1.f - lx); t.w11 = ly * lx;
    return t;
}

struct ImgTap { int x0, y0; float fx, fy; bool in00, in01, in10, in11; };

// grid_sample(align_corners=True, zeros padding) taps for the normalised coordinate (gx, gy)
__device__ __forceinline__ ImgTap img_taps(const ResampleGeom& g, float gx, float gy)
{
    const float ix = (gx + 1.f) * 0.5f * (float)(g.W - 1), iy = (gy + 1.f) * 0.5f * (float)(g.H - 1);
    const float fx0 = floorf(ix), fy0 = floorf(iy);
    ImgTap t;
    // far-away coordinates (|ix| beyond int range) are simply out of bounds
    t.x0 = (fx0 > -2.f && fx0 < (float)g.W + 1.f) ? (int)fx0 : -2;
    t.y0 = (fy0 > -2.f && fy0 < (float)g.H + 1.f) ? (int)fy0 : -2;
    t.fx = ix - fx0; t.fy = iy - fy0;
    const bool xa = t.x0 >= 0 && t.x0 < g.W, xb = t.x0 + 1 >= 0 && t.x0 + 1 < g.W;
    const bool ya = t.y0 >= 0 && t.y0 < g.H, yb = t.y0 + 1 >= 0 && t.y0 + 1 < g.H;
    t.in00 = xa && ya; t.in01 = xb && ya; t.in10 = xa && yb; t.in11 = xb && yb;
    if (!isfinite(ix) || !isfinite(iy)) { t.in00 = t.in01 = t.in10 = t.in11 = false; t.fx = t.fy = 0.f; }
    return t;
}

// The backward's lists: dL/dimage is accumulated per RS_TILE x RS_TILE SOURCE tile from the output tiles listed on it; a list
// holds RS_CAP output tiles, a longer one is not read (the gather tests every output tile's box instead: slow, exact).
#define RS_TILE 16
#define RS_CAP 32

// A term w * go of a tile's sum as a 64-bit fixed-point integer: `up` = 2^(24 - e) with the tile's largest |dL/dout| < 2^e, so that
// |x| < 2^24 and its integer part fits an int32; 24 more fractional bits; then 2^(shift - 24).  Every step is exact.
__device__ __forceinline__ unsigned long long rs_fixed(float v, float up, int shift)
{
    const float x = v * up;
    const int hi = (int)x;
    const int lo = (int)((x - (float)hi) * 16777216.0f);
    const long long fx = shift >= 24 ? (((long long)hi << 24) + (long long)lo) << (shift - 24)
                                     : (((long long)hi << 24) + (long long)lo) >> (24 - shift);
    return (unsigned long long)fx;
}
