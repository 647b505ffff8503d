// Shared host/device declarations of libbags_raster.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "../../include/bags_raster.h"

typedef uint32_t u32;
typedef uint64_t u64;

#define BAGS_WAVE 64
#define RADIX_BITS 8
#define RADIX_BINS 256
#define SORT_BLOCK 256
#ifndef SORT_ITEMS
#define SORT_ITEMS 8                      // keys per thread per radix pass (large inputs)
#endif
#ifndef SORT_ITEMS_SMALL
#define SORT_ITEMS_SMALL 4                // ... for inputs up to 2M keys
#endif
#define SCAN_BLOCK 256
#define SCAN_ITEMS 8
#define SCAN_TILE (SCAN_BLOCK * SCAN_ITEMS)   // 2048 offsets per workgroup
#ifndef PART_FLOATS
#define PART_FLOATS 12
#endif                                    // one 48-byte partial-gradient record per sorted instance (11 sums), densely packed:
                                          // every byte of every line is written, and K8a streams 25 % less than with 64-B slots
#define POSE_VALS 40                      // pose-gradient slab row (35 used)
#define KEY_CULLED 0xFFFFFFFFu

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
static inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }
static inline int bit_length(u32 v) { int b = 0; while (v) { ++b; v >>= 1; } return b; }

// theta = atan2(rho, tz) for rho >= 0, tz > 0 from operations every IEEE implementation rounds identically (min / max / div /
// mul / add, no libm call), so that the depth keys and tile rectangles stay bit-comparable with the fp32 oracle when the
// shift_factors polynomial is non-zero (oracle/raster_oracle.py: _atan2_pos repeats the sequence in torch).  Both callers are
// compiled with -ffp-contract=off.  u = min/max in [0,1]; above tan(pi/8) it is folded with atan(u) = pi/4 + atan((u-1)/(u+1));
// |w| <= tan(pi/8): atan(w) = w + w (s P(s)), s = w^2, P fitted to 6e-8 relative (fp32 rounding level).
__device__ __forceinline__ float det_atan2_pos(float rho, float tz)
{
    const float lo = fminf(rho, tz), hi = fmaxf(rho, tz);
    const float u = lo / hi;
    const bool red = u > 0.414213568f;
    const float w = red ? (u - 1.0f) / (u + 1.0f) : u;
    const float s = w * w;
    float p = -0.0607120693f;
    p = p * s + 0.105907366f;
    p = p * s + -0.142430589f;
    p = p * s + 0.199984416f;
    p = p * s + -0.333333135f;
    float a = w + w * (s * p);
    if (red) a = 0.785398185f + a;
    return (rho > tz) ? 1.57079637f - a : a;
}

// (the ordered sums -- wave_total_f, slab_column_sum and the double sums of the losses -- are in ordered_sum.h)

// ---- tile masks of small rectangles (GeomView::keep) ------------------------------------------------------
// A rectangle of at most 8 x 8 tiles carries a 64-bit mask of the tiles it emits, bit ry * 8 + rx; a larger one emits all.
__device__ __forceinline__ bool rect_small(int w, int h) { return w <= 8 && h <= 8; }
__device__ __forceinline__ u64 rect_full_mask(int w, int h)
{
    if (w <= 0 || h <= 0) return 0ull;
    if (!rect_small(w, h)) return ~0ull;
    return ((1ull << w) - 1ull) * (0x0101010101010101ull >> (8 * (8 - h)));
}
// rank of tile (rx, ry) among the emitted tiles of its Gaussian = index of its partial-gradient record
__device__ __forceinline__ u32 rect_tile_rank(u64 keep, int w, int h, int rx, int ry)
{
    return rect_small(w, h) ? (u32)__popcll(keep & ((1ull << (ry * 8 + rx)) - 1ull)) : (u32)(ry * w + rx);
}
// position (ry * 8 + rx) of the n-th emitted tile of a small rectangle
__device__ __forceinline__ int rect_nth_tile(u64 keep, u32 n)
{
    for (u32 i = 0; i < n; ++i) keep &= keep - 1ull;
    return __ffsll((long long)keep) - 1;
}

// ---- carving of the caller-owned buffers ------------------------------------------------------------------
// Every buffer the library works in is the caller's.  ONE layout function per buffer walks a Carver over it, fills a plain view
// struct and returns used(); the buffer's size function is the same walk over a null base (sizing mode: the pointers it hands
// out are never dereferenced) plus the buffer's slack, so a size and its layout cannot drift apart.
struct Carver {
    size_t base, pos;
    // round_base: start at the next multiple of 256 (the buffer's size then carries BASE_SLACK); false: the base as given
    explicit Carver(const void* b, bool round_base = true)
        : base(round_base ? align_up(reinterpret_cast<size_t>(b), 256) : reinterpret_cast<size_t>(b)), pos(base) {}
    // `count` elements of T; the next region starts 256 bytes aligned again
    template <typename T> T* take(size_t count) { T* out = reinterpret_cast<T*>(pos); pos += align_up(count * sizeof(T), 256); return out; }
    size_t used() const { return pos - base; }                // bytes handed out so far
};
static const size_t BASE_SLACK = 256;     // what rounding the caller's pointer up to 256 can cost (it costs at most 255)

// ---- carved views of the caller-owned state buffers (api.hip: carve_geom / _binning / _image / _backward) -----
struct GeomView {            // per Gaussian, indexed by Gaussian id unless stated
    u32*    depth_key;       // float bits of the sort depth, KEY_CULLED when not rendered
    // One 64-byte line per Gaussian with everything the blend kernels gather per (tile, Gaussian) instance, so an
    // instance costs ONE line fetch instead of five partial ones from id-ordered (spatially random) SoA arrays:
    //   q0 = conic a, b, c, opacity      q1 = pixel x, y, colour r, g
    //   q2 = colour b, view depth z, rect.x, rect.y (bits)      q3 = keep lo, block of Gaussians, offset inside the block, keep hi (bits)
    float4* g2d;             // [4 * P]
    u32*    inst_off;        // [P] first emission slot of the Gaussian's partial-gradient records -- RADIX PATH ONLY since round 4 (an array
                             // of its own: a 4-byte write into every 64-byte line of g2d after the scan cost 6.6 us per frame).  On the
                             // tile-binned path the record base is block_base[block] + local_off, both known to K1 (line.q3.y / q3.z)
    uint2*  rect;            // (minx | miny<<16, maxx | maxy<<16), max exclusive   (compact copy for emit)
    u32*    tiles_touched;   // instances the Gaussian emits (compact copy for the offsets scan / emit)
    u32*    rec_count;       // partial-gradient records of the Gaussian (= tiles_touched, except on the tile-binned path with the stock tile
                             // rule: there only the tiles the opacity rule keeps have a record, round 4)
    // [10 * P] d(colour)/d(view direction) of the SH colour path, written by K1 for the visible Gaussians (round 3):
    //   M[axis][c] = sum_t (d basis_t / d dir_axis) * sh[t][c]   as   Mxr Mxg Mxb  Myr Myg Myb  Mzr Mzg Mzb, then the clamp bits
    // so that preprocess_bwd reads 40 bytes per Gaussian instead of the 192-byte SH row a second time (and nothing of g2d)
    float*  shjac;
    u64*    keep;            // tile mask of a rectangle of at most 8 x 8 tiles: bit ry * 8 + rx set = tile (minx + rx, miny + ry)
                             // is emitted (D7: the alpha >= 1/255 ellipse reaches it); larger rectangles emit every tile
    // scratch (dead after forward)
    u32 *keys_a, *keys_b, *vals_a, *vals_b;   // depth ordering of Gaussians (ping-pong)
    u32*    rank_offset;     // exclusive instance offset per depth rank
    u32*    scan_partials;
    u32*    radix_hist;      // [256][nblocks]
    u32*    digit_totals;    // [256]
    u32*    num_rendered;    // [0] instance count; [2..3] device-visible address of the caller's pinned count word (or 0); [8..] debug counters
    // tile-binned path (binning.hip)
    u32*    local_off;       // [P] instance offset of a Gaussian inside its block of Gaussians (id order)
    u32*    block_total;     // [256] instances per block
    u32*    block_base;      // [256] exclusive scan of block_total
    int     nblocks_sort;    // radix workgroups for P keys
    int     nblocks_scan;
};
struct BinView {
    u32 *keys_a, *keys_b, *vals_a, *vals_b;   // tile id / Gaussian id per instance (ping-pong)
    uint2*  ranges;          // [T]
    u32*    radix_hist;
    u32*    digit_totals;
    int     nblocks_sort;
    int     passes;          // radix passes over the tile id
    u32*    point_list;      // vals after the last pass (radix path) / the per-tile sorted ids (tile-binned path)
    u32*    tile_sorted;     // keys after the last pass (radix path only)
    u64*    words;           // tile-binned path: (depth key << 32 | Gaussian id) per instance, grouped by tile, unsorted inside a tile
    u64*    scratch;         // tile-binned path: scratch of the two-level / global-memory sorts (lists of > 4096 entries only)
    // A 32-bit word per sorted instance -- bits 0..15 the reach mask of the tile's 4x4-pixel blocks, bit 16 "has a gradient record" --
    // written by blend_fwd when it stages the instance, read back by blend_bwd instead of evaluating block_mask16 again.  Lives in
    // memory that is dead once the lists are sorted: the radix path's spare key buffer (instance i: word i), or -- tile-binned path --
    // the tile's OWN slice of `words` (instance j of a tile that starts at instance s: byte 8 s + 4 j; blend_fwd sorts its tile's
    // list itself, so other tiles' words may still be unsorted when it writes; the second half of the slice holds the compacted
    // positions of the record holders, stock tile rule).
    unsigned short* reach_mask;
};
struct ImgView {
    float* final_T;          // [H*W]
    u32*   n_contrib;        // [H*W]
    // [tiles] the tiles heavy-first by instance count: {tile, first instance, instance count, deepest contributor}.
    // x,y,z by tile_order_kernel, w by blend_fwd; decides which workgroup of a blend launch takes which tile.
    uint4* tile_desc;
    u32*   n_active;         // [1] tiles that hold at least one instance (they come first in tile_desc)
    uint4* tile_aux;         // [tiles] by descriptor slot, stock tile rule on the tile-binned path only (blend_fwd -> blend_bwd):
                             // {record-holding instances in front of the deepest contributor, record-holding instances staged,
                             //  list positions staged, -}
    // tile-binned path (binning.hip): (block of Gaussians, tile) instance counts and their prefix over the blocks
    u32*   cnt_rows;         // [256][(T+1)/2] packed 16-bit counters
    u32*   pre;              // [256][T]
    u32*   tile_total;       // [T]
    uint2* ranges;           // [T]
    u32*   tile_lstart;      // [T] first instance of a tile relative to its group of 64 tiles (tile_prefix_kernel)
    u32*   group_total;      // [512] instances per group of 64 tiles
};
struct BwdWorkView {         // the backward workspace
    float* partials;         // [I] one record of PART_FLOATS floats per sorted instance (blend_bwd -> preprocess_bwd)
    float* pose_slab;        // [ceil(P / 256)] rows of POSE_VALS (preprocess_bwd -> pose_reduce)
    unsigned char* live_map; size_t live_bytes;   // dense-scene mode: one byte per record; the bytes launch_blend_bwd clears
};

// ---- kernel launches that can carry the stage profiler's events ON THEIR OWN DISPATCH (hipExtLaunchKernelGGL: the timestamps of the
// kernel's completion signal) instead of between two hipEventRecord packets.  The profiler (api.hip: ProfScope) parks a start / stop pair
// in these two thread-local words right before it calls a launcher whose stage is ONE kernel; the first LAUNCH_K of that launcher takes
// them.  Without a pair parked this is hipLaunchKernelGGL.
#include <hip/hip_ext.h>
extern thread_local hipEvent_t g_attach_start, g_attach_stop;
template <typename... KArgs, typename... Args>
static inline void launch_k(void (*kernel)(KArgs...), dim3 grid, dim3 block, size_t lds, hipStream_t st, Args... args)
{
    if (g_attach_start || g_attach_stop) {
        hipEvent_t ea = g_attach_start, eb = g_attach_stop;
        g_attach_start = nullptr; g_attach_stop = nullptr;
        hipExtLaunchKernelGGL(kernel, grid, block, (std::uint32_t)lds, st, ea, eb, 0, static_cast<KArgs>(args)...);
    } else {
        hipLaunchKernelGGL(kernel, grid, block, lds, st, static_cast<KArgs>(args)...);
    }
}
#define LAUNCH_K(kernel, grid, block, lds, st, ...) launch_k(kernel, grid, block, lds, st, __VA_ARGS__)
// a run-time bool as a compile-time one: f(std::true_type{}) or f(std::false_type{}); nested, it picks a kernel's template instance
template <typename F> static inline auto with_bool(bool b, F f) { return b ? f(std::true_type{}) : f(std::false_type{}); }

int radix_items_for(long long n);
int radix_blocks_for(long long n);

// ---- launchers (each enqueues on `st`; returns hipError_t) --------------------------------------------------
// count_into != nullptr (tile-binned path): K1 also counts the (block of Gaussians, tile) matrix and the block-local instance
// offsets (step 1 of binning.hip), grid_x = tiles per image row
hipError_t launch_preprocess_fwd(const BagsSettings& s, const BagsInputs& in, const GeomView& g, int32_t* radii,
                                 float* mean2D, hipStream_t st, const ImgView* count_into = nullptr, int grid_x = 0);
hipError_t launch_radix_sort(const u32* src_k, const u32* src_v, u32* a_k, u32* a_v, u32* b_k, u32* b_v, long long n,
                             int bits, bool iota_vals, u32* hist, u32* totals, int nblocks, hipStream_t st,
                             const u32* n_dev = nullptr);
hipError_t launch_offsets_scan(const GeomView& g, const u32* sorted_ids, int P, hipStream_t st);
hipError_t launch_emit(const GeomView& g, const u32* sorted_ids, int P, int grid_x, u32* keys, u32* vals, u32 capacity,
                       hipStream_t st, const u32* n_dev, uint2* ranges, int T);
hipError_t launch_tile_ranges(const u32* tile_sorted, long long I, uint2* ranges, int T, hipStream_t st,
                              const u32* n_dev, bool cleared);
hipError_t launch_tile_order(const uint2* ranges, int T, uint4* tile_desc, u32* n_active, hipStream_t st);
hipError_t launch_blend_fwd(const BagsSettings& s, const GeomView& g, const BinView& b, const ImgView& im,
                            const BagsForwardOut& out, hipStream_t st, const u32* n_dev = nullptr, u32 capacity = 0, bool sort_here = false);
// binned: the record base of a Gaussian is block_base[line.q3.y] + line.q3.z (K1 wrote both into the geometry line); otherwise
// (radix path) it is gathered from g.inst_off
hipError_t launch_blend_bwd(const BagsSettings& s, const GeomView& g, const BinView& b, const ImgView& im,
                            const float* grad_color, float* partials, bool want_abs, bool binned, hipStream_t st,
                            long long n_records = 0,                      // instance count
                            unsigned char* live_map = nullptr,            // one byte per record (dense-scene mode: the caller's decision), or null
                            size_t live_bytes = 0,                        // ... and the bytes of it to clear (BwdWorkView::live_bytes)
                            hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr,   // attached to the kernel's dispatch when given
                            const float* grad_depth = nullptr, const float* grad_weights = nullptr);   // BagsExtraGrads (ABI 11)
bool bwd_dense_mode(long long n_records, int T, int dense_per_tile);      // does a backward of this size run in dense-scene mode?
// extra: the records carry dL/dz in their twelfth float (blend_bwd ran with BagsExtraGrads): it is summed and added to dL/dtzs
hipError_t launch_preprocess_bwd(const BagsSettings& s, const BagsInputs& in, const GeomView& g, const float* partials, float* pose_slab,
                                 int* nblocks_out, const BagsBackwardArgs& a, hipStream_t st, bool binned,
                                 const unsigned char* live_map = nullptr, bool extra = false);
hipError_t launch_pose_reduce(const float* pose_slab, int nblocks, const BagsBackwardArgs& a, hipStream_t st);
hipError_t launch_sh_grad_from_views(int P, int M, int deg, const float* means3D, const BagsShViews& views, float* g_shs, float* g_shs_rest,
                                     int accumulate, hipStream_t st);
// loss.hip: fused L1 + SSIM terms and their image gradient
size_t loss_workspace_bytes(int C, int H, int W);
hipError_t launch_loss_fwd(const float* img, const float* gt, int C, int H, int W, void* ws, float* out_terms, hipStream_t st,
                           bool combined = false, float lambda_dssim = 0.f);
hipError_t launch_loss_bwd(const float* img, const float* gt, int C, int H, int W, const void* ws, const float* grad_terms,
                           float* grad_img, hipStream_t st, bool combined = false, float lambda_dssim = 0.f);
// camera.hip: pose leaves -> viewmatrix / projmatrix / intrinsic / campos, and the adjoint
hipError_t launch_camera_fwd(const float* q0, const float* dq, const float* t0, const float* dt, const float* fovx, const float* fovy,
                             const float* grot, const float* gscale, float znear, float zfar,
                             float* V, float* M, float* K, float* C, hipStream_t st);
hipError_t launch_camera_bwd(const float* q0, const float* dq, const float* t0, const float* dt, const float* fovx, const float* fovy,
                             const float* grot, const float* gscale, float znear, float zfar,
                             const float* gV, const float* gM, const float* gK, const float* gC,
                             float* g_dq, float* g_dt, float* g_fovx, float* g_fovy, float* g_grot, float* g_gscale, hipStream_t st);
hipError_t launch_pose_bank_fwd(const BagsPoseBank& bank, float* V, float* M, float* K, float* C, hipStream_t st);
hipError_t launch_pose_bank_bwd(const BagsPoseBank& bank, const float* gV, const float* gM, const float* gK, const float* gC,
                                float* grad_leaves, float* g_grot, float* g_gscale, hipStream_t st);
// resample.hip: flow upsample + grid_sample + centre crop + mask in one pass, and the adjoint
hipError_t launch_resample_fwd(const float* image, int C, int H, int W, const float* ctrl, int h, int w, int Hf, int Wf, int Hc, int Wc,
                               float* out, float* mask, float* flow_out, hipStream_t st);
hipError_t launch_resample_bwd(const float* image, int C, int H, int W, const float* ctrl, int h, int w, int Hf, int Wf, int Hc, int Wc,
                               const float* grad_out, void* workspace, float* grad_image, float* grad_ctrl, hipStream_t st);
size_t resample_workspace_bytes(int H, int W, int Hc, int Wc);
hipError_t launch_resample_ctrl_gather(int h, int w, int Hf, int Wf, int Hc, int Wc, const float2* gflow, float* grad_ctrl, hipStream_t st);
// resample_faces.hip: the same warp from the F faces of a cubemap, stitched (first valid face per pixel), and the adjoint
hipError_t launch_resample_faces_fwd(const BagsFaces& f, const float* ctrl, int h, int w, int Hf, int Wf, int Hc, int Wc, float* out,
                                     int8_t* face_index, hipStream_t st);
hipError_t launch_resample_faces_bwd(const BagsFaces& f, const float* ctrl, int h, int w, int Hf, int Wf, int Hc, int Wc,
                                     const int8_t* face_index, const float* grad_out, void* workspace, float* const* grad_faces,
                                     float* grad_ctrl, hipStream_t st);
size_t resample_faces_workspace_bytes(int F, int H, int W, int Hc, int Wc);
// activations.hip: cat / sigmoid / exp / normalize of the raw Gaussian parameters, and the adjoint; filter (P): the same with the 3D
// smoothing filter applied to the scales and the opacity
hipError_t launch_activations_fwd(int P, int K, const float* dc, const float* rest, const float* opacity, const float* scaling,
                                  const float* rotation, float* shs, float* o_opacity, float* o_scales, float* o_rot, hipStream_t st,
                                  const float* filter = nullptr);
hipError_t launch_activations_bwd(int P, int K, const float* dc, const float* rest, const float* opacity, const float* scaling,
                                  const float* rotation, const float* g_shs, const float* g_opacity, const float* g_scales,
                                  const float* g_rot, float* g_dc, float* g_rest, float* g_opacity_raw, float* g_scaling,
                                  float* g_rotation, hipStream_t st, const float* filter = nullptr);
// filter3d.hip: the 3D smoothing filter of a Gaussian set under N cameras; dist: P floats, partials: filter3d_blocks(P) floats
// (carve_filter3d in api.hip)
int filter3d_blocks(int P);
hipError_t launch_filter3d(const float* xyz, int P, const float* viewmatrices, const float* intrinsics, const int32_t* sizes, int N,
                           float variance, float* dist, float* partials, float* out, hipStream_t st);
// sh_colors.hip: SH -> RGB of the Python colour path (view direction, basis, +0.5, clamp at 0), and the adjoint; slab: SH_SLAB floats per
// workgroup of 256 Gaussians (carve_sh_colors in api.hip)
#define SH_SLAB 4
hipError_t launch_sh_colors_fwd(const BagsShColors& a, float* rgb, hipStream_t st);
hipError_t launch_sh_colors_bwd(const BagsShColors& a, const float* g_rgb, float* slab, float* g_shs, float* g_shs_rest, float* g_xyz,
                                float* g_campos, hipStream_t st);
// ... and the V views of one step in one pass each way; slab: V x SH_SLAB floats per workgroup, view-major (carve_sh_colors_views)
hipError_t launch_sh_colors_views_fwd(const BagsShColorsViews& a, float* const* rgb, hipStream_t st);
hipError_t launch_sh_colors_views_bwd(const BagsShColorsViews& a, const float* const* g_rgb, float* slab, float* g_shs, float* g_shs_rest,
                                      float* g_xyz, float* const* g_campos, hipStream_t st);
// adam.hip: torch.optim.Adam step of up to BAGS_ADAM_MAX_GROUPS parameter groups (+ densification statistics) in one launch
hipError_t launch_adam(const BagsAdamArgs& args, const BagsDensifyStats* stats, hipStream_t st);
hipError_t launch_pose_adam(const BagsPoseAdamArgs& args, hipStream_t st);
// densify.hip: densify-and-prune (decide + scan, then map + gather) and the opacity reset
size_t densify_workspace_bytes(int P);
hipError_t launch_densify_plan(const BagsDensifyRule& r, void* workspace, u32 host_totals[5], hipStream_t st);
hipError_t launch_densify_apply(const BagsDensifyRule& r, const BagsDensifyGroup* groups, int n_groups, void* workspace, long long P_new,
                                float* accum_out, float* denom_out, float* radii_out, int32_t* provenance, hipStream_t st);
hipError_t launch_reset_opacity(float* opacity, float* exp_avg, float* exp_avg_sq, int P, float cap, hipStream_t st);
// mcmc.hip: compute_relocation, relocate / add_new of the MCMC strategy (count + stage, then one copy pass) and the SGLD noise step
size_t mcmc_workspace_bytes(int P);
hipError_t launch_compute_relocation(const float* opacity_old, const float* scale_old, const int32_t* N, const float* binoms, int n_max, int P,
                                     float* opacity_new, float* scale_new, hipStream_t st);
hipError_t launch_mcmc_relocate(const BagsMcmcGroup* groups, int n_groups, int P, const int32_t* dead, const int32_t* sampled, int n_sampled,
                                const float* binoms, int n_max, double min_opacity, void* workspace, hipStream_t st);
hipError_t launch_mcmc_add_new(const BagsMcmcGroup* groups, int n_groups, int P, const int32_t* sampled, int n_sampled, const float* binoms,
                               int n_max, double min_opacity, void* workspace, float* accum_out, float* denom_out, float* radii_out, hipStream_t st);
hipError_t launch_mcmc_noise(float* xyz, const float* opacity, const float* scaling, const float* rotation, int P, const float* noise, uint64_t seed,
                             double scale, double k, double x0, double scaling_modifier, hipStream_t st);
// antialias.hip: the mip filter's opacity scale in front of the operator, and its adjoint; slab: antialias_blocks(P) rows of AA_SLAB
// floats (17 used), or nullptr when no pose gradient is wanted (carve_antialias in api.hip)
#define AA_SLAB 20
int antialias_blocks(int P);
hipError_t launch_antialias_fwd(const BagsAntialias& a, float* out, hipStream_t st);
hipError_t launch_antialias_bwd(const BagsAntialias& a, const float* grad_out, float* slab, float* g_opac, float* g_means3D, float* g_scales,
                                float* g_rot, float* g_cov3D, float* g_view, float* g_intr, float* g_shift, hipStream_t st);
// appearance.hip: per-camera vignetting and exposure on the V images of a step, and the adjoint; partials: n_rows *
// appearance_slots(H, W) rows of 16 doubles, or nullptr when g_table is not wanted (carve_appearance in api.hip)
int appearance_slots(int H, int W);
// depth_prior.hip: the Pearson / L1 depth prior on the V views of a step; partials: n_rows * depth_prior_slots(H, W) rows of 8
// doubles (carve_depth_prior in api.hip); stats (n_rows,8) goes from the forward to the backward
int depth_prior_slots(int H, int W);
hipError_t launch_depth_prior_fwd(const BagsDepthPrior& a, double* partials, float* loss, float* count, double* stats, hipStream_t st);
hipError_t launch_depth_prior_bwd(const BagsDepthPrior& a, const double* stats, const float* g_loss, float* const* g_depth,
                                  float* const* g_weights, float* g_table, hipStream_t st);
// normal_prior.hip: the normals of the rendered depth held to a prior, on the V views of a step; partials: n_rows *
// normal_prior_tiles(H, W) rows of 2 doubles (carve_normal_prior in api.hip); stats (n_rows,2) goes from the forward to the backward
long long normal_prior_tiles(int H, int W);
hipError_t launch_normal_prior_fwd(const BagsNormalPrior& a, double* partials, float* loss, float* count, double* stats, hipStream_t st);
hipError_t launch_normal_prior_bwd(const BagsNormalPrior& a, const double* stats, const float* g_loss, float* const* g_depth,
                                   float* const* g_weights, hipStream_t st);
hipError_t launch_depth_to_normal(const float* depth, const float* weights, int H, int W, const double* pinhole, float min_weight, float max_jump,
                                  float* normal, uint8_t* valid, hipStream_t st);
// correspondence.hip: the reprojection of matched pixels on the ordered pairs of a step; partials: n_rows *
// correspondence_chunks(H, W) rows of 2 doubles forward, 12 doubles backward (carve_correspondence in api.hip); stats (n_rows,2)
long long correspondence_chunks(int H, int W);
hipError_t launch_correspondence_fwd(const BagsCorrespondence& a, double* partials, float* loss, float* count, double* stats, hipStream_t st);
hipError_t launch_correspondence_bwd(const BagsCorrespondence& a, const double* stats, const float* g_loss, double* sums, float* const* g_depth,
                                     float* const* g_weights, float* const* g_view_src, float* const* g_view_dst, hipStream_t st);
hipError_t launch_reproject_pixels(const BagsCorrespondence& a, int H_dst, int W_dst, float* proj, uint8_t* valid, hipStream_t st);
// warp.hip: the photometric reprojection of a view's pixels into another view's image on the ordered pairs of a step; partials and
// stats as correspondence.hip's, with the same correspondence_chunks(H, W) rows per pair (carve_correspondence in api.hip)
hipError_t launch_warp_fwd(const BagsWarp& a, double* partials, float* loss, float* count, double* stats, hipStream_t st);
hipError_t launch_warp_bwd(const BagsWarp& a, const double* stats, const float* g_loss, double* sums, float* const* g_depth, float* const* g_weights,
                           float* const* g_view_src, float* const* g_view_dst, hipStream_t st);
hipError_t launch_warp_image(const BagsWarp& a, float* out, uint8_t* valid, hipStream_t st);
// gaussian_normals.hip: the shortest axis of every Gaussian in the camera frame of V views, and its adjoint; slab:
// gaussian_normals_blocks(P) rows of GN_SLAB_PER_VIEW * V floats, or nullptr when no view-matrix gradient is wanted
// (carve_gaussian_normals in api.hip)
#define GN_SLAB_PER_VIEW 9
int gaussian_normals_blocks(int P);
hipError_t launch_gaussian_normals_fwd(const BagsGaussianNormals& a, float* const* out, hipStream_t st);
hipError_t launch_gaussian_normals_bwd(const BagsGaussianNormals& a, const float* const* grad_out, float* slab, float* g_rot,
                                       float* const* g_view, hipStream_t st);
// normal_map.hip: a rendered normal map held to a target on the V views of a step; partials: n_rows * depth_prior_slots(H, W) rows of
// 2 doubles (carve_normal_map in api.hip); stats (n_rows,2) goes from the forward to the backward
hipError_t launch_normal_map_fwd(const BagsNormalMap& a, double* partials, float* loss, float* count, double* stats, hipStream_t st);
hipError_t launch_normal_map_bwd(const BagsNormalMap& a, const double* stats, const float* g_loss, float* const* g_normal, hipStream_t st);
// alpha.hip: the weights map held to a target, or its entropy, on the V views of a step; partials: BAGS_MAX_POSE_ROWS *
// BAGS_ALPHA_GROUPS rows of 2 doubles, a constant (api.hip checks BAGS_ALPHA_WORKSPACE_BYTES); stats (n_rows,2) goes from the
// forward to the backward
hipError_t launch_alpha_fwd(const BagsAlpha& a, double* partials, float* loss, float* count, double* stats, hipStream_t st);
hipError_t launch_alpha_bwd(const BagsAlpha& a, const double* stats, const float* g_loss, float* const* g_weights, hipStream_t st);
// smooth.hip: the edge-aware smoothness of the depth / weights maps or of a normal map on the V views of a step; partials: n_rows *
// smooth_tiles(H, W) rows of 6 doubles, mean_rows: n_rows * smooth_mean_slots(H, W) rows of 2 doubles (carve_smooth in api.hip);
// stats (n_rows,8) goes from the forward to the backward
long long smooth_tiles(int H, int W);
int smooth_mean_slots(int H, int W);
hipError_t launch_smooth_fwd(const BagsSmooth& a, double* partials, double* mean_rows, float* loss, float* count, double* stats, hipStream_t st);
hipError_t launch_smooth_bwd(const BagsSmooth& a, const double* stats, const float* g_loss, float* const* g_field, float* const* g_weights,
                             hipStream_t st);
// gaussian_reg.hip: the six regularisers on the raw _opacity / _scaling leaves; records: gaussian_reg_records(P) records of 8 doubles
// (carve_gaussian_reg in api.hip); stats (8) goes from the forward to the backward
int gaussian_reg_records(int P);
hipError_t launch_gaussian_reg_fwd(const BagsGaussianReg& a, double* records, float* terms, float* count, double* stats, hipStream_t st);
hipError_t launch_gaussian_reg_bwd(const BagsGaussianReg& a, const double* stats, const float* g_terms, float* g_opacity, float* g_scaling,
                                   hipStream_t st);
hipError_t launch_appearance_fwd(const BagsAppearance& a, hipStream_t st);
hipError_t launch_appearance_bwd(const BagsAppearance& a, const float* const* g_out, double* partials, float* const* g_image, float* g_table,
                                 hipStream_t st);
// bilagrid.hip: the per-image bilateral grid on the V images of a step and its adjoint (no workspace: a vertex's sums are one
// workgroup's), and the total variation of the grids; partials: bilagrid_tv_blocks(elems) rows of 4 doubles (carve_bilagrid_tv in api.hip)
int bilagrid_tv_blocks(long long elems);
hipError_t launch_bilagrid_fwd(const BagsBilagrid& a, hipStream_t st);
hipError_t launch_bilagrid_bwd(const BagsBilagrid& a, const float* const* g_out, float* const* g_image, float* g_grids, hipStream_t st);
hipError_t launch_bilagrid_tv_fwd(const float* grids, int N, int Gx, int Gy, int L, double* partials, float* loss, hipStream_t st);
hipError_t launch_bilagrid_tv_bwd(const float* grids, int N, int Gx, int Gy, int L, const float* g_loss, float* g_grids, hipStream_t st);
// lens_field.hip: the invertible-ResNet lens network on M points of R^2 (forward / fixed-point inverse in one launch, backward in two)
__host__ __device__ static inline int lens_block_floats(int H, int n) { return 3 * H + n * (H * H + H) + 2 * H + 2; }   // of the flat vector, per block
size_t lens_field_workspace_bytes(int B, int H, int n, long long M);
hipError_t launch_lens_field_fwd(const BagsLensField& a, const float* src, long long M, float* dst, bool inverse, int iterations, hipStream_t st);
hipError_t launch_lens_field_bwd(const BagsLensField& a, const float* x, long long M, const float* grad_y, void* workspace, float* grad_x,
                                 float* grad_params, hipStream_t st);
// knn.hip: mean squared distance to the three nearest neighbours (distCUDA2)
size_t knn_workspace_bytes(int P);
hipError_t launch_knn(const float* pts, int P, void* ws, float* out, hipStream_t st);
// binning.hip: tile-binned instance lists (no global sort)
int binned_per_block(int P);
bool binned_supported(int P, int T);
hipError_t launch_binned_empty(const GeomView& g, const ImgView& im, int T, hipStream_t st);
// the tile descriptor list alone (launch_binned_finish builds it beside the emission): for forwards that emit nothing
hipError_t launch_binned_desc_only(const ImgView& im, int T, hipStream_t st);
// host_count: device-visible address of a pinned host word that also receives the instance count (may be null)
// (the (block, tile) counts themselves come from launch_preprocess_fwd(count_into = &im))
hipError_t launch_binned_prepare(const GeomView& g, const ImgView& im, int P, int grid_x, int T, hipStream_t st, u32* host_count = nullptr,
                                 bool count_now = true);
hipError_t launch_binned_finish(const GeomView& g, const ImgView& im, int P, int grid_x, int T, u64* words, u32 capacity, hipStream_t st,
                                bool deliver_count = false);
hipError_t launch_debug_keys_ranges(const uint2* ranges, const u32* point_list, const u32* depth_key, int T, u64* out, hipStream_t st);
hipError_t launch_debug_keys(const u32* tile_sorted, const u32* point_list, const u32* depth_key, long long I, u64* out, hipStream_t st);
hipError_t launch_unpack_rect(const uint2* rect, int P, u32* out, hipStream_t st);
