/* bags_raster.h -- C ABI of libbags_raster.so, the MI355X (gfx950) pose-differentiable Gaussian rasterizer.
 *
 * Drop-in boundary.  The reference reaches its rasterizer through the Python package
 * `diff_gaussian_rasterization` (gaussian_renderer/__init__.py:14), whose native half is a pybind11 torch
 * extension living in the (empty) `3dgs-pose` submodule (.gitmodules:4-6, README.md:126).  That extension's
 * entry points -- rasterize forward, rasterize backward -- are what this header replaces, as plain C:
 *
 *   reference call site                                              replaced by
 *   ---------------------------------------------------------------  ----------------------------------
 *   GaussianRasterizer.forward(...)  gaussian_renderer/__init__.py:110-121   bags_forward_prepare + bags_forward_finish
 *   autograd backward of that call   train.py:331 (loss.backward)            bags_backward
 *   GaussianRasterizationSettings    gaussian_renderer/__init__.py:50-65     BagsSettings (POD)
 *   state kept between fwd and bwd   (fork: geom/binning/image byte tensors)  caller-owned buffers sized by bags_*_size
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless named host_*; fp32, contiguous, row-major;
 *   - the library allocates nothing that outlives a call, keeps no per-call state, never frees caller memory;
 *   - all work is enqueued on `stream` (a hipStream_t; NULL = default stream) of the current device;
 *     bags_forward_prepare performs ONE stream synchronisation (to hand the instance count to the host);
 *   - return value: 0 = ok, negative = error; bags_last_error() gives a thread-local message;
 *   - matrices follow the reference's row-vector convention: p_view = [x y z 1] * viewmatrix
 *     (utils/graphics_utils.py:26-33, scene/cameras.py:107-108), 16 floats row-major.
 */
#ifndef BAGS_RASTER_H
#define BAGS_RASTER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BAGS_ABI_VERSION 11
#define BAGS_TILE 16

enum { BAGS_OK = 0, BAGS_ERR_ARG = -1, BAGS_ERR_HIP = -2, BAGS_ERR_SIZE = -3, BAGS_ERR_DEVICE = -4 };
enum { BAGS_DEPTH_Z = 0, BAGS_DEPTH_DISTANCE = 1 };   /* README.md:126: sort key is view z, or distance for cubemaps */
/* Which tiles a Gaussian is binned into.  BAGS_TILES_AABB is the stock rule: every tile overlapping the square
 * [p - r, p + r + 15] with r = ceil(3 sqrt(lambda_max)).  BAGS_TILES_OPACITY intersects that rectangle with the
 * axis-aligned bounds of the ellipse alpha >= 1/255 (half extents sqrt(2 ln(255 o) cov_xx), sqrt(.. cov_yy), with a
 * 2 % + 0.1 px safety margin): every (tile, Gaussian) pair it drops has alpha < 1/255 on all 256 pixels, i.e. is skipped
 * by the compositing loop anyway, so image, radii and every gradient are unchanged while the sorted instance list
 * shrinks.  Inside a rectangle of at most 8 x 8 tiles it further drops every tile the ellipse itself does not reach
 * (minimum of d^T Q d over the square of the tile's pixel centres > 1.02 (2 ln(255 o) + 0.022)): the same guarantee.
 * Together 40 % fewer instances on BASELINE config 3 (3.45 M -> 2.07 M). */
enum { BAGS_TILES_AABB = 0, BAGS_TILES_OPACITY = 1 };
/* How the per-tile depth-ordered instance lists are built.  AUTO: tile-binned (csrc/binning.hip: (block, tile) count matrix
 * in LDS, per-tile sort of (depth, id) pairs in LDS; five launches, no global sort) whenever the image has at most 32768
 * tiles and P <= 16.7 M, else RADIX.  RADIX: depth-sort the Gaussians, emit, stable radix sort by tile (csrc/sort.hip).
 * Both produce the same lists bit for bit. */
enum { BAGS_BINNING_AUTO = 0, BAGS_BINNING_RADIX = 1 };
/* Gradient of the EWA Jacobian for a Gaussian whose view-space point lies outside 1.3 x the field of view, where the forward
 * uses the clamped t.x = +-1.3 tanfovx t.z (same for y).  Forward values do not depend on this switch.
 * STOCK (default): the rule of upstream diff-gaussian-rasterization's computeCov2DCUDA backward, which the reference's fork
 * (README.md:126) inherits: dL/dt.x is zeroed (x_grad_mul) and dL/dt.z takes 2 h_x t.x / t.z^3 dL/dJ02 with the clamped t.x
 * held CONSTANT.  EXACT: differentiates the clamped expression itself (t.x moves with t.z), i.e. half of that one term. */
enum { BAGS_CLAMP_GRAD_STOCK = 0, BAGS_CLAMP_GRAD_EXACT = 1 };
/* Backward of conic = cov2D^-1.  STOCK (default, ABI 8): upstream computeCov2DCUDA divides by det^2 + 1e-7 where the derivative of the
 * 2x2 inverse has det^2 ("denom2inv"); the reference's fork (README.md:126) inherits it.  EXACT: det^2 (what rounds 1-4 shipped).
 * det >= 0.09 (the 0.3 px dilation), so the two differ by at most 1.2e-5 relative on one Gaussian's dL/dcov2D (measured 2e-7 on the
 * gradient tensors of a scene of small splats, tests/test_oracle_cpu.py).  Forward values do not depend on this switch. */
enum { BAGS_CONIC_GRAD_STOCK = 0, BAGS_CONIC_GRAD_EXACT = 1 };
enum { BAGS_BWD_ALL = 0, BAGS_BWD_BLEND = 1, BAGS_BWD_PREPROCESS = 2 };   /* BagsBackwardArgs.phase (ABI 9) */

/* GaussianRasterizationSettings (gaussian_renderer/__init__.py:50-65) */
typedef struct BagsSettings {
    int32_t image_height, image_width;
    float tanfovx, tanfovy;          /* from the camera's STATIC fov (gaussian_renderer/__init__.py:47-48) */
    float scale_modifier;
    int32_t sh_degree;               /* active degree 0..3 */
    int32_t sh_coeffs;               /* M: coefficients stored per Gaussian in `shs` ((max_sh_degree+1)^2) */
    int32_t depth_key;               /* BAGS_DEPTH_Z | BAGS_DEPTH_DISTANCE */
    int32_t debug;                   /* !=0: synchronise + check after every kernel */
    int32_t debug_iter;              /* carried for error messages only */
    int32_t tile_bounds;             /* BAGS_TILES_AABB | BAGS_TILES_OPACITY */
    int32_t binning;                 /* BAGS_BINNING_AUTO | BAGS_BINNING_RADIX */
    int32_t clamp_grad;              /* BAGS_CLAMP_GRAD_STOCK | BAGS_CLAMP_GRAD_EXACT (backward only) */
    int32_t conic_grad;              /* BAGS_CONIC_GRAD_STOCK | BAGS_CONIC_GRAD_EXACT (backward only; was reserved0 = 0 before ABI 8) */
    const float* bg;                 /* (3)   */
    const float* viewmatrix;         /* (4,4) world->view, transposed (W2C^T) */
    const float* projmatrix;         /* (4,4) viewmatrix * intrinsic */
    const float* intrinsic;          /* (4,4) projection^T; [0][0],[1][1] give the focal lengths, row 2 the shift direction */
    const float* campos;             /* (3)   */
} BagsSettings;

/* the keyword tensors of GaussianRasterizer.forward (gaussian_renderer/__init__.py:110-121) */
typedef struct BagsInputs {
    int32_t P;
    const float* means3D;            /* (P,3) */
    const float* means2D;            /* (P,3) additive NDC offset, normally zeros; may be NULL */
    const float* shift_factors;      /* (3) entrance-pupil polynomial; may be NULL (= zeros) */
    const float* shs;                /* (P,M,3) or NULL */
    const float* colors_precomp;     /* (P,3)   or NULL  (exactly one of shs / colors_precomp) */
    const float* opacities;          /* (P,1) */
    const float* scales;             /* (P,3) or NULL */
    const float* rotations;          /* (P,4) (w,x,y,z) or NULL */
    const float* cov3D_precomp;      /* (P,6) xx,xy,xz,yy,yz,zz or NULL (exactly one of scales+rotations / cov3D) */
    /* (ABI 7) the reference's two feature parameters as they are stored, without GaussianModel.get_features' torch.cat
     * (scene/gaussian_model.py:131-134: 96 MB read + 96 MB written per call at 500 k Gaussians, and as much again for the split of
     * the gradient): when non-NULL, `shs` is features_dc (P,1,3) and this is features_rest (P,M-1,3), M = settings.sh_coeffs >= 2 */
    const float* shs_rest;
} BagsInputs;

/* Caller-owned memory.  Every buffer the library works in is the caller's: the three state buffers below, the backward's workspace
 * and the workspace of every other entry point, each sized by its bags_*_size function.  None needs initialisation (it may hold
 * anything), nothing outside its `bytes` is read or written, and a buffer one byte short of its size function is refused before
 * anything is launched.  Two rules for the base pointer, by buffer (tests/test_memory_contract_gpu.py holds each entry point to its):
 *   rounded   the library rounds the base up to 256 itself and the size carries the slack for it: ANY base is accepted.  The state
 *             buffers (geom, binning, image), the backward workspace, and the workspaces of resample, resample_faces, sh_colors,
 *             sh_colors_views, densify, lens_field, knn, mcmc, antialias, filter3d and gaussian_normals.
 *   as given  the base is used as it is and must be aligned as the entry point says; another base is refused, not rounded, before
 *             anything is launched.  16 bytes: appearance, bilagrid_tv, depth_prior, normal_prior, correspondence, warp, normal_map,
 *             smooth, gaussian_reg, alpha (whose size is the constant BAGS_ALPHA_WORKSPACE_BYTES, not a function).  4 bytes: the
 *             photometric loss.  (bags_bilagrid_workspace_size is 0: nothing is taken.) */
/* caller-owned state that survives from forward to backward */
typedef struct BagsState {
    void* geom;    size_t geom_bytes;     /* >= bags_geom_size(P)            */
    void* binning; size_t binning_bytes;  /* >= bags_binning_size(I, W, H)   */
    void* image;   size_t image_bytes;    /* >= bags_image_size(W, H)        */
} BagsState;

typedef struct BagsForwardOut {
    float*   color;      /* (3,H,W) */
    int32_t* radii;      /* (P)     */
    float*   depth;      /* (1,H,W) expected view-space z            */
    float*   weights;    /* (1,H,W) accumulated alpha = 1 - T_final  */
    float*   mean2D;     /* (P,2)   pixel centres (0 for culled)     */
} BagsForwardOut;

typedef struct BagsBackwardArgs {
    const float* grad_color;         /* (3,H,W) dL/dimage */
    int64_t num_rendered;            /* I returned by bags_forward_prepare */
    void* workspace; size_t workspace_bytes;   /* >= bags_backward_workspace_size(P, I) */
    /* outputs; any may be NULL when not needed.  All are fully overwritten unless `accumulate` (below) says otherwise. */
    float* grad_means3D;             /* (P,3)   */
    float* grad_means2D;             /* (P,3)   NDC units, z = 0 */
    float* grad_means2D_densify;     /* (P,3)   sum over pixels of |per-pixel NDC gradient|, z = 0 */
    float* grad_shs;                 /* (P,M,3) */
    float* grad_colors_precomp;      /* (P,3)   */
    float* grad_opacities;           /* (P,1)   */
    float* grad_scales;              /* (P,3)   */
    float* grad_rotations;           /* (P,4)   */
    float* grad_cov3D_precomp;       /* (P,6)   */
    float* grad_viewmatrix;          /* (4,4)   */
    float* grad_projmatrix;          /* (4,4)   */
    float* grad_intrinsic;           /* (4,4)   */
    float* grad_campos;              /* (3)     */
    float* grad_shift_factors;       /* (3)     */
    /* capacity the forward's binning buffer was carved for when that was a speculative finish (state.binning then holds
     * bags_binning_size(binning_capacity, W, H) bytes and num_rendered is the TRUE count, which sizes the workspace);
     * 0 = the buffer was sized for num_rendered itself (bags_forward_finish) */
    int64_t binning_capacity;
    /* != 0: the seven Gaussian-parameter gradients (means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp) are
     * ADDED to what their buffers hold instead of overwriting them -- the views of one optimisation step accumulate in place, as
     * autograd would do with one add pass per view and tensor; every other output is overwritten as before (ABI 6) */
    int32_t accumulate;
    /* Dense-scene mode of the backward.  blend_bwd writes one 48-byte record per instance and preprocess_bwd sums each Gaussian's
     * records; an instance behind its tile's deepest contributor holds a ZERO record.  Above this many instances per tile (scene
     * average) a byte per record says whether blend_bwd wrote it: no zero record is written or read (at 1800 instances per tile
     * 85 % of them are).  0 = the library's default (480; profiles/r05/ab_dense.txt), < 0 = never, > 0 = that threshold.  Results
     * do not depend on it (ABI 8; the field was reserved1 = 0 before, and rounds 3-4 read an environment variable here). */
    int32_t dense_per_tile;
    float* grad_shs_rest;            /* (P,M-1,3), with inputs.shs_rest: grad_shs is then the (P,1,3) gradient of features_dc (ABI 7) */
    /* (ABI 9) Which half of the backward this call enqueues.  BAGS_BWD_ALL (0): everything, as before.  BAGS_BWD_BLEND: the per-tile
     * half only (blend_bwd: dL/dimage -> one partial-gradient record per instance, in the workspace).  BAGS_BWD_PREPROCESS: the
     * per-Gaussian half only (preprocess_bwd + pose_reduce: records -> every output above); same workspace, same arguments, after a
     * BLEND call.  The split exists for callers that differentiate several views of one step on several streams with `accumulate`:
     * the read-modify-write of the shared gradient buffers must run in view order, so the second half of view k waits for the
     * second half of view k-1 (an event between two calls) while its first half -- 85 % of the backward's time -- does not. */
    int32_t phase;
    int32_t reserved2;               /* 0 */
    /* (ABI 10) Factored SH gradient, for steps that differentiate SEVERAL views into the same Gaussians.  dL/dshs of one view is an
     * outer product per Gaussian -- basis(direction from that view's camera) x dL/dcolour, 16 x 3 floats made of 3 -- and writing
     * (and, with `accumulate`, first reading) that 192-byte row is two thirds of the per-Gaussian half's traffic.  With grad_dldc
     * non-NULL (and grad_shs / grad_shs_rest NULL) the backward writes only the (P,3) dL/dcolour (after the colour clamp; zero for a
     * culled Gaussian) here; bags_sh_gradient_from_views then forms the gradient rows of ALL the step's views in one pass, reading
     * 12 bytes per Gaussian and view and writing each row once.  Same products, added in view order: bit-identical to V backwards
     * with `accumulate`.  SH colour path only (inputs.shs given). */
    float* grad_dldc;
} BagsBackwardArgs;

/* integer artefacts for bit-exact parity checks (all device pointers, any may be NULL) */
typedef struct BagsDebugViews {
    uint32_t* tiles_touched;         /* (P) */
    uint32_t* rect;                  /* (P,4) minx,miny,maxx,maxy */
    uint32_t* depth_bits;            /* (P) float bits of the sort depth (0xFFFFFFFF if culled) */
    uint32_t* point_list;            /* (I) Gaussian id per sorted instance */
    uint64_t* keys_sorted;           /* (I) (tile<<32)|depth_bits per sorted instance */
    uint32_t* ranges;                /* (T,2) */
    uint32_t* n_contrib;             /* (H,W) */
    float*    final_T;               /* (H,W) */
} BagsDebugViews;

int         bags_abi_version(void);
const char* bags_last_error(void);
/* "src=<12 hex digits> commit=<git short hash|nogit>[+dirty]": a hash of the kernel sources this library was compiled from and
 * the last commit that touched them (ABI 8).  Measurement bookkeeping only: profiles/rNN/traffic.json records the string of the
 * build its counters were collected on, and bench.py prints roofline.traffic only when it matches the library it is timing. */
const char* bags_build_info(void);

size_t bags_geom_size(int32_t P);
size_t bags_binning_size(int64_t num_rendered, int32_t width, int32_t height);
size_t bags_image_size(int32_t width, int32_t height);
size_t bags_backward_workspace_size(int32_t P, int64_t num_rendered);

/* Phase 1: per-Gaussian projection/covariance/colour, depth ordering of the Gaussians, instance offsets.
 * Writes radii and mean2D.  Synchronises `stream` once and returns the instance count in *host_num_rendered. */
int bags_forward_prepare(const BagsSettings*, const BagsInputs*, const BagsState*, const BagsForwardOut*,
                         int64_t* host_num_rendered, void* stream);
/* Phase 2: instance emission, per-tile stable sort, tile ranges, front-to-back blend.  state.binning must hold
 * bags_binning_size(num_rendered, W, H) bytes. */
int bags_forward_finish(const BagsSettings*, const BagsInputs*, const BagsState*, const BagsForwardOut*,
                        int64_t num_rendered, void* stream);
/* Forward without a host round trip in the middle (speculative instance capacity).
 *   1. bags_forward_prepare_async: phase 1 as above, without the synchronisation.  *host_num_rendered is a caller-owned
 *      PINNED host word (hipHostMalloc / torch pinned memory: device-mapped) that will receive the instance count; set it to a
 *      sentinel (e.g. 0xFFFFFFFF) before the call.
 *   2. bags_forward_finish_speculative: phase 2 enqueued immediately, sized for a caller-guessed upper bound `capacity`
 *      (e.g. 1.2 x the previous frame's count; state.binning holds bags_binning_size(capacity, W, H) bytes); the
 *      kernels read the true count on the device and render every tile empty if it exceeds `capacity`.
 *      WHEN THE COUNT ARRIVES (ABI 5): on the tile-binned path no launch of phase 1 computes it any more -- the first launch
 *      of THIS call does (tile ranges, count and block bases are formed inside the emission launch) and stores it into the
 *      pinned word at system scope, a few tens of microseconds into phase 2.  On the radix path, for P == 0, or when the
 *      word is not device-mapped, step 1 delivers it by an enqueued copy as before.  Either way: the word holds the count
 *      no later than the end of step 2; a caller that needs the count BEFORE it enqueues phase 2 uses bags_forward_prepare.
 *   3. The caller polls the word (or waits for an event recorded behind step 2) -- right away, while the GPU is busy with
 *      phase 2, or as late as the entry of bags_backward -- and compares: if the count exceeds `capacity` the outputs are
 *      invalid (every tile was rendered empty) and phase 2 must be redone with bags_forward_finish on a buffer of
 *      bags_binning_size(count, W, H) bytes (phase 1 results in state.geom stay valid; that exact re-run does not touch the
 *      pinned word again, so the word may be reused for another call as soon as it has been read).  When it fits,
 *      bags_backward takes the true count as num_rendered and `capacity` as binning_capacity. */
int bags_forward_prepare_async(const BagsSettings*, const BagsInputs*, const BagsState*, const BagsForwardOut*,
                               uint32_t* host_num_rendered, void* stream);
int bags_forward_finish_speculative(const BagsSettings*, const BagsInputs*, const BagsState*, const BagsForwardOut*,
                                    int64_t capacity, void* stream);
/* Backward of the whole op from dL/dimage. */
int bags_backward(const BagsSettings*, const BagsInputs*, const BagsState*, const BagsBackwardArgs*, void* stream);

/* (ABI 11) Cotangents of the forward's depth and weights maps.  depth = sum_i w_i z_i (z_i: view depth with the shift-factor
 * term, for either depth_key) and weights = 1 - T_final = sum_i w_i composite like two more colour channels (colours z_i and 1,
 * background 0), so they add z_i dL/ddepth + dL/dweights to every (pixel, splat) term of the colour backward, and sum_i w_i
 * dL/ddepth reaches the view depth, hence means3D, the pose tensors and shift_factors.  Either pointer may be NULL (= zero). */
typedef struct BagsExtraGrads {
    const float* grad_depth;         /* (1,H,W) dL/ddepth   or NULL */
    const float* grad_weights;       /* (1,H,W) dL/dweights or NULL */
} BagsExtraGrads;
/* bags_backward with the extra cotangents.  extra == NULL, or both its pointers NULL: exactly bags_backward (same kernels, same
 * bits).  Otherwise args->grad_color may be NULL too (= zero: a loss on depth / weights alone).  Every BagsBackwardArgs mode
 * applies; with `phase` both calls must be given the same extras. */
int bags_backward_ex(const BagsSettings*, const BagsInputs*, const BagsState*, const BagsBackwardArgs*, const BagsExtraGrads* extra,
                     void* stream);

/* (ABI 10) The SH-gradient rows of up to BAGS_MAX_SH_VIEWS views of one step from their factored form (BagsBackwardArgs.grad_dldc):
 *   grad_shs[g][t][c] (+)= sum over the views v, in order, of basis_t(normalize(means3D[g] - campos_v)) * dldc_v[g][c]
 * for the active degree's coefficients (the others are written as zeros / left as they are when accumulating).  M = coefficients
 * per Gaussian in grad_shs ((P,M,3)), or -- grad_shs_rest non-NULL -- grad_shs is (P,1,3) and grad_shs_rest (P,M-1,3) (the pair
 * of BagsInputs.shs_rest).  accumulate != 0: the views are added, in order, to what the buffers hold; else the first view overwrites.
 * More than BAGS_MAX_SH_VIEWS views: call again with accumulate = 1 for the next batch (the order of the additions is preserved). */
#define BAGS_MAX_SH_VIEWS 16
typedef struct BagsShViews {
    int32_t n_views;
    int32_t reserved;
    const float* campos[BAGS_MAX_SH_VIEWS];   /* (3) each: the campos tensor the view's op call was given */
    const float* dldc[BAGS_MAX_SH_VIEWS];     /* (P,3) each: that view's BagsBackwardArgs.grad_dldc */
} BagsShViews;
int bags_sh_gradient_from_views(int32_t P, int32_t M, int32_t sh_degree, const float* means3D, const BagsShViews* views,
                                float* grad_shs, float* grad_shs_rest, int32_t accumulate, void* stream);

/* Copies integer artefacts out of the state buffers (parity tests / debugging). */
int bags_debug_views(const BagsSettings*, const BagsInputs*, const BagsState*, int64_t num_rendered,
                     const BagsDebugViews*, void* stream);

/* Opt-in per-stage device timing on the caller's stream: bench.py's roofline leg.  mode 0 = off (default; the hot path records
 * nothing), 1 = only the dominant kernel (blend_bwd), by a start / stop hipEvent pair ATTACHED TO THE KERNEL'S DISPATCH
 * (hipExtLaunchKernelGGL: no packet between the step's launches; round 5 bracketed it with two hipEventRecord calls, 10-25 us of
 * bubbles per step inside the region being timed), 2 = every stage, bracketed by recorded events (each pair costs a few microseconds
 * of stream bubble: for a separate, untimed pass).  bags_profile_stride(n): in mode 1 only every n-th launch carries events (the mean
 * launch time of a steady loop needs no more; n = 1 by default).  bags_profile_read synchronises on the events, returns the number of
 * stages, fills up to `max_stages` entries (stage name, summed milliseconds, number of timed intervals) and clears the accumulators. */
#define BAGS_PROFILE_MAX_STAGES 16
int bags_profile_enable(int mode);
int bags_profile_stride(int n);
int bags_profile_read(int max_stages, const char** names, double* total_ms, int64_t* calls);

/* Fused photometric loss terms.  Replaces the reference's l1_loss + ssim pair
 * (utils/loss_utils.py:18-19 and :48-76: five dense 11x11 depthwise conv2d calls and their autograd backward; call
 * site train.py:311-313, combined at train.py:325 as (1-lambda) L1 + lambda (1-SSIM)).
 *   image, gt     device, fp32, contiguous (C,H,W)
 *   workspace     caller-owned, bags_loss_workspace_size(C,H,W) bytes, kept from forward to backward.  The base is used as given
 *                 (the size has no slack for rounding it up): it holds float planes, so it is 4-byte aligned -- another base is
 *                 refused before anything is launched -- and a 16-byte aligned one (with W % 4 == 0) takes the backward's vector
 *                 path, with the same bits either way.  No initialisation.
 *   out_terms    device float[2]: { mean |image-gt| , mean SSIM }
 *   grad_terms    device float[2]: upstream dL/d{L1 mean, SSIM mean} (read on the device: no host round trip)
 *   grad_image    device (C,H,W): dL/dimage
 * Stream-ordered on `stream`; sums are taken in a fixed order (bitwise reproducible). */
size_t bags_loss_workspace_size(int32_t C, int32_t H, int32_t W);
int bags_loss_forward(const float* image, const float* gt, int32_t C, int32_t H, int32_t W, void* workspace,
                      size_t workspace_bytes, float* out_terms, void* stream);
int bags_loss_backward(const float* image, const float* gt, int32_t C, int32_t H, int32_t W, const void* workspace,
                       size_t workspace_bytes, const float* grad_terms, float* grad_image, void* stream);

/* The same pair with train.py:325's combination inside (ABI 7): loss = (1 - lambda_dssim) * L1 + lambda_dssim * (1 - SSIM), formed
 * in fp32 with the roundings of the reference's PyTorch expression.  The scalar arithmetic around the two terms and its autograd
 * backward were ten one-element PyTorch launches per iteration (48 us of a 1.05 ms iteration at 1080p).
 *   out_loss_terms  device float[3]: { loss, mean |image-gt|, mean SSIM }
 *   grad_loss       device float[1]: upstream dL/dloss (read on the device)
 * Same workspace as above (bags_loss_workspace_size), kept from forward to backward. */
int bags_photometric_loss_forward(const float* image, const float* gt, int32_t C, int32_t H, int32_t W, void* workspace,
                                  size_t workspace_bytes, float lambda_dssim, float* out_loss_terms, void* stream);
int bags_photometric_loss_backward(const float* image, const float* gt, int32_t C, int32_t H, int32_t W, const void* workspace,
                                   size_t workspace_bytes, float lambda_dssim, const float* grad_loss, float* grad_image, void* stream);

/* The pose -> matrix chain of scene/cameras.py:356-381 in one launch each way: replaces
 * get_world_view_transform / get_full_proj_transform / get_intrinsic / get_camera_center (~40 PyTorch kernels and six 4x4
 * inversions per render() call, gaussian_renderer/__init__.py:57,58,61) and their autograd backward.  All pointers are
 * device pointers; optional ones may be NULL. */
typedef struct BagsCamera {
    const float* init_quaternion;    /* (4) w,x,y,z of the world-to-camera rotation (scene/cameras.py:98) */
    const float* delta_quaternion;   /* (4) learnable, added before normalisation (scene/cameras.py:360) */
    const float* init_translation;   /* (3) */
    const float* delta_translation;  /* (3) learnable */
    const float* fovx;               /* scalar, learnable (scene/cameras.py:109-110) */
    const float* fovy;
    const float* global_rotation;    /* (3,3) row-major or NULL: R <- G R (scene/cameras.py:361) */
    const float* global_translation_scale;   /* scalar or NULL: t <- s t (scene/cameras.py:367-370) */
    float znear, zfar;
} BagsCamera;
/* viewmatrix, projmatrix, intrinsic: (4,4); campos: (3) */
int bags_camera_forward(const BagsCamera* cam, float* viewmatrix, float* projmatrix, float* intrinsic, float* campos, void* stream);
/* upstream gradients may be NULL (= zero); gradient outputs may be NULL (= not wanted) */
int bags_camera_backward(const BagsCamera* cam, const float* g_viewmatrix, const float* g_projmatrix, const float* g_intrinsic,
                         const float* g_campos, float* g_delta_quaternion, float* g_delta_translation, float* g_fovx,
                         float* g_fovy, float* g_global_rotation, float* g_global_translation_scale, void* stream);

/* The camera bank: the pose leaves of all N training cameras in device tables, and the chain above for the n_rows <=
 * BAGS_MAX_POSE_ROWS cameras of one step in ONE launch each way (csrc/camera.hip).  Row v of every output belongs to camera
 * rows[v] and holds the bits bags_camera_forward / bags_camera_backward give for that camera's leaves.  The row list travels by
 * value; nothing is uploaded, nothing allocated, no host synchronisation, no atomics.  rows are distinct and each in [0, N). */
#define BAGS_MAX_POSE_ROWS 16
typedef struct BagsPoseBank {
    int32_t N;                       /* cameras in the bank, >= 1 */
    const float* init_quaternion;    /* (N,4) w,x,y,z */
    const float* init_translation;   /* (N,3) */
    const float* near_far;           /* (N,2) znear, zfar per camera, 0 < znear < zfar */
    const float* leaves;             /* (N,9): delta_quaternion 0..3 | delta_translation 4..6 | fovx 7 | fovy 8 */
    const float* global_rotation;    /* (3,3) row-major or NULL, shared by the rows of a call */
    const float* global_translation_scale;   /* scalar or NULL */
    int32_t n_rows;                  /* 1..BAGS_MAX_POSE_ROWS */
    int32_t rows[BAGS_MAX_POSE_ROWS];
} BagsPoseBank;
/* viewmatrix, projmatrix, intrinsic: (n_rows,4,4); campos: (n_rows,3) */
int bags_pose_bank_forward(const BagsPoseBank* bank, float* viewmatrix, float* projmatrix, float* intrinsic, float* campos,
                           void* stream);
/* Upstream gradients (n_rows,...) may be NULL (= zero).  grad_leaves (N,9): EVERY element is written by this call, the rows not
 * listed as exact zeros (no fill launch is needed before it).  g_global_rotation (3,3) and g_global_translation_scale (1) may be
 * NULL (= not wanted); each needs its input in the bank struct.  They are the sum over the listed rows in row-list order
 * v = 0, 1, ...: an fp32 left fold by one thread. */
int bags_pose_bank_backward(const BagsPoseBank* bank, const float* g_viewmatrix, const float* g_projmatrix, const float* g_intrinsic,
                            const float* g_campos, float* grad_leaves, float* g_global_rotation, float* g_global_translation_scale,
                            void* stream);

/* Image-space distortion resampling: the apply2gt == False branch of apply_distortion
 * (utils/util_distortion.py:271-311, call site train.py:255-263) in one pass each way:
 *   flow  = interpolate(control flow (h,w,2) -> (flow_H, flow_W), bilinear, align_corners=False)
 *   out   = center_crop(grid_sample(image (C,H,W), flow, bilinear, zeros, align_corners=True), crop_H, crop_W)
 *   mask  = !(out[0] == 0 && out[1] == 0)                                    (may be NULL)
 *   flow_out (crop_H, crop_W, 2): the upsampled flow at the cropped pixels     (may be NULL)
 * Pass h == flow_H, w == flow_W to resample with an already dense flow (the cached flow_apply2_gt_or_img path).
 * Backward: grad_image (C,H,W) is gathered per 16x16 source tile into a 64-bit fixed-point accumulator in LDS (every
 * element is written: no memset needed); grad_ctrl (h,w,2) is gathered per control node in a fixed order.  No global float
 * atomics (integer ones only on per-tile list counters), so both gradients are bitwise reproducible.  Needs a caller-owned
 * workspace of bags_resample_workspace_size(H, W, crop_H, crop_W) bytes (per-tile lists and the dense dL/dflow).  Either
 * gradient may be NULL.  C <= 24 per call (2 KB of LDS per channel).  A non-finite grad_out element makes the source tiles
 * its output tile is listed on NaN; magnitudes below 2^-100 are treated as zero. */
size_t bags_resample_workspace_size(int32_t H, int32_t W, int32_t crop_H, int32_t crop_W);
int bags_resample_forward(const float* image, int32_t C, int32_t H, int32_t W, const float* ctrl_flow, int32_t h, int32_t w,
                          int32_t flow_H, int32_t flow_W, int32_t crop_H, int32_t crop_W, float* out, float* mask,
                          float* flow_out, void* stream);
int bags_resample_backward(const float* image, int32_t C, int32_t H, int32_t W, const float* ctrl_flow, int32_t h, int32_t w,
                           int32_t flow_H, int32_t flow_W, int32_t crop_H, int32_t crop_W, const float* grad_out,
                           void* workspace, size_t workspace_bytes, float* grad_image, float* grad_ctrl, void* stream);

/* The cubemap stitch (utils/cubemap_utils.py:181-186,219-288; csrc/resample_faces.hip): the F <= BAGS_MAX_FACES
 * perspective faces of one step, each (C,H,W) with C <= 4, warped into the distorted output image and stitched in one pass.
 * Per cropped output pixel, with (gx, gy) the upsampled control flow there exactly as bags_resample_* compute it (grid_sample
 * coordinates of the FRONT image):
 *   (a, b, c) = mats[f] (gx, gy, 1)^T,  u = a / c,  v = b / c;  face f is valid iff c > 0 && |u| <= 1 && |v| <= 1  (a NaN: not valid)
 *   the pixel belongs to the FIRST valid face in list order: image = bilinear sample of that face at (u, v) (grid_sample,
 *   align_corners=True, zeros padding), face_index = f;  no valid face: image = 0 in every channel, face_index = -1.
 * mats[f] = diag(1/tx_f, 1/ty_f, 1) R_f diag(tx_0, ty_0, 1), row-major: R_f rotates a ray of the front camera into face f's camera
 * frame, tx / ty are the tangents of the half fields of view (index 0: the front camera, which ctrl_flow is meant for).  The
 * matrices travel by value and are not differentiated.
 * Backward: the choice is REPLAYED from face_index (the forward's output), never decided again.  grad_faces[f] (C,H,W), any of
 * them NULL, is gathered per 16x16 tile of face f into a 64-bit fixed-point accumulator in LDS, every element written (zeros
 * where nothing lands, a face no pixel chose all zeros: no memset needed); grad_ctrl (h,w,2), may be NULL, is gathered per
 * control node through u = a/c, v = b/c.  No global float atomics: both are bitwise reproducible, and each is the same whichever
 * others are asked for.  Workspace: bags_resample_faces_workspace_size bytes, caller-owned (0 for invalid arguments). */
#define BAGS_MAX_FACES 8
typedef struct BagsFaces {
    int32_t n_faces, C, H, W;            /* 1..BAGS_MAX_FACES faces of (C,H,W), C <= 4 */
    const float* image[BAGS_MAX_FACES];  /* the first n_faces given */
    float mats[BAGS_MAX_FACES][9];
} BagsFaces;
size_t bags_resample_faces_workspace_size(int32_t n_faces, int32_t H, int32_t W, int32_t crop_H, int32_t crop_W);
int bags_resample_faces_forward(const BagsFaces* faces, const float* ctrl_flow, int32_t h, int32_t w, int32_t flow_H, int32_t flow_W,
                                int32_t crop_H, int32_t crop_W, float* out, int8_t* face_index, void* stream);
int bags_resample_faces_backward(const BagsFaces* faces, const float* ctrl_flow, int32_t h, int32_t w, int32_t flow_H, int32_t flow_W,
                                 int32_t crop_H, int32_t crop_W, const int8_t* face_index, const float* grad_out, void* workspace,
                                 size_t workspace_bytes, float* const grad_faces[BAGS_MAX_FACES], float* grad_ctrl, void* stream);

/* The parameter activations that feed the op, one launch each way: GaussianModel.get_features
 * (cat of features_dc and features_rest), get_opacity (sigmoid), get_scaling (exp), get_rotation (normalize) --
 * scene/gaussian_model.py:118-141.  K = SH coefficients per Gaussian (1 + rest).  Outputs / gradients may be NULL; with
 * shs (g_shs) NULL the feature pointers may be NULL too and the launch is one thread per Gaussian (a container that keeps
 * features_dc and features_rest as views of one (P,K,3) tensor needs no concatenation: bags_raster.gaussians.GaussianBag). */
typedef struct BagsRawGaussians {
    int32_t P, K;
    const float* features_dc;        /* (P,1,3)   */
    const float* features_rest;      /* (P,K-1,3) */
    const float* opacity;            /* (P,1) pre-sigmoid */
    const float* scaling;            /* (P,3) log-scale   */
    const float* rotation;           /* (P,4) unnormalised quaternion */
} BagsRawGaussians;
int bags_activations_forward(const BagsRawGaussians* raw, float* shs, float* opacity, float* scales, float* rotations, void* stream);
int bags_activations_backward(const BagsRawGaussians* raw, const float* g_shs, const float* g_opacity, const float* g_scales,
                              const float* g_rotations, float* g_features_dc, float* g_features_rest, float* g_opacity_raw,
                              float* g_scaling, float* g_rotation, void* stream);

/* SH -> RGB outside the rasterizer: the colours render() hands over as colors_precomp on its default (hybrid) path,
 * gaussian_renderer/__init__.py:90-95, one launch each way (csrc/sh_colors.hip):
 *     d = xyz - campos,  u = d / |d|,  raw = sum_{t < (sh_degree+1)^2} basis_t(u) * sh[t] + 0.5,  rgb = raw < 0 ? 0 : raw
 * K = stored coefficient rows per Gaussian, one of 1, 4, 9, 16, K >= (sh_degree+1)^2.  Coefficients packed, shs (P,K,3) with
 * shs_rest NULL, or split, shs (P,1,3) + shs_rest (P,K-1,3) (K >= 4; the two parameters as they are stored).  campos: 3 floats in
 * device memory.  xyz == campos is 0/0, as in the reference.
 * Backward: dL/dsh rows beyond the active degree are exactly zero; raw == 0 passes its gradient; a Gaussian with an all-zero
 * cotangent row gets zeros and costs 12 bytes of reads.  Any of the four gradient pointers may be NULL (the SH gradient tensors
 * must be 16-byte aligned); the workspace (the size function's bytes) is only touched when grad_campos is given.  No atomics:
 * the gradients are bitwise reproducible. */
typedef struct BagsShColors {
    int32_t P, K, sh_degree, reserved;
    const float* shs;                /* (P,K,3), or (P,1,3) when shs_rest is given */
    const float* shs_rest;           /* (P,K-1,3) or NULL */
    const float* xyz;                /* (P,3) */
    const float* campos;             /* (3)   */
} BagsShColors;
size_t bags_sh_colors_workspace_size(int32_t P);
int bags_sh_colors_forward(const BagsShColors* a, float* rgb, void* stream);
int bags_sh_colors_backward(const BagsShColors* a, const float* grad_rgb, void* workspace, size_t workspace_bytes, float* grad_shs,
                            float* grad_shs_rest, float* grad_xyz, float* grad_campos, void* stream);

/* The same colours for the V views of one step over the same Gaussians (1 <= V <= BAGS_MAX_SH_VIEWS; more views: one call per
 * chunk), one launch each way: the coefficient rows are read once in the forward and once in the backward, and the gradient rows
 * are summed over the views on the chip and written once.  campos[v]: the v-th view's camera centre, 3 floats in device memory.
 * Forward: rgb[v] (P,3), v < V, all given; view v's colours are the bits bags_sh_colors_forward gives for campos[v].
 * Backward: grad_rgb has V entries, any of which may be NULL (no loss depends on that view); a view contributes to a Gaussian
 * when its cotangent triple there is not all zero.  grad_shs / grad_shs_rest / grad_xyz receive the fp32 sum over the
 * contributing views in view order, ((g_0 + g_1) + g_2) ..., of what bags_sh_colors_backward gives per view, bit for bit; a
 * Gaussian without a contributing view gets zeros and costs 12 V bytes of reads.  grad_campos: NULL, or V entries, any of which
 * may be NULL; entry v receives view v's dL/dcampos (zeros for a view without a cotangent).  The workspace
 * (bags_sh_colors_views_workspace_size bytes) is only touched when some grad_campos entry is given.  Alignment rules as above.
 * No atomics: the gradients are bitwise reproducible. */
typedef struct BagsShColorsViews {
    int32_t P, K, sh_degree, V;
    const float* shs;                /* (P,K,3), or (P,1,3) when shs_rest is given */
    const float* shs_rest;           /* (P,K-1,3) or NULL */
    const float* xyz;                /* (P,3) */
    const float* campos[BAGS_MAX_SH_VIEWS];   /* (3) each, the first V given */
} BagsShColorsViews;
size_t bags_sh_colors_views_workspace_size(int32_t P, int32_t V);
int bags_sh_colors_views_forward(const BagsShColorsViews* a, float* const rgb[], void* stream);
int bags_sh_colors_views_backward(const BagsShColorsViews* a, const float* const grad_rgb[], void* workspace, size_t workspace_bytes,
                                  float* grad_shs, float* grad_shs_rest, float* grad_xyz, float* const grad_campos[], void* stream);

/* One optimizer step of the Gaussian parameters: torch.optim.Adam (amsgrad = False, weight_decay = 0, maximize = False) over up to
 * BAGS_ADAM_MAX_GROUPS parameter groups of one Gaussian count P in ONE launch (csrc/adam.hip).  The reference builds
 * torch.optim.Adam(l, lr=0.0, eps=1e-15) over xyz, f_dc, f_rest, opacity, scaling, rotation (scene/gaussian_model.py:192-210)
 * and steps it once per iteration (train.py:420-421).  Per element, fp32, each operation rounded once:
 *     m = fma(1 - beta1, g - m, m);   v = fma(1 - beta2, g * g, v * beta2);   p = fma(-step_size, m / (sqrt(v) / bias_correction2_sqrt + eps), p)
 * Every group is a contiguous (P, width) fp32 array.  step_size = lr / (1 - beta1^step) and bias_correction2_sqrt =
 * sqrt(1 - beta2^step) are the caller's, per group, computed in double as PyTorch does.  A group whose grad is NULL is skipped.
 * visible (int32 (P), may be NULL; the op's radii fits): row r of every group is updated iff visible[r] > 0; param, exp_avg and
 * exp_avg_sq of any other row are not written.  NULL updates every row (the reference's behaviour).
 * No atomics, no host synchronisation, nothing allocated; results are bitwise reproducible, and a row updated under a mask gets
 * the bits the unmasked step gives it. */
#define BAGS_ADAM_MAX_GROUPS 8
typedef struct BagsAdamGroup {
    float* param;                    /* (P, width), updated in place */
    const float* grad;               /* (P, width) or NULL: group skipped */
    float* exp_avg;                  /* (P, width), updated in place */
    float* exp_avg_sq;               /* (P, width), updated in place */
    int32_t width;                   /* floats per Gaussian, >= 1 */
    int32_t reserved;
    float step_size;                 /* lr / (1 - beta1^step) */
    float bias_correction2_sqrt;     /* sqrt(1 - beta2^step) */
} BagsAdamGroup;
typedef struct BagsAdamArgs {
    int32_t P, n_groups;             /* n_groups in 1..BAGS_ADAM_MAX_GROUPS */
    double beta1, beta2, eps;        /* doubles: 1 - beta is formed in double before it is rounded to fp32, as PyTorch forms it */
    const int32_t* visible;          /* (P) or NULL */
    BagsAdamGroup groups[BAGS_ADAM_MAX_GROUPS];
} BagsAdamArgs;
/* The densification statistics of the same iteration, folded into that launch (GaussianModel.add_densification_stats,
 * scene/gaussian_model.py:449-455, and train.py's max_radii2D line): for every row with radii > 0
 *     xyz_gradient_accum += sqrt(gx * gx + gy * gy),  denom += 1,  max_radii2D = max(max_radii2D, (float)radii)
 * with (gx, gy) the first two floats of the row of grad_means2D (row pitch grad_stride floats, >= 2).  Other rows are not
 * written.  All five pointers NULL = off; some but not all is an error. */
typedef struct BagsDensifyStats {
    const int32_t* radii;            /* (P) */
    const float* grad_means2D;       /* (P, grad_stride): means2D.grad, or the means2D_densify one for abs_grad */
    int32_t grad_stride;
    int32_t reserved;
    float* xyz_gradient_accum;       /* (P,1) */
    float* denom;                    /* (P,1) */
    float* max_radii2D;              /* (P) */
} BagsDensifyStats;
/* stats may be NULL.  P == 0 is a successful no-op. */
int bags_adam_step(const BagsAdamArgs* args, const BagsDensifyStats* stats, void* stream);

/* The per-camera Adam of a camera bank (BagsPoseBank above) in ONE launch for the n_rows cameras of a step: every camera has its
 * own torch.optim.Adam over three groups -- rotation (columns 0..3 of its row), translation (4..6), fov (7..8) -- as the reference
 * keeps them per camera (train.py steps the first two under --opt_cam, the fov pair under --opt_intrinsic), stepped only when the
 * camera is listed.  The update per element is the one of BagsAdamArgs, operation for operation.  groups[v][g] belongs to camera
 * rows[v]: step_size and bias_correction2_sqrt come from that (camera, group)'s OWN step count, formed by the caller in double.
 * A column whose group is not enabled, and every row not listed, is neither read nor written.  rows as for BagsPoseBank. */
typedef struct BagsPoseAdamGroup {
    int32_t enabled;                 /* 0: the group's columns of this row are left alone */
    float step_size;                 /* lr / (1 - beta1^step) */
    float bias_correction2_sqrt;     /* sqrt(1 - beta2^step) */
} BagsPoseAdamGroup;
typedef struct BagsPoseAdamArgs {
    int32_t N, n_rows;               /* n_rows in 1..BAGS_MAX_POSE_ROWS */
    float* leaves;                   /* (N,9), updated in place */
    const float* grad;               /* (N,9) */
    float* exp_avg;                  /* (N,9), updated in place */
    float* exp_avg_sq;               /* (N,9), updated in place */
    double beta1, beta2, eps;
    int32_t rows[BAGS_MAX_POSE_ROWS];
    BagsPoseAdamGroup groups[BAGS_MAX_POSE_ROWS][3];
} BagsPoseAdamArgs;
int bags_pose_adam_step(const BagsPoseAdamArgs* args, void* stream);

/* Densify-and-prune of the Gaussian set and the opacity reset (csrc/densify.hip): GaussianModel.densify_and_prune
 * (scene/gaussian_model.py:393-447, called from train.py:381-386) with the optimizer surgery of cat_tensors_to_optimizer
 * (:366-386) and _prune_optimizer (:324-340), and GaussianModel.reset_opacity.  With g = xyz_gradient_accum / denom (NaN -> 0),
 * s = max(exp(scaling)), o = sigmoid(opacity) of a source row:
 *   clone  |g| >= max_grad and s <= dense_threshold: the row stays and a copy is appended (moments zero);
 *   split  |g| >= max_grad and s >  dense_threshold: the row is removed, N children are appended with
 *          xyz = R(normalize(rotation)) (exp(scaling) * z) + xyz, scaling = log(exp(scaling) / (0.8 N)), the rest copied, moments zero;
 *   prune  last, every row present then: o < min_opacity, or, with use_screen_size, max_radii2D > max_screen_size or
 *          s > world_threshold (s of the row itself: a child is tested with its shrunk scale).
 * The published code zeroes max_radii2D before the prune step reads it (BAGS_SCREEN_PUBLISHED, the default: the radius test sees 0
 * for every row); BAGS_SCREEN_PRE_DENSIFY tests a kept original against the value it had before the call (clones, children: 0).
 * Output rows: kept originals in source order, clones in source order, then child k of the j-th surviving split row at k * S + j.
 * z: noise (P, N, 3), indexed by source row and child, or, with noise NULL, Philox-4x32-10 + Box-Muller keyed by
 * (seed, source row, child) inside the kernel: independent of the compaction, the same on every rank that passes the same seed.
 * A kept row keeps parameters and moments bit for bit.  No atomics; results are bitwise reproducible. */
#define BAGS_DENSIFY_MAX_GROUPS 8
#define BAGS_DENSIFY_MAX_CHILDREN 16
enum { BAGS_ROLE_OTHER = 0, BAGS_ROLE_XYZ = 1, BAGS_ROLE_SCALING = 2, BAGS_ROLE_ROTATION = 3, BAGS_ROLE_OPACITY = 4 };
enum { BAGS_SCREEN_PUBLISHED = 0, BAGS_SCREEN_PRE_DENSIFY = 1 };
enum { BAGS_COUNT_KEPT = 0, BAGS_COUNT_CLONES = 1, BAGS_COUNT_SPLIT = 2, BAGS_COUNT_PRUNED = 3, BAGS_COUNT_P_NEW = 4,
       BAGS_COUNT_CLONES_OUT = 5, BAGS_COUNT_CHILDREN_OUT = 6, BAGS_DENSIFY_COUNTS = 8 };
typedef struct BagsDensifyRule {
    int32_t P;                       /* source rows */
    int32_t N;                       /* children per split row, 1..BAGS_DENSIFY_MAX_CHILDREN (the reference: 2) */
    float max_grad;
    float min_opacity;
    float dense_threshold;           /* percent_dense * extent */
    float world_threshold;           /* 0.1 * extent */
    float max_screen_size;
    int32_t use_screen_size;         /* 0: the reference's max_screen_size = None (neither size test) */
    int32_t screen_size_mode;        /* BAGS_SCREEN_* */
    int32_t reserved;
    uint64_t seed;                   /* of the in-kernel generator; unused with noise */
    const float* noise;              /* (P, N, 3) standard normals or NULL */
    const float* xyz_gradient_accum; /* (P,1) */
    const float* denom;              /* (P,1) */
    const float* max_radii2D;        /* (P) */
    const float* scaling;            /* (P,3) log-scale */
    const float* opacity;            /* (P,1) pre-sigmoid */
} BagsDensifyRule;
typedef struct BagsDensifyGroup {
    const float* param;              /* (P, width) */
    const float* exp_avg;            /* (P, width), or NULL with exp_avg_sq and both outputs: a group without optimizer state */
    const float* exp_avg_sq;
    float* param_out;                /* (P_new, width), 16-byte aligned like every output */
    float* exp_avg_out;
    float* exp_avg_sq_out;
    int32_t width;                   /* floats per Gaussian, >= 1 */
    int32_t role;                    /* BAGS_ROLE_*: xyz, scaling and rotation must each be given exactly once */
} BagsDensifyGroup;
/* plan: decide + scan, then ONE stream synchronisation that hands host_counts[BAGS_DENSIFY_COUNTS] to the caller: kept originals,
 * rows cloned, rows split, rows the prune step removed, P_new, clones and children in the output.  workspace: caller-owned device
 * memory of the size bags_densify_workspace_size gives for P; it carries the plan to apply.
 * apply: takes the same rule and workspace and the P_new of the plan, and writes every output array, the three statistics arrays
 * of the new size (zero) and provenance, int32 (P_new, 2): source row and kind (0 kept, 1 clone, 2 + k child k).  provenance is
 * required: it is the gather index of the copy.  Outputs must not alias inputs.  P == 0 (plan) and P_new == 0 (apply) are
 * successful no-ops. */
size_t bags_densify_workspace_size(int32_t P);
int bags_densify_plan(const BagsDensifyRule* rule, void* workspace, size_t workspace_bytes, int64_t* host_counts, void* stream);
int bags_densify_apply(const BagsDensifyRule* rule, const BagsDensifyGroup* groups, int32_t n_groups, void* workspace,
                       size_t workspace_bytes, int64_t P_new, float* xyz_gradient_accum_out, float* denom_out,
                       float* max_radii2D_out, int32_t* provenance, void* stream);
/* GaussianModel.reset_opacity: opacity = logit(min(sigmoid(opacity), 0.01)) in place, its two moments (either may be NULL) zeroed. */
int bags_reset_opacity(float* opacity, float* exp_avg, float* exp_avg_sq, int32_t P, void* stream);

/* The lens network that produces the control flow of bags_resample_* (csrc/lens_field.hip): the reference's invertible ResNet
 * (scene/iresnet.py, FrEIA's IResNetLayer shape) evaluated on M points of R^2.  A point goes through `blocks` residual blocks
 * x <- x + g_b(x); g_b is Linear(2, H), ELU, then `internal_layers` times (Linear(H, H), ELU), then Linear(H, 2), with ELU's
 * alpha = 1 and every weight in nn.Linear's (out, in) row-major layout.  params is ONE flat fp32 vector; per block, in order:
 * W_0 (H,2), b_0 (H), then W_i (H,H), b_i (H) for i = 1..internal_layers, then W_out (2,H), b_out (2), that is
 * 3H + n(H^2 + H) + 2H + 2 floats per block.  A wider net is a GEMM problem, not a launch-count one: it stays with PyTorch.
 * forward:  y (M,2) in one launch; a block's weights are staged once per workgroup in LDS and nothing per point leaves the chip but y.
 * backward: nothing is saved by the forward; every block's input and activations are recomputed from x.  grad_x (M,2) and
 *           grad_params (the length of params) may each be NULL; with grad_x NULL the first layer's input gradient is not formed.
 *           grad_params is written, not accumulated: per-workgroup partial sums in the workspace, added in workgroup order by a
 *           second launch.  No atomics: two runs give the same bits on any stream.  The workspace
 *           (bags_lens_field_workspace_size bytes) needs no initialisation; beside the partial sums it holds 8 bytes per point
 *           and block boundary.
 * inverse:  the blocks in reverse order, each by `iterations` steps of the fixed-point iteration x <- y - g_b(x) from x = y,
 *           which converges when every g_b is a contraction (LensField.lipschitz_correction keeps them so).  No gradient.
 * x, y and grad_y must not alias an output of the same call (forward and inverse may run in place: y == x).  M == 0 is a
 * successful no-op that still zero-fills grad_params. */
#define BAGS_LENS_MAX_HIDDEN 64
#define BAGS_LENS_MAX_INTERNAL_LAYERS 4
#define BAGS_LENS_MAX_BLOCKS 32
typedef struct BagsLensField {
    int32_t blocks, hidden, internal_layers, reserved;
    const float* params;             /* blocks * (3H + n(H^2 + H) + 2H + 2) floats */
} BagsLensField;
size_t bags_lens_field_workspace_size(int32_t blocks, int32_t hidden, int32_t internal_layers, int64_t M);
int bags_lens_field_forward(const BagsLensField* net, const float* x, int64_t M, float* y, void* stream);
int bags_lens_field_backward(const BagsLensField* net, const float* x, int64_t M, const float* grad_y, void* workspace,
                             size_t workspace_bytes, float* grad_x, float* grad_params, void* stream);
int bags_lens_field_inverse(const BagsLensField* net, const float* y, int64_t M, int32_t iterations, float* x, void* stream);

/* distCUDA2 of the reference's second native dependency (simple_knn._C, imported at scene/gaussian_model.py:20, called at
 * scene/gaussian_model.py:177 to initialise the scales): out[i] = mean of the squared distances from point i to its three
 * nearest neighbours (self excluded by index; coincident points count with distance 0; with fewer than four points the
 * missing neighbours contribute FLT_MAX).  points: device (P,3) fp32; out: device (P); workspace: caller-owned,
 * bags_knn_workspace_size(P) bytes.  Exact (uniform grid + shell walk), no host round trip, stream-ordered. */
size_t bags_knn_workspace_size(int32_t P);
int bags_knn_mean_dist2(const float* points, int32_t P, void* workspace, size_t workspace_bytes, float* out, void* stream);

/* The 3DGS-MCMC densification strategy (csrc/mcmc.hip): compute_relocation of utils/reloc_utils.py, relocate_gs / add_new_gs of
 * the reference's --mcmc path (train.py:366-367) and the per-iteration SGLD noise on xyz (train.py's noise_lr * xyz_lr block).
 *
 * compute_relocation, per row, with n = clamp(N, 1, n_max - 1) (clamped on read: N is not written):
 *     opacity_new = 1 - (1 - opacity_old)^(1/n)
 *     denom       = sum_{i=1..n} sum_{k=0..i-1} binoms[i-1][k] * (-1)^k / sqrt(k+1) * opacity_new^(k+1)
 *     scale_new   = (opacity_old / denom) * scale_old
 * binoms: (n_max, n_max) row-major, binoms[n][k] = C(n, k); n_max in 2..BAGS_MCMC_MAX_BINOMS.  The sums are formed in double, by
 * column (sum_i binoms[i-1][k] is exact there), and every output is rounded to fp32 once.  A NULL binoms, an n_max outside its
 * range and, with P > 0, a NULL input or output are argument errors, reported before any launch and also when P == 0; after that
 * check P == 0 is a successful no-op. */
#define BAGS_MCMC_MAX_BINOMS 51
int bags_compute_relocation(const float* opacity_old, const float* scale_old, const int32_t* N, const float* binoms,
                            int32_t n_max, int32_t P, float* opacity_new, float* scale_new, void* stream);

/* relocate_gs and add_new_gs.  `sampled` (n_sampled) lists source rows (repeats allowed); c[s] = how often s is listed.  Every
 * listed row s gets (o', sc') = compute_relocation(sigmoid(opacity[s]), exp(scaling[s]), c[s] + 1), o' clamped to
 * [min_opacity, 1 - FLT_EPSILON]; its opacity becomes logit(o'), its scaling log(sc'), and its exp_avg / exp_avg_sq are zeroed in
 * every group that has them.  The new values are staged in the workspace from the old rows before any row is written.
 *   relocate: in place.  Row dead[j] takes every parameter of row sampled[j] (opacity and scaling: the new ones), j = 0..n_sampled-1;
 *             its moments stay.  dead and sampled must be disjoint and dead must not repeat (the caller's check: the rows are on
 *             the device).  param_out / exp_avg_out / exp_avg_sq_out are not used.  Rows neither dead nor sampled are not touched.
 *   add_new:  writes (P + n_sampled)-row outputs in one pass over the output elements: rows 0..P-1 are the old rows (sources
 *             updated as above), row P + j is a copy of the updated row sampled[j] with zero moments; the three statistics arrays
 *             of the new size are zero-filled.  Outputs must not alias inputs and are 16-byte aligned.
 * roles: opacity and scaling must each be given exactly once (xyz and rotation are plain copies here).  workspace:
 * bags_mcmc_workspace_size(P) bytes, no initialisation needed.  n_sampled == 0 (and P == 0) is a successful no-op. */
typedef struct BagsMcmcGroup {
    float* param;                    /* (P, width) */
    float* exp_avg;                  /* (P, width), or NULL with exp_avg_sq (and both outputs): a group without optimizer state */
    float* exp_avg_sq;
    float* param_out;                /* add_new: (P + n_sampled, width) */
    float* exp_avg_out;
    float* exp_avg_sq_out;
    int32_t width;                   /* floats per Gaussian, >= 1 */
    int32_t role;                    /* BAGS_ROLE_* */
} BagsMcmcGroup;
size_t bags_mcmc_workspace_size(int32_t P);
int bags_mcmc_relocate(const BagsMcmcGroup* groups, int32_t n_groups, int32_t P, const int32_t* dead, const int32_t* sampled,
                       int32_t n_sampled, const float* binoms, int32_t n_max, double min_opacity, void* workspace,
                       size_t workspace_bytes, void* stream);
int bags_mcmc_add_new(const BagsMcmcGroup* groups, int32_t n_groups, int32_t P, const int32_t* sampled, int32_t n_sampled,
                      const float* binoms, int32_t n_max, double min_opacity, void* workspace, size_t workspace_bytes,
                      float* xyz_gradient_accum_out, float* denom_out, float* max_radii2D_out, void* stream);

/* The SGLD step on xyz, in place, one launch, nothing per row but the new xyz written:
 *     g = 1 / (1 + exp(-k * ((1 - sigmoid(opacity)) - x0)))
 *     Sigma = R diag(s^2) R^T,  s = scaling_modifier * exp(scaling),  R from the normalised quaternion (w, x, y, z)
 *     xyz += Sigma (z * g * scale)
 * z: noise (P,3), or, with noise NULL, three standard normals from the generator of bags_densify_apply keyed by (seed, row, 0).
 * Evaluated in double from the fp32 inputs and rounded once.  P == 0 is a successful no-op. */
int bags_mcmc_noise(float* xyz, const float* opacity, const float* scaling, const float* rotation, int32_t P, const float* noise,
                    uint64_t seed, double scale, double k, double x0, double scaling_modifier, void* stream);

/* Antialiased rendering (csrc/antialias.hip): upstream diff_gaussian_rasterization's `antialiasing` setting, the opacity scale
 * of Mip-Splatting's 2D filter.  The rasterizer adds 0.3 px^2 to the diagonal of every projected covariance; per Gaussian
 *     out = opacity * h,   h = sqrt(max(0.000025, det(cov2D) / det(cov2D + 0.3 I)))
 * makes the dilated Gaussian carry the energy of the original one.  h = 1 for a Gaussian the forward culls (view depth <= 0.2,
 * det(cov2D + 0.3 I) == 0).  cov2D is the operator's own: the same view-space point, entrance-pupil shift, Sigma, 1.3 x
 * field-of-view clamp and Jacobian as its forward, rounded the same way.  The operator is not involved: `out` goes in as its
 * `opacities`, and its dL/dopacities comes back as grad_out, which is upstream's antialiased forward and backward by the chain rule.
 * forward:  one launch, 4 bytes written per Gaussian.
 * backward: recomputes the forward from the inputs.  Every gradient pointer may be NULL (not wanted); a wanted one is written, not
 *           accumulated, and its bits do not depend on which others are wanted.  g_scales is the gradient of the scales as given
 *           (scale_modifier applied), g_rotations of the quaternion as given; g_viewmatrix and g_intrinsic are full (16) outputs
 *           (the entries nothing depends on are written as zeros: viewmatrix's fourth column, all of intrinsic but [0] and [5]).
 *           A culled Gaussian, or one on the floor, contributes grad_out * h to g_opacities and nothing else.  The three pose
 *           outputs are per-workgroup sums in the workspace added in double in workgroup order by a second launch: no atomics,
 *           two runs give the same bits.  The workspace (bags_antialias_workspace_size bytes, no initialisation) is needed only
 *           when a pose output is wanted.
 * P == 0 is a successful no-op (nothing is written). */
typedef struct BagsAntialias {
    int32_t P, image_width, image_height, clamp_grad;      /* clamp_grad: 0 stock, 1 exact, as BagsSettings */
    float tanfovx, tanfovy, scale_modifier; int32_t reserved;
    const float *means3D, *scales, *rotations, *cov3D_precomp;   /* scales + rotations, or cov3D_precomp */
    const float *opacities, *shift_factors;                     /* shift_factors (3) or NULL = zeros */
    const float *viewmatrix, *intrinsic;                        /* (16) each, device */
} BagsAntialias;
int    bags_antialias_forward(const BagsAntialias* args, float* out /* (P) */, void* stream);
size_t bags_antialias_workspace_size(int32_t P);
int    bags_antialias_backward(const BagsAntialias* args, const float* grad_out, void* workspace, size_t workspace_bytes,
                               float* g_opacities, float* g_means3D, float* g_scales, float* g_rotations, float* g_cov3D,
                               float* g_viewmatrix, float* g_intrinsic, float* g_shift_factors, void* stream);

/* Per-camera appearance (csrc/appearance.hip): lens vignetting, then upstream 3DGS's per-image 3x4 exposure matrix, applied to the
 * rendered image in sensor coordinates -- after the resample / stitch, in front of the loss.  The parameters of all N training
 * images sit in one (N,16) device table, the image-space twin of BagsPoseBank; row r is
 *     E (3,4) row-major in columns 0..11 | k1 k2 k3 in 12..14 | column 15 unused (never read; its gradient is exact zero).
 * For pixel (x, y) of a (3,H,W) image with channels p_0..p_2, centre (cx, cy) in pixels and s2 = (W*W + H*H) / 4:
 *     dx = x + 0.5 - cx ; dy = y + 0.5 - cy ; r2 = (dx*dx + dy*dy) / s2            (0 at the centre, 1 at a corner)
 *     f  = 1 + r2*(k1 + r2*(k2 + r2*k3))
 *     q_k = f * p_k
 *     out_c = q_0*E[0][c] + q_1*E[1][c] + q_2*E[2][c] + E[c][3]                    (upstream: image^T @ E[:3,:3] + E[:3,3])
 * evaluated in float32 in exactly this order; the neutral row E = [I | 0], k = 0 returns its input bit for bit.
 * forward:  ONE launch for the n_rows <= BAGS_MAX_POSE_ROWS images of a step; image[v] goes through row rows[v] into out[v].  The
 *           pointers and the row list travel by value: nothing is stacked, copied or uploaded.  out[v] must not overlap an input.
 * backward: two launches.  g_image (NULL, or n_rows pointers of which any may be NULL) receives dL/dimage.  g_table (N,16), or
 *           NULL, is written in EVERY element: the listed rows get their 15 sums -- per-workgroup partial rows in the workspace,
 *           added in double in a fixed order and rounded once -- every other row and column 15 exact zeros (no fill launch is
 *           needed in front).  No atomics, no host synchronisation; a repeated call gives the same bits, and each output the same
 *           bits whichever other is wanted.  How many workgroups a view has is decided by H and W alone (the constants
 *           below), so row v of a many-view call has the bits of a call of its own.  `out` of the struct is not read.
 * A thread takes four consecutive pixels of a row: one 16-byte access per channel where W % 4 == 0 and every pointer of the call
 * is 16-byte aligned, element by element otherwise, with the same bits either way.
 * workspace: bags_appearance_workspace_size bytes (0 for invalid arguments), 16-byte aligned, no initialisation; needed only
 *           when g_table is wanted.  H * W must be below 2^31. */
#define BAGS_APPEARANCE_BLOCK 256            /* threads per workgroup; a workgroup's tile is 256 quads = up to 1024 pixels */
#define BAGS_APPEARANCE_MIN_SLOTS 64         /* a view's backward has min(tiles, max(64, ceil(tiles / 4))) workgroups */
#define BAGS_APPEARANCE_TILES_PER_SLOT 4
typedef struct BagsAppearance {
    int32_t N;                               /* rows of the table, >= 1 */
    const float* table;                      /* (N,16) */
    int32_t n_rows;                          /* 1..BAGS_MAX_POSE_ROWS */
    int32_t rows[BAGS_MAX_POSE_ROWS];        /* distinct, each in [0, N) */
    int32_t C, H, W;                         /* C == 3 */
    float cx, cy;                            /* the optical centre in pixels; (W/2, H/2) is the image centre */
    const float* image[BAGS_MAX_POSE_ROWS];  /* (3,H,W) each, the first n_rows given */
    float* out[BAGS_MAX_POSE_ROWS];          /* (3,H,W) each (forward only) */
} BagsAppearance;
int    bags_appearance_forward(const BagsAppearance* app, void* stream);
size_t bags_appearance_workspace_size(int32_t n_rows, int32_t H, int32_t W);
int    bags_appearance_backward(const BagsAppearance* app, const float* const g_out[BAGS_MAX_POSE_ROWS], void* workspace,
                                size_t workspace_bytes, float* const g_image[BAGS_MAX_POSE_ROWS], float* g_table, void* stream);

/* Mip-Splatting's 3D smoothing filter (csrc/filter3d.hip), the other half of antialiased rendering: compute_3D_filter of its
 * GaussianModel for N cameras at once.  viewmatrices and intrinsics are (N,16) in the operator's row-vector convention (v, k below:
 * one camera's rows), sizes (N,2) int32 = (W, H) per camera.  Per Gaussian (x, y, z) and camera, in float32, each product and
 * sum rounded once, left to right:
 *     tx = x v0 + y v4 + z v8 + v12 ;  ty = x v1 + y v5 + z v9 + v13 ;  tz = x v2 + y v6 + z v10 + v14
 *     fx = k0 * (0.5 W) ;  fy = k5 * (0.5 H) ;  px = tx / tz * fx + 0.5 W ;  py = ty / tz * fy + 0.5 H
 *     valid = tz > 0.2  and  -0.15 W <= px <= 1.15 W  and  -0.15 H <= py <= 1.15 H
 *     dist  = min of tz over the valid cameras ;  focal = max of fx over all cameras
 *     dmax  = max of dist over the Gaussians with a valid camera (100000 when there is none)
 *     out   = ((a camera is valid ? dist : dmax) / focal) * sqrt(variance)
 * Two launches, no atomics, no host synchronisation, nothing allocated; min and max are exact, so the result repeats bit for bit
 * and does not depend on the order of the rows or of the cameras.  The workspace (bags_filter3d_workspace_size bytes, no
 * initialisation) holds dist and one maximum per workgroup.  P == 0 is a successful no-op; N <= 0 is an error. */
size_t bags_filter3d_workspace_size(int32_t P);
int    bags_filter3d_compute(const float* xyz /* (P,3) */, int32_t P, const float* viewmatrices, const float* intrinsics,
                             const int32_t* sizes, int32_t N, float variance, void* workspace, size_t workspace_bytes,
                             float* out /* (P) */, void* stream);

/* bags_activations_forward / _backward with the 3D filter applied (get_scaling_with_3D_filter / get_opacity_with_3D_filter), still
 * one launch each way; filter_3D (P) is the output of bags_filter3d_compute and a constant of the backward.  With s = exp(scaling),
 * f = filter_3D, sig = sigmoid(opacity):
 *     s'_a = sqrt(s_a^2 + f^2) ;  c = prod_a s_a / s'_a  ( = sqrt(prod s^2 / prod (s^2 + f^2)) )
 *     scales = s' ;  opacity = sig * c ;  shs and rotations as bags_activations_forward
 *     g_scaling_a = g_scales_a * s_a^2 / s'_a + g_opacity * sig * c * f^2 / s'_a^2 ;  g_opacity_raw = g_opacity * c * sig (1 - sig)
 * A cotangent that is NULL counts as zero (the opacity depends on the scaling too); an output pointer that is NULL is not written. */
int bags_activations_filtered_forward(const BagsRawGaussians* raw, const float* filter_3D, float* shs, float* opacity, float* scales,
                                      float* rotations, void* stream);
int bags_activations_filtered_backward(const BagsRawGaussians* raw, const float* filter_3D, const float* g_shs, const float* g_opacity,
                                       const float* g_scales, const float* g_rotations, float* g_features_dc, float* g_features_rest,
                                       float* g_opacity_raw, float* g_scaling, float* g_rotation, void* stream);

/* Depth priors on the rasterizer's maps (csrc/depth_prior.hip): depth D = sum w_i z_i and weights A = 1 - T_final of a view, a prior
 * p and an optional pixel weight m >= 0 (NULL: 1), all (H,W) float32.  A pixel is valid iff m > 0, A >= min_weight, D > 0 and
 * p > 0 (a NaN prior fails the last test); elsewhere nothing is summed and the gradients are exact zeros.  On valid pixels
 *     x = D / A (BAGS_DEPTH_PRIOR_DEPTH)  or  x = A / D (BAGS_DEPTH_PRIOR_INVERSE: the prior is an inverse depth), one float32
 *     division; w = m; n = sum w; everything after x is evaluated in double.
 *     BAGS_DEPTH_PRIOR_L1:       r = x - (a*p + b), L = sum w|r| / n, sign(0) = 0; (a, b) = row rows[v] of the (N,2) table (upstream's
 *                                depth_params), or (1, 0) with table == NULL.  n <= 0: L = 0.
 *     BAGS_DEPTH_PRIOR_PEARSON:  L = 1 - rho, rho = C / sqrt(Vx*Vp), Vx = sum w x^2 / n - (sum w x / n)^2, Vp likewise,
 *                                C = sum w x p / n - (sum w x / n)(sum w p / n).  A view with n <= 0, Vx <= 1e-12 * sum w x^2 / n or
 *                                Vp <= 1e-12 * sum w p^2 / n is degenerate: L = 0 and every gradient zero, never NaN.  table must be NULL.
 * forward:  two launches for the n_rows <= BAGS_MAX_POSE_ROWS views of a step (pointers by value, nothing stacked): a pixels kernel
 *           leaves one row of 8 doubles per workgroup in the workspace, a finalize kernel adds a view's rows in a fixed order and
 *           writes loss[v], count[v] = n and row v of stats (n_rows,8) float64:
 *               xbar, pbar, 1/sqrt(Vx*Vp), rho/Vx, 1/n, sum w sign(r) p, sum w sign(r), degenerate flag (1.0 or 0.0).
 *           No atomics, no memset, no host synchronisation.  A view has min(tiles, max(64, ceil(tiles / 4))) workgroups whatever
 *           n_rows is, so its results have the bits of a call of its own.
 * backward: g_loss (n_rows) are the cotangents of loss.  g_depth / g_weights (NULL, or n_rows pointers of which any may be NULL)
 *           receive dL/dD and dL/dA of every pixel, each rounded once from double, in one launch; g_table (N,2) or NULL (L1 with a
 *           table only) is written in EVERY element by one small launch from the stats row alone: listed rows
 *           g_v * (-sum w sign(r) p / n, -sum w sign(r) / n), every other row exact zeros.  stats is the forward's, for the same
 *           struct.  Each output has the same bits whichever other is wanted.
 * A thread takes four consecutive pixels of a row: one 16-byte access per map where W % 4 == 0 and every pointer of the call is
 * 16-byte aligned, element by element otherwise, with the same bits either way.
 * workspace: bags_depth_prior_workspace_size bytes (0 for invalid arguments), 16-byte aligned, no initialisation (forward only).
 * H * W must be below 2^31. */
#define BAGS_DEPTH_PRIOR_BLOCK 256           /* threads per workgroup; a workgroup's tile is 256 quads = up to 1024 pixels */
#define BAGS_DEPTH_PRIOR_MIN_SLOTS 64        /* a view's sums kernel has min(tiles, max(64, ceil(tiles / 4))) workgroups */
#define BAGS_DEPTH_PRIOR_TILES_PER_SLOT 4
#define BAGS_DEPTH_PRIOR_STATS 8             /* doubles per stats row (and per partial row of the workspace) */
#define BAGS_DEPTH_PRIOR_PEARSON 0           /* mode */
#define BAGS_DEPTH_PRIOR_L1 1
#define BAGS_DEPTH_PRIOR_DEPTH 0             /* space */
#define BAGS_DEPTH_PRIOR_INVERSE 1
typedef struct BagsDepthPrior {
    int32_t mode, space;
    int32_t H, W;
    float min_weight;
    int32_t n_rows;                          /* views of the call, 1..BAGS_MAX_POSE_ROWS */
    int32_t N;                               /* rows of the table (>= 1) when table is given, else ignored */
    int32_t reserved;
    const float* table;                      /* (N,2) rows (a, b), BAGS_DEPTH_PRIOR_L1 only; NULL: (1, 0) for every view */
    int32_t rows[BAGS_MAX_POSE_ROWS];        /* with a table: distinct, each in [0, N) */
    const float* depth[BAGS_MAX_POSE_ROWS];  /* (H,W) each, the first n_rows given */
    const float* weights[BAGS_MAX_POSE_ROWS];
    const float* prior[BAGS_MAX_POSE_ROWS];
    const float* mask[BAGS_MAX_POSE_ROWS];   /* any of them NULL: every pixel weighs 1 */
} BagsDepthPrior;
size_t bags_depth_prior_workspace_size(int32_t n_rows, int32_t H, int32_t W);
int    bags_depth_prior_forward(const BagsDepthPrior* args, void* workspace, size_t workspace_bytes, float* loss /* (n_rows) */,
                                float* count /* (n_rows) */, double* stats /* (n_rows,8) */, void* stream);
int    bags_depth_prior_backward(const BagsDepthPrior* args, const double* stats, const float* g_loss /* (n_rows) */,
                                 float* const g_depth[BAGS_MAX_POSE_ROWS], float* const g_weights[BAGS_MAX_POSE_ROWS],
                                 float* g_table /* (N,2) */, void* stream);

/* A normal prior on the rasterizer's maps (csrc/normal_prior.hip): the normals of the rendered depth by central differences, held
 * to a prior normal map.  Per view: maps D, A (H,W) float32, a pinhole (fx, fy, cx, cy) in pixels, prior normals p (3,H,W) in the
 * camera frame of the operator's view space (x right, y down, z forward), an optional pixel weight m >= 0 (H,W) (NULL: 1).
 *     solid(u,v)  = A >= min_weight  and  D > 0
 *     z           = D / A                      one division in the dtype of the maps; everything after it in float64
 *     P(u,v)      = z * ((u - cx)/fx, (v - cy)/fy, 1)
 *     dx = P(u+1,v) - P(u-1,v) ;  dy = P(u,v+1) - P(u,v-1)          (central differences, as 2DGS's depth_to_normal)
 *     N  = dy x dx ;  q = |N|^2 ;  n = N / sqrt(q)                   (faces the camera: n_z < 0 for a fronto-parallel wall)
 *     geometric(u,v) = the pixel and its four neighbours are inside the image and solid,
 *                      |z(u+1,v) - z(u-1,v)| <= max_jump * z(u,v)  and  |z(u,v+1) - z(u,v-1)| <= max_jump * z(u,v),
 *                      q is a positive finite number
 *     valid(u,v)  = geometric  and  m > 0  and  |p|^2 is finite and > 0.25      (a zero or NaN prior: "no prior here")
 *     ph = p / |p| ;  w = m on valid pixels ;  cnt = sum w
 *     mode="cos":  l = 1 - n . ph          mode="l1":  l = |n - ph|_1   (sign(0) = 0)
 *     L_v = sum w l / cnt                  cnt <= 0 (also every image with H < 3 or W < 3): L_v = 0, all gradients zero, never NaN
 * max_jump = inf switches the guard off.  Validity and the guard are decisions, not differentiated through; invalid pixels get
 * exact-zero gradients.  The pinhole is constant data (host doubles, by value): no gradient to it.  Backward, with
 * s = cot_v * w_c / cnt_v, g = dl/dn (-ph for cos, sign(n - ph) for l1) and G = s * (g - n (n . g)) / sqrt(q):
 *     dL/ddy = dx x G ;   dL/ddx = G x dy
 *     dL/dP(u+1,v) += dL/ddx ;  dL/dP(u-1,v) -= dL/ddx ;  dL/dP(u,v+1) += dL/ddy ;  dL/dP(u,v-1) -= dL/ddy
 *     dL/dz = ray . dL/dP ,  ray = ((u-cx)/fx, (v-cy)/fy, 1) ;   dL/dD = dL/dz / A ;   dL/dA = -(z / A) dL/dz
 * The centre pixel's own z enters only the guard.
 * forward:  two launches for the n_rows <= BAGS_MAX_POSE_ROWS views of a step (pointers and pinholes by value).  A workgroup takes
 *           a tile of BAGS_NORMAL_PRIOR_TILE_W x BAGS_NORMAL_PRIOR_TILE_H pixels, stages z and solid of the tile and a one-pixel
 *           halo in LDS and leaves one row (sum w l, sum w) of doubles in the workspace; a finalize kernel adds a view's rows in a
 *           fixed order and writes loss[v], count[v] = cnt and row v of stats (n_rows,2) float64: 1/cnt (0 where cnt <= 0), cnt.
 * backward: one launch.  g_loss (n_rows) are the cotangents of loss; g_depth / g_weights (NULL, or n_rows pointers of which any
 *           may be NULL) receive dL/dD and dL/dA of EVERY pixel, each rounded once from double; a pixel gathers from its four
 *           neighbouring centres in the fixed order left, right, upper, lower.  stats is the forward's, for the same struct.
 * No atomics, no memset, no host synchronisation; a view's loss, count and gradients have the bits of a call of its own.
 * bags_depth_to_normal: one launch, one view: normal (3,H,W) float32 = n and valid (H,W) uint8 by the geometric rule alone (no
 *           prior, no mask), zeros where not valid.
 * workspace: bags_normal_prior_workspace_size bytes (0 for invalid arguments), 16-byte aligned, no initialisation (forward only).
 * min_weight must be a positive number, max_jump a non-negative number or inf.  H * W must be below 2^31. */
#define BAGS_NORMAL_PRIOR_TILE_W 32          /* a workgroup of 256 threads takes a tile of 32 x 8 pixels */
#define BAGS_NORMAL_PRIOR_TILE_H 8
#define BAGS_NORMAL_PRIOR_STATS 2            /* doubles per stats row (and per partial row of the workspace) */
#define BAGS_NORMAL_PRIOR_COS 0              /* mode */
#define BAGS_NORMAL_PRIOR_L1 1
typedef struct BagsNormalPrior {
    int32_t mode;
    int32_t H, W;
    float min_weight;
    float max_jump;
    int32_t n_rows;                          /* views of the call, 1..BAGS_MAX_POSE_ROWS */
    double pinhole[BAGS_MAX_POSE_ROWS][4];   /* (fx, fy, cx, cy) in pixels per view; fx, fy non-zero and finite */
    const float* depth[BAGS_MAX_POSE_ROWS];  /* (H,W) each, the first n_rows given */
    const float* weights[BAGS_MAX_POSE_ROWS];
    const float* prior[BAGS_MAX_POSE_ROWS];  /* (3,H,W) each */
    const float* mask[BAGS_MAX_POSE_ROWS];   /* any of them NULL: every pixel weighs 1 */
} BagsNormalPrior;
size_t bags_normal_prior_workspace_size(int32_t n_rows, int32_t H, int32_t W);
int    bags_normal_prior_forward(const BagsNormalPrior* args, void* workspace, size_t workspace_bytes, float* loss /* (n_rows) */,
                                 float* count /* (n_rows) */, double* stats /* (n_rows,2) */, void* stream);
int    bags_normal_prior_backward(const BagsNormalPrior* args, const double* stats, const float* g_loss /* (n_rows) */,
                                  float* const g_depth[BAGS_MAX_POSE_ROWS], float* const g_weights[BAGS_MAX_POSE_ROWS], void* stream);
int    bags_depth_to_normal(const float* depth, const float* weights, int32_t H, int32_t W, const double pinhole[4], float min_weight,
                            float max_jump, float* normal /* (3,H,W) */, uint8_t* valid /* (H,W) */, void* stream);

/* The multi-view correspondence loss on the rasterizer's maps (csrc/correspondence.hip): a pixel of the source view is un-projected
 * with the rendered depth, carried into the target view with the two view matrices and held to the pixel a matcher says it
 * corresponds to (SPARF, CoR-GS).  Row vectors, x_cam = [X_w, 1] @ viewmatrix; view space x right, y down, z forward.  Per ordered
 * pair: source maps D, A (H,W) float32, view matrices Vi, Vj (4,4) float32 row-major ON THE DEVICE (the host never reads them),
 * match (2,H,W) = the target pixel (x, y) of source pixel (u, v), an optional confidence conf >= 0 (H,W) (NULL: 1), and host
 * pinholes (fx, fy, cx, cy) in pixels of both sides.
 *     solid(u,v) = A >= min_weight and D > 0
 *     z          = D / A                      one division in the dtype of the maps; everything after it in float64
 *     Ai = Vi[:3,:3]  bi = Vi[3,:3]  Aj = Vj[:3,:3]  bj = Vj[3,:3]
 *     M  = inv(Ai) @ Aj ;  c = bj - bi @ M    (the true inverse adj(Ai) / det(Ai), not the transpose)
 *     x_i = z * ((u - cx_i)/fx_i, (v - cy_i)/fy_i, 1) ;  x_j = x_i @ M + c
 *     valid(u,v) = solid and conf > 0 and match finite (both components) and x_j.z >= min_depth
 *     proj = (fx_j x_j.x / x_j.z + cx_j,  fy_j x_j.y / x_j.z + cy_j) ;  r = proj - match ;  e = |r|_2
 *     rho  = e^2 / 2 where e <= delta,  delta (e - delta / 2) elsewhere        (delta = inf: half the squared distance)
 *     w = conf on valid pixels ;  cnt = sum w ;  L_k = sum w rho / cnt
 * cnt <= 0, or det(Ai) zero or not finite: L_k = 0 and every gradient an exact zero, never NaN.  Validity is a decision, not
 * differentiated through; invalid pixels get exact-zero gradients.  No gradient to match, conf or the pinholes.
 * forward:  two launches for the n_rows <= BAGS_MAX_POSE_ROWS pairs of a call (pointers and pinholes by value).  A thread is a
 *           pixel, a workgroup the BAGS_CORRESPONDENCE_CHUNK consecutive pixels of a chunk, the grid (chunk, pair); lane 0 of a
 *           workgroup forms M and c in double.  A workgroup leaves one row (sum w rho, sum w) of doubles in the workspace; a
 *           finalize kernel adds a pair's rows in a fixed order and writes loss[k], count[k] = cnt and row k of stats (n_rows,2)
 *           float64: 1/cnt (0 where cnt <= 0), cnt.
 * backward: at most two launches.  g_loss (n_rows) are the cotangents of loss.  g_depth / g_weights (NULL, or n_rows pointers of
 *           which any may be NULL) receive dL/dD and dL/dA of EVERY pixel, each rounded once from double.  g_view_src / g_view_dst
 *           (likewise) receive dL/dVi and dL/dVj, all 16 floats each, the fourth column exact zeros: the pixel kernel leaves twelve
 *           partial sums per workgroup (sum x_i^T g_xj and sum g_xj) in the workspace and a second kernel adds them in a fixed
 *           order and chains in double through c = bj - bi @ M, M = inv(Ai) @ Aj and d inv(A) = -inv(A) dA inv(A).  The workspace
 *           is needed only where a matrix gradient is wanted.  stats is the forward's, for the same struct.
 * No atomics, no memset, no host synchronisation; a pair's loss, count and gradients have the bits of a call of its own, and each
 * output the same bits whichever other is wanted.
 * bags_reproject_pixels: one launch, the first pair of the struct alone (n_rows == 1; match and conf are not read): proj (2,H,W)
 *           float32 where the pixel is solid and x_j.z >= min_depth, zeros elsewhere; valid (H,W) uint8 where proj also lies inside
 *           the W_dst x H_dst image, -0.5 <= x < W_dst - 0.5 and -0.5 <= y < H_dst - 0.5.
 * workspace: bags_correspondence_workspace_size bytes (0 for invalid arguments), 16-byte aligned, no initialisation; one size
 *           serves the forward and the backward.
 * min_weight, min_depth and delta must be positive, delta may be inf.  H * W must be below 2^31. */
#define BAGS_CORRESPONDENCE_CHUNK 256        /* pixels per workgroup: a workgroup of 256 threads, a thread a pixel */
#define BAGS_CORRESPONDENCE_STATS 2          /* doubles per stats row (and per partial row of the forward) */
#define BAGS_CORRESPONDENCE_SUMS 12          /* doubles per workgroup of the backward's partial sums */
typedef struct BagsCorrespondence {
    int32_t H, W;
    int32_t n_rows;                          /* pairs of the call, 1..BAGS_MAX_POSE_ROWS */
    float min_weight;
    double min_depth;
    double delta;
    double pinhole_src[BAGS_MAX_POSE_ROWS][4];   /* (fx, fy, cx, cy) in pixels per pair; fx, fy non-zero and finite */
    double pinhole_dst[BAGS_MAX_POSE_ROWS][4];
    const float* depth[BAGS_MAX_POSE_ROWS];  /* (H,W) each, the first n_rows given: the SOURCE view's maps */
    const float* weights[BAGS_MAX_POSE_ROWS];
    const float* match[BAGS_MAX_POSE_ROWS];  /* (2,H,W) each */
    const float* conf[BAGS_MAX_POSE_ROWS];   /* any of them NULL: every pixel weighs 1 */
    const float* view_src[BAGS_MAX_POSE_ROWS];   /* (4,4) each, on the device */
    const float* view_dst[BAGS_MAX_POSE_ROWS];
} BagsCorrespondence;
size_t bags_correspondence_workspace_size(int32_t n_rows, int32_t H, int32_t W);
int    bags_correspondence_forward(const BagsCorrespondence* args, void* workspace, size_t workspace_bytes, float* loss /* (n_rows) */,
                                   float* count /* (n_rows) */, double* stats /* (n_rows,2) */, void* stream);
int    bags_correspondence_backward(const BagsCorrespondence* args, const double* stats, const float* g_loss /* (n_rows) */,
                                    void* workspace, size_t workspace_bytes, float* const g_depth[BAGS_MAX_POSE_ROWS],
                                    float* const g_weights[BAGS_MAX_POSE_ROWS], float* const g_view_src[BAGS_MAX_POSE_ROWS],
                                    float* const g_view_dst[BAGS_MAX_POSE_ROWS], void* stream);
int    bags_reproject_pixels(const BagsCorrespondence* args, int32_t H_dst, int32_t W_dst, float* proj /* (2,H,W) */,
                             uint8_t* valid /* (H,W) */, void* stream);

/* The photometric reprojection (warping) loss on the rasterizer's maps (csrc/warp.hip): a pixel of the source view is un-projected
 * with the rendered depth, carried into the target view with the two view matrices, the target view's image is sampled there,
 * bilinearly, and the sampled colour is held to the colour of the pixel (CF-3DGS, Nope-NeRF, the self-supervised-depth family).
 * Conventions, solid, z, M, c, x_i, x_j and proj are the correspondence loss's above, word for word.  Per ordered pair: source maps
 * D, A (H,W) float32, view matrices Vi, Vj (4,4) ON THE DEVICE, color_src (C,H,W) = the colour each source pixel is held to,
 * image_dst (C,H_dst,W_dst) = the image of view j that is sampled, an optional confidence conf >= 0 (H,W) (NULL: 1), optional target
 * maps depth_dst, weights_dst (H_dst,W_dst) for the occlusion test (both or neither), host pinholes of both sides.  C is 1 or 3.
 *     inside  = 0 <= proj.x <= W_dst - 1 and 0 <= proj.y <= H_dst - 1            (all four taps exist; pixel centres at whole numbers)
 *     x0 = floor(proj.x)  y0 = floor(proj.y)  ax = proj.x - x0  ay = proj.y - y0  x1 = min(x0 + 1, W_dst - 1)  y1 = min(y0 + 1, H_dst - 1)
 *     S_c = (1-ay) ((1-ax) T_c[y0,x0] + ax T_c[y0,x1]) + ay ((1-ax) T_c[y1,x0] + ax T_c[y1,x1])       T = image_dst, in float64
 *     dS_c/dproj = ((1-ay)(T_c[y0,x1]-T_c[y0,x0]) + ay (T_c[y1,x1]-T_c[y1,x0]),  (1-ax)(T_c[y1,x0]-T_c[y0,x0]) + ax (T_c[y1,x1]-T_c[y0,x1]))
 *     visible = no target maps given, or at the nearest target pixel (floor(proj + 0.5)), with z_t = D_t / A_t (one float32 division):
 *               A_t >= min_weight and D_t > 0 and |x_j.z - z_t| <= occlusion * z_t
 *     valid   = solid and det(Ai) usable and x_j.z >= min_depth and conf > 0 and inside and visible and every S_c, color_src_c finite
 *     r_c = S_c - color_src_c ;  rho = (1/C) sum_c (sqrt(r_c^2 + eps^2) - eps)                       (Charbonnier: L1 as eps -> 0)
 *     w = conf on valid pixels ;  cnt = sum w ;  L_k = sum w rho / cnt
 *     dL/dproj = s_k (w / cnt) (1/C) sum_c r_c / sqrt(r_c^2 + eps^2) * dS_c/dproj                    (s_k the cotangent)
 * From dL/dproj on, the backward is the correspondence loss's.  cnt <= 0, or det(Ai) zero or not finite: L_k = 0 and every gradient an
 * exact zero, never NaN.  Validity is a decision, not differentiated through (the bilinear cell and the occlusion test included);
 * invalid pixels get exact-zero gradients.  NO gradient to image_dst, color_src, the target maps, conf or the pinholes: a gradient to
 * the sampled image is a scatter, and this library writes no gradient with atomics.
 * forward / backward: launches, workspace rows (BAGS_CORRESPONDENCE_CHUNK pixels per workgroup), stats (n_rows,2), the NULL rules of
 *           the four gradient tables and the bitwise guarantees are those of bags_correspondence_forward / _backward.
 * bags_warp_image: one launch, the first pair of the struct alone (n_rows == 1; conf and color_src are not read): out (C,H,W) float32
 *           = S_c where the pixel is solid, x_j.z >= min_depth, inside, visible and every S_c finite, zeros elsewhere; valid (H,W)
 *           uint8 marks those pixels.
 * workspace: bags_warp_workspace_size bytes (0 for invalid arguments), 16-byte aligned, no initialisation; one size serves the forward
 *           and the backward.
 * min_weight and min_depth must be positive and finite, eps and occlusion too.  H * W and H_dst * W_dst must be below 2^31. */
typedef struct BagsWarp {
    int32_t H, W;
    int32_t n_rows;                          /* pairs of the call, 1..BAGS_MAX_POSE_ROWS */
    float min_weight;
    double min_depth;
    int32_t C;                               /* channels of color_src and image_dst: 1 or 3 */
    int32_t H_dst, W_dst;                    /* one target size per call; may differ from H, W */
    int32_t reserved;                        /* 0 */
    double eps;
    double occlusion;
    double pinhole_src[BAGS_MAX_POSE_ROWS][4];   /* (fx, fy, cx, cy) in pixels per pair; fx, fy non-zero and finite */
    double pinhole_dst[BAGS_MAX_POSE_ROWS][4];
    const float* depth[BAGS_MAX_POSE_ROWS];  /* (H,W) each, the first n_rows given: the SOURCE view's maps */
    const float* weights[BAGS_MAX_POSE_ROWS];
    const float* conf[BAGS_MAX_POSE_ROWS];   /* any of them NULL: every pixel weighs 1 */
    const float* view_src[BAGS_MAX_POSE_ROWS];   /* (4,4) each, on the device */
    const float* view_dst[BAGS_MAX_POSE_ROWS];
    const float* color_src[BAGS_MAX_POSE_ROWS];  /* (C,H,W) each */
    const float* image_dst[BAGS_MAX_POSE_ROWS];  /* (C,H_dst,W_dst) each */
    const float* depth_dst[BAGS_MAX_POSE_ROWS];  /* (H_dst,W_dst) each; NULL per pair, together with weights_dst: no occlusion test */
    const float* weights_dst[BAGS_MAX_POSE_ROWS];
} BagsWarp;
size_t bags_warp_workspace_size(int32_t n_rows, int32_t H, int32_t W);
int    bags_warp_forward(const BagsWarp* args, void* workspace, size_t workspace_bytes, float* loss /* (n_rows) */,
                         float* count /* (n_rows) */, double* stats /* (n_rows,2) */, void* stream);
int    bags_warp_backward(const BagsWarp* args, const double* stats, const float* g_loss /* (n_rows) */, void* workspace,
                          size_t workspace_bytes, float* const g_depth[BAGS_MAX_POSE_ROWS], float* const g_weights[BAGS_MAX_POSE_ROWS],
                          float* const g_view_src[BAGS_MAX_POSE_ROWS], float* const g_view_dst[BAGS_MAX_POSE_ROWS], void* stream);
int    bags_warp_image(const BagsWarp* args, float* out /* (C,H,W) */, uint8_t* valid /* (H,W) */, void* stream);

/* Per-image bilateral-grid colour (csrc/bilagrid.hip): gsplat's lib_bilagrid slice-and-apply on the rendered image, behind the
 * appearance step and in front of the loss, and the total variation of the grids.  The grids of all N training images are one
 * (N,12,L,Gy,Gx) device tensor in gsplat's layout: coefficient k = 4*c + j of a vertex is entry [c][j] of a 3x4 affine matrix; the
 * neutral grid is [I | 0] at every vertex.  For pixel (x, y) of a (3,H,W) image with channels p_0..p_2 and the grid G of its row:
 *     u = (x + 0.5) / W * (Gx - 1) ;  x0 = min(floor(u), Gx-1) ;  x1 = min(x0+1, Gx-1) ;  tx = u - x0      (v, y0, y1, ty likewise)
 *     luma = 0.299 p_0 + 0.587 p_1 + 0.114 p_2 ;  s = luma * (L-1) ;  w = clamp(s, 0, L-1)
 *     z0 = min(floor(w), L-1) ;  z1 = min(z0+1, L-1) ;  tz = w - z0 ;  lerp(a, b, t) = a + t * (b - a)
 *     plane(z) = lerp( lerp(G[k,z,y0,x0], G[k,z,y0,x1], tx), lerp(G[k,z,y1,x0], G[k,z,y1,x1], tx), ty )
 *     A[k] = lerp(plane(z0), plane(z1), tz) ;  out_c = A[4c] p_0 + A[4c+1] p_1 + A[4c+2] p_2 + A[4c+3]
 * in float32 in exactly this order (F.grid_sample, bilinear, align_corners, border padding, in its lerp form); the neutral grid
 * returns a finite image bit for bit.  dL/dimage has the direct term sum_c g_c A[4c+j] and the term through the guidance,
 * dtz * (L-1) * (0.299, 0.587, 0.114) with dtz = sum_k dL/dA[k] * (plane(z1)[k] - plane(z0)[k]), exactly zero where s <= 0 or
 * s >= L-1; nothing flows to u or v.
 * forward:  ONE launch for the n_rows <= BAGS_MAX_POSE_ROWS images of a step; image[v] goes through grid rows[v] into out[v].
 *           Pointers and the row list travel by value.  A workgroup takes a tile of BAGS_BILAGRID_TILE_W x BAGS_BILAGRID_TILE_H
 *           pixels; a tile that reaches at most BAGS_BILAGRID_STAGE_VERTS xy-vertices reads them from LDS, any other tile (an
 *           image smaller than its grid) from the grid directly, with the same bits; path = BAGS_BILAGRID_PATH_DIRECT makes
 *           every tile read directly.  out[v] must not overlap an input.
 * backward: at most two launches.  g_image (NULL, or n_rows pointers of which any may be NULL) receives dL/dimage in one pass
 *           over the pixels.  g_grids (N,12,L,Gy,Gx), or NULL, is written in EVERY element by one launch: a workgroup per
 *           (xy-vertex, output channel, view) walks the vertex's support rectangle, adds in double in a fixed order and rounds
 *           once; vertices no pixel reaches and rows that are not listed are exact zeros (no fill launch in front).  No atomics,
 *           no host synchronisation; a repeated call gives the same bits, each output the same bits whichever other is wanted,
 *           and a row of a many-view call the bits of a call of its own.  `out` of the struct is not read.
 * workspace: this decomposition keeps no partial sums; the size query is there for callers written against the other entry points
 *           of this header and reports 0 bytes, and the backward takes (NULL, 0).
 * total variation (gsplat's total_variation_loss): per axis d with n_d >= 2 the sum of the squared forward differences along d over
 *           12 * (n_d - 1) * the product of the other two sizes; the three terms added and divided by N; an axis of one vertex
 *           counts 0.  Forward: two launches (per-workgroup partial sums in double, then the one scalar `loss`); the workgroup
 *           count is decided by the element count alone.  Backward: one launch, a gather that writes every element of g_grids
 *           from the cotangent g_loss (one float on the device).  Its workspace holds the partial rows, no initialisation.
 * Supported: 1 <= Gx, Gy <= BAGS_BILAGRID_MAX_G, 1 <= L <= BAGS_BILAGRID_MAX_L, H * W below 2^31; anything else is an argument
 * error whose text points to bilagrid_torch, the same function in PyTorch. */
#define BAGS_BILAGRID_TILE_W 64              /* a workgroup of 256 threads takes a tile of 64 x 4 pixels, a thread a pixel */
#define BAGS_BILAGRID_TILE_H 4
#define BAGS_BILAGRID_STAGE_VERTS 9          /* xy-vertices a tile may reach and still stage them in LDS (3 x 3) */
#define BAGS_BILAGRID_MAX_G 64
#define BAGS_BILAGRID_MAX_L 16
#define BAGS_BILAGRID_TV_BLOCK 256           /* the TV forward has min(ceil(elements / 256), 1024) workgroups */
#define BAGS_BILAGRID_TV_MAX_BLOCKS 1024
#define BAGS_BILAGRID_PATH_AUTO 0            /* path */
#define BAGS_BILAGRID_PATH_DIRECT 1
typedef struct BagsBilagrid {
    int32_t N;                               /* grids of the bank, >= 1 */
    const float* grids;                      /* (N,12,L,Gy,Gx) */
    int32_t n_rows;                          /* 1..BAGS_MAX_POSE_ROWS */
    int32_t rows[BAGS_MAX_POSE_ROWS];        /* distinct, each in [0, N) */
    int32_t C, H, W;                         /* C == 3 */
    int32_t Gx, Gy, L;
    int32_t path;                            /* BAGS_BILAGRID_PATH_* */
    const float* image[BAGS_MAX_POSE_ROWS];  /* (3,H,W) each, the first n_rows given */
    float* out[BAGS_MAX_POSE_ROWS];          /* (3,H,W) each (forward only) */
} BagsBilagrid;
int    bags_bilagrid_forward(const BagsBilagrid* grid, void* stream);
size_t bags_bilagrid_workspace_size(int32_t n_rows, int32_t H, int32_t W);
int    bags_bilagrid_backward(const BagsBilagrid* grid, const float* const g_out[BAGS_MAX_POSE_ROWS], void* workspace,
                              size_t workspace_bytes, float* const g_image[BAGS_MAX_POSE_ROWS], float* g_grids, void* stream);
size_t bags_bilagrid_tv_workspace_size(int32_t N, int32_t Gx, int32_t Gy, int32_t L);
int    bags_bilagrid_tv_forward(const float* grids, int32_t N, int32_t Gx, int32_t Gy, int32_t L, void* workspace,
                                size_t workspace_bytes, float* loss /* (1) */, void* stream);
int    bags_bilagrid_tv_backward(const float* grids, int32_t N, int32_t Gx, int32_t Gy, int32_t L, const float* g_loss /* (1) */,
                                 float* g_grids, void* stream);

/* Per-Gaussian normals (csrc/gaussian_normals.hip): the shortest axis of every Gaussian in the camera frame of the V views of a
 * step (1 <= V <= BAGS_MAX_SH_VIEWS; more views: one call per chunk), turned towards the camera.  Its output is the operator's
 * colors_precomp of a second pass, which splats it into a normal map.  Per Gaussian and view, q = (w,x,y,z) as given:
 *     k     = first minimum of the three scales (a decision; only their order is read, so log-scales serve)
 *     c     = column k of Q(q) = |q|^2 R(q/|q|), formed without a division
 *     m_j   = sum_i c_i V[i,j] ;  t = mean @ V[:3,:3] + V[3,:3]               (row-vector convention, V (16) on the device)
 *     sigma = -1 if m . t > 0 else +1 ;  l2 = |m|^2 ;  live = l2 finite and > 0
 *     out   = sigma m / sqrt(l2) where live, (0,0,0) elsewhere
 * forward:  ONE launch whatever V is; a row is read once, 12 bytes are written per Gaussian and view.
 * backward: recomputes the forward.  grad_out[v] may be NULL: a view no loss uses, a zero cotangent.  g_rotations (P,4) or NULL: the gradient of the quaternion as given, summed over the V views,
 *           written once.  g_viewmatrix: NULL, or V pointers of which any may be NULL; a wanted one is a full (16) output whose
 *           fourth row and column are written as zeros.  There is no gradient to the scales or the means (k and sigma are
 *           decisions).  A dead row contributes exactly nothing.  The view-matrix outputs are per-workgroup sums in the workspace
 *           added in double in workgroup order by a second launch: no atomics, two runs give the same bits, and a view's result does
 *           not depend on the others of the call.  The workspace (bags_gaussian_normals_workspace_size bytes, no initialisation)
 *           is needed only when a view-matrix output is wanted.  A wanted output's bits do not depend on which others are wanted.
 * P == 0 is a successful no-op (nothing is written). */
typedef struct BagsGaussianNormals {
    int32_t P, V;
    const float *rotations, *scales, *means3D;           /* (P,4), (P,3), (P,3) */
    const float* viewmatrix[BAGS_MAX_SH_VIEWS];          /* (16) each, device, the first V given */
} BagsGaussianNormals;
int    bags_gaussian_normals_forward(const BagsGaussianNormals* args, float* const out[] /* V x (P,3) */, void* stream);
size_t bags_gaussian_normals_workspace_size(int32_t P, int32_t V);
int    bags_gaussian_normals_backward(const BagsGaussianNormals* args, const float* const grad_out[] /* V x (P,3) */, void* workspace,
                                      size_t workspace_bytes, float* g_rotations, float* const g_viewmatrix[], void* stream);

/* A rendered normal map held to a target normal map (csrc/normal_map.hip).  Per view: normal N (3,H,W), the weights map A (H,W), a
 * target p (3,H,W), an optional pixel weight m (H,W).
 *     valid = A >= min_weight and |N|^2 finite and > min_norm^2 and m > 0 and |p|^2 finite and > 0.25
 *     nh = N/|N| ; ph = p/|p| ; w = m on valid pixels ; cnt = sum w
 *     BAGS_NORMAL_PRIOR_COS: l = 1 - nh . ph     BAGS_NORMAL_PRIOR_L1: l = |nh - ph|_1, sign(0) = 0
 *     L = sum w l / cnt ;  cnt <= 0: L = 0 and all gradients zero
 * forward:  two launches for the n_rows <= BAGS_MAX_POSE_ROWS views of a step (pointers by value, nothing stacked): a pixels kernel
 *           whose workgroups each leave one row of 2 doubles in the workspace, and a finalize kernel that adds a view's rows in a
 *           fixed order and writes loss, count and the stats row (n_rows, BAGS_NORMAL_MAP_STATS) the backward reads.
 * backward: one launch; g_normal[v] (3,H,W) or NULL.  Invalid pixels get exact zeros.  No gradient to A, p or m.
 * No atomics, no memset: two runs give the same bits and a view's result does not depend on the others of the call.
 * workspace: bags_normal_map_workspace_size bytes (0 for invalid arguments), 16-byte aligned, no initialisation (forward only). */
#define BAGS_NORMAL_MAP_STATS 2              /* doubles per stats row (and per partial row of the workspace) */
typedef struct BagsNormalMap {
    int32_t mode, H, W;                      /* mode: BAGS_NORMAL_PRIOR_COS / BAGS_NORMAL_PRIOR_L1 */
    int32_t n_rows;                          /* views of the call, 1..BAGS_MAX_POSE_ROWS */
    float min_weight, min_norm;              /* min_norm >= 0 */
    const float* normal[BAGS_MAX_POSE_ROWS]; /* (3,H,W) each, the first n_rows given */
    const float* weights[BAGS_MAX_POSE_ROWS];/* (H,W) each */
    const float* prior[BAGS_MAX_POSE_ROWS];  /* (3,H,W) each */
    const float* mask[BAGS_MAX_POSE_ROWS];   /* any of them NULL: every pixel weighs 1 */
} BagsNormalMap;
size_t bags_normal_map_workspace_size(int32_t n_rows, int32_t H, int32_t W);
int    bags_normal_map_forward(const BagsNormalMap* args, void* workspace, size_t workspace_bytes, float* loss /* (n_rows) */,
                               float* count /* (n_rows) */, double* stats, void* stream);
int    bags_normal_map_backward(const BagsNormalMap* args, const double* stats, const float* g_loss /* (n_rows) */,
                                float* const g_normal[BAGS_MAX_POSE_ROWS], void* stream);

/* Edge-aware smoothness of the depth / weights maps and of a splatted normal map (csrc/smooth.hip): the regulariser beside the data
 * terms above (Monodepth2's get_smooth_loss, DN-Splatter's EdgeAwareTV and TVLoss, and their second-order variants).  Per view: a
 * field map, the weights map A (H,W), an optional guide image I (guide_channels,H,W) (guide_channels = 0: none), an optional pixel
 * weight m (H,W).
 *     BAGS_SMOOTH_DEPTH:  field = D (H,W) ; usable = A >= min_weight and D > 0 and m > 0 and x finite ; x = A / D
 *                         (BAGS_DEPTH_PRIOR_INVERSE) or D / A (BAGS_DEPTH_PRIOR_DEPTH), one division in float32 ;
 *                         normalize: mu = sum_usable x / n, F = x / mu ; else F = x
 *     BAGS_SMOOTH_NORMAL: field = N (3,H,W) ; usable = A >= min_weight and |N|^2 finite and > min_norm^2 and m > 0 ; F = N / |N|
 *     order 1: d = F(u+1,v) - F(u,v), g = mean_c |I(u+1,v) - I(u,v)| ;  order 2: d = F(u-1,v) - 2 F(u,v) + F(u+1,v),
 *              g = mean_c |I(u+1,v) - I(u-1,v)| / 2 ;  the same along v
 *     a stencil is valid when its members are inside the image and usable and g is finite ; e = exp(-gamma g) ; w = min of m over
 *     the members ; rho = mean over the channels of BAGS_SMOOTH_L1: sqrt(t^2 + eps^2) - eps (eps = 0: |t|, sign(0) = 0) or
 *     BAGS_SMOOTH_L2: t^2 (eps must be 0)
 *     L = S_x / cnt_x + S_y / cnt_y, S_dir = sum w e rho(d), cnt_dir = sum w (cnt_dir <= 0: that direction counts 0) ;
 *     count = cnt_x + cnt_y ;  a view with no valid stencil: L = 0 and all gradients zero
 * forward:  two launches for the n_rows <= BAGS_MAX_POSE_ROWS views of a step (pointers by value, nothing stacked), three where the
 *           depth kind is normalised: [the mean: bags_smooth_mean_slots rows of (sum x, n) per view;] a tile kernel whose workgroups
 *           each leave one row of BAGS_SMOOTH_PARTIALS doubles; a finalize kernel that adds a view's rows in a fixed order and writes
 *           loss, count and the stats row (n_rows, BAGS_SMOOTH_STATS): 1/cnt_x, 1/cnt_y, 1/mu, n, T, cnt_x, cnt_y, mu.
 * backward: one launch; g_field[v] ((H,W) or (3,H,W)) and, for the depth kind, g_weights[v] (H,W), each or NULL.  The normalised
 *           depth field also sends -T / (mu n) to every usable pixel.  Pixels that are not usable get exact zeros.  No gradient to
 *           the guide or the mask, and none to A of the normal kind (g_weights is not looked at there).
 * No atomics, no memset: two runs give the same bits, a view's result does not depend on the others of the call, and what is stored
 * is the same bits whichever outputs are wanted.
 * workspace: bags_smooth_workspace_size bytes (0 for invalid arguments), 16-byte aligned, no initialisation (forward only). */
#define BAGS_SMOOTH_TILE_W 32                /* a workgroup of 256 threads takes a tile of 32 x 8 pixels */
#define BAGS_SMOOTH_TILE_H 8
#define BAGS_SMOOTH_PARTIALS 6               /* doubles per partial row of the workspace */
#define BAGS_SMOOTH_STATS 8                  /* doubles per stats row */
#define BAGS_SMOOTH_MEAN_SLOTS 512           /* the mean has min(ceil(H W / 256), 512) workgroups per view */
#define BAGS_SMOOTH_DEPTH 0                  /* kind */
#define BAGS_SMOOTH_NORMAL 1
#define BAGS_SMOOTH_L1 0                     /* penalty */
#define BAGS_SMOOTH_L2 1
typedef struct BagsSmooth {
    int32_t kind;                            /* BAGS_SMOOTH_DEPTH / BAGS_SMOOTH_NORMAL */
    int32_t space;                           /* depth kind: BAGS_DEPTH_PRIOR_DEPTH / BAGS_DEPTH_PRIOR_INVERSE */
    int32_t order;                           /* 1 or 2 */
    int32_t penalty;                         /* BAGS_SMOOTH_L1 / BAGS_SMOOTH_L2 */
    int32_t normalize;                       /* depth kind: 0 or 1; the normal kind takes 0 */
    int32_t H, W;
    int32_t n_rows;                          /* views of the call, 1..BAGS_MAX_POSE_ROWS */
    int32_t guide_channels;                  /* 0 (no guide), 1 or 3 */
    int32_t reserved;                        /* 0 */
    float min_weight, min_norm;              /* min_norm >= 0 (normal kind) */
    double eps, gamma;                       /* both >= 0; eps == 0 with BAGS_SMOOTH_L2 */
    const float* field[BAGS_MAX_POSE_ROWS];  /* (H,W) or (3,H,W) each, the first n_rows given */
    const float* weights[BAGS_MAX_POSE_ROWS];/* (H,W) each */
    const float* guide[BAGS_MAX_POSE_ROWS];  /* (guide_channels,H,W) each; not looked at where guide_channels == 0 */
    const float* mask[BAGS_MAX_POSE_ROWS];   /* any of them NULL: every pixel weighs 1 */
} BagsSmooth;
size_t bags_smooth_workspace_size(int32_t n_rows, int32_t H, int32_t W);
int    bags_smooth_forward(const BagsSmooth* args, void* workspace, size_t workspace_bytes, float* loss /* (n_rows) */,
                           float* count /* (n_rows) */, double* stats, void* stream);
int    bags_smooth_backward(const BagsSmooth* args, const double* stats, const float* g_loss /* (n_rows) */,
                            float* const g_field[BAGS_MAX_POSE_ROWS], float* const g_weights[BAGS_MAX_POSE_ROWS], void* stream);

/* The regularisers on the Gaussians themselves (csrc/gaussian_reg.hip), over all P rows of the raw leaves: 3DGS-MCMC's opacity_reg and
 * scale_reg means, the minimum-scale (flatness) loss of PGSR / 2DGS-style recipes, PhysGaussian's anisotropy-ratio hinge, a hinge on
 * large scales and the opacity entropy of pruning recipes.  x = opacity_raw (P), r = scaling_raw (P,3), f = filter (P) or NULL,
 * select (P bytes, 0 / 1) or NULL: every row.
 *     no filter:  o = 1 / (1 + exp(-x)), s_a = exp(r_a) ;  filter:  s_a = sqrt(exp(r_a)^2 + f^2), o = sigmoid * prod_a exp(r_a) / s_a
 *     n = the selected rows ;  kmin / kmax: the first minimum / maximum of a row's raw r
 *     terms[0] opacity  sum o / n                                   terms[1] scale    sum sum_a s_a / (3 n)
 *     terms[2] flat     sum s_kmin / n                              terms[3] aniso    sum max(s_kmax / s_kmin - max_ratio, 0) / n
 *     terms[4] big      sum sum_a max(s_a - max_scale, 0) / (3 n)   terms[5] entropy  sum -(o log o + (1 - o) log(1 - o)) / n
 * The sums run over the selected rows.  Both hinges are strict; a row with o <= 0 or o >= 1 in float32 has no entropy.  A term whose
 * bit (1 << index) is not set in `terms` is an exact 0 and sends no gradient.  n == 0 (also P == 0): six zeros, zero gradients.
 * forward:  two launches: workgroups of BAGS_GAUSSIAN_REG_BLOCK threads each take BAGS_GAUSSIAN_REG_ROWS rows and leave one record of
 *           BAGS_GAUSSIAN_REG_STATS doubles; one workgroup adds the records in index order and writes terms (6), count (1) and the
 *           stats record (BAGS_GAUSSIAN_REG_STATS doubles: the six raw sums, n, 0).
 * backward: one launch; g_terms (6) and stats are read on the device.  g_opacity (P) and g_scaling (P,3), each or NULL, are written
 *           completely (rows that are not selected: zeros).  With a filter the opacity-based terms reach g_scaling through c.
 * No atomics, no memset: two runs give the same bits, and what is stored is the same bits whichever output is wanted.
 * workspace: bags_gaussian_reg_workspace_size bytes (0 for P <= 0: NULL is accepted), 16-byte aligned, no initialisation. */
#define BAGS_GAUSSIAN_REG_BLOCK 256          /* threads per workgroup */
#define BAGS_GAUSSIAN_REG_ROWS 1024          /* rows per workgroup of the sums kernel (and per workspace record) */
#define BAGS_GAUSSIAN_REG_STATS 8            /* doubles per workspace record and in the stats record */
#define BAGS_GAUSSIAN_REG_TERMS 6
typedef struct BagsGaussianReg {
    int32_t P;
    uint32_t terms;                          /* bit k: terms[k] is wanted; bits above BAGS_GAUSSIAN_REG_TERMS are refused */
    float max_ratio;                         /* >= 1 */
    float max_scale;                         /* >= 0 */
    const float* opacity_raw;                /* (P,1) */
    const float* scaling_raw;                /* (P,3) */
    const float* filter;                     /* (P,1) or NULL: unfiltered */
    const void* select;                      /* (P) bytes, non-zero: the row counts; NULL: every row */
} BagsGaussianReg;
size_t bags_gaussian_reg_workspace_size(int32_t P);
int    bags_gaussian_reg_forward(const BagsGaussianReg* args, void* workspace, size_t workspace_bytes, float* terms /* (6) */,
                                 float* count /* (1) */, double* stats, void* stream);
int    bags_gaussian_reg_backward(const BagsGaussianReg* args, const double* stats, const float* g_terms /* (6) */,
                                  float* g_opacity /* (P,1) or NULL */, float* g_scaling /* (P,3) or NULL */, void* stream);

/* The weights map itself held to a target, or to solid-or-empty (csrc/alpha.hip): the silhouette / mask loss of object-centric
 * captures, the sky loss of the urban recipes (target 1 - sky) and the alpha entropy.  Per view: the weights map A (H,W), an optional
 * target t (H,W) (constant data), an optional pixel weight m (H,W).
 *     usable = A finite and m > 0 and (BAGS_ALPHA_ENTROPY: always | the target modes: t finite; BAGS_ALPHA_BCE also 0 <= t <= 1)
 *     w = m on usable pixels ; cnt = sum w
 *     inside = lo < A < hi, compared in float32 (the caller rounds lo = eps and hi = 1 - eps once) ;
 *     a = A inside, lo where A <= lo, hi where A >= hi
 *     BAGS_ALPHA_BCE:     l = -(t log a + (1 - t) log(1 - a))     dl/dA = (a - t) / (a (1 - a)) inside, 0 outside
 *     BAGS_ALPHA_ENTROPY: l = -(a log a + (1 - a) log(1 - a))     dl/dA = log((1 - a) / a) inside, 0 outside ; target is not looked at
 *     BAGS_ALPHA_L1:      l = |A - t|, sign(0) = 0                BAGS_ALPHA_L2: l = (A - t)^2
 *     L = sum w l / cnt ;  cnt <= 0: L = 0 and the gradient all zeros
 * forward:  two launches for the n_rows <= BAGS_MAX_POSE_ROWS views of a step (pointers by value, nothing stacked): a sums kernel of
 *           BAGS_ALPHA_GROUPS workgroups per view, whatever the size of the maps, each of which walks its own contiguous span of the
 *           view's pixels and leaves one row of BAGS_ALPHA_STATS doubles (cnt, sum w l; a zero row for an empty span), and a finalize
 *           kernel that adds a view's rows in index order and writes loss, count and the stats row (n_rows, BAGS_ALPHA_STATS) the
 *           backward reads.
 * backward: one launch; g_weights[v] (H,W) or NULL, written completely (pixels that are not usable: exact zeros); g_loss is read on
 *           the device.  No gradient to t or m; the clamp and the validity are decisions.
 * No atomics, no memset: two runs give the same bits and a view's result does not depend on the others of the call.
 * workspace: the grid is fixed, so the scratch is a constant and this family has no size function: BAGS_ALPHA_WORKSPACE_BYTES bytes
 *           whatever n_rows, H and W, 16-byte aligned, as given (another base is refused, not rounded), no initialisation (forward
 *           only).  Argument errors -- a base off 16 bytes, a buffer one byte short, an unknown mode, n_rows outside
 *           1..BAGS_MAX_POSE_ROWS, H W >= 2^31, a NULL among the first n_rows weights -- are reported before anything is enqueued. */
#define BAGS_ALPHA_BCE 0                     /* mode */
#define BAGS_ALPHA_L1 1
#define BAGS_ALPHA_L2 2
#define BAGS_ALPHA_ENTROPY 3
#define BAGS_ALPHA_STATS 2                   /* doubles per stats row (and per partial row of the workspace) */
#ifndef BAGS_ALPHA_GROUPS
#define BAGS_ALPHA_GROUPS 256                /* workgroups per view of the sums kernel: a power of two <= 256 (profiles/alpha/NOTES.md) */
#endif
#define BAGS_ALPHA_WORKSPACE_BYTES (BAGS_MAX_POSE_ROWS * BAGS_ALPHA_GROUPS * BAGS_ALPHA_STATS * 8)
typedef struct BagsAlpha {
    int32_t mode, H, W;                      /* mode: BAGS_ALPHA_BCE / _L1 / _L2 / _ENTROPY */
    int32_t n_rows;                          /* views of the call, 1..BAGS_MAX_POSE_ROWS */
    float lo, hi;                            /* 0 < lo < hi < 1: eps and 1 - eps, each rounded once to float32 */
    const float* weights[BAGS_MAX_POSE_ROWS];/* (H,W) each, the first n_rows given */
    const float* target[BAGS_MAX_POSE_ROWS]; /* (H,W) each; not looked at with BAGS_ALPHA_ENTROPY */
    const float* mask[BAGS_MAX_POSE_ROWS];   /* any of them NULL: every pixel weighs 1 */
} BagsAlpha;
int    bags_alpha_forward(const BagsAlpha* args, void* workspace, size_t workspace_bytes, float* loss /* (n_rows) */,
                          float* count /* (n_rows) */, double* stats, void* stream);
int    bags_alpha_backward(const BagsAlpha* args, const double* stats, const float* g_loss /* (n_rows) */,
                           float* const g_weights[BAGS_MAX_POSE_ROWS], void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BAGS_RASTER_H */
