"""ctypes binding of libbags_raster.so (include/bags_raster.h).  No torch types cross this boundary: only raw
device pointers (``tensor.data_ptr()``), ints and floats.  The library is built in-tree by ``__graft_entry__.build()``
(or ``make -C csrc``); importing this module without it raises -- there is no CPU or eager fallback.

A wrapper crosses the boundary with the helpers at the end of this module: ``require`` checks an argument, ``as_f32c`` /
``ptr`` / ``workspace`` prepare what is passed, ``call`` launches -- on the argument's device, on its current stream, which
every launching entry point takes as its LAST parameter."""
from __future__ import annotations

import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# BAGS_RASTER_LIB: another build of the SAME library (csrc/Makefile `asan`: host-side AddressSanitizer build for the CPU ABI
# tests).  Not a fallback: a missing file still raises.
LIB_PATH = os.environ.get("BAGS_RASTER_LIB") or os.path.join(_HERE, "libbags_raster.so")

ABI_VERSION = 11
TILES_AABB, TILES_OPACITY = 0, 1
DEPTH_Z, DEPTH_DISTANCE = 0, 1
BINNING_AUTO, BINNING_RADIX = 0, 1
CLAMP_GRAD_STOCK, CLAMP_GRAD_EXACT = 0, 1
CONIC_GRAD_STOCK, CONIC_GRAD_EXACT = 0, 1
BWD_ALL, BWD_BLEND, BWD_PREPROCESS = 0, 1, 2

c_fp = C.c_void_p  # device pointers travel as integers


class BagsSettings(C.Structure):
    _fields_ = [("image_height", C.c_int32), ("image_width", C.c_int32), ("tanfovx", C.c_float), ("tanfovy", C.c_float),
                ("scale_modifier", C.c_float), ("sh_degree", C.c_int32), ("sh_coeffs", C.c_int32),
                ("depth_key", C.c_int32), ("debug", C.c_int32), ("debug_iter", C.c_int32),
                ("tile_bounds", C.c_int32), ("binning", C.c_int32), ("clamp_grad", C.c_int32), ("conic_grad", C.c_int32),
                ("bg", c_fp), ("viewmatrix", c_fp), ("projmatrix", c_fp), ("intrinsic", c_fp), ("campos", c_fp)]


class BagsInputs(C.Structure):
    _fields_ = [("P", C.c_int32), ("means3D", c_fp), ("means2D", c_fp), ("shift_factors", c_fp), ("shs", c_fp),
                ("colors_precomp", c_fp), ("opacities", c_fp), ("scales", c_fp), ("rotations", c_fp),
                ("cov3D_precomp", c_fp), ("shs_rest", c_fp)]


class BagsState(C.Structure):
    _fields_ = [("geom", c_fp), ("geom_bytes", C.c_size_t), ("binning", c_fp), ("binning_bytes", C.c_size_t),
                ("image", c_fp), ("image_bytes", C.c_size_t)]


class BagsForwardOut(C.Structure):
    _fields_ = [("color", c_fp), ("radii", c_fp), ("depth", c_fp), ("weights", c_fp), ("mean2D", c_fp)]


class BagsBackwardArgs(C.Structure):
    _fields_ = [("grad_color", c_fp), ("num_rendered", C.c_int64), ("workspace", c_fp), ("workspace_bytes", C.c_size_t),
                ("grad_means3D", c_fp), ("grad_means2D", c_fp), ("grad_means2D_densify", c_fp), ("grad_shs", c_fp),
                ("grad_colors_precomp", c_fp), ("grad_opacities", c_fp), ("grad_scales", c_fp), ("grad_rotations", c_fp),
                ("grad_cov3D_precomp", c_fp), ("grad_viewmatrix", c_fp), ("grad_projmatrix", c_fp),
                ("grad_intrinsic", c_fp), ("grad_campos", c_fp), ("grad_shift_factors", c_fp),
                ("binning_capacity", C.c_int64), ("accumulate", C.c_int32), ("dense_per_tile", C.c_int32), ("grad_shs_rest", c_fp),
                ("phase", C.c_int32), ("reserved2", C.c_int32), ("grad_dldc", c_fp)]


class BagsExtraGrads(C.Structure):          # (ABI 11) cotangents of the depth and weights maps; either may be NULL
    _fields_ = [("grad_depth", c_fp), ("grad_weights", c_fp)]


class BagsDebugViews(C.Structure):
    _fields_ = [("tiles_touched", c_fp), ("rect", c_fp), ("depth_bits", c_fp), ("point_list", c_fp),
                ("keys_sorted", c_fp), ("ranges", c_fp), ("n_contrib", c_fp), ("final_T", c_fp)]


MAX_SH_VIEWS = 16


class BagsShViews(C.Structure):
    _fields_ = [("n_views", C.c_int32), ("reserved", C.c_int32), ("campos", c_fp * MAX_SH_VIEWS), ("dldc", c_fp * MAX_SH_VIEWS)]


# every symbol include/bags_raster.h declares: (restype, argtypes)
class BagsCamera(C.Structure):
    _fields_ = [("init_quaternion", C.c_void_p), ("delta_quaternion", C.c_void_p), ("init_translation", C.c_void_p),
                ("delta_translation", C.c_void_p), ("fovx", C.c_void_p), ("fovy", C.c_void_p),
                ("global_rotation", C.c_void_p), ("global_translation_scale", C.c_void_p),
                ("znear", C.c_float), ("zfar", C.c_float)]


MAX_POSE_ROWS = 16
POSE_LEAVES = 9                             # a row of the bank's tables: delta_quaternion 0..3 | delta_translation 4..6 | fovx 7 | fovy 8


class BagsPoseBank(C.Structure):            # the cameras of one step out of a bank of N; the row list travels by value
    _fields_ = [("N", C.c_int32), ("init_quaternion", c_fp), ("init_translation", c_fp), ("near_far", c_fp), ("leaves", c_fp),
                ("global_rotation", c_fp), ("global_translation_scale", c_fp), ("n_rows", C.c_int32), ("rows", C.c_int32 * MAX_POSE_ROWS)]


class BagsPoseAdamGroup(C.Structure):
    _fields_ = [("enabled", C.c_int32), ("step_size", C.c_float), ("bias_correction2_sqrt", C.c_float)]


class BagsPoseAdamArgs(C.Structure):
    _fields_ = [("N", C.c_int32), ("n_rows", C.c_int32), ("leaves", c_fp), ("grad", c_fp), ("exp_avg", c_fp), ("exp_avg_sq", c_fp),
                ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("rows", C.c_int32 * MAX_POSE_ROWS),
                ("groups", (BagsPoseAdamGroup * 3) * MAX_POSE_ROWS)]


class BagsRawGaussians(C.Structure):
    _fields_ = [("P", C.c_int32), ("K", C.c_int32), ("features_dc", C.c_void_p), ("features_rest", C.c_void_p),
                ("opacity", C.c_void_p), ("scaling", C.c_void_p), ("rotation", C.c_void_p)]


class BagsShColors(C.Structure):
    _fields_ = [("P", C.c_int32), ("K", C.c_int32), ("sh_degree", C.c_int32), ("reserved", C.c_int32), ("shs", c_fp), ("shs_rest", c_fp),
                ("xyz", c_fp), ("campos", c_fp)]


class BagsShColorsViews(C.Structure):       # the V <= MAX_SH_VIEWS views of one step; the pointer tables of its entry points: c_fp * V
    _fields_ = [("P", C.c_int32), ("K", C.c_int32), ("sh_degree", C.c_int32), ("V", C.c_int32), ("shs", c_fp), ("shs_rest", c_fp),
                ("xyz", c_fp), ("campos", c_fp * MAX_SH_VIEWS)]


ADAM_MAX_GROUPS = 8


class BagsAdamGroup(C.Structure):
    _fields_ = [("param", c_fp), ("grad", c_fp), ("exp_avg", c_fp), ("exp_avg_sq", c_fp), ("width", C.c_int32), ("reserved", C.c_int32),
                ("step_size", C.c_float), ("bias_correction2_sqrt", C.c_float)]


class BagsAdamArgs(C.Structure):
    _fields_ = [("P", C.c_int32), ("n_groups", C.c_int32), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
                ("visible", c_fp), ("groups", BagsAdamGroup * ADAM_MAX_GROUPS)]


class BagsDensifyStats(C.Structure):
    _fields_ = [("radii", c_fp), ("grad_means2D", c_fp), ("grad_stride", C.c_int32), ("reserved", C.c_int32),
                ("xyz_gradient_accum", c_fp), ("denom", c_fp), ("max_radii2D", c_fp)]


DENSIFY_MAX_GROUPS = 8
DENSIFY_MAX_CHILDREN = 16
ROLE_OTHER, ROLE_XYZ, ROLE_SCALING, ROLE_ROTATION, ROLE_OPACITY = 0, 1, 2, 3, 4
SCREEN_PUBLISHED, SCREEN_PRE_DENSIFY = 0, 1
COUNT_KEPT, COUNT_CLONES, COUNT_SPLIT, COUNT_PRUNED, COUNT_P_NEW, COUNT_CLONES_OUT, COUNT_CHILDREN_OUT, DENSIFY_COUNTS = 0, 1, 2, 3, 4, 5, 6, 8


class BagsDensifyRule(C.Structure):
    _fields_ = [("P", C.c_int32), ("N", C.c_int32), ("max_grad", C.c_float), ("min_opacity", C.c_float), ("dense_threshold", C.c_float),
                ("world_threshold", C.c_float), ("max_screen_size", C.c_float), ("use_screen_size", C.c_int32),
                ("screen_size_mode", C.c_int32), ("reserved", C.c_int32), ("seed", C.c_uint64), ("noise", c_fp),
                ("xyz_gradient_accum", c_fp), ("denom", c_fp), ("max_radii2D", c_fp), ("scaling", c_fp), ("opacity", c_fp)]


class BagsDensifyGroup(C.Structure):
    _fields_ = [("param", c_fp), ("exp_avg", c_fp), ("exp_avg_sq", c_fp), ("param_out", c_fp), ("exp_avg_out", c_fp),
                ("exp_avg_sq_out", c_fp), ("width", C.c_int32), ("role", C.c_int32)]


MCMC_MAX_BINOMS = 51


class BagsMcmcGroup(C.Structure):           # relocate: in place (the outputs unused); add_new: the (P + n_sampled)-row outputs
    _fields_ = [("param", c_fp), ("exp_avg", c_fp), ("exp_avg_sq", c_fp), ("param_out", c_fp), ("exp_avg_out", c_fp),
                ("exp_avg_sq_out", c_fp), ("width", C.c_int32), ("role", C.c_int32)]


LENS_MAX_HIDDEN, LENS_MAX_INTERNAL_LAYERS, LENS_MAX_BLOCKS = 64, 4, 32


class BagsLensField(C.Structure):           # the lens network: params is ONE flat vector, per block W_0 b_0 (W_i b_i) x n W_out b_out
    _fields_ = [("blocks", C.c_int32), ("hidden", C.c_int32), ("internal_layers", C.c_int32), ("reserved", C.c_int32), ("params", c_fp)]


MAX_FACES = 8


class BagsFaces(C.Structure):               # the faces of a cubemap: image pointers and the 3x3 matrices (row-major) by value
    _fields_ = [("n_faces", C.c_int32), ("C", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("image", c_fp * MAX_FACES),
                ("mats", (C.c_float * 9) * MAX_FACES)]


class BagsAntialias(C.Structure):           # one view's inputs of the antialiasing factor (csrc/antialias.hip); None = NULL
    _fields_ = [("P", C.c_int32), ("image_width", C.c_int32), ("image_height", C.c_int32), ("clamp_grad", C.c_int32),
                ("tanfovx", C.c_float), ("tanfovy", C.c_float), ("scale_modifier", C.c_float), ("reserved", C.c_int32),
                ("means3D", c_fp), ("scales", c_fp), ("rotations", c_fp), ("cov3D_precomp", c_fp), ("opacities", c_fp),
                ("shift_factors", c_fp), ("viewmatrix", c_fp), ("intrinsic", c_fp)]


APPEARANCE_BLOCK, APPEARANCE_MIN_SLOTS, APPEARANCE_TILES_PER_SLOT = 256, 64, 4      # include/bags_raster.h: BAGS_APPEARANCE_*


class BagsAppearance(C.Structure):          # the images of one step and their rows of the (N,16) appearance table (csrc/appearance.hip)
    _fields_ = [("N", C.c_int32), ("table", c_fp), ("n_rows", C.c_int32), ("rows", C.c_int32 * MAX_POSE_ROWS), ("C", C.c_int32),
                ("H", C.c_int32), ("W", C.c_int32), ("cx", C.c_float), ("cy", C.c_float), ("image", c_fp * MAX_POSE_ROWS),
                ("out", c_fp * MAX_POSE_ROWS)]


BILAGRID_TILE_W, BILAGRID_TILE_H, BILAGRID_STAGE_VERTS, BILAGRID_MAX_G, BILAGRID_MAX_L = 64, 4, 9, 64, 16      # include/bags_raster.h: BAGS_BILAGRID_*
BILAGRID_TV_BLOCK, BILAGRID_TV_MAX_BLOCKS = 256, 1024
BILAGRID_PATH_AUTO, BILAGRID_PATH_DIRECT = 0, 1


class BagsBilagrid(C.Structure):            # the images of one step and their rows of the (N,12,L,Gy,Gx) bilateral grids (csrc/bilagrid.hip)
    _fields_ = [("N", C.c_int32), ("grids", c_fp), ("n_rows", C.c_int32), ("rows", C.c_int32 * MAX_POSE_ROWS), ("C", C.c_int32),
                ("H", C.c_int32), ("W", C.c_int32), ("Gx", C.c_int32), ("Gy", C.c_int32), ("L", C.c_int32), ("path", C.c_int32),
                ("image", c_fp * MAX_POSE_ROWS), ("out", c_fp * MAX_POSE_ROWS)]


DEPTH_PRIOR_BLOCK, DEPTH_PRIOR_MIN_SLOTS, DEPTH_PRIOR_TILES_PER_SLOT, DEPTH_PRIOR_STATS = 256, 64, 4, 8      # include/bags_raster.h: BAGS_DEPTH_PRIOR_*
DEPTH_PRIOR_PEARSON, DEPTH_PRIOR_L1 = 0, 1
DEPTH_PRIOR_DEPTH, DEPTH_PRIOR_INVERSE = 0, 1


class BagsDepthPrior(C.Structure):          # the depth / weights / prior / mask maps of one step's views (csrc/depth_prior.hip); None = NULL
    _fields_ = [("mode", C.c_int32), ("space", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("min_weight", C.c_float),
                ("n_rows", C.c_int32), ("N", C.c_int32), ("reserved", C.c_int32), ("table", c_fp), ("rows", C.c_int32 * MAX_POSE_ROWS),
                ("depth", c_fp * MAX_POSE_ROWS), ("weights", c_fp * MAX_POSE_ROWS), ("prior", c_fp * MAX_POSE_ROWS),
                ("mask", c_fp * MAX_POSE_ROWS)]


NORMAL_PRIOR_TILE_W, NORMAL_PRIOR_TILE_H, NORMAL_PRIOR_STATS = 32, 8, 2      # include/bags_raster.h: BAGS_NORMAL_PRIOR_*
NORMAL_PRIOR_COS, NORMAL_PRIOR_L1 = 0, 1


class BagsNormalPrior(C.Structure):         # the maps, pinholes and prior normals of one step's views (csrc/normal_prior.hip); None = NULL
    _fields_ = [("mode", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("min_weight", C.c_float), ("max_jump", C.c_float),
                ("n_rows", C.c_int32), ("pinhole", (C.c_double * 4) * MAX_POSE_ROWS),
                ("depth", c_fp * MAX_POSE_ROWS), ("weights", c_fp * MAX_POSE_ROWS), ("prior", c_fp * MAX_POSE_ROWS),
                ("mask", c_fp * MAX_POSE_ROWS)]


CORRESPONDENCE_CHUNK, CORRESPONDENCE_STATS, CORRESPONDENCE_SUMS = 256, 2, 12      # include/bags_raster.h: BAGS_CORRESPONDENCE_*


class BagsCorrespondence(C.Structure):      # the source maps, matches, view matrices and pinholes of one call's ordered pairs (csrc/correspondence.hip); None = NULL
    _fields_ = [("H", C.c_int32), ("W", C.c_int32), ("n_rows", C.c_int32), ("min_weight", C.c_float), ("min_depth", C.c_double),
                ("delta", C.c_double), ("pinhole_src", (C.c_double * 4) * MAX_POSE_ROWS), ("pinhole_dst", (C.c_double * 4) * MAX_POSE_ROWS),
                ("depth", c_fp * MAX_POSE_ROWS), ("weights", c_fp * MAX_POSE_ROWS), ("match", c_fp * MAX_POSE_ROWS),
                ("conf", c_fp * MAX_POSE_ROWS), ("view_src", c_fp * MAX_POSE_ROWS), ("view_dst", c_fp * MAX_POSE_ROWS)]


class BagsWarp(C.Structure):                # the source maps, colours, target images and maps, view matrices and pinholes of one call's ordered pairs (csrc/warp.hip); None = NULL
    _fields_ = [("H", C.c_int32), ("W", C.c_int32), ("n_rows", C.c_int32), ("min_weight", C.c_float), ("min_depth", C.c_double),
                ("C", C.c_int32), ("H_dst", C.c_int32), ("W_dst", C.c_int32), ("reserved", C.c_int32), ("eps", C.c_double),
                ("occlusion", C.c_double), ("pinhole_src", (C.c_double * 4) * MAX_POSE_ROWS), ("pinhole_dst", (C.c_double * 4) * MAX_POSE_ROWS),
                ("depth", c_fp * MAX_POSE_ROWS), ("weights", c_fp * MAX_POSE_ROWS), ("conf", c_fp * MAX_POSE_ROWS),
                ("view_src", c_fp * MAX_POSE_ROWS), ("view_dst", c_fp * MAX_POSE_ROWS), ("color_src", c_fp * MAX_POSE_ROWS),
                ("image_dst", c_fp * MAX_POSE_ROWS), ("depth_dst", c_fp * MAX_POSE_ROWS), ("weights_dst", c_fp * MAX_POSE_ROWS)]


class BagsGaussianNormals(C.Structure):    # the Gaussians and the V <= MAX_SH_VIEWS view matrices of one call (csrc/gaussian_normals.hip)
    _fields_ = [("P", C.c_int32), ("V", C.c_int32), ("rotations", c_fp), ("scales", c_fp), ("means3D", c_fp),
                ("viewmatrix", c_fp * MAX_SH_VIEWS)]


NORMAL_MAP_STATS = 2                        # include/bags_raster.h: BAGS_NORMAL_MAP_STATS


class BagsNormalMap(C.Structure):           # the normal / weights / target / mask maps of one step's views (csrc/normal_map.hip); None = NULL
    _fields_ = [("mode", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("n_rows", C.c_int32), ("min_weight", C.c_float),
                ("min_norm", C.c_float), ("normal", c_fp * MAX_POSE_ROWS), ("weights", c_fp * MAX_POSE_ROWS),
                ("prior", c_fp * MAX_POSE_ROWS), ("mask", c_fp * MAX_POSE_ROWS)]


SMOOTH_TILE_W, SMOOTH_TILE_H, SMOOTH_PARTIALS, SMOOTH_STATS, SMOOTH_MEAN_SLOTS = 32, 8, 6, 8, 512      # include/bags_raster.h: BAGS_SMOOTH_*
SMOOTH_DEPTH, SMOOTH_NORMAL = 0, 1
SMOOTH_L1, SMOOTH_L2 = 0, 1


class BagsSmooth(C.Structure):              # the field / weights / guide / mask maps of one step's views (csrc/smooth.hip); None = NULL
    _fields_ = [("kind", C.c_int32), ("space", C.c_int32), ("order", C.c_int32), ("penalty", C.c_int32), ("normalize", C.c_int32),
                ("H", C.c_int32), ("W", C.c_int32), ("n_rows", C.c_int32), ("guide_channels", C.c_int32), ("reserved", C.c_int32),
                ("min_weight", C.c_float), ("min_norm", C.c_float), ("eps", C.c_double), ("gamma", C.c_double),
                ("field", c_fp * MAX_POSE_ROWS), ("weights", c_fp * MAX_POSE_ROWS), ("guide", c_fp * MAX_POSE_ROWS),
                ("mask", c_fp * MAX_POSE_ROWS)]


GAUSSIAN_REG_BLOCK, GAUSSIAN_REG_ROWS, GAUSSIAN_REG_STATS, GAUSSIAN_REG_TERMS = 256, 1024, 8, 6      # include/bags_raster.h: BAGS_GAUSSIAN_REG_*


class BagsGaussianReg(C.Structure):         # the raw leaves, the 3D filter and the row mask of one call (csrc/gaussian_reg.hip); None = NULL
    _fields_ = [("P", C.c_int32), ("terms", C.c_uint32), ("max_ratio", C.c_float), ("max_scale", C.c_float), ("opacity_raw", c_fp),
                ("scaling_raw", c_fp), ("filter", c_fp), ("select", c_fp)]


ALPHA_BCE, ALPHA_L1, ALPHA_L2, ALPHA_ENTROPY = 0, 1, 2, 3                          # include/bags_raster.h: BAGS_ALPHA_*
ALPHA_STATS, ALPHA_GROUPS = 2, 256
ALPHA_WORKSPACE_BYTES = MAX_POSE_ROWS * ALPHA_GROUPS * ALPHA_STATS * 8            # a constant: this family has no size function


class BagsAlpha(C.Structure):               # the weights / target / mask maps of one step's views (csrc/alpha.hip); None = NULL
    _fields_ = [("mode", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("n_rows", C.c_int32), ("lo", C.c_float), ("hi", C.c_float),
                ("weights", c_fp * MAX_POSE_ROWS), ("target", c_fp * MAX_POSE_ROWS), ("mask", c_fp * MAX_POSE_ROWS)]


SYMBOLS = {    "bags_abi_version": (C.c_int, []),
    "bags_build_info": (C.c_char_p, []),
    "bags_last_error": (C.c_char_p, []),
    "bags_geom_size": (C.c_size_t, [C.c_int32]),
    "bags_binning_size": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32]),
    "bags_image_size": (C.c_size_t, [C.c_int32, C.c_int32]),
    "bags_backward_workspace_size": (C.c_size_t, [C.c_int32, C.c_int64]),
    "bags_forward_prepare": (C.c_int, [C.POINTER(BagsSettings), C.POINTER(BagsInputs), C.POINTER(BagsState),
                                       C.POINTER(BagsForwardOut), C.POINTER(C.c_int64), C.c_void_p]),
    "bags_forward_finish": (C.c_int, [C.POINTER(BagsSettings), C.POINTER(BagsInputs), C.POINTER(BagsState),
                                      C.POINTER(BagsForwardOut), C.c_int64, C.c_void_p]),
    "bags_forward_prepare_async": (C.c_int, [C.POINTER(BagsSettings), C.POINTER(BagsInputs), C.POINTER(BagsState),
                                             C.POINTER(BagsForwardOut), C.c_void_p, C.c_void_p]),
    "bags_forward_finish_speculative": (C.c_int, [C.POINTER(BagsSettings), C.POINTER(BagsInputs), C.POINTER(BagsState),
                                                  C.POINTER(BagsForwardOut), C.c_int64, C.c_void_p]),
    "bags_backward": (C.c_int, [C.POINTER(BagsSettings), C.POINTER(BagsInputs), C.POINTER(BagsState),
                                C.POINTER(BagsBackwardArgs), C.c_void_p]),
    "bags_backward_ex": (C.c_int, [C.POINTER(BagsSettings), C.POINTER(BagsInputs), C.POINTER(BagsState),
                                   C.POINTER(BagsBackwardArgs), C.POINTER(BagsExtraGrads), C.c_void_p]),
    "bags_sh_gradient_from_views": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(BagsShViews), C.c_void_p, C.c_void_p,
                                              C.c_int32, C.c_void_p]),
    "bags_debug_views": (C.c_int, [C.POINTER(BagsSettings), C.POINTER(BagsInputs), C.POINTER(BagsState), C.c_int64,
                                   C.POINTER(BagsDebugViews), C.c_void_p]),
    "bags_profile_enable": (C.c_int, [C.c_int]),
    "bags_profile_stride": (C.c_int, [C.c_int]),
    "bags_profile_read": (C.c_int, [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "bags_loss_workspace_size": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "bags_loss_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t,
                                    C.c_void_p, C.c_void_p]),
    "bags_loss_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t,
                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    "bags_photometric_loss_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t,
                                                C.c_float, C.c_void_p, C.c_void_p]),
    "bags_photometric_loss_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t,
                                                 C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bags_camera_forward": (C.c_int, [C.POINTER(BagsCamera), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bags_camera_backward": (C.c_int, [C.POINTER(BagsCamera)] + [C.c_void_p] * 11),
    "bags_pose_bank_forward": (C.c_int, [C.POINTER(BagsPoseBank), c_fp, c_fp, c_fp, c_fp, C.c_void_p]),
    "bags_pose_bank_backward": (C.c_int, [C.POINTER(BagsPoseBank)] + [c_fp] * 7 + [C.c_void_p]),
    "bags_pose_adam_step": (C.c_int, [C.POINTER(BagsPoseAdamArgs), C.c_void_p]),
    "bags_resample_forward": (C.c_int, [C.c_void_p] + [C.c_int32] * 3 + [C.c_void_p] + [C.c_int32] * 6 + [C.c_void_p] * 4),
    "bags_resample_workspace_size": (C.c_size_t, [C.c_int32] * 4),
    "bags_resample_backward": (C.c_int, [C.c_void_p] + [C.c_int32] * 3 + [C.c_void_p] + [C.c_int32] * 6 +
                               [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bags_resample_faces_workspace_size": (C.c_size_t, [C.c_int32] * 5),
    "bags_resample_faces_forward": (C.c_int, [C.POINTER(BagsFaces), c_fp] + [C.c_int32] * 6 + [c_fp, c_fp, C.c_void_p]),
    "bags_resample_faces_backward": (C.c_int, [C.POINTER(BagsFaces), c_fp] + [C.c_int32] * 6 + [c_fp, c_fp, C.c_void_p, C.c_size_t,
                                               C.POINTER(c_fp), c_fp, C.c_void_p]),
    "bags_activations_forward": (C.c_int, [C.POINTER(BagsRawGaussians)] + [C.c_void_p] * 5),
    "bags_activations_backward": (C.c_int, [C.POINTER(BagsRawGaussians)] + [C.c_void_p] * 10),
    "bags_sh_colors_workspace_size": (C.c_size_t, [C.c_int32]),
    "bags_sh_colors_forward": (C.c_int, [C.POINTER(BagsShColors), c_fp, C.c_void_p]),
    "bags_sh_colors_backward": (C.c_int, [C.POINTER(BagsShColors), c_fp, C.c_void_p, C.c_size_t, c_fp, c_fp, c_fp, c_fp, C.c_void_p]),
    "bags_sh_colors_views_workspace_size": (C.c_size_t, [C.c_int32, C.c_int32]),
    "bags_sh_colors_views_forward": (C.c_int, [C.POINTER(BagsShColorsViews), C.POINTER(c_fp), C.c_void_p]),
    "bags_sh_colors_views_backward": (C.c_int, [C.POINTER(BagsShColorsViews), C.POINTER(c_fp), C.c_void_p, C.c_size_t, c_fp, c_fp, c_fp,
                                                C.POINTER(c_fp), C.c_void_p]),
    "bags_adam_step": (C.c_int, [C.POINTER(BagsAdamArgs), C.POINTER(BagsDensifyStats), C.c_void_p]),
    "bags_densify_workspace_size": (C.c_size_t, [C.c_int32]),
    "bags_densify_plan": (C.c_int, [C.POINTER(BagsDensifyRule), C.c_void_p, C.c_size_t, C.POINTER(C.c_int64), C.c_void_p]),
    "bags_densify_apply": (C.c_int, [C.POINTER(BagsDensifyRule), C.POINTER(BagsDensifyGroup), C.c_int32, C.c_void_p, C.c_size_t, C.c_int64,
                                     c_fp, c_fp, c_fp, c_fp, C.c_void_p]),
    "bags_reset_opacity": (C.c_int, [c_fp, c_fp, c_fp, C.c_int32, C.c_void_p]),
    "bags_lens_field_workspace_size": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int64]),
    "bags_lens_field_forward": (C.c_int, [C.POINTER(BagsLensField), c_fp, C.c_int64, c_fp, C.c_void_p]),
    "bags_lens_field_backward": (C.c_int, [C.POINTER(BagsLensField), c_fp, C.c_int64, c_fp, C.c_void_p, C.c_size_t, c_fp, c_fp, C.c_void_p]),
    "bags_lens_field_inverse": (C.c_int, [C.POINTER(BagsLensField), c_fp, C.c_int64, C.c_int32, c_fp, C.c_void_p]),
    "bags_knn_workspace_size": (C.c_size_t, [C.c_int32]),
    "bags_knn_mean_dist2": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "bags_compute_relocation": (C.c_int, [c_fp, c_fp, c_fp, c_fp, C.c_int32, C.c_int32, c_fp, c_fp, C.c_void_p]),
    "bags_mcmc_workspace_size": (C.c_size_t, [C.c_int32]),
    "bags_mcmc_relocate": (C.c_int, [C.POINTER(BagsMcmcGroup), C.c_int32, C.c_int32, c_fp, c_fp, C.c_int32, c_fp, C.c_int32, C.c_double,
                                     C.c_void_p, C.c_size_t, C.c_void_p]),
    "bags_mcmc_add_new": (C.c_int, [C.POINTER(BagsMcmcGroup), C.c_int32, C.c_int32, c_fp, C.c_int32, c_fp, C.c_int32, C.c_double,
                                    C.c_void_p, C.c_size_t, c_fp, c_fp, c_fp, C.c_void_p]),
    "bags_mcmc_noise": (C.c_int, [c_fp, c_fp, c_fp, c_fp, C.c_int32, c_fp, C.c_uint64] + [C.c_double] * 4 + [C.c_void_p]),
    "bags_antialias_forward": (C.c_int, [C.POINTER(BagsAntialias), c_fp, C.c_void_p]),
    "bags_antialias_workspace_size": (C.c_size_t, [C.c_int32]),
    "bags_antialias_backward": (C.c_int, [C.POINTER(BagsAntialias), c_fp, C.c_void_p, C.c_size_t] + [c_fp] * 8 + [C.c_void_p]),
    "bags_appearance_forward": (C.c_int, [C.POINTER(BagsAppearance), C.c_void_p]),
    "bags_appearance_workspace_size": (C.c_size_t, [C.c_int32] * 3),
    "bags_appearance_backward": (C.c_int, [C.POINTER(BagsAppearance), C.POINTER(c_fp), C.c_void_p, C.c_size_t, C.POINTER(c_fp), c_fp, C.c_void_p]),
    "bags_bilagrid_forward": (C.c_int, [C.POINTER(BagsBilagrid), C.c_void_p]),
    "bags_bilagrid_workspace_size": (C.c_size_t, [C.c_int32] * 3),
    "bags_bilagrid_backward": (C.c_int, [C.POINTER(BagsBilagrid), C.POINTER(c_fp), C.c_void_p, C.c_size_t, C.POINTER(c_fp), c_fp, C.c_void_p]),
    "bags_bilagrid_tv_workspace_size": (C.c_size_t, [C.c_int32] * 4),
    "bags_bilagrid_tv_forward": (C.c_int, [c_fp] + [C.c_int32] * 4 + [C.c_void_p, C.c_size_t, c_fp, C.c_void_p]),
    "bags_bilagrid_tv_backward": (C.c_int, [c_fp] + [C.c_int32] * 4 + [c_fp, c_fp, C.c_void_p]),
    "bags_depth_prior_workspace_size": (C.c_size_t, [C.c_int32] * 3),
    "bags_depth_prior_forward": (C.c_int, [C.POINTER(BagsDepthPrior), C.c_void_p, C.c_size_t, c_fp, c_fp, c_fp, C.c_void_p]),
    "bags_depth_prior_backward": (C.c_int, [C.POINTER(BagsDepthPrior), c_fp, c_fp, C.POINTER(c_fp), C.POINTER(c_fp), c_fp, C.c_void_p]),
    "bags_normal_prior_workspace_size": (C.c_size_t, [C.c_int32] * 3),
    "bags_normal_prior_forward": (C.c_int, [C.POINTER(BagsNormalPrior), C.c_void_p, C.c_size_t, c_fp, c_fp, c_fp, C.c_void_p]),
    "bags_normal_prior_backward": (C.c_int, [C.POINTER(BagsNormalPrior), c_fp, c_fp, C.POINTER(c_fp), C.POINTER(c_fp), C.c_void_p]),
    "bags_depth_to_normal": (C.c_int, [c_fp, c_fp, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.c_float, C.c_float, c_fp, C.c_void_p, C.c_void_p]),
    "bags_correspondence_workspace_size": (C.c_size_t, [C.c_int32] * 3),
    "bags_correspondence_forward": (C.c_int, [C.POINTER(BagsCorrespondence), C.c_void_p, C.c_size_t, c_fp, c_fp, c_fp, C.c_void_p]),
    "bags_correspondence_backward": (C.c_int, [C.POINTER(BagsCorrespondence), c_fp, c_fp, C.c_void_p, C.c_size_t, C.POINTER(c_fp), C.POINTER(c_fp),
                                               C.POINTER(c_fp), C.POINTER(c_fp), C.c_void_p]),
    "bags_reproject_pixels": (C.c_int, [C.POINTER(BagsCorrespondence), C.c_int32, C.c_int32, c_fp, C.c_void_p, C.c_void_p]),
    "bags_warp_workspace_size": (C.c_size_t, [C.c_int32] * 3),
    "bags_warp_forward": (C.c_int, [C.POINTER(BagsWarp), C.c_void_p, C.c_size_t, c_fp, c_fp, c_fp, C.c_void_p]),
    "bags_warp_backward": (C.c_int, [C.POINTER(BagsWarp), c_fp, c_fp, C.c_void_p, C.c_size_t, C.POINTER(c_fp), C.POINTER(c_fp), C.POINTER(c_fp),
                                     C.POINTER(c_fp), C.c_void_p]),
    "bags_warp_image": (C.c_int, [C.POINTER(BagsWarp), c_fp, C.c_void_p, C.c_void_p]),
    "bags_gaussian_normals_forward": (C.c_int, [C.POINTER(BagsGaussianNormals), C.POINTER(c_fp), C.c_void_p]),
    "bags_gaussian_normals_workspace_size": (C.c_size_t, [C.c_int32, C.c_int32]),
    "bags_gaussian_normals_backward": (C.c_int, [C.POINTER(BagsGaussianNormals), C.POINTER(c_fp), C.c_void_p, C.c_size_t, c_fp, C.POINTER(c_fp),
                                                 C.c_void_p]),
    "bags_normal_map_workspace_size": (C.c_size_t, [C.c_int32] * 3),
    "bags_normal_map_forward": (C.c_int, [C.POINTER(BagsNormalMap), C.c_void_p, C.c_size_t, c_fp, c_fp, c_fp, C.c_void_p]),
    "bags_normal_map_backward": (C.c_int, [C.POINTER(BagsNormalMap), c_fp, c_fp, C.POINTER(c_fp), C.c_void_p]),
    "bags_smooth_workspace_size": (C.c_size_t, [C.c_int32] * 3),
    "bags_smooth_forward": (C.c_int, [C.POINTER(BagsSmooth), C.c_void_p, C.c_size_t, c_fp, c_fp, c_fp, C.c_void_p]),
    "bags_smooth_backward": (C.c_int, [C.POINTER(BagsSmooth), c_fp, c_fp, C.POINTER(c_fp), C.POINTER(c_fp), C.c_void_p]),
    "bags_gaussian_reg_workspace_size": (C.c_size_t, [C.c_int32]),
    "bags_gaussian_reg_forward": (C.c_int, [C.POINTER(BagsGaussianReg), C.c_void_p, C.c_size_t, c_fp, c_fp, c_fp, C.c_void_p]),
    "bags_gaussian_reg_backward": (C.c_int, [C.POINTER(BagsGaussianReg), c_fp, c_fp, c_fp, c_fp, C.c_void_p]),
    "bags_alpha_forward": (C.c_int, [C.POINTER(BagsAlpha), C.c_void_p, C.c_size_t, c_fp, c_fp, c_fp, C.c_void_p]),
    "bags_alpha_backward": (C.c_int, [C.POINTER(BagsAlpha), c_fp, c_fp, C.POINTER(c_fp), C.c_void_p]),
    "bags_filter3d_workspace_size": (C.c_size_t, [C.c_int32]),
    "bags_filter3d_compute": (C.c_int, [c_fp, C.c_int32, c_fp, c_fp, c_fp, C.c_int32, C.c_float, C.c_void_p, C.c_size_t, c_fp, C.c_void_p]),
    "bags_activations_filtered_forward": (C.c_int, [C.POINTER(BagsRawGaussians), c_fp] + [C.c_void_p] * 5),
    "bags_activations_filtered_backward": (C.c_int, [C.POINTER(BagsRawGaussians), c_fp] + [C.c_void_p] * 10),
}

_lib = None


def load() -> C.CDLL:
    """dlopen the HIP library (once).  Raises if it is absent or its ABI does not match."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"bags_raster: {LIB_PATH} is missing. Build the HIP extension first "
            f"(python -c 'import __graft_entry__ as g; g.build()' or make -C csrc). There is no fallback path.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)           # AttributeError if the .so lacks a declared symbol
        fn.restype, fn.argtypes = res, args
    if lib.bags_abi_version() != ABI_VERSION:
        raise ImportError(f"bags_raster: ABI {lib.bags_abi_version()} != expected {ABI_VERSION}; rebuild the library")
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().bags_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"{what}: {msg} (code {rc})")


def profile_enable(mode) -> None:
    """0/False off, 1 dominant kernel only, 2/True every stage."""
    load().bags_profile_enable(2 if mode is True else int(mode))


def profile_stride(n: int) -> None:
    """mode 1: only every n-th launch of the dominant kernel carries timing events."""
    load().bags_profile_stride(int(n))


def profile_read():
    """{stage: (total_ms, intervals)} since the last read; synchronises on the recorded events."""
    n = 16
    names = (C.c_char_p * n)()
    ms = (C.c_double * n)()
    calls = (C.c_int64 * n)()
    k = load().bags_profile_read(n, names, ms, calls)
    return {names[i].decode(): (ms[i], calls[i]) for i in range(min(k, n))}


# ------------------------------------------------------------------------------------------------ crossing the boundary
def ptr(t):
    """What a ``c_void_p`` parameter or struct field takes for an optional tensor: None (NULL) or its device address."""
    return None if t is None else t.data_ptr()


def ptr_table(ts):
    """A ``const float* const []`` parameter or struct field: the device addresses of ``ts`` (None entries are NULL), host side."""
    return (c_fp * len(ts))(*[ptr(t) for t in ts])


def workspace(nbytes: int, device) -> torch.Tensor:
    """``nbytes`` of uninitialised scratch for the library.  Zero bytes give an empty tensor, whose ``data_ptr()`` is 0: the
    library receives (NULL, 0), which every entry point accepts wherever it needs no workspace."""
    return torch.empty(int(nbytes), dtype=torch.uint8, device=device)


def as_f32c(t):
    """A tensor as the library reads it: detached, float32, contiguous.  None stays None; a tensor that already qualifies comes
    back as it is (no copy, no launch)."""
    if t is None:
        return None
    if t.requires_grad:
        t = t.detach()
    return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.to(torch.float32).contiguous()


def require(op: str, name: str, t, *, gpu: bool = False, f32: bool = False, contiguous: bool = False, on=None, host: str = "",
            type_error=TypeError, layout_error=RuntimeError) -> None:
    """The argument check of every wrapper: argument ``name`` of operation ``op`` is a tensor and, as asked for, on a GPU
    (``gpu``), float32 (``f32``), dense and contiguous (``contiguous``), on the device of the tensor ``on``.  ``host`` ends the GPU
    message with the host-side alternative, e.g. " (use torch.optim.Adam on the host)".  A wrong device is a RuntimeError; a wrong
    type or dtype raises ``type_error`` and a wrong layout ``layout_error``, for the call sites whose callers catch another type."""
    if not isinstance(t, torch.Tensor):
        raise type_error(f"{op}: {name} must be a tensor, got {type(t).__name__}")
    if gpu and not t.is_cuda:
        raise RuntimeError(f"{op} runs only on an AMD GPU: {name} must be on a 'cuda' (ROCm) device, got {t.device}; it takes a GPU tensor, "
                           f"there is no CPU fallback{host}")
    if contiguous and t.is_sparse:
        raise RuntimeError(f"{op}: {name} is sparse; only dense tensors are supported")
    if f32 and t.dtype != torch.float32:
        raise type_error(f"{op}: {name} must be float32, got {t.dtype}")
    if contiguous and not t.is_contiguous():
        raise layout_error(f"{op}: {name} must be contiguous (shape {tuple(t.shape)}, strides {t.stride()})")
    if on is not None and t.device != on.device:
        raise RuntimeError(f"{op}: {name} is on {t.device}, expected {on.device}")


def call(name: str, device, *args) -> None:
    """Launch entry point ``name`` on ``device``: ``args`` followed by the ``cuda_stream`` of that device's current stream, which every
    launching entry point of ``SYMBOLS`` takes last; a failure raises with ``name`` and ``bags_last_error()``.  (The size queries and
    ``bags_profile_*`` take no stream: they are plain ``load().bags_...`` calls.)"""
    if name not in SYMBOLS:
        raise AttributeError(f"bags_raster: {name} is not an entry point of include/bags_raster.h (bags_raster._lib.SYMBOLS)")
    fn = getattr(load(), name)
    with torch.cuda.device(device):
        check(fn(*args, torch.cuda.current_stream(device).cuda_stream), name)
