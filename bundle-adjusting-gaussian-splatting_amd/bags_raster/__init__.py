"""bags_raster -- MI355X-native pose-differentiable Gaussian rasterizer (host side).

Mirrors the operator API of the reference's ``diff_gaussian_rasterization`` package
(gaussian_renderer/__init__.py:14,50-65,110-121): ``GaussianRasterizationSettings``, ``GaussianRasterizer``.
"""
from .rasterizer import GaussianRasterizationSettings, GaussianRasterizer, rasterize_gaussians, debug_views

from .render import render, render_views, render_normals, PipelineParams
from .gaussians import GaussianBag, eval_sh, sh_colors, sh_colors_views
from .mcmc import compute_relocation, compute_relocation_torch, relocation_binoms
from .antialias import antialias_opacity, antialias_opacity_torch
from .filter3d import filter_3D, filter_3D_torch, filtered_activations_torch
from .appearance import AppearanceBank, apply_appearance, appearance_torch
from .bilagrid import BilateralGridBank, apply_bilagrid, bilagrid_torch, bilagrid_tv_loss, bilagrid_tv_loss_torch
from .depth_prior import DepthPriorBank, depth_prior_loss, depth_prior_loss_torch
from .normal_prior import normal_prior_loss, normal_prior_loss_torch, depth_to_normal, depth_to_normal_torch, pinhole_of
from .correspondence import correspondence_loss, correspondence_loss_torch, reproject_pixels, reproject_pixels_torch
from .warp import warp_image, warp_image_torch, warp_loss, warp_loss_torch
from .gaussian_normals import gaussian_normals, gaussian_normals_views, gaussian_normals_torch, gaussian_normals_views_torch
from .normal_map import normal_map_loss, normal_map_loss_torch
from .smooth import depth_smooth_loss, depth_smooth_loss_torch, normal_smooth_loss, normal_smooth_loss_torch
from .gaussian_reg import REG_TERMS, gaussian_reg_loss, gaussian_reg_loss_torch
from .alpha import alpha_loss, alpha_loss_torch
from .io import save_ply, load_ply, save_checkpoint, load_checkpoint, save_exposure_json, load_exposure_json
from .optim import GaussianAdam
from .pose_bank import PoseBank, PoseAdam
from .lens_field import LensField, lens_field, lens_field_torch
from .distortion import resample_faces, resample_faces_torch, cube_face_matrices

__all__ = ["GaussianRasterizationSettings", "GaussianRasterizer", "rasterize_gaussians", "debug_views",
           "compute_relocation", "compute_relocation_torch", "relocation_binoms", "antialias_opacity", "antialias_opacity_torch", "render", "render_views", "PipelineParams",
           "GaussianBag", "eval_sh", "sh_colors", "sh_colors_views",
           "save_ply", "load_ply", "save_checkpoint", "load_checkpoint", "GaussianAdam",
           "PoseBank", "PoseAdam", "LensField", "lens_field", "lens_field_torch",
           "resample_faces", "resample_faces_torch", "cube_face_matrices",
           "AppearanceBank", "apply_appearance", "appearance_torch", "save_exposure_json", "load_exposure_json",
           "BilateralGridBank", "apply_bilagrid", "bilagrid_torch", "bilagrid_tv_loss", "bilagrid_tv_loss_torch",
           "filter_3D", "filter_3D_torch", "filtered_activations_torch",
           "DepthPriorBank", "depth_prior_loss", "depth_prior_loss_torch",
           "normal_prior_loss", "normal_prior_loss_torch", "depth_to_normal", "depth_to_normal_torch", "pinhole_of",
           "correspondence_loss", "correspondence_loss_torch", "reproject_pixels", "reproject_pixels_torch",
           "warp_loss", "warp_loss_torch", "warp_image", "warp_image_torch",
           "gaussian_normals", "gaussian_normals_views", "gaussian_normals_torch", "gaussian_normals_views_torch", "render_normals",
           "normal_map_loss", "normal_map_loss_torch",
           "depth_smooth_loss", "depth_smooth_loss_torch", "normal_smooth_loss", "normal_smooth_loss_torch",
           "REG_TERMS", "gaussian_reg_loss", "gaussian_reg_loss_torch",
           "alpha_loss", "alpha_loss_torch"]
