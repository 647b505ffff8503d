"""``render()`` -- the Python caller of the rasterizer.

Mirror of the reference's ``gaussian_renderer.render`` (gaussian_renderer/__init__.py:30-133): same positional
arguments, same choice of covariance path (``pipe.compute_cov3D_python``) and colour path (``hybrid`` /
``pipe.convert_SHs_python`` / rasterizer-side SH), same returned dictionary.  Differences, all deliberate:

  * tensors are created on the device of ``pc.get_xyz`` instead of a hard-coded ``"cuda"``;
  * the camera chain (three calls in the reference, :57,58,61) is evaluated once per tensor, not once per use;
  * ``global_alignment`` may be ``None`` (the reference always passes a pair, ``train.py:250``);
  * ``shift_factors`` may be ``None`` (= zeros(3)); two extra keywords, ``depth_key`` (decision D6 of DESIGN.md) and
    ``depth_weights_grad`` (the returned ``depth`` / ``weights`` maps carry gradients; decision D5);
  * the two screen-space gradient sinks are leaf tensors (the reference: ``zeros + 0`` with ``retain_grad()``, :37-44);
  * on a GPU the Python-side SH colours (``hybrid`` / ``pipe.convert_SHs_python``) come from ``bags_raster.sh_colors``, one HIP
    launch each way, fed with ``_features_dc`` / ``_features_rest`` as stored; ``_python_colors`` is the host path.

``render_views()`` is ``render()`` for the V cameras of one step: the same dictionaries, the activations once, on the fused
colour path one ``bags_raster.sh_colors_views`` call for the colours of all the cameras, and for the cameras of a
``bags_raster.PoseBank`` one chain launch each way for all of them.

``render_normals()`` is the second pass of the normal-supervision recipes: the normal of every Gaussian
(``bags_raster.gaussian_normals_views``) splatted through the ``override_color`` path over a zero background.
"""
from __future__ import annotations

import math
from types import SimpleNamespace
from typing import Optional

import torch

from ._lib import MAX_POSE_ROWS, MAX_SH_VIEWS
from .gaussian_normals import gaussian_normals_views
from .gaussians import eval_sh, sh_colors, sh_colors_views
from .pose_bank import PoseBankCamera
from .rasterizer import GaussianRasterizationSettings, GaussianRasterizer


class PipelineParams(SimpleNamespace):
    """The three switches of arguments/__init__.py:67-72, and upstream's fourth, ``antialiasing`` (``pipe.antialiasing`` of the
    current 3DGS training scripts): the rasterizer settings' field of that name."""

    def __init__(self, convert_SHs_python: bool = False, compute_cov3D_python: bool = False, debug: bool = False,
                 antialiasing: bool = False):
        super().__init__(convert_SHs_python=convert_SHs_python, compute_cov3D_python=compute_cov3D_python, debug=debug,
                         antialiasing=antialiasing)


_ZERO3 = {}        # device -> zeros(3): the `shift_factors=None` stand-in (read-only: one fill launch per device, not per call)


def quaternion_multiply(q1: torch.Tensor, q2: torch.Tensor) -> torch.Tensor:
    """Hamilton product, (w,x,y,z)   (gaussian_renderer/__init__.py:19-28)."""
    w1, x1, y1, z1 = q1.unbind(-1)
    w2, x2, y2, z2 = q2.unbind(-1)
    return torch.stack((w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2,
                        w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                        w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                        w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2), dim=-1)


def _python_colors(pc, xyz, feats, campos: torch.Tensor, mlp_color) -> torch.Tensor:
    """SH -> RGB in Python: eval_sh on unit view directions, +0.5, clamp at 0  (gaussian_renderer/__init__.py:90-95)."""
    shs_view = feats.transpose(1, 2).reshape(-1, 3, (pc.max_sh_degree + 1) ** 2)
    dir_pp = xyz - campos.unsqueeze(0)
    dir_pp = dir_pp / dir_pp.norm(dim=1, keepdim=True)
    rgb = torch.clamp_min(eval_sh(pc.active_sh_degree, shs_view, dir_pp) + 0.5, 0.0)
    return rgb + mlp_color


def _activate(pc, pipe, hybrid: bool, override_color, features: bool = True) -> SimpleNamespace:
    """What a call needs from the Gaussian set, whichever camera it is for: the colour path and the activated parameters.
    ``features=False`` (``render_normals``): no colour is evaluated, so the feature tensor is not formed."""
    # activations: one fused launch when the container offers it (GaussianBag on a GPU), else the reference's properties
    # rasterizer-side SH colours and, on a GPU, the Python-side ones (bags_raster.sh_colors): the two feature parameters go to the
    # kernel as they are stored (shs = features_dc, shs_rest = features_rest), without get_features' torch.cat; every other colour
    # path needs the (P,K,3) tensor
    if pipe.compute_cov3D_python and getattr(pc, "filter_3D", None) is not None:
        raise NotImplementedError("render: pipe.compute_cov3D_python builds the covariance from the unfiltered leaves (get_covariance); with a "
                                  "3D filter set (GaussianBag.filter_3D) use the scale / rotation path")
    raster_sh = override_color is None and not (hybrid or pipe.convert_SHs_python)
    fused_colors = override_color is None and not raster_sh and pc.get_xyz.is_cuda
    rest = getattr(pc, "_features_rest", None)
    split = ((raster_sh or fused_colors) and torch.is_tensor(rest) and torch.is_tensor(getattr(pc, "_features_dc", None))
             and rest.dim() == 3 and rest.shape[1] >= 1 and rest.is_cuda)
    if hasattr(pc, "activated"):                               # GaussianBag: one fused launch each way
        xyz, features, opacity, scaling, rotation = pc.activated(features=features and not split)
    else:                                                      # any container with the reference's properties (GaussianModel)
        xyz, opacity, scaling, rotation = pc.get_xyz, pc.get_opacity, pc.get_scaling, pc.get_rotation
        features = None if (split or not features) else pc.get_features
    return SimpleNamespace(fused_colors=fused_colors, split=split, xyz=xyz, features=features, opacity=opacity, scaling=scaling,
                           rotation=rotation)


def _camera_chain(viewpoint_camera, global_alignment):
    """viewmatrix, projmatrix, intrinsic, campos of one camera (gaussian_renderer/__init__.py:57,58,61)."""
    ga = global_alignment if global_alignment is not None else (None, None)
    if hasattr(viewpoint_camera, "get_matrices"):              # one HIP launch (bags_raster.camera.PoseCamera)
        return viewpoint_camera.get_matrices(ga[0], ga[1])
    # any camera object with the reference's four getters
    viewmatrix = viewpoint_camera.get_world_view_transform(ga[0], ga[1])
    intrinsic = viewpoint_camera.get_intrinsic()
    projmatrix = (viewmatrix.unsqueeze(0).bmm(intrinsic.unsqueeze(0))).squeeze(0)
    return viewmatrix, projmatrix, intrinsic, viewmatrix.inverse()[3, :3]


def _rasterize_view(viewpoint_camera, pc, pipe, bg_color, mlp_color, shift_factors, hybrid, scaling_modifier, override_color, iteration,
                    depth_key, depth_weights_grad, act, matrices, fused_rgb, sinks=True):
    """One camera's rasterizer call and the returned dictionary.  ``act``: ``_activate``'s result; ``matrices``: ``_camera_chain``'s;
    ``fused_rgb``: this view's ``sh_colors`` / ``sh_colors_views`` output where ``act.fused_colors``, else None.  ``sinks=False``
    (``render_normals``): no screen-space gradient sinks are made, and the two entries are None."""
    xyz = act.xyz
    # zero tensors whose .grad receives the screen-space gradients (:37-44)
    # (leaves: `.grad` is populated as with the reference's `zeros + 0` / retain_grad() pair, without the two adds and the two
    # 6 MB gradient copies that pair costs per call)
    screenspace_points = torch.zeros_like(xyz, requires_grad=True) if sinks else None
    screenspace_points_densify = torch.zeros_like(xyz, requires_grad=True) if sinks else None
    viewmatrix, projmatrix, intrinsic, campos = matrices

    raster_settings = GaussianRasterizationSettings(
        image_height=int(viewpoint_camera.image_height),
        image_width=int(viewpoint_camera.image_width),
        tanfovx=math.tan(viewpoint_camera.FoVx * 0.5),        # the STATIC fov, not the learnable one (:47-48)
        tanfovy=math.tan(viewpoint_camera.FoVy * 0.5),
        bg=bg_color,
        scale_modifier=scaling_modifier,
        viewmatrix=viewmatrix,
        projmatrix=projmatrix,
        intrinsic=intrinsic,
        sh_degree=pc.active_sh_degree,
        campos=campos,
        prefiltered=False,
        debug=pipe.debug,
        debug_iter=iteration,
        depth_key=depth_key,
        antialiasing=getattr(pipe, "antialiasing", False),   # (a reference `pipe` may not have the attribute)
        depth_weights_grad=depth_weights_grad,
    )
    rasterizer = GaussianRasterizer(raster_settings=raster_settings)

    scales = rotations = cov3D_precomp = None
    if pipe.compute_cov3D_python:
        cov3D_precomp = pc.get_covariance(scaling_modifier)
    else:
        scales, rotations = act.scaling, act.rotation

    shs = shs_rest = colors_precomp = None
    if override_color is not None:
        colors_precomp = override_color
    elif act.fused_colors:                                     # one HIP launch each way; `+ mlp_color` stays in PyTorch
        colors_precomp = fused_rgb
        if not (isinstance(mlp_color, (int, float)) and mlp_color == 0):          # the reference passes 0
            colors_precomp = colors_precomp + mlp_color
    elif hybrid or pipe.convert_SHs_python:
        colors_precomp = _python_colors(pc, xyz, act.features, campos, mlp_color)
    elif act.split:
        shs, shs_rest = pc._features_dc, pc._features_rest
    else:
        shs = act.features

    if shift_factors is None:
        shift_factors = _ZERO3.get(xyz.device)
        if shift_factors is None:
            shift_factors = _ZERO3[xyz.device] = torch.zeros(3, device=xyz.device)

    rendered_image, radii, depth, weights, mean2D = rasterizer(
        means3D=xyz, means2D=screenspace_points, means2D_densify=screenspace_points_densify,
        shift_factors=shift_factors, shs=shs, colors_precomp=colors_precomp, opacities=act.opacity,
        scales=scales, rotations=rotations, cov3D_precomp=cov3D_precomp, **({"shs_rest": shs_rest} if shs_rest is not None else {}))

    return {"render": rendered_image,
            "viewspace_points": screenspace_points,
            "viewspace_points_densify": screenspace_points_densify,
            "visibility_filter": radii > 0,
            "radii": radii,
            "depth": depth,
            "weights": weights,
            "means2D": mean2D}


def render(viewpoint_camera, pc, pipe, bg_color: torch.Tensor, mlp_color, shift_factors, hybrid: bool = True,
           scaling_modifier: float = 1.0, override_color: Optional[torch.Tensor] = None, iteration: Optional[int] = None,
           global_alignment=None, depth_key: str = "z", depth_weights_grad: bool = False):
    """Signature and defaults of gaussian_renderer/__init__.py:30: ``mlp_color`` and ``shift_factors`` are positional and
    required, ``hybrid`` defaults to True (Python-side SH colours + ``mlp_color``).  ``shift_factors=None`` stands for the
    zero vector the reference keeps (train.py:125-126: its optimizer is never stepped)."""
    act = _activate(pc, pipe, hybrid, override_color)
    matrices = _camera_chain(viewpoint_camera, global_alignment)
    fused_rgb = None
    if act.fused_colors:
        if act.split:
            fused_rgb = sh_colors(pc.active_sh_degree, pc._features_dc, act.xyz, matrices[3], shs_rest=pc._features_rest)
        else:
            fused_rgb = sh_colors(pc.active_sh_degree, act.features, act.xyz, matrices[3])
    return _rasterize_view(viewpoint_camera, pc, pipe, bg_color, mlp_color, shift_factors, hybrid, scaling_modifier, override_color,
                           iteration, depth_key, depth_weights_grad, act, matrices, fused_rgb)


def _camera_chains(cameras, global_alignment):
    """``_camera_chain`` of every camera of a step.  Distinct rows of ONE ``PoseBank`` (``bank.camera(i)``) on a GPU go through the
    chain together, one launch each way per 16 cameras, and are unbound per view; any other list takes the per-camera path."""
    if cameras and all(isinstance(c, PoseBankCamera) and c.bank is cameras[0].bank for c in cameras):
        bank, rows = cameras[0].bank, [c.row for c in cameras]
        if bank.leaves.is_cuda and len(set(rows)) == len(rows):
            ga = global_alignment if global_alignment is not None else (None, None)
            matrices = []
            for b in range(0, len(rows), MAX_POSE_ROWS):
                matrices.extend(zip(*(t.unbind(0) for t in bank.get_matrices(rows[b:b + MAX_POSE_ROWS], ga[0], ga[1]))))
            return matrices
    return [_camera_chain(cam, global_alignment) for cam in cameras]


# render_views' fused colour branch: True = one sh_colors_views call per chunk of cameras, False = one sh_colors call per camera.
# (profiles/sh_colors/NOTES.md holds the measurement this default rests on.)
MULTI_VIEW_COLORS = True


def render_views(cameras, pc, pipe, bg_color: torch.Tensor, mlp_color, shift_factors, hybrid: bool = True,
                 scaling_modifier: float = 1.0, override_color: Optional[torch.Tensor] = None, iteration: Optional[int] = None,
                 global_alignment=None, depth_key: str = "z", depth_weights_grad: bool = False):
    """``[render(cam, pc, ...) for cam in cameras]`` for the views of ONE step (a cubemap's faces, a rank's V views): a list of
    ``render()``'s dictionaries, every tensor in them the bits ``render()`` gives for that camera.

    The activations are evaluated once for the list and the camera chain once per camera -- or, for the ``camera(i)`` objects of
    one ``PoseBank``, once per 16 cameras.  On ``render()``'s fused colour branch
    (a GPU, ``hybrid`` or ``pipe.convert_SHs_python``, no ``override_color``) the colours of up to 16 cameras come from one
    ``sh_colors_views`` call: the coefficient rows are read once each way for all of them, and one backward through the summed
    loss writes each Gaussian gradient once instead of accumulating it view by view.  On every other colour path each camera
    takes the path ``render()`` takes."""
    cameras = list(cameras)
    act = _activate(pc, pipe, hybrid, override_color)
    matrices = _camera_chains(cameras, global_alignment)
    fused_rgb = [None] * len(cameras)
    if act.fused_colors:
        shs, rest = (pc._features_dc, pc._features_rest) if act.split else (act.features, None)
        if MULTI_VIEW_COLORS:
            for b in range(0, len(cameras), MAX_SH_VIEWS):
                fused_rgb[b:b + MAX_SH_VIEWS] = sh_colors_views(pc.active_sh_degree, shs, act.xyz, [m[3] for m in matrices[b:b + MAX_SH_VIEWS]],
                                                                shs_rest=rest)
        else:
            fused_rgb = [sh_colors(pc.active_sh_degree, shs, act.xyz, m[3], shs_rest=rest) for m in matrices]
    return [_rasterize_view(cam, pc, pipe, bg_color, mlp_color, shift_factors, hybrid, scaling_modifier, override_color, iteration,
                            depth_key, depth_weights_grad, act, m, rgb) for cam, m, rgb in zip(cameras, matrices, fused_rgb)]


def render_normals(cameras, pc, pipe, shift_factors, scaling_modifier: float = 1.0, global_alignment=None, depth_key: str = "z",
                   depth_weights_grad: bool = False):
    """The rendered normal map of one camera (a dictionary) or of a list of cameras (a list of dictionaries): what ``render()`` gives
    with ``override_color = gaussian_normals(...)`` and a zero background.  ``"normal"`` is ``(3,H,W)``, ``sum_i w_i n_i`` in the
    camera frame of the operator's view space (x right, y down, z forward; a wall seen head-on has ``n_z < 0``, the convention of
    ``normal_prior_loss``); ``"weights"``, ``"depth"`` and ``"radii"`` are the operator's, the bits a ``render()`` call on the same
    inputs gives.  There are no densification sinks in it: those belong to the colour pass.  A precomputed colour reaches the blend
    unclamped, so the negative components arrive as they are.

    The activations are evaluated once and the camera chain as ``render_views`` does (the cameras of one ``PoseBank``: one chain
    launch each way per 16); the normals of up to 16 cameras come from one ``gaussian_normals_views`` call.  The decision input of
    ``gaussian_normals`` -- which axis is the shortest -- is ``pc._scaling`` as stored where the container has it (any monotone
    function of the scales serves), else the activated scaling: under a 3D filter much larger than a scale, ``sqrt(s^2 + f^2)`` can
    round to a tie in float32.  The gradient reaches the rotations (through the normals and through the operator), the positions,
    opacities and scales (through the operator) and the pose (both ways).  The pass costs one operator call per camera."""
    single = not isinstance(cameras, (list, tuple))
    cams = [cameras] if single else list(cameras)
    act = _activate(pc, pipe, hybrid=True, override_color="normals", features=False)      # (an override colour: no SH path, no feature tensor)
    matrices = _camera_chains(cams, global_alignment)
    order = getattr(pc, "_scaling", None)
    if not (torch.is_tensor(order) and tuple(order.shape) == tuple(act.scaling.shape)):
        order = act.scaling
    dev = act.xyz.device
    zero3 = _ZERO3.get(dev)
    if zero3 is None:
        zero3 = _ZERO3[dev] = torch.zeros(3, device=dev)
    out = []
    for b in range(0, len(cams), MAX_SH_VIEWS):
        normals = gaussian_normals_views(act.rotation, order.detach(), act.xyz.detach(), [m[0] for m in matrices[b:b + MAX_SH_VIEWS]])
        for cam, m, n in zip(cams[b:b + MAX_SH_VIEWS], matrices[b:b + MAX_SH_VIEWS], normals):
            r = _rasterize_view(cam, pc, pipe, zero3, 0, shift_factors, True, scaling_modifier, n, None, depth_key, depth_weights_grad, act,
                                m, None, sinks=False)
            out.append({"normal": r["render"], "weights": r["weights"], "depth": r["depth"], "radii": r["radii"]})
    return out[0] if single else out
