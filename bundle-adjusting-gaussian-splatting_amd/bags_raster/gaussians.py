"""Gaussian parameter container and the activations that feed the rasterizer.

Host-side mirror of the pieces of the reference's ``GaussianModel`` that sit on the hot path:

  * activations  ``get_xyz / get_scaling / get_rotation / get_opacity / get_features / get_covariance``
    (scene/gaussian_model.py:118-141; set up in ``setup_functions``, scene/gaussian_model.py:26-43)
  * ``build_rotation / build_scaling_rotation / strip_lowerdiag / strip_symmetric`` (utils/general_utils.py:114-163)
  * ``eval_sh / RGB2SH / SH2RGB`` (utils/sh_utils.py:57-122) -- the Python colour path of ``render()``; on a GPU that path is
    ``sh_colors``, one HIP launch each way (csrc/sh_colors.hip)
  * the consumers of the op's screen-space gradients, ``add_densification_stats``
    (scene/gaussian_model.py:449-455)

Everything here is device-agnostic torch (the reference hard-codes ``device="cuda"``); values are pinned by
tests/golden/{sh_basis,gaussian_activations}.npz, generated from the reference's own functions.
``GaussianBag.densify_and_prune`` and ``GaussianBag.reset_opacity`` (scene/gaussian_model.py:393-447 and ``reset_opacity``) are
fused HIP calls (csrc/densify.hip), as are the three call sites of the 3DGS-MCMC strategy, ``GaussianBag.relocate`` / ``add_new`` /
``mcmc_noise`` (csrc/mcmc.hip); unlike the rest of this module they run only on a GPU.  The optimizer step is
``bags_raster.optim.GaussianAdam``, PLY / checkpoint I/O ``bags_raster.io``.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import torch

from . import _lib as L
from .filter3d import filter_3D, filter_3D_torch, filtered_activations_torch
from .gaussian_reg import REG_TERMS, gaussian_reg_loss, gaussian_reg_loss_torch
from .mcmc import N_MAX, relocation_binoms

SH_C0 = 0.28209479177387814
_SH_C1 = 0.4886025119029199
_SH_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
_SH_C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
          1.445305721320277, -0.5900435899266435)


def sh_basis(deg: int, dirs: torch.Tensor) -> torch.Tensor:
    """Real SH basis values, ``(..., (deg+1)^2)``, in the reference's ordering and sign convention
    (utils/sh_utils.py:26-43 constants, :73-110 polynomials)."""
    if not 0 <= deg <= 3:
        raise ValueError("SH degree must be in 0..3")
    x, y, z = dirs[..., 0], dirs[..., 1], dirs[..., 2]
    cols = [torch.full_like(x, SH_C0)]
    if deg > 0:
        cols += [-_SH_C1 * y, _SH_C1 * z, -_SH_C1 * x]
    if deg > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        cols += [_SH_C2[0] * xy, _SH_C2[1] * yz, _SH_C2[2] * (2.0 * zz - xx - yy), _SH_C2[3] * xz, _SH_C2[4] * (xx - yy)]
        if deg > 2:
            cols += [_SH_C3[0] * y * (3.0 * xx - yy), _SH_C3[1] * xy * z, _SH_C3[2] * y * (4.0 * zz - xx - yy),
                     _SH_C3[3] * z * (2.0 * zz - 3.0 * xx - 3.0 * yy), _SH_C3[4] * x * (4.0 * zz - xx - yy),
                     _SH_C3[5] * z * (xx - yy), _SH_C3[6] * x * (xx - 3.0 * yy)]
    return torch.stack(cols, dim=-1)


def eval_sh(deg: int, sh: torch.Tensor, dirs: torch.Tensor) -> torch.Tensor:
    """``sh (..., C, K)`` coefficients, ``dirs (..., 3)`` unit directions -> ``(..., C)``  (utils/sh_utils.py:57-112)."""
    n = (deg + 1) ** 2
    if sh.shape[-1] < n:
        raise ValueError(f"need {n} SH coefficients, got {sh.shape[-1]}")
    return (sh[..., :n] * sh_basis(deg, dirs).unsqueeze(-2)).sum(-1)


def RGB2SH(rgb):
    return (rgb - 0.5) / SH_C0


def SH2RGB(sh):
    return sh * SH_C0 + 0.5


def inverse_sigmoid(x: torch.Tensor) -> torch.Tensor:
    return torch.log(x / (1.0 - x))


def build_rotation(r: torch.Tensor) -> torch.Tensor:
    """(N,4) quaternions (w,x,y,z), normalised here -> (N,3,3)   (utils/general_utils.py:129-152)."""
    q = r / torch.sqrt((r * r).sum(dim=1, keepdim=True))
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    rows = [1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
            2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
            2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]
    return torch.stack(rows, dim=1).view(-1, 3, 3)


def build_scaling_rotation(s: torch.Tensor, r: torch.Tensor) -> torch.Tensor:
    """L = R(q) diag(s)   (utils/general_utils.py:154-163)."""
    return build_rotation(r) * s.unsqueeze(1)


def strip_lowerdiag(L: torch.Tensor) -> torch.Tensor:
    """(N,3,3) -> (N,6) = xx, xy, xz, yy, yz, zz   (utils/general_utils.py:114-123)."""
    return torch.stack([L[:, 0, 0], L[:, 0, 1], L[:, 0, 2], L[:, 1, 1], L[:, 1, 2], L[:, 2, 2]], dim=1)


def strip_symmetric(sym: torch.Tensor) -> torch.Tensor:
    return strip_lowerdiag(sym)


def covariance_from_scaling_rotation(scaling: torch.Tensor, scaling_modifier: float, rotation: torch.Tensor) -> torch.Tensor:
    """The reference's ``covariance_activation`` (scene/gaussian_model.py:27-31): strip(L L^T), L = R diag(mod * s)."""
    L = build_scaling_rotation(scaling_modifier * scaling, rotation)
    return strip_symmetric(L @ L.transpose(1, 2))


class GaussianBag:
    """The Gaussian set as the reference stores it: raw (pre-activation) leaves plus activation properties.

    ``_features_dc (P,1,3)`` and ``_features_rest (P,K-1,3)`` are concatenated along dim 1 by ``get_features``
    (scene/gaussian_model.py:131-134), which is the ``(P,K,3)`` layout the rasterizer's ``shs`` argument takes.
    """

    def __init__(self, sh_degree: int):
        self.active_sh_degree = 0
        self.max_sh_degree = sh_degree
        e = torch.empty(0)
        self._xyz = self._features_dc = self._features_rest = self._scaling = self._rotation = self._opacity = e
        self.max_radii2D = self.xyz_gradient_accum = self.denom = e
        self.filter_3D = None                # (P,1) once compute_3D_filter has run; None: everything is unfiltered

    # ---- construction
    @classmethod
    def from_activated(cls, scene: Dict[str, torch.Tensor], sh_degree: int, device="cpu", requires_grad: bool = True) -> "GaussianBag":
        """Build from activated values (``synth_scene`` output): inverts the activations, as ``create_from_pcd`` does for
        its initial values (scene/gaussian_model.py:164-195)."""
        pc = cls(sh_degree)
        dev = torch.device(device)

        def leaf(t):
            return t.detach().to(dev, torch.float32).contiguous().requires_grad_(requires_grad)
        shs = scene["shs"]
        pc._xyz = leaf(scene["means3D"])
        pc._features_dc = leaf(shs[:, :1, :])
        pc._features_rest = leaf(shs[:, 1:, :])
        pc._scaling = leaf(torch.log(scene["scales"]))
        pc._rotation = leaf(scene["rotations"])
        pc._opacity = leaf(inverse_sigmoid(scene["opacities"]))
        P = pc._xyz.shape[0]
        pc.max_radii2D = torch.zeros(P, device=dev)
        pc.xyz_gradient_accum = torch.zeros(P, 1, device=dev)
        pc.denom = torch.zeros(P, 1, device=dev)
        pc.active_sh_degree = int(round(math.sqrt(shs.shape[1]))) - 1
        return pc

    def leaves(self):
        return [self._xyz, self._features_dc, self._features_rest, self._scaling, self._rotation, self._opacity]

    # ---- activations (scene/gaussian_model.py:118-141)
    @property
    def get_scaling(self):
        return torch.exp(self._scaling)

    @property
    def get_rotation(self):
        return torch.nn.functional.normalize(self._rotation)

    @property
    def get_xyz(self):
        return self._xyz

    @property
    def get_features(self):
        return torch.cat((self._features_dc, self._features_rest), dim=1)

    @property
    def get_opacity(self):
        return torch.sigmoid(self._opacity)

    def get_covariance(self, scaling_modifier: float = 1.0):
        return covariance_from_scaling_rotation(self.get_scaling, scaling_modifier, self._rotation)

    # ---- Mip-Splatting's 3D smoothing filter (its scene/gaussian_model.py: compute_3D_filter and the two *_with_3D_filter properties)
    def _checked_filter(self, what: str):
        """``filter_3D`` if it fits the set as it is now; a filter left over from before the set changed size raises."""
        f, P = self.filter_3D, self._xyz.shape[0]
        if f is None:
            raise RuntimeError(f"{what}: no 3D filter is set; call compute_3D_filter(viewmatrices, intrinsics, sizes) first")
        if not torch.is_tensor(f) or f.numel() != P or f.shape[0] != P:
            raise RuntimeError(f"{what}: filter_3D has {f.shape[0] if torch.is_tensor(f) and f.dim() else '?'} rows for {P} Gaussians: it is stale "
                               "(densify_and_prune / add_new changed the set); recompute it with compute_3D_filter")
        if f.device != self._xyz.device:
            raise RuntimeError(f"{what}: filter_3D is on {f.device}, the Gaussians on {self._xyz.device}; recompute it with compute_3D_filter")
        return f

    def compute_3D_filter(self, viewmatrices, intrinsics, sizes, variance: float = 0.2):
        """Set ``filter_3D`` ``(P,1)`` from the training cameras and return it: ``viewmatrices`` / ``intrinsics (N,4,4)`` (``get_matrices``'
        ``viewmatrix`` and ``intrinsic`` of every camera, stacked) and ``sizes (N,2)`` integer ``(W, H)``.  Two HIP launches on a GPU
        (bags_raster.filter_3D), ``filter_3D_torch`` on the host.  From then on ``activated()`` -- and so ``render()`` /
        ``render_views()`` -- evaluates scale and opacity through the filter.  The filter belongs to the set as it is now: recompute
        it after ``densify_and_prune``, ``add_new`` and ``relocate``, and whenever the poses have moved far enough."""
        xyz = self._xyz.detach()
        fn = filter_3D if xyz.is_cuda else filter_3D_torch
        self.filter_3D = fn(xyz, viewmatrices, intrinsics, sizes, variance)
        return self.filter_3D

    @property
    def get_scaling_with_3D_filter(self):
        return filtered_activations_torch(self._opacity, self._scaling, self._checked_filter("GaussianBag.get_scaling_with_3D_filter"))[1]

    @property
    def get_opacity_with_3D_filter(self):
        return filtered_activations_torch(self._opacity, self._scaling, self._checked_filter("GaussianBag.get_opacity_with_3D_filter"))[0]

    @torch.no_grad()
    def fuse_3D_filter(self) -> "GaussianBag":
        """A new bag whose raw ``_opacity`` / ``_scaling`` are ``inverse_sigmoid(opacity')`` / ``log(scales')`` and whose ``filter_3D``
        is None: upstream's ``save_fused_ply`` step, for viewers that know nothing of the filter.  Every other leaf is a detached
        copy; the statistics are zeros."""
        f = self._checked_filter("GaussianBag.fuse_3D_filter")
        opacity, scales = filtered_activations_torch(self._opacity.detach(), self._scaling.detach(), f)
        pc = GaussianBag(self.max_sh_degree)
        pc.active_sh_degree = self.active_sh_degree
        grad = self._xyz.requires_grad
        for name in ("_xyz", "_features_dc", "_features_rest", "_rotation"):
            setattr(pc, name, getattr(self, name).detach().clone().requires_grad_(grad))
        pc._opacity = inverse_sigmoid(opacity).requires_grad_(grad)
        pc._scaling = torch.log(scales).requires_grad_(grad)
        P, dev = self._xyz.shape[0], self._xyz.device
        pc.max_radii2D = torch.zeros(P, device=dev)
        pc.xyz_gradient_accum = torch.zeros(P, 1, device=dev)
        pc.denom = torch.zeros(P, 1, device=dev)
        return pc

    def activated(self, features: bool = True):
        """(get_xyz, get_features, get_opacity, get_scaling, get_rotation) in one HIP launch each way on a GPU
        (bags_activations_forward / _backward, csrc/activations.hip); the same properties evaluated one by one on the host.
        ``features=False``: no concatenation (second entry None) -- for the rasterizer's ``shs`` / ``shs_rest`` pair, which
        takes ``_features_dc`` and ``_features_rest`` as they are (bags_raster.render).

        With ``filter_3D`` set, opacity and scaling are the filtered ones (``get_opacity_with_3D_filter`` /
        ``get_scaling_with_3D_filter``): still one launch each way on a GPU (bags_activations_filtered_forward / _backward).  A filter
        whose row count is not P is a RuntimeError."""
        f = None if self.filter_3D is None else self._checked_filter("GaussianBag.activated")
        if self._xyz.is_cuda:
            if not features:
                _, op, sc, rot = _FusedActivations.apply(None, None, self._opacity, self._scaling, self._rotation, f)
                return self._xyz, None, op, sc, rot
            shs, op, sc, rot = fused_activations(self._features_dc, self._features_rest, self._opacity, self._scaling, self._rotation, f)
            return self._xyz, shs, op, sc, rot
        if f is not None:
            op, sc = filtered_activations_torch(self._opacity, self._scaling, f)
            return self.get_xyz, (self.get_features if features else None), op, sc, self.get_rotation
        return self.get_xyz, (self.get_features if features else None), self.get_opacity, self.get_scaling, self.get_rotation

    def regularizers(self, select=None, terms=REG_TERMS, max_ratio: float = 10.0, max_scale: float = 0.05):
        """``(terms (6,), count ())``: the regularisers on the Gaussians themselves (bags_raster.gaussian_reg_loss: opacity, scale,
        flat, aniso, big, entropy) of ``_opacity`` and ``_scaling``, over the rows ``select (P,)`` bool keeps (None: all).  With
        ``filter_3D`` set they are taken on the filtered opacity and scales, exactly where ``activated()`` uses the filter.  Two HIP
        launches forward and one backward on a GPU, ``gaussian_reg_loss_torch`` on the host."""
        f = None if self.filter_3D is None else self._checked_filter("GaussianBag.regularizers")
        fn = gaussian_reg_loss if self._xyz.is_cuda else gaussian_reg_loss_torch
        return fn(self._opacity, self._scaling, f, select, terms, max_ratio, max_scale)

    def oneupSHdegree(self):
        if self.active_sh_degree < self.max_sh_degree:
            self.active_sh_degree += 1

    # ---- densification (scene/gaussian_model.py:393-447) and opacity reset: csrc/densify.hip
    _GROUPS = {"xyz": ("_xyz", 1), "f_dc": ("_features_dc", 0), "f_rest": ("_features_rest", 0), "opacity": ("_opacity", 4),
               "scaling": ("_scaling", 2), "rotation": ("_rotation", 3)}          # group name -> (leaf, BAGS_ROLE_*)

    def _named_groups(self, optimizer, what: str):
        """{name: (group, parameter, state or None)} of the six groups, each checked to hold this bag's leaf."""
        found = {}
        for group in optimizer.param_groups:
            name = group.get("name")
            if name in self._GROUPS:
                if name in found or len(group["params"]) != 1:
                    raise RuntimeError(f"{what}: the optimizer must hold exactly one group named {name!r} with one parameter")
                p = group["params"][0]
                if p is not getattr(self, self._GROUPS[name][0]):
                    raise RuntimeError(f"{what}: the parameter of group {name!r} is not this bag's {self._GROUPS[name][0]}")
                st = optimizer.state.get(p, None)
                found[name] = (group, p, st if st is not None and "exp_avg" in st else None)
        missing = [n for n in self._GROUPS if n not in found]
        if missing:
            raise RuntimeError(f"{what}: the optimizer has no parameter group named {missing[0]!r} (groups are found by their 'name' key: "
                               f"{', '.join(self._GROUPS)})")
        return found

    _ARG = dict(gpu=True, f32=True, contiguous=True, layout_error=TypeError)         # what the densify kernels take (_lib.require)

    # ---- what densify_and_prune and add_new share: a set of another size is written in one launch (csrc/row_rebuild.h) and installed
    def _resized_outputs(self, found, P_new: int):
        """``({name: [param, exp_avg, exp_avg_sq]}, (accum, denom, radii))`` of ``P_new`` rows, uninitialised; no state: None moments."""
        dev = self._xyz.device
        new = {n: [torch.empty((P_new,) + tuple(p.shape[1:]), dtype=torch.float32, device=dev) for _ in range(3 if st is not None else 1)] + [None, None]
               for n, (_, p, st) in found.items()}
        return new, (torch.empty(P_new, 1, dtype=torch.float32, device=dev), torch.empty(P_new, 1, dtype=torch.float32, device=dev),
                     torch.empty(P_new, dtype=torch.float32, device=dev))

    def _group_structs(self, struct, found, outs=None):
        """``(array, length)`` of ``L.BagsDensifyGroup`` or ``L.BagsMcmcGroup`` (one layout); ``outs``: of ``_resized_outputs``, or None."""
        gs = []
        for n, (_, p, st) in found.items():
            m, v = (st["exp_avg"], st["exp_avg_sq"]) if st is not None else (None, None)
            o = outs[n] if outs is not None else (None, None, None)
            width = int(math.prod(p.shape[1:]))
            if width:                                                             # (SH degree 0: _features_rest is (P,0,3), nothing to move)
                gs.append(struct(p.data_ptr(), L.ptr(m), L.ptr(v), L.ptr(o[0]), L.ptr(o[1]), L.ptr(o[2]), width, self._GROUPS[n][1]))
        return (struct * len(gs))(*gs), len(gs)

    def _install_resized(self, optimizer, found, new, stats) -> None:
        """New ``nn.Parameter`` s in the bag and in ``group["params"][0]``, the state re-keyed with the new moments, the statistics."""
        for n, (group, p, st) in found.items():
            param = torch.nn.Parameter(new[n][0].requires_grad_(True))
            if p in optimizer.state:
                stored = optimizer.state.pop(p)
                if st is not None:
                    stored["exp_avg"], stored["exp_avg_sq"] = new[n][1], new[n][2]
                optimizer.state[param] = stored
            group["params"][0] = param
            setattr(self, self._GROUPS[n][0], param)
        self.xyz_gradient_accum, self.denom, self.max_radii2D = stats

    @torch.no_grad()
    def densify_and_prune(self, optimizer, max_grad: float, min_opacity: float, extent: float, max_screen_size, percent_dense: float = 0.01,
                          N: int = 2, noise: Optional[torch.Tensor] = None, seed: Optional[int] = None, screen_size: str = "published"):
        """``GaussianModel.densify_and_prune`` with its optimizer surgery, in four HIP launches and one host synchronisation.

        Rows whose mean screen-space gradient reaches ``max_grad`` are cloned (largest scale <= ``percent_dense * extent``) or
        split into ``N`` children (larger); then rows with opacity below ``min_opacity`` and, when ``max_screen_size`` is given,
        rows larger than ``0.1 * extent`` are pruned.  New ``nn.Parameter`` s are installed in the bag and in
        ``group["params"][0]``; ``exp_avg`` / ``exp_avg_sq`` follow (kept rows bit for bit, new rows zero), ``step`` stays; the
        three statistics are zeros of the new size.  Result rows: kept originals, clones, children (child k of the j-th split
        row at ``k * S + j``), each in source order.

        ``screen_size="published"`` (default) repeats the published order, which zeroes ``max_radii2D`` before the prune step
        reads it, so that no row is ever pruned for its screen size; ``"pre_densify"`` tests a kept original against the radius
        it had before the call.  ``noise`` ``(P, N, 3)``: the standard normals of the children, by source row and child;
        without it they come from a counter-based generator in the kernel keyed by ``(seed, source row, child)``, ``seed`` drawn
        from torch's CPU generator when None (so ``torch.manual_seed`` governs it).

        Returns a dict: ``kept``, ``clones``, ``split``, ``pruned`` (rows the prune step removed), ``P_new`` and ``provenance``,
        int32 ``(P_new, 2)`` = (source row, kind: 0 kept, 1 clone, 2 + k child k)."""
        what = "GaussianBag.densify_and_prune"
        if screen_size not in ("published", "pre_densify"):
            raise ValueError(f"{what}: screen_size must be 'published' or 'pre_densify', got {screen_size!r}")
        if not 1 <= int(N) <= L.DENSIFY_MAX_CHILDREN:
            raise ValueError(f"{what}: N must be in 1..{L.DENSIFY_MAX_CHILDREN}, got {N}")
        N = int(N)
        found = self._named_groups(optimizer, what)
        P = self._xyz.shape[0]
        dev = self._xyz.device
        stats = (("xyz_gradient_accum", self.xyz_gradient_accum), ("denom", self.denom), ("max_radii2D", self.max_radii2D))
        for name, t in [(self._GROUPS[n][0], found[n][1]) for n in found] + list(stats):
            L.require(what, name, t, **self._ARG)
            if t.shape[0] != P or t.device != dev:
                raise RuntimeError(f"{what}: {name} has {t.shape[0]} rows on {t.device}, _xyz {P} on {dev}")
        for name, t in stats:
            if t.numel() != P:
                raise RuntimeError(f"{what}: {name} has {t.numel()} elements for {P} Gaussians")
        if noise is not None:
            L.require(what, "noise", noise, **self._ARG)
            if tuple(noise.shape) != (P, N, 3) or noise.device != dev:
                raise RuntimeError(f"{what}: noise must be ({P}, {N}, 3) on {dev}, got {tuple(noise.shape)} on {noise.device}")
        elif seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
        for n, (_, p, st) in found.items():
            if st is not None:
                for key in ("exp_avg", "exp_avg_sq"):
                    L.require(what, f"{key} of group {n!r}", st[key], **self._ARG)
                    if st[key].shape != p.shape or st[key].device != dev:
                        raise RuntimeError(f"{what}: {key} of group {n!r} has shape {tuple(st[key].shape)}, its parameter {tuple(p.shape)}")
        rule = L.BagsDensifyRule(P, N, max_grad, min_opacity, percent_dense * extent, 0.1 * extent,
                                 0.0 if max_screen_size is None else max_screen_size, 0 if max_screen_size is None else 1,
                                 L.SCREEN_PRE_DENSIFY if screen_size == "pre_densify" else L.SCREEN_PUBLISHED, 0,
                                 (0 if seed is None else int(seed)) & (2 ** 64 - 1), L.ptr(noise),
                                 self.xyz_gradient_accum.data_ptr(), self.denom.data_ptr(), self.max_radii2D.data_ptr(),
                                 self._scaling.data_ptr(), self._opacity.data_ptr())
        counts = (L.C.c_int64 * L.DENSIFY_COUNTS)()
        ws = L.workspace(L.load().bags_densify_workspace_size(P), dev)
        L.call("bags_densify_plan", dev, rule, ws.data_ptr(), ws.numel(), counts)
        P_new = int(counts[L.COUNT_P_NEW])
        new, stats = self._resized_outputs(found, P_new)
        groups, n_groups = self._group_structs(L.BagsDensifyGroup, found, new)
        prov = torch.empty(P_new, 2, dtype=torch.int32, device=dev)
        if P > 0:
            L.call("bags_densify_apply", dev, rule, groups, n_groups, ws.data_ptr(), ws.numel(), P_new,
                   stats[0].data_ptr(), stats[1].data_ptr(), stats[2].data_ptr(), prov.data_ptr())
        self._install_resized(optimizer, found, new, stats)
        return {"kept": int(counts[L.COUNT_KEPT]), "clones": int(counts[L.COUNT_CLONES]), "split": int(counts[L.COUNT_SPLIT]),
                "pruned": int(counts[L.COUNT_PRUNED]), "P_new": P_new, "provenance": prov}

    @torch.no_grad()
    def reset_opacity(self, optimizer) -> None:
        """``GaussianModel.reset_opacity``: ``_opacity = inverse_sigmoid(min(sigmoid(_opacity), 0.01))`` and zero moments, in one
        HIP launch and in place (the reference replaces the parameter; the values and the optimizer state are the same)."""
        what = "GaussianBag.reset_opacity"
        group = [g for g in optimizer.param_groups if g.get("name") == "opacity"]
        if len(group) != 1 or len(group[0]["params"]) != 1 or group[0]["params"][0] is not self._opacity:
            raise RuntimeError(f"{what}: the optimizer must hold exactly one group named 'opacity' whose parameter is this bag's _opacity")
        p = self._opacity
        L.require(what, "_opacity", p, **self._ARG)
        st = optimizer.state.get(p, None)
        m = v = None
        if st is not None and "exp_avg" in st:
            m, v = st["exp_avg"], st["exp_avg_sq"]
            for key, t in (("exp_avg", m), ("exp_avg_sq", v)):
                L.require(what, key, t, **self._ARG)
                if t.shape != p.shape or t.device != p.device:
                    raise RuntimeError(f"{what}: {key} has shape {tuple(t.shape)} on {t.device}, _opacity {tuple(p.shape)} on {p.device}")
        L.call("bags_reset_opacity", p.device, p.data_ptr(), L.ptr(m), L.ptr(v), p.numel())
        p.grad = None

    # ---- the 3DGS-MCMC strategy (train.py:366-367 under --mcmc, and its noise block): csrc/mcmc.hip
    def _mcmc_groups(self, what: str, found):
        """The six groups' parameters and moments as the MCMC kernels take them: ``_ARG``, on one device, the set's row count."""
        P, dev = self._xyz.shape[0], self._xyz.device
        for n, (_, p, st) in found.items():
            for key, t in (("parameter", p),) + ((("exp_avg", st["exp_avg"]), ("exp_avg_sq", st["exp_avg_sq"])) if st is not None else ()):
                L.require(what, f"{key} of group {n!r}", t, **self._ARG)
                if t.shape != p.shape or t.shape[0] != P or t.device != dev:
                    raise RuntimeError(f"{what}: {key} of group {n!r} has shape {tuple(t.shape)} on {t.device}, expected {(P,) + tuple(p.shape[1:])} on {dev}")

    @staticmethod
    def _mcmc_rows(what: str, name: str, rows, P: int, like, count=None):
        """``rows``: an int32 / int64 vector of row numbers in 0..P-1 on the device of ``like``; checked where it lives."""
        L.require(what, name, rows, on=like)
        if rows.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"{what}: {name} must be int32 or int64, got {rows.dtype}")
        if rows.dim() != 1 or (count is not None and rows.numel() != count):
            raise RuntimeError(f"{what}: {name} must be a vector" + (f" of {count} rows" if count is not None else "") + f", got shape {tuple(rows.shape)}")
        if rows.numel() and (int(rows.min()) < 0 or int(rows.max()) >= P):
            raise IndexError(f"{what}: {name} holds rows outside 0..{P - 1}")

    @staticmethod
    def _mcmc_sample(p, n: int, generator):
        """``n`` draws from the rows of ``p`` (opacities, any positive weights) in proportion to them, with replacement: the
        published ``_sample_alives``."""
        return torch.multinomial(p / p.sum(), n, replacement=True, generator=generator)

    @torch.no_grad()
    def relocate(self, optimizer, dead_mask, sampled=None, generator=None, min_opacity: float = 0.005):
        """The published ``relocate_gs``, in place, in three HIP launches: every dead row (``dead_mask (P,)`` bool) is moved onto an
        alive row drawn in proportion to its opacity, and the opacity and scale of the rows drawn are corrected so that the
        rendering is kept (``compute_relocation`` with the count of draws + 1; the opacity clamped to
        ``[min_opacity, 1 - eps]``).  Dead row j takes every parameter of ``sampled[j]``; the sources get the same new ``_opacity`` and
        ``_scaling``, and their ``exp_avg`` / ``exp_avg_sq`` are zeroed in all six groups; dead rows keep their moments and ``step``
        stays, as published.  No other row is touched.

        ``sampled`` ``(D,)``, D the number of dead rows: the source of each dead row, in the order of the dead rows; it must list
        alive rows.  None: drawn here with ``torch.multinomial`` under ``generator``; on a GPU that draw does not repeat bit for bit at
        large P (its prefix sum does not), so view-sharded ranks draw once and pass one tensor.
        No dead rows, or no alive ones: nothing happens.  Returns ``{"dead": D, "sources": distinct rows drawn}``.

        P stays, so a ``filter_3D`` that is set still fits and is NOT touched: the moved rows keep the filter of the place they
        left until the caller recomputes it (``compute_3D_filter``)."""
        what = "GaussianBag.relocate"
        found = self._named_groups(optimizer, what)
        P = self._xyz.shape[0]
        L.require(what, "dead_mask", dead_mask, on=self._xyz)
        if dead_mask.dtype != torch.bool:
            raise TypeError(f"{what}: dead_mask must be bool, got {dead_mask.dtype}")
        if tuple(dead_mask.shape) != (P,):
            raise RuntimeError(f"{what}: dead_mask must be ({P},), got {tuple(dead_mask.shape)}")
        D = int(dead_mask.sum())
        if sampled is not None:
            self._mcmc_rows(what, "sampled", sampled, P, dead_mask, count=D)
            if D and bool(dead_mask[sampled.long()].any()):
                raise ValueError(f"{what}: sampled lists a dead row; the sources must be alive")
        self._mcmc_groups(what, found)
        if D == 0 or D == P:
            return {"dead": D, "sources": 0}
        dev = self._xyz.device
        dead = dead_mask.nonzero().reshape(-1)
        if sampled is None:
            alive = (~dead_mask).nonzero().reshape(-1)
            sampled = alive[self._mcmc_sample(torch.sigmoid(self._opacity.detach()[alive, 0]), D, generator)]
        groups, n = self._group_structs(L.BagsMcmcGroup, found)
        dead32, sampled32 = dead.to(torch.int32), sampled.to(torch.int32).contiguous()
        ws = L.workspace(L.load().bags_mcmc_workspace_size(P), dev)
        L.call("bags_mcmc_relocate", dev, groups, n, P, dead32.data_ptr(), sampled32.data_ptr(), D, relocation_binoms(N_MAX, dev).data_ptr(), N_MAX,
               float(min_opacity), ws.data_ptr(), ws.numel())
        return {"dead": D, "sources": int(torch.unique(sampled32).numel())}

    @torch.no_grad()
    def add_new(self, optimizer, cap_max: int, sampled=None, generator=None, min_opacity: float = 0.005):
        """The published ``add_new_gs`` with its optimizer surgery, in three HIP launches: the set grows by 5 % up to ``cap_max`` rows,
        ``A = max(0, min(cap_max, int(1.05 * P)) - P)`` new rows, each a copy of a row drawn in proportion to its opacity; the rows
        drawn and their copies get the corrected opacity and scale of ``relocate``.  New ``nn.Parameter`` s are installed in the bag
        and in ``group["params"][0]`` as ``densify_and_prune`` installs them: old rows bit for bit (but the sources' opacity, scaling
        and zeroed moments), new rows' moments zero, ``step`` unchanged, the three statistics zeros of the new size.

        ``sampled`` ``(A,)``: the source of each new row (any rows of the set); None: drawn here.  ``A == 0``: nothing happens.
        Returns ``{"added": A, "P_new": P + A}``."""
        what = "GaussianBag.add_new"
        found = self._named_groups(optimizer, what)
        P = self._xyz.shape[0]
        A = max(0, min(int(cap_max), int(1.05 * P)) - P)
        if sampled is not None:
            self._mcmc_rows(what, "sampled", sampled, P, self._xyz, count=A)
        self._mcmc_groups(what, found)
        if A == 0:
            return {"added": 0, "P_new": P}
        dev = self._xyz.device
        if sampled is None:
            sampled = self._mcmc_sample(torch.sigmoid(self._opacity.detach()[:, 0]), A, generator)
        P_new = P + A
        new, stats = self._resized_outputs(found, P_new)
        groups, n_groups = self._group_structs(L.BagsMcmcGroup, found, new)
        sampled32 = sampled.to(torch.int32).contiguous()
        ws = L.workspace(L.load().bags_mcmc_workspace_size(P), dev)
        L.call("bags_mcmc_add_new", dev, groups, n_groups, P, sampled32.data_ptr(), A, relocation_binoms(N_MAX, dev).data_ptr(), N_MAX, float(min_opacity),
               ws.data_ptr(), ws.numel(), stats[0].data_ptr(), stats[1].data_ptr(), stats[2].data_ptr())
        self._install_resized(optimizer, found, new, stats)
        return {"added": A, "P_new": P_new}

    @torch.no_grad()
    def mcmc_noise(self, scale: float, noise: Optional[torch.Tensor] = None, seed: Optional[int] = None, k: float = 100.0, x0: float = 0.995,
                   scaling_modifier: float = 1.0) -> None:
        """The per-iteration SGLD step of the MCMC strategy (train.py's ``noise_lr * xyz_lr`` block) in one HIP launch, in place on
        ``_xyz``: ``_xyz += Sigma (z * g * scale)`` with ``g = 1 / (1 + exp(-k ((1 - sigmoid(_opacity)) - x0)))`` and
        ``Sigma = R diag(s^2) R^T``, ``s = scaling_modifier * exp(_scaling)``.  Only the new ``_xyz`` is written; no covariance is
        built in memory.  ``z``: ``noise (P,3)``, or three standard normals per row from the generator of ``densify_and_prune`` keyed
        by ``(seed, row)`` -- the same bits from the same seed on every rank; ``seed`` None: drawn from torch's CPU generator."""
        what = "GaussianBag.mcmc_noise"
        P, dev = self._xyz.shape[0], self._xyz.device
        for name, t, w in (("_xyz", self._xyz, 3), ("_opacity", self._opacity, 1), ("_scaling", self._scaling, 3), ("_rotation", self._rotation, 4)):
            L.require(what, name, t, **self._ARG)
            if tuple(t.shape) != (P, w) or t.device != dev:
                raise RuntimeError(f"{what}: {name} must be ({P}, {w}) on {dev}, got {tuple(t.shape)} on {t.device}")
        if noise is not None:
            L.require(what, "noise", noise, **self._ARG)
            if tuple(noise.shape) != (P, 3) or noise.device != dev:
                raise RuntimeError(f"{what}: noise must be ({P}, 3) on {dev}, got {tuple(noise.shape)} on {noise.device}")
        elif seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
        L.call("bags_mcmc_noise", dev, self._xyz.data_ptr(), self._opacity.data_ptr(), self._scaling.data_ptr(), self._rotation.data_ptr(), P, L.ptr(noise),
               (0 if seed is None else int(seed)) & (2 ** 64 - 1), float(scale), float(k), float(x0), float(scaling_modifier))

    # ---- consumers of the op's screen-space gradients (scene/gaussian_model.py:449-455)
    def add_densification_stats(self, viewspace_point_tensor, viewspace_point_tensor_densify, update_filter, abs_grad: bool):
        if abs_grad:
            assert viewspace_point_tensor_densify is not None
            g = viewspace_point_tensor_densify.grad
        else:
            g = viewspace_point_tensor.grad
        self.xyz_gradient_accum[update_filter] += torch.norm(g[update_filter, :2], dim=-1, keepdim=True)
        self.denom[update_filter] += 1


class _FusedActivations(torch.autograd.Function):
    """``dc`` and ``rest`` may both be None (packed features): no SH concatenation, the first output is None.  ``filter_3D`` (P,1) or
    None: the 3D smoothing filter applied to opacity and scaling (a constant: it gets no gradient)."""

    @staticmethod
    def forward(ctx, dc, rest, opacity, scaling, rotation, filter_3D):
        feats = dc is not None
        if (dc is None) != (rest is None):
            raise RuntimeError("fused_activations: features_dc and features_rest are given together or not at all")
        ts = [L.as_f32c(t) for t in (dc, rest, opacity, scaling, rotation)]
        for name, t in zip(("features_dc", "features_rest", "opacity", "scaling", "rotation"), ts):
            if t is not None:
                L.require("fused_activations", name, t, gpu=True, host=" (use the GaussianBag properties on the host)")
        P = ts[3].shape[0]
        K = 1 + ts[1].shape[1] if feats else 1
        if (feats and (ts[0].shape != (P, 1, 3) or ts[1].shape != (P, K - 1, 3))) or ts[2].numel() != P or ts[3].shape != (P, 3) or ts[4].shape != (P, 4):
            raise RuntimeError("fused_activations: expected features_dc (P,1,3), features_rest (P,K-1,3), opacity (P,1), scaling (P,3), rotation (P,4)")
        dev = ts[3].device
        filt = L.as_f32c(filter_3D)
        if filt is not None:
            L.require("fused_activations", "filter_3D", filt, gpu=True, on=ts[3], host=" (use the GaussianBag properties on the host)")
            if filt.numel() != P or filt.shape[0] != P:
                raise RuntimeError(f"fused_activations: filter_3D must be (P,1) with P = {P}, got {tuple(filt.shape)}")
        shs = torch.empty(P, K, 3, dtype=torch.float32, device=dev) if feats else None
        op = torch.empty(P, 1, dtype=torch.float32, device=dev)
        sc = torch.empty(P, 3, dtype=torch.float32, device=dev)
        rot = torch.empty(P, 4, dtype=torch.float32, device=dev)
        raw = L.BagsRawGaussians(P, K, *[L.ptr(t) for t in ts])
        if filt is None:
            L.call("bags_activations_forward", dev, raw, L.ptr(shs), op.data_ptr(), sc.data_ptr(), rot.data_ptr())
        else:
            L.call("bags_activations_filtered_forward", dev, raw, filt.data_ptr(), L.ptr(shs), op.data_ptr(), sc.data_ptr(), rot.data_ptr())
        ctx.feats = feats
        ctx.filt = filt                           # (not a differentiable input: kept beside the saved ones)
        ctx.save_for_backward(*[t for t in ts if t is not None])
        ctx.set_materialize_grads(False)          # an unused output arrives as None, not as 96 MB of zeros
        return shs, op, sc, rot

    @staticmethod
    def backward(ctx, g_shs, g_op, g_sc, g_rot):
        ts = list(ctx.saved_tensors)
        if not ctx.feats:
            ts = [None, None] + ts
        P = ts[3].shape[0]
        K = 1 + ts[1].shape[1] if ctx.feats else 1
        need = ctx.needs_input_grad
        g_shs, g_op, g_sc, g_rot = L.as_f32c(g_shs), L.as_f32c(g_op), L.as_f32c(g_sc), L.as_f32c(g_rot)
        filt = ctx.filt
        # filtered: the opacity depends on the scaling too, so dL/d_scaling exists as soon as either cotangent does
        g_for_scaling = g_sc is not None or (filt is not None and g_op is not None)
        out = [torch.empty_like(ts[0]) if (ctx.feats and need[0] and g_shs is not None) else None,
               torch.empty_like(ts[1]) if (ctx.feats and need[1] and g_shs is not None) else None,
               torch.empty_like(ts[2]) if (need[2] and g_op is not None) else None,
               torch.empty_like(ts[3]) if (need[3] and g_for_scaling) else None,
               torch.empty_like(ts[4]) if (need[4] and g_rot is not None) else None]
        raw = L.BagsRawGaussians(P, K, *[L.ptr(t) for t in ts])
        cotangents = (L.ptr(g_shs), L.ptr(g_op), L.ptr(g_sc), L.ptr(g_rot))
        if filt is None:
            L.call("bags_activations_backward", ts[3].device, raw, *cotangents, *[L.ptr(o) for o in out])
        else:
            L.call("bags_activations_filtered_backward", ts[3].device, raw, filt.data_ptr(), *cotangents, *[L.ptr(o) for o in out])
        return tuple(out) + (None,)


def fused_activations(features_dc, features_rest, opacity, scaling, rotation, filter_3D=None):
    """(get_features, get_opacity, get_scaling, get_rotation) of scene/gaussian_model.py:118-141 in one HIP launch; with
    ``filter_3D (P,1)`` the opacity and the scaling are Mip-Splatting's filtered ones (``filtered_activations_torch``), still one
    launch each way."""
    return _FusedActivations.apply(features_dc, features_rest, opacity, scaling, rotation, filter_3D)


def _sh_saved(ctx):
    """The backward half both SH colour operators share: ``ctx``'s saved inputs as ``(shs, rest, xyz, camposes)``, ``K``, and the
    gradients of the first three, allocated where autograd needs them (None elsewhere)."""
    ts = list(ctx.saved_tensors)
    if not ctx.split:
        ts.insert(1, None)
    shs, rest, xyz, camposes = ts[0], ts[1], ts[2], ts[3:]
    K = shs.shape[1] + (0 if rest is None else rest.shape[1])
    need = ctx.needs_input_grad
    out = [torch.empty_like(t) if (t is not None and need[k]) else None for k, t in ((1, shs), (2, rest), (3, xyz))]
    return shs, rest, xyz, camposes, K, out


class _ShColors(torch.autograd.Function):
    """``shs_rest`` None: ``shs`` is the packed (P,K,3) tensor; otherwise ``shs`` (P,1,3) and ``shs_rest`` (P,K-1,3)."""

    @staticmethod
    def forward(ctx, deg, shs, shs_rest, xyz, campos):
        ts = [L.as_f32c(t) for t in (shs, shs_rest, xyz, campos)]                # (float32 already: sh_colors checks)
        P = ts[2].shape[0]
        K = ts[0].shape[1] + (0 if ts[1] is None else ts[1].shape[1])
        rgb = torch.empty(P, 3, dtype=torch.float32, device=ts[2].device)
        L.call("bags_sh_colors_forward", rgb.device, L.BagsShColors(P, K, deg, 0, *[L.ptr(t) for t in ts]), rgb.data_ptr())
        ctx.deg, ctx.split = deg, ts[1] is not None
        ctx.save_for_backward(*[t for t in ts if t is not None])       # the inputs and nothing else: the clamp mask is recomputed
        ctx.set_materialize_grads(False)
        return rgb

    @staticmethod
    def backward(ctx, g_rgb):
        if g_rgb is None:
            return None, None, None, None, None
        shs, rest, xyz, (campos,), K, out = _sh_saved(ctx)
        P = xyz.shape[0]
        g_rgb = L.as_f32c(g_rgb)
        out.append(torch.empty_like(campos) if ctx.needs_input_grad[4] else None)
        args = L.BagsShColors(P, K, ctx.deg, 0, L.ptr(shs), L.ptr(rest), L.ptr(xyz), L.ptr(campos))
        ws = L.workspace(L.load().bags_sh_colors_workspace_size(P) if out[3] is not None else 0, xyz.device)      # (only dL/dcampos needs one)
        L.call("bags_sh_colors_backward", xyz.device, args, g_rgb.data_ptr(), ws.data_ptr(), ws.numel(), *[L.ptr(o) for o in out])
        return (None,) + tuple(out)


def _sh_degree(what: str, deg) -> int:
    deg = int(deg)
    if not 0 <= deg <= 3:
        raise ValueError(f"{what}: SH degree must be in 0..3, got {deg}")
    return deg


def _sh_operands(what: str, deg: int, shs, xyz, shs_rest, cams) -> int:
    """What ``sh_colors`` and ``sh_colors_views`` ask of their operands, in the order the errors are raised; ``cams``: the camera
    centres as ``(name, tensor)`` pairs.  Returns K, the number of stored coefficients."""
    named = [("shs", shs), ("xyz", xyz)] + cams + ([("shs_rest", shs_rest)] if shs_rest is not None else [])
    for name, t in named:
        L.require(what, name, t, f32=True)
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise RuntimeError(f"{what}: xyz must be (P,3), got {tuple(xyz.shape)}")
    P = xyz.shape[0]
    for name, c in cams:
        if tuple(c.shape) != (3,):
            raise RuntimeError(f"{what}: {name} must be (3,), got {tuple(c.shape)}")
    if shs_rest is None:
        if shs.dim() != 3 or shs.shape[0] != P or shs.shape[2] != 3:
            raise RuntimeError(f"{what}: shs must be ({P},K,3) for xyz {tuple(xyz.shape)}, got {tuple(shs.shape)}")
        K = shs.shape[1]
    else:
        if tuple(shs.shape) != (P, 1, 3):
            raise RuntimeError(f"{what}: with shs_rest, shs must be the ({P},1,3) DC part for xyz {tuple(xyz.shape)}, got {tuple(shs.shape)}")
        if shs_rest.dim() != 3 or shs_rest.shape[0] != P or shs_rest.shape[2] != 3 or shs_rest.shape[1] < 1:
            raise RuntimeError(f"{what}: shs_rest must be ({P},K-1,3) with K >= 2 for shs {tuple(shs.shape)}, got {tuple(shs_rest.shape)}")
        K = 1 + shs_rest.shape[1]
    if K not in (1, 4, 9, 16):
        raise RuntimeError(f"{what}: K = {K} stored coefficients (shs {tuple(shs.shape)}"
                           + (f", shs_rest {tuple(shs_rest.shape)}" if shs_rest is not None else "") + "): K must be 1, 4, 9 or 16")
    if K < (deg + 1) ** 2:
        raise RuntimeError(f"{what}: degree {deg} needs {(deg + 1) ** 2} coefficients, shs"
                           + (" + shs_rest hold " if shs_rest is not None else " holds ") + f"{K} (shs {tuple(shs.shape)})")
    for name, t in named:
        L.require(what, name, t, gpu=True, on=xyz, host=" (bags_raster.eval_sh is the host-side evaluation)")
    return K


def sh_colors(deg: int, shs: torch.Tensor, xyz: torch.Tensor, campos: torch.Tensor, shs_rest: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``clamp_min(eval_sh(deg, shs, normalize(xyz - campos)) + 0.5, 0)`` -> ``(P,3)``: the Python colour path of ``render()``
    (gaussian_renderer/__init__.py:90-95) in one HIP launch each way, gradients to the coefficients, ``xyz`` and ``campos``.

    ``shs`` is the ``(P,K,3)`` feature tensor, or, with ``shs_rest (P,K-1,3)``, the ``(P,1,3)`` DC part: the two stored parameters
    go in as they are, without ``get_features``' concatenation.  K is 1, 4, 9 or 16 and at least ``(deg+1)^2``; the gradient of the
    stored rows beyond the active degree is exactly zero.  float32 tensors on a GPU; there is no CPU fallback (use ``eval_sh``)."""
    what = "sh_colors"
    deg = _sh_degree(what, deg)
    _sh_operands(what, deg, shs, xyz, shs_rest, [("campos", campos)])
    return _ShColors.apply(deg, shs, shs_rest, xyz, campos)


class _ShColorsViews(torch.autograd.Function):
    """``sh_colors`` for the V views of one step: V separate ``(P,3)`` outputs, one launch each way.  A view no loss depends on
    arrives in ``backward`` as None (``set_materialize_grads(False)``) and goes down as a NULL pointer."""

    @staticmethod
    def forward(ctx, deg, shs, shs_rest, xyz, *camposes):
        ts = [L.as_f32c(t) for t in (shs, shs_rest, xyz) + camposes]
        V, P = len(camposes), ts[2].shape[0]
        K = ts[0].shape[1] + (0 if ts[1] is None else ts[1].shape[1])
        rgb = tuple(torch.empty(P, 3, dtype=torch.float32, device=ts[2].device) for _ in range(V))
        args = L.BagsShColorsViews(P, K, deg, V, L.ptr(ts[0]), L.ptr(ts[1]), L.ptr(ts[2]), L.ptr_table(ts[3:] + [None] * (L.MAX_SH_VIEWS - V)))
        L.call("bags_sh_colors_views_forward", ts[2].device, args, L.ptr_table(rgb))
        ctx.deg, ctx.split = deg, ts[1] is not None
        ctx.save_for_backward(*[t for t in ts if t is not None])       # the inputs and nothing else, as _ShColors
        ctx.set_materialize_grads(False)
        return rgb

    @staticmethod
    def backward(ctx, *g_rgb):
        V = len(g_rgb)
        if all(g is None for g in g_rgb):
            return (None,) * (4 + V)
        shs, rest, xyz, camposes, K, out = _sh_saved(ctx)
        P = xyz.shape[0]
        need = ctx.needs_input_grad
        g_rgb = [L.as_f32c(g) for g in g_rgb]
        g_campos = [torch.empty_like(c) if need[4 + v] else None for v, c in enumerate(camposes)]
        args = L.BagsShColorsViews(P, K, ctx.deg, V, L.ptr(shs), L.ptr(rest), L.ptr(xyz), L.ptr_table(camposes + [None] * (L.MAX_SH_VIEWS - V)))
        wanted = any(g is not None for g in g_campos)                  # (only dL/dcampos needs a workspace)
        ws = L.workspace(L.load().bags_sh_colors_views_workspace_size(P, V) if wanted else 0, xyz.device)
        L.call("bags_sh_colors_views_backward", xyz.device, args, L.ptr_table(g_rgb), ws.data_ptr(), ws.numel(), *[L.ptr(o) for o in out],
               L.ptr_table(g_campos))
        return (None,) + tuple(out) + tuple(g_campos)


def sh_colors_views(deg: int, shs: torch.Tensor, xyz: torch.Tensor, camposes, shs_rest: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, ...]:
    """``sh_colors`` for the V views of one step over the same Gaussians: ``camposes`` is a sequence of V ``(3,)`` camera centres
    (1 <= V <= 16), the result a tuple of V ``(P,3)`` tensors, view v's the bits ``sh_colors(deg, shs, xyz, camposes[v])`` gives.

    One HIP launch each way for all the views: the coefficient rows are read once in the forward and once in the backward, and the
    gradients of ``shs`` / ``shs_rest`` / ``xyz`` are summed over the views on the chip, in view order, and written once -- the bits
    of the fp32 fold of the per-view gradients, without autograd's ``grad += g`` per view.  Each camera centre gets its own
    gradient.  A view whose colours no loss uses costs nothing in the backward.  Layouts and limits as ``sh_colors``."""
    what = "sh_colors_views"
    deg = _sh_degree(what, deg)
    if isinstance(camposes, torch.Tensor) or not isinstance(camposes, (list, tuple)):
        raise TypeError(f"{what}: camposes must be a list or tuple of (3,) tensors, got {type(camposes).__name__}")
    V = len(camposes)
    if not 1 <= V <= L.MAX_SH_VIEWS:
        raise ValueError(f"{what}: the number of views must be in 1..{L.MAX_SH_VIEWS}, got {V} (more views: one call per chunk)")
    _sh_operands(what, deg, shs, xyz, shs_rest, [(f"camposes[{v}]", c) for v, c in enumerate(camposes)])
    return _ShColorsViews.apply(deg, shs, shs_rest, xyz, *camposes)
