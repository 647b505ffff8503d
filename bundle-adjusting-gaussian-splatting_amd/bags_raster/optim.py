"""GaussianAdam -- ``torch.optim.Adam`` over the Gaussian parameter groups as one HIP launch per step (csrc/adam.hip).

The reference builds ``torch.optim.Adam(l, lr=0.0, eps=1e-15)`` over six groups named xyz, f_dc, f_rest, opacity, scaling,
rotation (scene/gaussian_model.py:192-210) and steps it once per iteration (train.py:420-421).  ``GaussianAdam`` takes the
same list of group dicts, keeps PyTorch's state layout (``step`` as a CPU tensor, ``exp_avg``, ``exp_avg_sq``), so
``state_dict()`` / ``load_state_dict()`` and the reference's densification surgery on ``optimizer.state`` and
``group["params"][0]`` work unchanged: ``step()`` reads pointers, sizes and ``lr`` from the groups at every call.

Beyond the reference: ``step(visibility=radii)`` leaves the Gaussians a view did not touch alone (parameters and both
moments), and ``step(stats=(bag, viewspace_points, radii))`` folds ``add_densification_stats`` and the ``max_radii2D``
update into the same launch.  There is no CPU or eager fallback.
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from . import _lib as L

_UNSUPPORTED = (("amsgrad", False), ("maximize", False), ("capturable", False), ("differentiable", False))
_ARG = dict(gpu=True, f32=True, contiguous=True, host=" (use torch.optim.Adam on the host)")      # what the kernel takes (_lib.require)


class GaussianAdam(torch.optim.Optimizer):
    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0, amsgrad: bool = False,
                 maximize: bool = False, capturable: bool = False, differentiable: bool = False):
        if isinstance(lr, torch.Tensor):
            raise TypeError("GaussianAdam: lr must be a Python number (a tensor lr belongs to capturable Adam, which is not supported)")
        if lr < 0.0 or eps < 0.0 or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"GaussianAdam: invalid hyper-parameters lr={lr}, betas={betas}, eps={eps}")
        # the keys of torch.optim.Adam's param_groups, so that state dicts move between the two in both directions
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=None,
                        capturable=capturable, differentiable=differentiable, fused=None, decoupled_weight_decay=False)
        super().__init__(params, defaults)
        for g in self.param_groups:
            self._check_group(g)
        self._mask = None                  # int32 copy of a visibility tensor of another dtype, reused while P stays

    @staticmethod
    def _check_group(g) -> None:
        if g.get("weight_decay", 0) != 0:
            raise RuntimeError("GaussianAdam: weight_decay is not supported (the fused kernel implements weight_decay=0 only)")
        for key, default in _UNSUPPORTED:
            if g.get(key, default) != default:
                raise RuntimeError(f"GaussianAdam: {key}={g[key]!r} is not supported (the fused kernel implements "
                                   f"torch.optim.Adam with amsgrad=False, maximize=False, capturable=False, differentiable=False)")

    def _stats_block(self, stats):
        bag, viewspace, radii = stats
        grad = viewspace.grad
        if grad is None:
            raise RuntimeError("GaussianAdam: stats: viewspace_points has no .grad (call backward() first)")
        P = radii.numel()
        if radii.dtype != torch.int32 or not radii.is_cuda or not radii.is_contiguous():
            raise TypeError("GaussianAdam: stats: radii must be the rasterizer's contiguous int32 GPU tensor")
        if grad.dim() != 2 or grad.shape[0] != P or grad.shape[1] < 2:
            raise RuntimeError(f"GaussianAdam: stats: the screen-space gradient must be (P, >= 2) with P = {P}, got {tuple(grad.shape)}")
        L.require("GaussianAdam", "stats: the screen-space gradient", grad, **_ARG)
        for name in ("xyz_gradient_accum", "denom", "max_radii2D"):
            t = getattr(bag, name)
            L.require("GaussianAdam", f"stats: {name}", t, **_ARG)
            if t.numel() != P:
                raise RuntimeError(f"GaussianAdam: stats: {name} has {t.numel()} elements, radii {P}")
            if t.device != radii.device:
                raise RuntimeError(f"GaussianAdam: stats: {name} is on {t.device}, radii on {radii.device}")
        return P, L.BagsDensifyStats(radii.data_ptr(), grad.data_ptr(), grad.shape[1], 0, bag.xyz_gradient_accum.data_ptr(),
                                     bag.denom.data_ptr(), bag.max_radii2D.data_ptr())

    def _visible(self, visibility: torch.Tensor) -> torch.Tensor:
        if visibility.dim() != 1:
            raise RuntimeError(f"GaussianAdam: visibility must be a (P,) tensor, got shape {tuple(visibility.shape)}")
        L.require("GaussianAdam", "visibility", visibility, gpu=True)
        if visibility.dtype == torch.int32 and visibility.is_contiguous():
            return visibility                                   # the op's radii: used as it is
        if visibility.dtype not in (torch.bool, torch.int32):
            raise TypeError(f"GaussianAdam: visibility must be int32 (the rasterizer's radii) or bool, got {visibility.dtype}")
        if self._mask is None or self._mask.shape != visibility.shape or self._mask.device != visibility.device:
            self._mask = torch.empty(visibility.shape, dtype=torch.int32, device=visibility.device)
        self._mask.copy_(visibility)
        return self._mask

    @torch.no_grad()
    def step(self, visibility: Optional[torch.Tensor] = None, stats=None, closure=None):
        """One Adam step.  ``visibility``: int32 (the rasterizer's ``radii``) or bool ``(P,)``; only rows with a positive / True
        entry are updated, the others keep parameters and moments bit for bit (bias corrections still follow the group's step
        count).  ``stats = (bag, viewspace_points, radii)``: also ``bag.add_densification_stats`` of this iteration
        (``viewspace_points.grad``; pass ``viewspace_points_densify`` for ``abs_grad``) and
        ``bag.max_radii2D[radii > 0] = max(bag.max_radii2D[radii > 0], radii[radii > 0])``.  Plain ``step()`` is the
        reference's dense step."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        vis = None if visibility is None else self._visible(visibility)
        stats_P = stats_block = stats_dev = None
        if stats is not None:
            stats_P, stats_block = self._stats_block(stats)
            stats_dev = stats[2].device
        # launches: one per (Gaussian count, betas, eps, device), split after ADAM_MAX_GROUPS parameters
        batches = {}
        for group in self.param_groups:
            self._check_group(group)
            beta1, beta2 = group["betas"]
            lr = group["lr"]
            if isinstance(lr, torch.Tensor):
                raise TypeError("GaussianAdam: lr must be a Python number")
            for p in group["params"]:
                if p.grad is None:
                    continue
                g = p.grad
                L.require("GaussianAdam", "a parameter", p, **_ARG)
                L.require("GaussianAdam", "a gradient", g, **_ARG)
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0, dtype=torch.float64 if torch.get_default_dtype() == torch.float64 else torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                m, v = state["exp_avg"], state["exp_avg_sq"]
                for name, t in (("exp_avg", m), ("exp_avg_sq", v)):
                    L.require("GaussianAdam", name, t, **_ARG)
                    if t.shape != p.shape:
                        raise RuntimeError(f"GaussianAdam: {name} has shape {tuple(t.shape)}, its parameter {tuple(p.shape)}")
                if g.shape != p.shape or g.device != p.device or m.device != p.device or v.device != p.device:
                    raise RuntimeError("GaussianAdam: parameter, gradient and moments must share one shape and device")
                P = p.shape[0] if p.dim() > 0 else 1
                if vis is not None and (vis.numel() != P or vis.device != p.device):
                    raise RuntimeError(f"GaussianAdam: visibility has {vis.numel()} entries on {vis.device}, but a parameter with a "
                                       f"gradient has {P} rows on {p.device}")
                if state["step"].is_cuda:                       # a checkpoint of fused / capturable torch Adam: back to the host once
                    state["step"] = state["step"].cpu()
                state["step"] += 1
                if p.numel() == 0:
                    continue
                step = state["step"].item()
                step_size = lr / (1.0 - beta1 ** step)
                bc2_sqrt = math.sqrt(1.0 - beta2 ** step)
                key = (P, float(beta1), float(beta2), float(group["eps"]), p.device)
                batches.setdefault(key, []).append(L.BagsAdamGroup(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(),
                                                                   p.numel() // P, 0, step_size, bc2_sqrt))
        if stats is not None:
            if not any(key[0] == stats_P and key[4] == stats_dev for key in batches):
                raise RuntimeError(f"GaussianAdam: stats were given, but no parameter with a gradient has as many rows as radii "
                                   f"({stats_P}) on {stats_dev}")
        for (P, beta1, beta2, eps, dev), groups in batches.items():
            for i in range(0, len(groups), L.ADAM_MAX_GROUPS):
                part = groups[i:i + L.ADAM_MAX_GROUPS]
                args = L.BagsAdamArgs(P, len(part), beta1, beta2, eps, L.ptr(vis), (L.BagsAdamGroup * L.ADAM_MAX_GROUPS)(*part))
                fold = stats_block is not None and P == stats_P and dev == stats_dev      # into exactly one launch
                L.call("bags_adam_step", dev, args, stats_block if fold else None)
                if fold:
                    stats_block = None
        return loss
