"""normal_map_loss -- a rendered normal map held to a target normal map (csrc/normal_map.hip).

``render_normals`` splats the normal of every Gaussian (``gaussian_normals``) into ``N = sum w_i n_i`` in the camera frame.  This
module holds that map to a target: a monocular normal prior, or the normals of the rendered depth (``depth_to_normal``), which is
the "normal consistency" term of the 2DGS / PGSR / GOF / RaDe-GS family -- the term that turns the Gaussians into disks that lie in
the surface.  Per view: ``N`` (3,H,W), the operator's weights map ``A`` (1,H,W), a target ``p`` (3,H,W) (constant data), an optional
pixel weight ``m >= 0`` (H,W) (``None``: 1).

    valid = A >= min_weight  and  |N|^2 finite and > min_norm^2  and  m > 0  and  |p|^2 finite and > 0.25
    nh = N/|N| ;  ph = p/|p| ;  w = m on valid pixels ;  cnt = sum w
    mode="cos":  l = 1 - nh . ph        mode="l1":  l = |nh - ph|_1   (sign(0) = 0)
    L_v = sum w l / cnt                  cnt <= 0: L_v = 0 and all gradients zero, never NaN

Opposing normals cancel in the blend, so a short ``N`` is not a direction: ``min_norm`` (default 0.1).  The target rule is
``normal_prior_loss``'s prior rule: a zero or NaN target means "no target here", so ``depth_to_normal``'s output goes in as it is.
Validity is a decision; the gradient goes to ``normal`` only -- none to ``weights``, the target or the mask -- and invalid pixels
get exact zeros.  ``A >= min_weight`` is a comparison in the dtype of the maps; everything after the loads is float64, in the
kernel and in ``normal_map_loss_torch`` alike.

``normal_map_loss_torch`` is the function in plain PyTorch on any device and dtype.  ``normal_map_loss`` is the HIP path: the V
views of a step in two launches forward and one backward per 16 views, sums in double through per-workgroup partial rows added in
a fixed order, no atomics and no memset, so it repeats bit for bit and a view's result does not depend on its neighbours.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib as L
from .depth_prior import _map_list, _ptr_field
from .normal_prior import MODES, PRIOR_MIN_SQ, _prior_list, _stack

_OP = "normal_map_loss"


def _normal_list(op: str, normal):
    seq = [normal] if torch.is_tensor(normal) else list(normal)
    if not seq:
        raise ValueError(f"{op}: no normal")
    for i, t in enumerate(seq):
        if not torch.is_tensor(t) or t.dim() != 3 or t.shape[0] != 3 or t.numel() < 3:
            raise ValueError(f"{op}: normal[{i}] must be a non-empty (3,H,W) tensor"
                             + (f", got {tuple(t.shape)}" if torch.is_tensor(t) else f", got {type(t).__name__}"))
        if tuple(t.shape) != tuple(seq[0].shape):
            raise ValueError(f"{op}: normal[{i}] is {tuple(t.shape)}, normal[0] is {tuple(seq[0].shape)}: one size per call")
    return seq


def _arguments(op: str, normal, weights, target, mask, mode, min_weight, min_norm):
    """The checks the HIP path and the PyTorch statement share: (normals, weights, targets, masks, min_weight, min_norm)."""
    if mode not in MODES:
        raise ValueError(f"{op}: mode must be 'cos' or 'l1', got {mode!r}")
    Ns = _normal_list(op, normal)
    As = _map_list(op, "weights", weights, like=Ns)
    ps = _prior_list(op, target, Ns)
    ms = [None] * len(Ns) if mask is None else _map_list(op, "mask", mask, like=Ns, optional=True)
    for i, m in enumerate(ms):
        if m is not None and m.dtype == torch.bool:
            raise TypeError(f"{op}: mask[{i}] is a bool tensor; the mask is a float pixel weight: pass mask.float()")
    min_weight, min_norm = float(min_weight), float(min_norm)
    if math.isnan(min_weight):
        raise ValueError(f"{op}: min_weight is NaN")
    if not (min_norm >= 0 and math.isfinite(min_norm)):
        raise ValueError(f"{op}: min_norm must be a non-negative number, got {min_norm}")
    return Ns, As, ps, ms, min_weight, min_norm


# ------------------------------------------------------------------------------------------------------------------ PyTorch
def normal_map_loss_torch(normal, weights, target, mask=None, *, mode="cos", min_weight=0.5, min_norm=0.1):
    """The function of the module docstring in plain PyTorch, on the device and in the dtype of ``normal``; autograd gives its
    backward.  Arguments and result as ``normal_map_loss``: ``(loss (V,), count (V,))`` in the dtype of ``normal``.  Everything after
    the loads is formed in float64, as the kernel does: in float64 this is the reference, in float32 the comparison path."""
    op = "normal_map_loss_torch"
    Ns, As, ps, ms, min_weight, min_norm = _arguments(op, normal, weights, target, mask, mode, min_weight, min_norm)
    H, W = Ns[0].shape[-2:]
    dt, dev = Ns[0].dtype, Ns[0].device
    N = torch.stack(list(Ns)).double().permute(0, 2, 3, 1)                                       # (V,H,W,3)
    p = torch.stack(list(ps)).to(device=dev, dtype=dt).double().permute(0, 2, 3, 1)
    A = _stack(As, H, W, dt, dev)
    m = torch.stack([torch.ones(H, W, dtype=dt, device=dev) if t is None else t.reshape(H, W).to(device=dev, dtype=dt) for t in ms])
    with torch.no_grad():                                      # decisions
        Nd = N.detach()
        nn = Nd[..., 0] * Nd[..., 0] + Nd[..., 1] * Nd[..., 1] + Nd[..., 2] * Nd[..., 2]
        pp = p[..., 0] * p[..., 0] + p[..., 1] * p[..., 1] + p[..., 2] * p[..., 2]
        mn = torch.as_tensor(min_norm, dtype=dt, device=dev).double()
        valid = ((A >= torch.as_tensor(min_weight, dtype=dt, device=dev)) & torch.isfinite(nn) & (nn > mn * mn) & (m > 0)
                 & torch.isfinite(pp) & (pp > PRIOR_MIN_SQ))
    away = torch.tensor((0.0, 0.0, -1.0), dtype=torch.float64, device=dev)
    Nv, pv = torch.where(valid[..., None], N, away), torch.where(valid[..., None], p, away)      # an invalid pixel: constants, w = 0
    nh = Nv / torch.sqrt(Nv[..., 0] * Nv[..., 0] + Nv[..., 1] * Nv[..., 1] + Nv[..., 2] * Nv[..., 2])[..., None]
    ph = pv / torch.sqrt(pv[..., 0] * pv[..., 0] + pv[..., 1] * pv[..., 1] + pv[..., 2] * pv[..., 2])[..., None]
    if mode == "l1":
        lpix = (nh[..., 0] - ph[..., 0]).abs() + (nh[..., 1] - ph[..., 1]).abs() + (nh[..., 2] - ph[..., 2]).abs()
    else:
        lpix = 1.0 - (nh[..., 0] * ph[..., 0] + nh[..., 1] * ph[..., 1] + nh[..., 2] * ph[..., 2])
    w = torch.where(valid, m, torch.zeros((), dtype=dt, device=dev)).double()
    cnt = w.sum((1, 2))
    some = cnt > 0
    inv = torch.where(some, 1.0 / torch.where(some, cnt, torch.ones_like(cnt)), torch.zeros_like(cnt))
    loss = (w * lpix).sum((1, 2)) * inv
    return loss.to(dt), cnt.detach().to(dt)


# ------------------------------------------------------------------------------------------------------------------ HIP
class _NormalMap(torch.autograd.Function):
    """``maps``: V normal maps, V weights maps, V targets, V masks (any of the masks None), as separate tensors: nothing is stacked."""

    @staticmethod
    def forward(ctx, mode, min_weight, min_norm, V, *maps):
        normals, weights, targets, masks = (list(maps[k * V:(k + 1) * V]) for k in range(4))
        dev, (H, W) = normals[0].device, normals[0].shape[-2:]
        loss = torch.empty(V, dtype=torch.float32, device=dev)
        count = torch.empty(V, dtype=torch.float32, device=dev)
        stats = torch.empty(V, L.NORMAL_MAP_STATS, dtype=torch.float64, device=dev)
        ws = L.workspace(L.load().bags_normal_map_workspace_size(min(V, L.MAX_POSE_ROWS), H, W), dev)
        structs = []
        for b in range(0, V, L.MAX_POSE_ROWS):
            part = slice(b, b + L.MAX_POSE_ROWS)
            n = len(normals[part])
            args = L.BagsNormalMap(mode, H, W, n, min_weight, min_norm, _ptr_field(normals[part]), _ptr_field(weights[part]),
                                   _ptr_field(targets[part]), _ptr_field(masks[part]))
            L.call("bags_normal_map_forward", dev, C.byref(args), L.ptr(ws), ws.numel(), loss[part].data_ptr(), count[part].data_ptr(),
                   stats[part].data_ptr())
            structs.append(args)
        ctx.mark_non_differentiable(count)
        if any(ctx.needs_input_grad):                          # nothing is kept under no_grad or for constant inputs
            ctx.save_for_backward(stats, *maps)                # versions are checked at backward: the adjoint re-reads the maps
            ctx.structs, ctx.V = structs, V
        return loss, count

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss, _g_count):
        stats, *maps = ctx.saved_tensors                       # raises if a map was written in place since the forward
        V, need = ctx.V, ctx.needs_input_grad
        dev = stats.device
        g = L.as_f32c(g_loss)
        g_normal = [torch.empty_like(t) if need[4 + i] else None for i, t in enumerate(maps[:V])]
        for k, args in enumerate(ctx.structs):
            part = slice(k * L.MAX_POSE_ROWS, (k + 1) * L.MAX_POSE_ROWS)
            L.call("bags_normal_map_backward", dev, C.byref(args), stats[part].data_ptr(), g[part].data_ptr(), _ptr_field(g_normal[part]))
        return (None, None, None, None, *g_normal, *([None] * (3 * V)))


_HOST = ": bags_raster.normal_map_loss_torch is the same function in PyTorch on any device and dtype"


def normal_map_loss(normal, weights, target, mask=None, *, mode="cos", min_weight=0.5, min_norm=0.1):
    """The loss of the module docstring on an AMD GPU: ``(loss (V,), count (V,))``, ``count[v] = cnt`` of view v.

    ``normal`` is ``(3,H,W)`` of one view and ``weights`` the operator's ``(1,H,W)`` map, or sequences of V of them -- the ``"normal"``
    and ``"weights"`` entries of what ``render_normals`` returns go in as they are, nothing is stacked or copied; ``target`` is
    ``(3,H,W)`` per view, ``mask`` ``(H,W)`` or ``(1,H,W)`` (``mask=None``, or a None entry: every pixel weighs 1).  float32,
    contiguous tensors on one device; a bool mask raises (pass ``mask.float()``).  Two HIP launches forward and one backward per 16
    views.  Differentiable in ``normal`` only; ``count`` is not differentiable.  The backward re-reads the maps: writing one of them
    in place between forward and backward raises."""
    Ns, As, ps, ms, min_weight, min_norm = _arguments(_OP, normal, weights, target, mask, mode, min_weight, min_norm)
    L.require(_OP, "normal[0]", Ns[0], gpu=True, f32=True, contiguous=True, host=_HOST)
    for name, ts in (("normal", Ns), ("weights", As), ("target", ps), ("mask", ms)):
        for i, t in enumerate(ts):
            if t is not None:
                L.require(_OP, f"{name}[{i}]", t, gpu=True, f32=True, contiguous=True, on=Ns[0], host=_HOST)
    H, W = Ns[0].shape[-2:]
    if H * W >= 2 ** 31:
        raise ValueError(f"{_OP}: a map of {W}x{H} has 2^31 pixels or more")
    return _NormalMap.apply(MODES[mode], min_weight, min_norm, len(Ns), *Ns, *As, *ps, *ms)
