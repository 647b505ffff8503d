"""depth_smooth_loss, normal_smooth_loss -- edge-aware smoothness of the rasterizer's maps (csrc/smooth.hip).

``depth_prior_loss``, ``normal_prior_loss``, ``correspondence_loss``, ``warp_loss`` and ``normal_map_loss`` are data terms: each holds a
map to a prior, a match or another view.  This module is the regulariser the same recipes put beside them: Monodepth2's
``get_smooth_loss`` (the edge-aware first-order smoothness of the mean-normalised inverse depth, carried by the self-supervised-depth
and CF-3DGS / Nope-NeRF line beside the photometric term), DN-Splatter's ``EdgeAwareTV`` on depth and ``TVLoss`` on the rendered
normals, and the second-order variants, which are zero on planes in inverse depth and so do not fight slanted walls.  Per view: a
field ``F`` of C channels on usable pixels, an optional guide image ``I`` (Cg,H,W) with Cg = 1 or 3 (the ground-truth image; constant
data), an optional pixel weight ``m >= 0`` (H,W) (``None``: 1).

    depth (C = 1):    solid = A >= min_weight and D > 0 ;  x = A / D (space="inverse") or D / A (space="depth"), one division in the
                      dtype of the maps ;  usable = solid and x finite and m > 0
                      normalize: mu = sum_usable x / n (n: the number of usable pixels), F = x / mu ;  else F = x
    normals (C = 3):  usable = A >= min_weight and |N|^2 finite and > min_norm^2 and m > 0 ;  F = N / |N|
    order=1: the stencil anchored at (u,v), u <= W-2, has members (u,v), (u+1,v):  d = F(u+1,v) - F(u,v) ;  g = mean_c |I(u+1,v) - I(u,v)|
    order=2: the stencil centred at (u,v), 1 <= u <= W-2, has members (u-1,v), (u,v), (u+1,v):  d = F(u-1,v) - 2 F(u,v) + F(u+1,v) ;
             g = mean_c |I(u+1,v) - I(u-1,v)| / 2                                                    (and the same along v)
    a stencil is valid when all its members are inside the image and usable and g is finite (no guide: g = 0)
    e = exp(-gamma g) ;  w = min of m over the members
    rho(d) = (1/C) sum_c rho1(d_c) ;  penalty="l1": rho1(t) = sqrt(t^2 + eps^2) - eps (eps = 0: |t|, sign(0) = 0) ;  "l2": rho1(t) = t^2
    S_dir = sum w e rho(d) ;  cnt_dir = sum w ;  L_v = S_x / cnt_x + S_y / cnt_y (cnt_dir <= 0: that direction counts 0)
    count = cnt_x + cnt_y

A view with no valid stencil, no usable pixel, a mean that is zero or not finite, or ``H``, ``W`` too small for the order has loss 0
and all-zero gradients, never NaN.  Validity, the edge weight and ``min`` are decisions or constant data and are not differentiated
through: the depth front-end has gradients to ``depth`` and ``weights`` (through ``mu`` as well, as Monodepth2's has), the normals
front-end to ``normal`` only; pixels that are not usable get exact zeros.  Everything after ``x`` (depth) or after the loads
(normals) is float64, in the kernels and in the ``*_torch`` statements alike; the kernels evaluate ``exp`` in float32.

With everything valid, ``depth_smooth_loss(..., space="inverse", normalize=True, order=1, penalty="l1", gamma=1)`` is Monodepth2's
``get_smooth_loss``, ``depth_smooth_loss(..., normalize=False)`` DN-Splatter's ``EdgeAwareTV`` and
``normal_smooth_loss(..., guide=None)`` its ``TVLoss`` on the unit normals (the mean of the squared differences with
``penalty="l2"``, of the absolute ones with ``"l1"``), to float64 round-off.

``depth_smooth_loss_torch`` / ``normal_smooth_loss_torch`` are the functions in plain PyTorch on any device and dtype.
``depth_smooth_loss`` / ``normal_smooth_loss`` are the HIP path: the V views of a step in two launches forward (three with
``normalize``) and one backward per 16 views, sums in double through per-workgroup partial rows added in a fixed order, no atomics
and no memset, so they repeat bit for bit and a view's result does not depend on its neighbours.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib as L
from .depth_prior import SPACES, _map_list, _ptr_field
from .normal_map import _normal_list
from .normal_prior import _stack

PENALTIES = {"l1": L.SMOOTH_L1, "l2": L.SMOOTH_L2}


def _guide_list(op: str, guide, like):
    """``guide`` as V tensors (Cg,H,W) with one Cg in {1, 3}, or None for the whole call."""
    if guide is None:
        return None
    seq = [guide] if torch.is_tensor(guide) else list(guide)
    if len(seq) != len(like):
        raise ValueError(f"{op}: {len(like)} views but {len(seq)} guide")
    for i, t in enumerate(seq):
        if t is None:
            raise ValueError(f"{op}: guide[{i}] is None; guide=None is for the whole call, not per entry")
        if not torch.is_tensor(t) or t.dim() != 3 or t.shape[0] not in (1, 3) or tuple(t.shape[-2:]) != tuple(like[0].shape[-2:]):
            raise ValueError(f"{op}: guide[{i}] must be (1,H,W) or (3,H,W) with the maps' H, W"
                             + (f", got {tuple(t.shape)}" if torch.is_tensor(t) else f", got {type(t).__name__}"))
        if t.shape[0] != seq[0].shape[0]:
            raise ValueError(f"{op}: guide[{i}] has {t.shape[0]} channels, guide[0] has {seq[0].shape[0]}: one count per call")
    return seq


def _arguments(op: str, normals: bool, field, weights, guide, mask, space, order, penalty, eps, gamma, min_weight, min_norm):
    """The checks the HIP path and the PyTorch statement share: (fields, weights, guides or None, masks, eps, gamma, min_weight,
    min_norm)."""
    if space not in SPACES:
        raise ValueError(f"{op}: space must be 'depth' or 'inverse', got {space!r}")
    if order not in (1, 2) or isinstance(order, bool):
        raise ValueError(f"{op}: order must be 1 or 2, got {order!r}")
    if penalty not in PENALTIES:
        raise ValueError(f"{op}: penalty must be 'l1' or 'l2', got {penalty!r}")
    eps, gamma, min_weight, min_norm = float(eps), float(gamma), float(min_weight), float(min_norm)
    if not (eps >= 0 and math.isfinite(eps)):
        raise ValueError(f"{op}: eps must be a non-negative number, got {eps}")
    if penalty == "l2" and eps != 0:
        raise ValueError(f"{op}: eps must be 0 with penalty='l2' (it is the Charbonnier width of 'l1'), got {eps}")
    if not (gamma >= 0 and math.isfinite(gamma)):
        raise ValueError(f"{op}: gamma must be a non-negative number, got {gamma}")
    if math.isnan(min_weight):
        raise ValueError(f"{op}: min_weight is NaN")
    if not (min_norm >= 0 and math.isfinite(min_norm)):
        raise ValueError(f"{op}: min_norm must be a non-negative number, got {min_norm}")
    if normals:
        Fs = _normal_list(op, field)
    else:
        Fs = _map_list(op, "depth", field)
        Fs = _map_list(op, "depth", Fs, like=Fs)
    As = _map_list(op, "weights", weights, like=Fs)
    Gs = _guide_list(op, guide, Fs)
    ms = [None] * len(Fs) if mask is None else _map_list(op, "mask", mask, like=Fs, optional=True)
    for i, m in enumerate(ms):
        if m is not None and m.dtype == torch.bool:
            raise TypeError(f"{op}: mask[{i}] is a bool tensor; the mask is a float pixel weight: pass mask.float()")
    return Fs, As, Gs, ms, eps, gamma, min_weight, min_norm


# ------------------------------------------------------------------------------------------------------------------ PyTorch
def _members(t, order, axis):
    """The members of every stencil along ``axis`` (-1: horizontal, -2: vertical) as slices of ``t``: (lo, hi) or (lo, centre, hi)."""
    n = t.shape[axis]
    if n <= order:                                             # too small for the order: no stencil
        return tuple(t.narrow(axis, 0, 0) for _ in range(order + 1))
    return tuple(t.narrow(axis, k, n - order) for k in range(order + 1))


def _smooth_torch(F, usable, m, I, order, penalty, eps, gamma):
    """``F`` (V,C,H,W) float64 (finite constants where not usable), ``usable`` (V,H,W), ``m`` (V,H,W) in the dtype of the maps, ``I``
    (V,Cg,H,W) float64 or None: (loss (V,), count (V,)) in float64."""
    loss, count = 0.0, 0.0
    for axis in (-1, -2):
        fs, us, ws = _members(F, order, axis), _members(usable, order, axis), _members(m, order, axis)
        with torch.no_grad():                                  # decisions and constant data
            valid, w = us[0], ws[0]
            for u_, w_ in zip(us[1:], ws[1:]):
                valid, w = valid & u_, torch.minimum(w, w_)
            if I is None:
                e = torch.ones_like(w, dtype=torch.float64)
            else:
                gi = _members(I, order, axis)
                g = (gi[-1] - gi[0]).abs().mean(1) / order
                valid = valid & torch.isfinite(g)
                e = torch.exp(-gamma * torch.where(valid, g, torch.zeros_like(g)))
            w = torch.where(valid, w, torch.zeros_like(w)).double()
        d = fs[1] - fs[0] if order == 1 else (fs[0] - 2.0 * fs[1]) + fs[2]
        if penalty == "l2":
            r = d * d
        elif eps == 0:
            r = d.abs()
        else:
            r = torch.sqrt(d * d + eps * eps) - eps
        S = ((w * e) * r.mean(1)).sum((1, 2))
        cnt = w.sum((1, 2))
        some = cnt > 0
        inv = torch.where(some, 1.0 / torch.where(some, cnt, torch.ones_like(cnt)), torch.zeros_like(cnt))
        loss, count = loss + S * inv, count + cnt
    return loss, count


def _guide_mask_torch(Gs, ms, H, W, dt, dev):
    I = None if Gs is None else torch.stack(list(Gs)).to(device=dev, dtype=dt).double()
    m = torch.stack([torch.ones(H, W, dtype=dt, device=dev) if t is None else t.reshape(H, W).to(device=dev, dtype=dt) for t in ms])
    return I, m


def depth_smooth_loss_torch(depth, weights, guide=None, mask=None, *, space="inverse", normalize=True, order=1, penalty="l1", eps=0.0,
                            gamma=1.0, min_weight=0.5):
    """The depth function of the module docstring in plain PyTorch, on the device and in the dtype of ``depth``; autograd gives its
    backward.  Arguments and result as ``depth_smooth_loss``: ``(loss (V,), count (V,))`` in the dtype of ``depth``.  ``x`` is formed
    in that dtype, everything after it in float64, as the kernel does: in float64 this is the reference, in float32 the comparison
    path."""
    op = "depth_smooth_loss_torch"
    Ds, As, Gs, ms, eps, gamma, min_weight, _ = _arguments(op, False, depth, weights, guide, mask, space, order, penalty, eps, gamma, min_weight, 0.0)
    H, W = Ds[0].shape[-2:]
    dt, dev = Ds[0].dtype, Ds[0].device
    D, A = _stack(Ds, H, W, dt, dev), _stack(As, H, W, dt, dev)
    I, m = _guide_mask_torch(Gs, ms, H, W, dt, dev)
    one = torch.ones((), dtype=dt, device=dev)
    with torch.no_grad():                                      # decisions
        solid = (A >= torch.as_tensor(min_weight, dtype=dt, device=dev)) & (D > 0)
        x0 = torch.where(solid, A, one) / torch.where(solid, D, one) if space == "inverse" else torch.where(solid, D, one) / torch.where(solid, A, one)
        usable = solid & torch.isfinite(x0) & (m > 0)
    Dv, Av = torch.where(usable, D, one), torch.where(usable, A, one)          # a pixel that is not usable: x = 1, no gradient
    x = (Av / Dv if space == "inverse" else Dv / Av).double()
    if normalize:
        n = usable.sum((1, 2)).double()
        mu = torch.where(usable, x, torch.zeros_like(x)).sum((1, 2)) / torch.where(n > 0, n, torch.ones_like(n))
        with torch.no_grad():
            live = (n > 0) & torch.isfinite(mu) & (mu != 0)
        inv_mu = torch.where(live, 1.0 / torch.where(live, mu, torch.ones_like(mu)), torch.zeros_like(mu))
        x = x * inv_mu[:, None, None]
    loss, count = _smooth_torch(x[:, None], usable, m, I, order, penalty, eps, gamma)
    return loss.to(dt), count.detach().to(dt)


def normal_smooth_loss_torch(normal, weights, guide=None, mask=None, *, order=1, penalty="l1", eps=0.0, gamma=1.0, min_weight=0.5,
                             min_norm=0.1):
    """The normals function of the module docstring in plain PyTorch, on the device and in the dtype of ``normal``; autograd gives
    its backward.  Arguments and result as ``normal_smooth_loss``: ``(loss (V,), count (V,))`` in the dtype of ``normal``.  Everything
    after the loads is formed in float64, as the kernel does: in float64 this is the reference, in float32 the comparison path."""
    op = "normal_smooth_loss_torch"
    Ns, As, Gs, ms, eps, gamma, min_weight, min_norm = _arguments(op, True, normal, weights, guide, mask, "inverse", order, penalty, eps, gamma,
                                                                  min_weight, min_norm)
    H, W = Ns[0].shape[-2:]
    dt, dev = Ns[0].dtype, Ns[0].device
    N = torch.stack(list(Ns)).double()                                                           # (V,3,H,W)
    A = _stack(As, H, W, dt, dev)
    I, m = _guide_mask_torch(Gs, ms, H, W, dt, dev)
    with torch.no_grad():                                      # decisions
        Nd = N.detach()
        nn = Nd[:, 0] * Nd[:, 0] + Nd[:, 1] * Nd[:, 1] + Nd[:, 2] * Nd[:, 2]
        mn = torch.as_tensor(min_norm, dtype=dt, device=dev).double()
        usable = (A >= torch.as_tensor(min_weight, dtype=dt, device=dev)) & torch.isfinite(nn) & (nn > mn * mn) & (m > 0)
    away = torch.tensor((0.0, 0.0, -1.0), dtype=torch.float64, device=dev)[None, :, None, None]
    Nv = torch.where(usable[:, None], N, away)                                                   # not usable: a constant, no gradient
    F = Nv / torch.sqrt(Nv[:, 0] * Nv[:, 0] + Nv[:, 1] * Nv[:, 1] + Nv[:, 2] * Nv[:, 2])[:, None]
    loss, count = _smooth_torch(F, usable, m, I, order, penalty, eps, gamma)
    return loss.to(dt), count.detach().to(dt)


# ------------------------------------------------------------------------------------------------------------------ HIP
class _Smooth(torch.autograd.Function):
    """``maps``: V field maps, V weights maps, V guides (all None without a guide), V masks (any of them None), as separate tensors:
    nothing is stacked.  ``cfg``: (kind, space, order, penalty, normalize, guide channels, eps, gamma, min_weight, min_norm)."""

    @staticmethod
    def forward(ctx, cfg, V, *maps):
        fields, weights, guides, masks = (list(maps[k * V:(k + 1) * V]) for k in range(4))
        kind, space, order, penalty, normalize, cg, eps, gamma, min_weight, min_norm = cfg
        dev, (H, W) = fields[0].device, fields[0].shape[-2:]
        loss = torch.empty(V, dtype=torch.float32, device=dev)
        count = torch.empty(V, dtype=torch.float32, device=dev)
        stats = torch.empty(V, L.SMOOTH_STATS, dtype=torch.float64, device=dev)
        ws = L.workspace(L.load().bags_smooth_workspace_size(min(V, L.MAX_POSE_ROWS), H, W), dev)
        structs = []
        for b in range(0, V, L.MAX_POSE_ROWS):
            part = slice(b, b + L.MAX_POSE_ROWS)
            n = len(fields[part])
            args = L.BagsSmooth(kind, space, order, penalty, normalize, H, W, n, cg, 0, min_weight, min_norm, eps, gamma,
                                _ptr_field(fields[part]), _ptr_field(weights[part]), _ptr_field(guides[part]), _ptr_field(masks[part]))
            L.call("bags_smooth_forward", dev, C.byref(args), L.ptr(ws), ws.numel(), loss[part].data_ptr(), count[part].data_ptr(),
                   stats[part].data_ptr())
            structs.append(args)
        ctx.mark_non_differentiable(count)
        if any(ctx.needs_input_grad):                          # nothing is kept under no_grad or for constant inputs
            ctx.save_for_backward(stats, *maps)                # versions are checked at backward: the adjoint re-reads the maps
            ctx.structs, ctx.V, ctx.kind = structs, V, kind
        return loss, count

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss, _g_count):
        stats, *maps = ctx.saved_tensors                       # raises if a map was written in place since the forward
        V, need = ctx.V, ctx.needs_input_grad
        dev = stats.device
        g = L.as_f32c(g_loss)
        g_field = [torch.empty_like(t) if need[2 + i] else None for i, t in enumerate(maps[:V])]
        depth = ctx.kind == L.SMOOTH_DEPTH                     # the normals front-end has no gradient to the weights
        g_weights = [torch.empty_like(t) if depth and need[2 + V + i] else None for i, t in enumerate(maps[V:2 * V])]
        for k, args in enumerate(ctx.structs):
            part = slice(k * L.MAX_POSE_ROWS, (k + 1) * L.MAX_POSE_ROWS)
            L.call("bags_smooth_backward", dev, C.byref(args), stats[part].data_ptr(), g[part].data_ptr(), _ptr_field(g_field[part]),
                   _ptr_field(g_weights[part]))
        return (None, None, *g_field, *g_weights, *([None] * (2 * V)))


def _hip(op: str, kind, Fs, As, Gs, ms, space, order, penalty, normalize, eps, gamma, min_weight, min_norm):
    host = f": bags_raster.{op}_torch is the same function in PyTorch on any device and dtype"
    first = "normal" if kind == L.SMOOTH_NORMAL else "depth"
    L.require(op, f"{first}[0]", Fs[0], gpu=True, f32=True, contiguous=True, host=host)
    for name, ts in ((first, Fs), ("weights", As), ("guide", Gs or []), ("mask", ms)):
        for i, t in enumerate(ts):
            if t is not None:
                L.require(op, f"{name}[{i}]", t, gpu=True, f32=True, contiguous=True, on=Fs[0], host=host)
    H, W = Fs[0].shape[-2:]
    if H * W >= 2 ** 31:
        raise ValueError(f"{op}: a map of {W}x{H} has 2^31 pixels or more")
    V = len(Fs)
    cfg = (kind, SPACES[space], order, PENALTIES[penalty], int(bool(normalize)), 0 if Gs is None else Gs[0].shape[0], eps, gamma, min_weight,
           min_norm)
    return _Smooth.apply(cfg, V, *Fs, *As, *(Gs if Gs is not None else [None] * V), *ms)


def depth_smooth_loss(depth, weights, guide=None, mask=None, *, space="inverse", normalize=True, order=1, penalty="l1", eps=0.0, gamma=1.0,
                      min_weight=0.5):
    """The depth smoothness of the module docstring on an AMD GPU: ``(loss (V,), count (V,))``, ``count[v] = cnt_x + cnt_y`` of view v.

    ``depth`` and ``weights`` are the operator's maps ``(1,H,W)`` of one view, or sequences of V of them -- the ``"depth"`` and
    ``"weights"`` entries of what ``render_views`` returns go in as they are, nothing is stacked or copied; ``guide`` is ``(1,H,W)``
    or ``(3,H,W)`` per view (the ground-truth image; ``None`` for the whole call: no edge weight), ``mask`` ``(H,W)`` or ``(1,H,W)``
    (``mask=None``, or a None entry: every pixel weighs 1).  float32, contiguous tensors on one device; a bool mask raises (pass
    ``mask.float()``).  The defaults are Monodepth2's ``get_smooth_loss``; ``normalize=False`` is DN-Splatter's ``EdgeAwareTV``;
    ``order=2`` is zero on planes in inverse depth.  Two HIP launches forward (three with ``normalize``) and one backward per 16
    views.  Differentiable in ``depth`` and ``weights``; ``count`` is not differentiable.  The backward re-reads the maps: writing
    one of them in place between forward and backward raises."""
    op = "depth_smooth_loss"
    Ds, As, Gs, ms, eps, gamma, min_weight, _ = _arguments(op, False, depth, weights, guide, mask, space, order, penalty, eps, gamma, min_weight, 0.0)
    return _hip(op, L.SMOOTH_DEPTH, Ds, As, Gs, ms, space, order, penalty, normalize, eps, gamma, min_weight, 0.0)


def normal_smooth_loss(normal, weights, guide=None, mask=None, *, order=1, penalty="l1", eps=0.0, gamma=1.0, min_weight=0.5, min_norm=0.1):
    """The normal smoothness of the module docstring on an AMD GPU: ``(loss (V,), count (V,))``, ``count[v] = cnt_x + cnt_y`` of view v.

    ``normal`` is ``(3,H,W)`` of one view and ``weights`` the operator's ``(1,H,W)`` map, or sequences of V of them -- the ``"normal"``
    and ``"weights"`` entries of what ``render_normals`` returns go in as they are; ``guide`` and ``mask`` as ``depth_smooth_loss``'s.
    ``guide=None, penalty="l2"`` is DN-Splatter's ``TVLoss``.  float32, contiguous tensors on one device.  Two HIP launches forward
    and one backward per 16 views.  Differentiable in ``normal`` only; ``count`` is not differentiable.  The backward re-reads the
    maps: writing one of them in place between forward and backward raises."""
    op = "normal_smooth_loss"
    Ns, As, Gs, ms, eps, gamma, min_weight, min_norm = _arguments(op, True, normal, weights, guide, mask, "inverse", order, penalty, eps, gamma,
                                                                  min_weight, min_norm)
    return _hip(op, L.SMOOTH_NORMAL, Ns, As, Gs, ms, "inverse", order, penalty, False, eps, gamma, min_weight, min_norm)
