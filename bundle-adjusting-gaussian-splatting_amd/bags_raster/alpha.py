"""alpha_loss -- the operator's weights map held to a silhouette or a sky mask, or pushed to solid-or-empty (csrc/alpha.hip).

The operator returns the accumulated opacity ``A = sum w_i`` of every pixel as its ``weights`` map.  The other fused losses use it as
a validity gate or as a denominator; this one holds the map itself to something: a foreground mask (the silhouette loss of the
object-centric recipes), ``1 - sky`` (the sky loss of the urban ones), or its own entropy (every pixel solid or empty: no haze).
Per view: ``A`` (1,H,W), an optional target ``t`` (H,W) (constant data), an optional pixel weight ``m >= 0`` (H,W) (``None``: 1).

    usable = A finite  and  m > 0  and  (entropy: always | target modes: t finite; bce also 0 <= t <= 1)
    w = m on usable pixels, else 0 ;  cnt = sum w
    inside = lo < A < hi,  lo = eps, hi = 1 - eps, both rounded once to the dtype of the maps and compared in that dtype
    a = A where inside, lo where A <= lo, hi where A >= hi            (bce, entropy only)
    mode="bce":      l = -(t log a + (1-t) log(1-a))          dl/dA = (a - t) / (a (1 - a))  inside, 0 outside
    mode="entropy":  l = -(a log a + (1-a) log(1-a))          dl/dA = log((1 - a) / a)       inside, 0 outside   (no target)
    mode="l1":       l = |A - t|                              dl/dA = sign(A - t), sign(0) = 0
    mode="l2":       l = (A - t)^2                            dl/dA = 2 (A - t)
    L_v = sum w l / cnt                                       cnt <= 0: L_v = 0 and the gradient all zeros, never NaN

The target rule is ``normal_map_loss``'s: a NaN or out-of-range target means "no target here".  Validity and the clamp are
decisions; the gradient goes to ``weights`` only -- none to the target or the mask -- and pixels that are not usable get exact
zeros.  Everything after the loads is float64, in the kernel and in ``alpha_loss_torch`` alike.  For the gradient to reach the
Gaussians the maps must come from ``render_views(..., depth_weights_grad=True)``.

``alpha_loss_torch`` is the function in plain PyTorch on any device and dtype.  ``alpha_loss`` is the HIP path: the V views of a
step in two launches forward and one backward per 16 views, sums in double through a fixed number of per-workgroup partial rows
added in index order, no atomics and no memset, so it repeats bit for bit and a view's result does not depend on its neighbours.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L
from .depth_prior import _map_list, _ptr_field

MODES = {"bce": L.ALPHA_BCE, "l1": L.ALPHA_L1, "l2": L.ALPHA_L2, "entropy": L.ALPHA_ENTROPY}
_OP = "alpha_loss"


def _arguments(op: str, weights, target, mask, mode, eps):
    """The checks the HIP path and the PyTorch statement share: (weights, targets or Nones, masks, eps)."""
    if mode not in MODES:
        raise ValueError(f"{op}: mode must be 'bce', 'l1', 'l2' or 'entropy', got {mode!r}")
    As = _map_list(op, "weights", weights)
    As = _map_list(op, "weights", As, like=As)
    if mode == "entropy":
        if target is not None:
            raise ValueError(f"{op}: mode='entropy' takes no target")
        ts = [None] * len(As)
    else:
        if target is None:
            raise ValueError(f"{op}: mode={mode!r} needs a target")
        ts = _map_list(op, "target", target, like=As)
    ms = [None] * len(As) if mask is None else _map_list(op, "mask", mask, like=As, optional=True)
    for i, m in enumerate(ms):
        if m is not None and m.dtype == torch.bool:
            raise TypeError(f"{op}: mask[{i}] is a bool tensor; the mask is a float pixel weight: pass mask.float()")
    eps = float(eps)
    if not 0.0 < eps < 0.5:
        raise ValueError(f"{op}: eps must be in (0, 0.5), got {eps}")
    return As, ts, ms, eps


# ------------------------------------------------------------------------------------------------------------------ PyTorch
def alpha_loss_torch(weights, target=None, mask=None, *, mode="bce", eps=1e-4):
    """The function of the module docstring in plain PyTorch, on the device and in the dtype of ``weights``; autograd gives its
    backward.  Arguments and result as ``alpha_loss``: ``(loss (V,), count (V,))`` in the dtype of ``weights``.  The comparisons are
    made in that dtype, everything after them in float64, as the kernel does: in float64 this is the reference, in float32 the
    comparison path."""
    op = "alpha_loss_torch"
    As, ts, ms, eps = _arguments(op, weights, target, mask, mode, eps)
    H, W = As[0].shape[-2:]
    dt, dev = As[0].dtype, As[0].device
    place = lambda x: x.reshape(H, W).to(device=dev, dtype=dt)                                   # noqa: E731
    A = torch.stack([place(x) for x in As])                                                      # (V,H,W)
    t = None if mode == "entropy" else torch.stack([place(x) for x in ts])
    m = torch.stack([torch.ones(H, W, dtype=dt, device=dev) if x is None else place(x) for x in ms])
    lo, hi = torch.as_tensor(eps, dtype=dt, device=dev), torch.as_tensor(1.0 - eps, dtype=dt, device=dev)
    half = torch.full((), 0.5, dtype=torch.float64, device=dev)
    with torch.no_grad():                                      # decisions
        Ad = A.detach()
        usable = torch.isfinite(Ad) & (m > 0)
        if t is not None:
            usable = usable & torch.isfinite(t)
        if mode == "bce":
            usable = usable & (t >= 0) & (t <= 1)
        low, high = Ad <= lo, Ad >= hi
    A64 = A.double()
    tv = None if t is None else torch.where(usable, t.double(), half)                            # an unusable pixel: constants, w = 0
    if mode in ("bce", "entropy"):
        a = torch.where(usable & ~low & ~high, A64, torch.where(low, lo.double(), hi.double()))
        a = torch.where(usable, a, half)
        la, l1a = torch.log(a), torch.log(1.0 - a)
        lpix = -(tv * la + (1.0 - tv) * l1a) if mode == "bce" else -(a * la + (1.0 - a) * l1a)
    else:
        r = torch.where(usable, A64, half) - tv
        lpix = r.abs() if mode == "l1" else r * r
    w = torch.where(usable, m, torch.zeros((), dtype=dt, device=dev)).double()
    cnt = w.sum((1, 2))
    some = cnt > 0
    inv = torch.where(some, 1.0 / torch.where(some, cnt, torch.ones_like(cnt)), torch.zeros_like(cnt))
    loss = (w * lpix).sum((1, 2)) * inv
    return loss.to(dt), cnt.detach().to(dt)


# ------------------------------------------------------------------------------------------------------------------ HIP
class _Alpha(torch.autograd.Function):
    """``maps``: V weights maps, V targets (all None in the entropy mode), V masks (any of them None), as separate tensors: nothing
    is stacked."""

    @staticmethod
    def forward(ctx, mode, lo, hi, V, *maps):
        weights, targets, masks = (list(maps[k * V:(k + 1) * V]) for k in range(3))
        dev, (H, W) = weights[0].device, weights[0].shape[-2:]
        loss = torch.empty(V, dtype=torch.float32, device=dev)
        count = torch.empty(V, dtype=torch.float32, device=dev)
        stats = torch.empty(V, L.ALPHA_STATS, dtype=torch.float64, device=dev)
        ws = L.workspace(L.ALPHA_WORKSPACE_BYTES, dev)         # a constant: the sums kernel's grid does not depend on the maps
        structs = []
        for b in range(0, V, L.MAX_POSE_ROWS):
            part = slice(b, b + L.MAX_POSE_ROWS)
            n = len(weights[part])
            args = L.BagsAlpha(mode, H, W, n, lo, hi, _ptr_field(weights[part]), _ptr_field(targets[part]), _ptr_field(masks[part]))
            L.call("bags_alpha_forward", dev, C.byref(args), L.ptr(ws), ws.numel(), loss[part].data_ptr(), count[part].data_ptr(),
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
        g_weights = [torch.empty_like(t) if need[4 + i] else None for i, t in enumerate(maps[:V])]
        for k, args in enumerate(ctx.structs):
            part = slice(k * L.MAX_POSE_ROWS, (k + 1) * L.MAX_POSE_ROWS)
            L.call("bags_alpha_backward", dev, C.byref(args), stats[part].data_ptr(), g[part].data_ptr(), _ptr_field(g_weights[part]))
        return (None, None, None, None, *g_weights, *([None] * (2 * V)))


_HOST = ": bags_raster.alpha_loss_torch is the same function in PyTorch on any device and dtype"


def alpha_loss(weights, target=None, mask=None, *, mode="bce", eps=1e-4):
    """The loss of the module docstring on an AMD GPU: ``(loss (V,), count (V,))``, ``count[v] = cnt`` of view v.

    ``weights`` is the operator's ``(1,H,W)`` map of one view or a sequence of V of them -- the ``"weights"`` entries of what
    ``render_views`` returns go in as they are, nothing is stacked or copied; ``target`` is ``(H,W)`` or ``(1,H,W)`` per view (none
    with ``mode="entropy"``), ``mask`` likewise (``mask=None``, or a None entry: every pixel weighs 1).  float32, contiguous tensors
    on one device; a bool mask raises (pass ``mask.float()``).  Two HIP launches forward and one backward per 16 views.
    Differentiable in ``weights`` only; ``count`` is not differentiable.  The backward re-reads the maps: writing one of them in
    place between forward and backward raises."""
    As, ts, ms, eps = _arguments(_OP, weights, target, mask, mode, eps)
    L.require(_OP, "weights[0]", As[0], gpu=True, f32=True, contiguous=True, host=_HOST)
    for name, seq in (("weights", As), ("target", ts), ("mask", ms)):
        for i, t in enumerate(seq):
            if t is not None:
                L.require(_OP, f"{name}[{i}]", t, gpu=True, f32=True, contiguous=True, on=As[0], host=_HOST)
    H, W = As[0].shape[-2:]
    if H * W >= 2 ** 31:
        raise ValueError(f"{_OP}: a map of {W}x{H} has 2^31 pixels or more")
    lo, hi = C.c_float(eps).value, C.c_float(1.0 - eps).value  # rounded once, here: the kernel compares in float32
    if not 0.0 < lo < hi < 1.0:
        raise ValueError(f"{_OP}: eps = {eps} leaves no float32 between eps and 1 - eps")
    return _Alpha.apply(MODES[mode], lo, hi, len(As), *As, *ts, *ms)
