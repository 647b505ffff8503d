"""normal_prior_loss -- a normal prior on the rasterizer's ``depth`` and ``weights`` maps (csrc/normal_prior.hip).

The operator returns ``depth = sum w_i z_i`` and ``weights = 1 - T_final``, differentiable with ``depth_weights_grad=True`` (DESIGN.md
decision D5).  ``depth_prior_loss`` holds the two maps to a monocular depth; this module holds the normals of the rendered depth, by
central differences, to a monocular normal map, which fixes the orientation of the surface (DN-Splatter, the 2DGS / GOF / RaDe-GS
family).  Per view: maps ``D``, ``A`` (1,H,W), a pinhole ``(fx, fy, cx, cy)`` in pixels, prior normals ``p`` (3,H,W) in the camera
frame of the operator's view space (x right, y down, z forward), an optional pixel weight ``m >= 0`` (H,W) (``None``: 1).

    solid(u,v)  = A >= min_weight  and  D > 0
    z           = D / A                      one division in the dtype of the maps; everything after it in float64
    P(u,v)      = z * ((u - cx)/fx, (v - cy)/fy, 1)
    dx = P(u+1,v) - P(u-1,v) ;  dy = P(u,v+1) - P(u,v-1)          (central differences, as 2DGS's depth_to_normal)
    N  = dy x dx ;  q = |N|^2 ;  n = N / sqrt(q)                   (faces the camera: n_z < 0 for a fronto-parallel wall)
    geometric(u,v) = the pixel and its four neighbours are inside the image and solid,
                     |z(u+1,v) - z(u-1,v)| <= max_jump * z(u,v)  and  |z(u,v+1) - z(u,v-1)| <= max_jump * z(u,v),
                     q is a positive finite number
    valid(u,v)  = geometric  and  m > 0  and  |p|^2 is finite and > 0.25      (a zero or NaN prior: "no prior here")
    ph = p / |p| ;  w = m on valid pixels ;  cnt = sum w
    mode="cos":  l = 1 - n . ph          mode="l1":  l = |n - ph|_1   (sign(0) = 0)
    L_v = sum w l / cnt                  cnt <= 0 (also every image with H < 3 or W < 3): L_v = 0, all gradients zero, never NaN

``max_jump = inf`` (the default) switches the guard off; a finite value drops depth discontinuities, where a difference across two
surfaces is not a normal.  Validity and the guard are decisions, not differentiated through; invalid pixels get exact-zero
gradients.  The pinhole is constant data, host floats: there is NO gradient to the intrinsics (out of scope); the pose and the
Gaussians are reached through ``depth`` and ``weights``.  ``min_weight`` must be positive.

``normal_prior_loss_torch`` is the function in plain PyTorch on any device and dtype.  ``normal_prior_loss`` is the HIP path: the V
views of a step in two launches forward and one backward per 16 views, sums without atomics, so it repeats bit for bit and a view's
result does not depend on its neighbours.  ``depth_to_normal`` / ``depth_to_normal_torch`` give ``n`` and ``geometric`` of one view,
``pinhole_of`` the pinhole of the operator's ``intrinsic``.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib as L
from .depth_prior import _map_list, _ptr_field

_OP = "normal_prior_loss"
MODES = {"cos": L.NORMAL_PRIOR_COS, "l1": L.NORMAL_PRIOR_L1}
PRIOR_MIN_SQ = 0.25                                            # |p|^2 at or below it: no prior here


def pinhole_of(intrinsic, H: int, W: int):
    """``(fx, fy, cx, cy)`` in pixels of the operator's ``intrinsic`` for an ``H x W`` image: ``fx = intrinsic[0,0] W/2`` and
    ``fy = intrinsic[1,1] H/2``, and, with the row-vector projection ``ndc = p_view @ intrinsic / w`` and the pixel rule
    ``px = ((ndc + 1) W - 1) / 2``, ``cx = (1 + intrinsic[2,0]) W/2 - 1/2`` and ``cy = (1 + intrinsic[2,1]) H/2 - 1/2``.  Host arithmetic
    in float64 on a CPU copy (for a GPU tensor that copy synchronises: take it once per camera, not per step)."""
    K = torch.as_tensor(intrinsic).detach().to("cpu", torch.float64)
    if K.dim() != 2 or K.shape[0] < 3 or K.shape[1] < 2:
        raise ValueError(f"pinhole_of: intrinsic must be a (3,3) matrix, got {tuple(K.shape)}")
    return (float(K[0, 0]) * W / 2, float(K[1, 1]) * H / 2, (1 + float(K[2, 0])) * W / 2 - 0.5, (1 + float(K[2, 1])) * H / 2 - 0.5)


def _pinholes(op: str, pinhole, V: int):
    """``pinhole`` as V tuples of four host floats: one ``(fx, fy, cx, cy)`` for every view, or V of them; numbers or a CPU tensor."""
    if torch.is_tensor(pinhole):
        if pinhole.is_cuda:
            raise ValueError(f"{op}: pinhole is a GPU tensor; it is constant host data (reading it here would synchronise): pass floats "
                             f"or a CPU tensor (bags_raster.pinhole_of)")
        pinhole = pinhole.detach().double().tolist()
    rows = list(pinhole)
    if not any(isinstance(r, (tuple, list)) or torch.is_tensor(r) for r in rows):         # plain numbers: one pinhole for every view
        rows = [rows] * V
    if len(rows) != V:
        raise ValueError(f"{op}: {V} views but {len(rows)} pinholes")
    out = []
    for i, r in enumerate(rows):
        if torch.is_tensor(r):
            if r.is_cuda:
                raise ValueError(f"{op}: pinhole[{i}] is a GPU tensor; it is constant host data: pass floats or a CPU tensor")
            r = r.detach().double().tolist()
        r = tuple(float(x) for x in r)
        if len(r) != 4 or not all(math.isfinite(x) for x in r) or r[0] == 0 or r[1] == 0:
            raise ValueError(f"{op}: pinhole[{i}] must be four finite numbers (fx, fy, cx, cy) with fx, fy non-zero, got {r}")
        out.append(r)
    return out


def _prior_list(op: str, prior, like):
    seq = [prior] if torch.is_tensor(prior) else list(prior)
    if len(seq) != len(like):
        raise ValueError(f"{op}: {len(like)} depth maps but {len(seq)} prior")
    for i, t in enumerate(seq):
        if not torch.is_tensor(t) or t.dim() != 3 or t.shape[0] != 3 or tuple(t.shape[-2:]) != tuple(like[0].shape[-2:]):
            raise ValueError(f"{op}: prior[{i}] must be (3,H,W) with the maps' H, W"
                             + (f", got {tuple(t.shape)}" if torch.is_tensor(t) else f", got {type(t).__name__}"))
    return seq


def _scalars(op: str, min_weight, max_jump):
    min_weight, max_jump = float(min_weight), float(max_jump)
    if not (min_weight > 0 and math.isfinite(min_weight)):
        raise ValueError(f"{op}: min_weight must be a positive number, got {min_weight}")
    if not max_jump >= 0:
        raise ValueError(f"{op}: max_jump must be a non-negative number or inf, got {max_jump}")
    return min_weight, max_jump


def _arguments(op: str, depth, weights, prior, pinhole, mask, mode, min_weight, max_jump):
    """The checks the HIP path and the PyTorch statement share: (depths, weights, priors, masks, pinholes, min_weight, max_jump)."""
    if mode not in MODES:
        raise ValueError(f"{op}: mode must be 'cos' or 'l1', got {mode!r}")
    Ds = _map_list(op, "depth", depth)
    Ds = _map_list(op, "depth", Ds, like=Ds)
    As = _map_list(op, "weights", weights, like=Ds)
    ps = _prior_list(op, prior, Ds)
    ms = [None] * len(Ds) if mask is None else _map_list(op, "mask", mask, like=Ds, optional=True)
    for i, m in enumerate(ms):
        if m is not None and m.dtype == torch.bool:
            raise TypeError(f"{op}: mask[{i}] is a bool tensor; the mask is a float pixel weight: pass mask.float()")
    return (Ds, As, ps, ms, _pinholes(op, pinhole, len(Ds))) + _scalars(op, min_weight, max_jump)


# ------------------------------------------------------------------------------------------------------------------ PyTorch
def _geometry_torch(D, A, pins, min_weight, max_jump):
    """``D``, ``A`` (V,H,W) in one dtype, ``pins`` (V,4) float64 on their device: (N (V,H,W,3) float64, q, geometric) of every
    pixel as a centre.  A neighbour outside the image is not solid; a pixel that is not solid has z = 1 and no gradient."""
    dt, dev = D.dtype, D.device
    V, H, W = D.shape
    solid = (A >= torch.as_tensor(min_weight, dtype=dt, device=dev)) & (D > 0)
    one = torch.ones((), dtype=dt, device=dev)
    z = (torch.where(solid, D, one) / torch.where(solid, A, one)).double()
    zp = torch.nn.functional.pad(z, (1, 1, 1, 1), value=1.0)
    sp = torch.nn.functional.pad(solid, (1, 1, 1, 1), value=False)
    c, l, r, up, dn = zp[:, 1:-1, 1:-1], zp[:, 1:-1, :-2], zp[:, 1:-1, 2:], zp[:, :-2, 1:-1], zp[:, 2:, 1:-1]
    all5 = sp[:, 1:-1, 1:-1] & sp[:, 1:-1, :-2] & sp[:, 1:-1, 2:] & sp[:, :-2, 1:-1] & sp[:, 2:, 1:-1]
    fx, fy, cx, cy = (pins[:, k, None, None] for k in range(4))
    u = torch.arange(W, dtype=torch.float64, device=dev)[None, None, :]
    v = torch.arange(H, dtype=torch.float64, device=dev)[None, :, None]
    rxl, rxc, rxr = ((u - 1) - cx) / fx, (u - cx) / fx, ((u + 1) - cx) / fx
    ryu, ryc, ryd = ((v - 1) - cy) / fy, (v - cy) / fy, ((v + 1) - cy) / fy
    dx = torch.stack([r * rxr - l * rxl, r * ryc - l * ryc, r - l], -1)
    dy = torch.stack([dn * rxc - up * rxc, dn * ryd - up * ryu, dn - up], -1)
    N = torch.linalg.cross(dy, dx, dim=-1)
    q = (N * N).sum(-1)
    with torch.no_grad():                                      # decisions
        lim = torch.as_tensor(max_jump, dtype=dt, device=dev).double() * c
        geometric = all5 & ((r - l).abs() <= lim) & ((dn - up).abs() <= lim) & (q > 0) & torch.isfinite(q)
    return N, q, geometric


def _stack(ts, H, W, dt, dev):
    return torch.stack([t.reshape(H, W) for t in ts]).to(device=dev, dtype=dt)


def normal_prior_loss_torch(depth, weights, prior, pinhole, mask=None, *, mode="cos", min_weight=0.5, max_jump=math.inf):
    """The function of the module docstring in plain PyTorch, on the device and in the dtype of ``depth``; autograd gives its
    backward.  Arguments and result as ``normal_prior_loss``: ``(loss (V,), count (V,))`` in the dtype of ``depth``.  ``z`` is formed
    in that dtype, everything after it in float64, as the kernel does: in float64 this is the reference, in float32 the comparison
    path."""
    op = "normal_prior_loss_torch"
    Ds, As, ps, ms, pins, min_weight, max_jump = _arguments(op, depth, weights, prior, pinhole, mask, mode, min_weight, max_jump)
    H, W = Ds[0].shape[-2:]
    dt, dev = Ds[0].dtype, Ds[0].device
    D, A = _stack(Ds, H, W, dt, dev), _stack(As, H, W, dt, dev)
    p = torch.stack(list(ps)).to(device=dev, dtype=dt).double().permute(0, 2, 3, 1)          # (V,H,W,3)
    m = torch.stack([torch.ones(H, W, dtype=dt, device=dev) if t is None else t.reshape(H, W).to(device=dev, dtype=dt) for t in ms])
    N, q, geometric = _geometry_torch(D, A, torch.tensor(pins, dtype=torch.float64, device=dev), min_weight, max_jump)
    pp = (p * p).sum(-1)
    valid = geometric & (m > 0) & torch.isfinite(pp) & (pp > PRIOR_MIN_SQ)
    away = torch.tensor((0.0, 0.0, -1.0), dtype=torch.float64, device=dev)
    Nv, pv = torch.where(valid[..., None], N, away), torch.where(valid[..., None], p, away)   # an invalid pixel: constants, w = 0
    n = Nv / torch.sqrt((Nv * Nv).sum(-1, keepdim=True))
    ph = pv / torch.sqrt((pv * pv).sum(-1, keepdim=True))
    lpix = (n - ph).abs().sum(-1) if mode == "l1" else 1.0 - (n * ph).sum(-1)
    w = torch.where(valid, m, torch.zeros((), dtype=dt, device=dev)).double()
    cnt = w.sum((1, 2))
    some = cnt > 0
    inv = torch.where(some, 1.0 / torch.where(some, cnt, torch.ones_like(cnt)), torch.zeros_like(cnt))
    loss = (w * lpix).sum((1, 2)) * inv
    return loss.to(dt), cnt.detach().to(dt)


def depth_to_normal_torch(depth, weights, pinhole, *, min_weight=0.5, max_jump=math.inf):
    """``(normal (3,H,W), valid (H,W) bool)`` of one view in plain PyTorch: ``n`` in the dtype of ``depth`` where the pixel is
    ``geometric`` (module docstring; no prior, no mask), zeros elsewhere."""
    op = "depth_to_normal_torch"
    Ds = _map_list(op, "depth", depth)
    As = _map_list(op, "weights", weights, like=Ds)
    if len(Ds) != 1:
        raise ValueError(f"{op}: one view per call")
    min_weight, max_jump = _scalars(op, min_weight, max_jump)
    pins = _pinholes(op, pinhole, 1)
    H, W = Ds[0].shape[-2:]
    dt, dev = Ds[0].dtype, Ds[0].device
    N, q, geometric = _geometry_torch(_stack(Ds, H, W, dt, dev), _stack(As, H, W, dt, dev), torch.tensor(pins, dtype=torch.float64, device=dev),
                                      min_weight, max_jump)
    n = N / torch.sqrt(torch.where(geometric, q, torch.ones_like(q)))[..., None]
    n = torch.where(geometric[..., None], n, torch.zeros_like(n))
    return n[0].permute(2, 0, 1).to(dt).contiguous(), geometric[0]


# ------------------------------------------------------------------------------------------------------------------ HIP
def _pinhole_field(pins):
    field = ((C.c_double * 4) * L.MAX_POSE_ROWS)()
    for i, r in enumerate(pins):
        field[i][:] = r
    return field


class _NormalPrior(torch.autograd.Function):
    """``maps``: V depth maps, V weights maps, V priors, V masks (any of the masks None), as separate tensors: nothing is stacked."""

    @staticmethod
    def forward(ctx, pins, mode, min_weight, max_jump, V, *maps):
        depths, weights, priors, masks = (list(maps[k * V:(k + 1) * V]) for k in range(4))
        dev, (H, W) = depths[0].device, depths[0].shape[-2:]
        loss = torch.empty(V, dtype=torch.float32, device=dev)
        count = torch.empty(V, dtype=torch.float32, device=dev)
        stats = torch.empty(V, L.NORMAL_PRIOR_STATS, dtype=torch.float64, device=dev)
        ws = L.workspace(L.load().bags_normal_prior_workspace_size(min(V, L.MAX_POSE_ROWS), H, W), dev)
        structs = []
        for b in range(0, V, L.MAX_POSE_ROWS):
            part = slice(b, b + L.MAX_POSE_ROWS)
            n = len(depths[part])
            args = L.BagsNormalPrior(mode, H, W, min_weight, max_jump, n, _pinhole_field(pins[part]), _ptr_field(depths[part]),
                                     _ptr_field(weights[part]), _ptr_field(priors[part]), _ptr_field(masks[part]))
            L.call("bags_normal_prior_forward", dev, C.byref(args), L.ptr(ws), ws.numel(), loss[part].data_ptr(), count[part].data_ptr(),
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
        g_depth = [torch.empty_like(t) if need[5 + i] else None for i, t in enumerate(maps[:V])]
        g_weights = [torch.empty_like(t) if need[5 + V + i] else None for i, t in enumerate(maps[V:2 * V])]
        for k, args in enumerate(ctx.structs):
            part = slice(k * L.MAX_POSE_ROWS, (k + 1) * L.MAX_POSE_ROWS)
            L.call("bags_normal_prior_backward", dev, C.byref(args), stats[part].data_ptr(), g[part].data_ptr(),
                   L.ptr_table(g_depth[part]), L.ptr_table(g_weights[part]))
        return (None, None, None, None, None, *g_depth, *g_weights, *([None] * (2 * V)))


_HOST = ": bags_raster.normal_prior_loss_torch is the same function in PyTorch on any device and dtype"


def normal_prior_loss(depth, weights, prior, pinhole, mask=None, *, mode="cos", min_weight=0.5, max_jump=math.inf):
    """The normal prior of the module docstring on an AMD GPU: ``(loss (V,), count (V,))``, ``count[v] = cnt`` of view v.

    ``depth`` and ``weights`` are the operator's maps ``(1,H,W)`` of one view, or sequences of V of them -- the ``"depth"`` and
    ``"weights"`` entries of what ``render_views`` returns go in as they are, nothing is stacked or copied; ``prior`` is ``(3,H,W)``
    per view, ``mask`` ``(H,W)`` or ``(1,H,W)`` (``mask=None``, or a None entry: every pixel weighs 1).  float32, contiguous tensors
    on one device; a bool mask raises (pass ``mask.float()``).  ``pinhole`` is one ``(fx, fy, cx, cy)`` for every view or V of them,
    as host floats or a CPU tensor (``pinhole_of``); a GPU tensor raises, because reading it would synchronise.  Two HIP launches
    forward and one backward per 16 views.  Differentiable in ``depth`` and ``weights``; there is no gradient to the intrinsics, and
    ``count`` is not differentiable.  The backward re-reads the maps: writing one of them in place between forward and backward
    raises."""
    Ds, As, ps, ms, pins, min_weight, max_jump = _arguments(_OP, depth, weights, prior, pinhole, mask, mode, min_weight, max_jump)
    L.require(_OP, "depth[0]", Ds[0], gpu=True, f32=True, contiguous=True, host=_HOST)
    for name, ts in (("depth", Ds), ("weights", As), ("prior", ps), ("mask", ms)):
        for i, t in enumerate(ts):
            if t is not None:
                L.require(_OP, f"{name}[{i}]", t, gpu=True, f32=True, contiguous=True, on=Ds[0], host=_HOST)
    H, W = Ds[0].shape[-2:]
    if H * W >= 2 ** 31:
        raise ValueError(f"{_OP}: a map of {W}x{H} has 2^31 pixels or more")
    return _NormalPrior.apply(pins, MODES[mode], min_weight, max_jump, len(Ds), *Ds, *As, *ps, *ms)


def depth_to_normal(depth, weights, pinhole, *, min_weight=0.5, max_jump=math.inf):
    """``(normal (3,H,W) float32, valid (H,W) bool)`` of one view on an AMD GPU, in one HIP launch: ``n`` where the pixel is
    ``geometric`` (module docstring; no prior, no mask), zeros elsewhere.  Not differentiable: for viewers and logging."""
    op = "depth_to_normal"
    Ds = _map_list(op, "depth", depth)
    As = _map_list(op, "weights", weights, like=Ds)
    if len(Ds) != 1:
        raise ValueError(f"{op}: one view per call")
    min_weight, max_jump = _scalars(op, min_weight, max_jump)
    pin = _pinholes(op, pinhole, 1)[0]
    host = ": bags_raster.depth_to_normal_torch is the same function in PyTorch on any device and dtype"
    L.require(op, "depth", Ds[0], gpu=True, f32=True, contiguous=True, host=host)
    L.require(op, "weights", As[0], gpu=True, f32=True, contiguous=True, on=Ds[0], host=host)
    H, W = Ds[0].shape[-2:]
    if H * W >= 2 ** 31:
        raise ValueError(f"{op}: a map of {W}x{H} has 2^31 pixels or more")
    normal = torch.empty(3, H, W, dtype=torch.float32, device=Ds[0].device)
    valid = torch.empty(H, W, dtype=torch.uint8, device=Ds[0].device)
    L.call("bags_depth_to_normal", Ds[0].device, L.as_f32c(Ds[0]).data_ptr(), L.as_f32c(As[0]).data_ptr(), H, W, (C.c_double * 4)(*pin),
           min_weight, max_jump, normal.data_ptr(), valid.data_ptr())
    return normal, valid.view(torch.bool)
