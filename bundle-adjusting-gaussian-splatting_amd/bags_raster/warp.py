"""warp_loss -- the photometric reprojection (warping) loss on the rasterizer's ``depth`` and ``weights`` maps (csrc/warp.hip).

``correspondence_loss`` ties two views together where a matcher has supplied pixel matches; this module is the term pose-free and
sparse-view recipes use when there is no matcher (CF-3DGS, Nope-NeRF, the self-supervised-depth family; the per-pixel core of
PGSR-style multi-view consistency): a pixel of view i is un-projected with the rendered depth, carried into view j with the two
poses, the image of view j is sampled there, bilinearly, and the sampled colour is held to the colour of the pixel.  The gradient
reaches the depth (and through the operator the Gaussians) and BOTH view matrices, through the spatial gradient of the bilinear
sample.  Conventions are those of ``correspondence.py``, word for word: row vectors, ``x_cam = [X_w, 1] @ viewmatrix``; pixel centres
at whole numbers; pinholes ``(fx, fy, cx, cy)`` as host data (``pinhole_of``); ``z = D / A`` one division in the dtype of the maps,
everything after it float64; ``M = inv(Ai) @ Aj``, ``c = bj - bi @ M`` with the true inverse; ``solid``, ``x_i``, ``x_j`` and ``proj`` as
there.  Per ordered pair k: source maps ``D``, ``A`` (1,H,W), view matrices ``Vi``, ``Vj`` (4,4), ``color_src`` (C,H,W) = the colour each
source pixel is held to (usually the ground-truth image of view i), ``image_dst`` (C,Hd,Wd) = the image of view j that is sampled, an
optional confidence ``conf >= 0`` (H,W) (``None``: 1), optional target maps ``depth_dst``, ``weights_dst`` (1,Hd,Wd) for the occlusion
test.  ``C`` is 1 or 3; ``Hd, Wd`` is one size per call and may differ from ``H, W``.

    inside  = 0 <= proj.x <= Wd - 1 and 0 <= proj.y <= Hd - 1            (all four taps exist)
    x0 = floor(proj.x)  y0 = floor(proj.y)  ax = proj.x - x0  ay = proj.y - y0  x1 = min(x0 + 1, Wd - 1)  y1 = min(y0 + 1, Hd - 1)
    S_c     = (1-ay) ((1-ax) T_c[y0,x0] + ax T_c[y0,x1]) + ay ((1-ax) T_c[y1,x0] + ax T_c[y1,x1])      T = image_dst, in float64
    dS_c/dproj = ((1-ay)(T_c[y0,x1]-T_c[y0,x0]) + ay (T_c[y1,x1]-T_c[y1,x0]),  (1-ax)(T_c[y1,x0]-T_c[y0,x0]) + ax (T_c[y1,x1]-T_c[y0,x1]))
    visible = no target maps given, or at the nearest target pixel (floor(proj + 0.5)), with z_t = D_t / A_t (one division in the
              dtype of the maps):  A_t >= min_weight and D_t > 0 and |x_j.z - z_t| <= occlusion * z_t
    valid   = solid and det(Ai) usable and x_j.z >= min_depth and conf > 0 and inside and visible and every S_c, color_src_c finite
    r_c     = S_c - color_src_c ;  rho = (1/C) sum_c (sqrt(r_c^2 + eps^2) - eps)          (Charbonnier: smooth, L1 as eps -> 0)
    w = conf on valid pixels ;  cnt = sum w ;  L_k = sum w rho / cnt
    dL/dproj = s_k (w / cnt) (1/C) sum_c r_c / sqrt(r_c^2 + eps^2) * dS_c/dproj        (s_k the cotangent)

From ``dL/dproj`` on, the backward is the correspondence loss's: ``dL/dD`` and ``dL/dA`` per pixel, ``dL/dVi`` and ``dL/dVj`` with
exact-zero fourth columns.  Validity is a decision and is not differentiated through, the bilinear cell and the occlusion test
included; invalid pixels get exact-zero gradients; ``cnt <= 0`` or a singular ``Ai`` gives loss 0 and zero gradients, never NaN.  There
is NO gradient to ``image_dst``, ``color_src``, the target maps, ``conf`` or the intrinsics: a gradient to the sampled image is a
scatter, and this library writes no gradient with atomics (out of scope) -- pass constant (detached) images.  ``depth`` is read as the
pinhole view depth: with non-zero ``shift_factors`` the operator's maps carry the D2 term, which this loss ignores.

``warp_loss_torch`` is the function in plain PyTorch on any device and dtype.  ``warp_loss`` is the HIP path: the pairs of a step in
two launches forward and two backward per 16 pairs, sums without atomics, so it repeats bit for bit and a pair's result does not
depend on its neighbours.  ``warp_image`` / ``warp_image_torch`` give the warped image and its validity mask of one pair: the
counterpart of ``reproject_pixels``, for viewers and masks.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib as L
from .correspondence import _geometry_torch, _project, _require_all, _scalars, _view_list
from .depth_prior import _map_list, _ptr_field
from .normal_prior import _pinhole_field, _pinholes

_OP = "warp_loss"
EPS, OCCLUSION = 1e-3, 0.05


def _image_list(op: str, name: str, images, K: int, channels=None, size=None, optional=False):
    """``images`` as a list of K per-pair ``(C,h,w)`` tensors with one C (1 or 3, or ``channels``) and one size (``size``, where
    given).  ``optional``: None entries stay."""
    seq = [images] if torch.is_tensor(images) else list(images)
    if len(seq) != K:
        raise ValueError(f"{op}: {K} depth maps but {len(seq)} {name}")
    first = None
    for i, t in enumerate(seq):
        if t is None and optional:
            continue
        if not torch.is_tensor(t) or t.dim() != 3 or t.numel() < 1:
            raise ValueError(f"{op}: {name}[{i}] must be a non-empty (C,H,W) tensor"
                             + (f", got {tuple(t.shape)}" if torch.is_tensor(t) else f", got {type(t).__name__}"))
        if channels is None and t.shape[0] not in (1, 3):
            raise ValueError(f"{op}: {name}[{i}] has {t.shape[0]} channels, must be 1 or 3")
        if channels is not None and t.shape[0] != channels:
            raise ValueError(f"{op}: {name}[{i}] has {t.shape[0]} channels, expected {channels}")
        if size is not None and tuple(t.shape[-2:]) != tuple(size):
            raise ValueError(f"{op}: {name}[{i}] is {tuple(t.shape)}, expected (C,{size[0]},{size[1]})")
        first = t if first is None else first
        if tuple(t.shape) != tuple(first.shape):
            raise ValueError(f"{op}: {name}[{i}] is {tuple(t.shape)}, {name}[0] is {tuple(first.shape)}: one size per call")
    return seq


def _warp_scalars(op: str, eps, occlusion, min_weight, min_depth):
    min_weight, min_depth, _ = _scalars(op, min_weight, min_depth)
    eps, occlusion = float(eps), float(occlusion)
    if not (eps > 0 and math.isfinite(eps)):
        raise ValueError(f"{op}: eps must be a positive number, got {eps}")
    if not (occlusion > 0 and math.isfinite(occlusion)):
        raise ValueError(f"{op}: occlusion must be a positive number, got {occlusion}")
    return eps, occlusion, min_weight, min_depth


def _target_maps(op: str, depth_dst, weights_dst, K: int, size):
    """K (depth_dst, weights_dst) entries, each (1,Hd,Wd) / (Hd,Wd) tensors or both None."""
    if (depth_dst is None) != (weights_dst is None):
        raise ValueError(f"{op}: depth_dst and weights_dst must be given together or not at all")
    if depth_dst is None:
        return [None] * K, [None] * K
    out = []
    for name, maps in (("depth_dst", depth_dst), ("weights_dst", weights_dst)):
        seq = [maps] if torch.is_tensor(maps) else list(maps)
        if len(seq) != K:
            raise ValueError(f"{op}: {K} depth maps but {len(seq)} {name}")
        if any(t is not None for t in seq):
            seq = _map_list(op, name, seq, optional=True)
        for i, t in enumerate(seq):
            if t is not None and tuple(t.shape[-2:]) != tuple(size):
                raise ValueError(f"{op}: {name}[{i}] is {tuple(t.shape)}, image_dst is (C,{size[0]},{size[1]}): the target maps have the target image's size")
        out.append(seq)
    for i, (d, w) in enumerate(zip(*out)):
        if (d is None) != (w is None):
            raise ValueError(f"{op}: depth_dst[{i}] and weights_dst[{i}] must be given together or not at all")
    return out[0], out[1]


def _arguments(op: str, depth, weights, view_src, view_dst, color_src, image_dst, pinhole_src, pinhole_dst, conf, depth_dst, weights_dst, eps,
               occlusion, min_weight, min_depth):
    """The checks the HIP path and the PyTorch statement share."""
    Ds = _map_list(op, "depth", depth)
    Ds = _map_list(op, "depth", Ds, like=Ds)
    As = _map_list(op, "weights", weights, like=Ds)
    K = len(Ds)
    Vs, Vd = _view_list(op, "view_src", view_src, K), _view_list(op, "view_dst", view_dst, K)
    if color_src is None:                                      # warp_image: nothing is held to a colour
        cols = [None] * K
        imgs = _image_list(op, "image_dst", image_dst, K)
    else:
        cols = _image_list(op, "color_src", color_src, K, size=Ds[0].shape[-2:])
        imgs = _image_list(op, "image_dst", image_dst, K, channels=cols[0].shape[0])
    cs = [None] * K if conf is None else _map_list(op, "conf", conf, like=Ds, optional=True)
    for i, t in enumerate(cs):
        if t is not None and t.dtype == torch.bool:
            raise TypeError(f"{op}: conf[{i}] is a bool tensor; the confidence is a float pixel weight: pass conf.float()")
    Dt, At = _target_maps(op, depth_dst, weights_dst, K, imgs[0].shape[-2:])
    return (Ds, As, Vs, Vd, cols, imgs, cs, Dt, At, _pinholes(op, pinhole_src, K), _pinholes(op, pinhole_dst, K)) \
        + _warp_scalars(op, eps, occlusion, min_weight, min_depth)


# ------------------------------------------------------------------------------------------------------------------ PyTorch
def _sample_torch(xj, geometric, pin_j, T, Dt, At, occlusion, min_weight):
    """The bilinear sample of one pair.  ``xj`` (H,W,3) float64 and ``geometric`` (H,W) of ``_geometry_torch``, ``T`` (C,Hd,Wd) and the
    target maps ``Dt``, ``At`` (Hd,Wd) or None in the dtype of the maps: (S (C,H,W) float64, differentiable in ``xj`` through ax and ay,
    with zero taps where not ok; ok (H,W) bool = geometric, inside, visible and every S_c finite)."""
    Hd, Wd = T.shape[-2:]
    proj = _project(xj, pin_j)
    with torch.no_grad():                                      # decisions: inside, the cell, the nearest pixel, visible
        x, y = proj[..., 0], proj[..., 1]
        inside = geometric & (x >= 0) & (x <= Wd - 1) & (y >= 0) & (y <= Hd - 1)
        xs, ys = torch.where(inside, x, torch.zeros_like(x)), torch.where(inside, y, torch.zeros_like(y))
        fx0, fy0 = torch.floor(xs), torch.floor(ys)
        x0, y0 = fx0.long(), fy0.long()
        x1, y1 = (x0 + 1).clamp(max=Wd - 1), (y0 + 1).clamp(max=Hd - 1)
        ok = inside
        if Dt is not None:
            nx, ny = torch.floor(xs + 0.5).long(), torch.floor(ys + 0.5).long()
            dt, at = Dt[ny, nx], At[ny, nx]
            solid_t = (at >= torch.as_tensor(min_weight, dtype=at.dtype, device=at.device)) & (dt > 0)
            one = torch.ones((), dtype=dt.dtype, device=dt.device)
            zt = (torch.where(solid_t, dt, one) / torch.where(solid_t, at, one)).double()
            ok = ok & solid_t & ((xj[..., 2] - zt).abs() <= occlusion * zt)
        T64 = T.double()
        taps = [T64[:, y0, x0], T64[:, y0, x1], T64[:, y1, x0], T64[:, y1, x1]]          # (C,H,W) each
        ax, ay = xs - fx0, ys - fy0
        raw = (1.0 - ay) * ((1.0 - ax) * taps[0] + ax * taps[1]) + ay * ((1.0 - ax) * taps[2] + ax * taps[3])
        ok = ok & torch.isfinite(raw).all(0)
        taps = [torch.where(ok, t, torch.zeros_like(t)) for t in taps]
    zero = torch.zeros_like(proj[..., 0])
    ax = torch.where(ok, proj[..., 0], zero) - torch.where(ok, fx0, zero)
    ay = torch.where(ok, proj[..., 1], zero) - torch.where(ok, fy0, zero)
    S = (1.0 - ay) * ((1.0 - ax) * taps[0] + ax * taps[1]) + ay * ((1.0 - ax) * taps[2] + ax * taps[3])
    return S, ok


def _pair_maps(Ds, As, k, H, W):
    dt, dev = Ds[0].dtype, Ds[0].device
    return Ds[k].reshape(H, W), As[k].reshape(H, W).to(device=dev, dtype=dt)


def _target_of(imgs, Dt, At, k, dt, dev):
    T = imgs[k].to(device=dev, dtype=dt)
    Hd, Wd = T.shape[-2:]
    if Dt[k] is None:
        return T, None, None
    return T, Dt[k].reshape(Hd, Wd).to(device=dev, dtype=dt), At[k].reshape(Hd, Wd).to(device=dev, dtype=dt)


def warp_loss_torch(depth, weights, view_src, view_dst, color_src, image_dst, pinhole_src, pinhole_dst, conf=None, depth_dst=None,
                    weights_dst=None, *, eps=EPS, occlusion=OCCLUSION, min_weight=0.5, min_depth=0.01):
    """The function of the module docstring in plain PyTorch, on the device and in the dtype of ``depth``; autograd gives its
    backward.  Arguments and result as ``warp_loss``: ``(loss (K,), count (K,))`` in the dtype of ``depth``.  ``z`` and ``z_t`` are formed
    in that dtype, everything after them in float64, as the kernel does: in float64 this is the reference, in float32 the comparison
    path."""
    op = "warp_loss_torch"
    Ds, As, Vs, Vd, cols, imgs, cs, Dt, At, pin_i, pin_j, eps, occlusion, min_weight, min_depth = _arguments(
        op, depth, weights, view_src, view_dst, color_src, image_dst, pinhole_src, pinhole_dst, conf, depth_dst, weights_dst, eps, occlusion,
        min_weight, min_depth)
    H, W = Ds[0].shape[-2:]
    dt, dev = Ds[0].dtype, Ds[0].device
    n_ch = cols[0].shape[0]
    losses, counts = [], []
    for k in range(len(Ds)):
        D, A = _pair_maps(Ds, As, k, H, W)
        _, xj, geometric, _, _ = _geometry_torch(D, A, Vs[k], Vd[k], pin_i[k], min_weight, min_depth)
        S, ok = _sample_torch(xj, geometric, pin_j[k], *_target_of(imgs, Dt, At, k, dt, dev), occlusion, min_weight)
        col = cols[k].to(device=dev, dtype=dt)
        cf = torch.ones(H, W, dtype=dt, device=dev) if cs[k] is None else cs[k].reshape(H, W).to(device=dev, dtype=dt)
        valid = ok & (cf > 0) & torch.isfinite(col).all(0)
        r = S - torch.where(valid, col, torch.zeros((), dtype=dt, device=dev)).double()
        r = torch.where(valid, r, torch.zeros_like(r))
        rho = sum(torch.sqrt(r[c] * r[c] + eps * eps) - eps for c in range(n_ch)) / n_ch
        w = torch.where(valid, cf, torch.zeros((), dtype=dt, device=dev)).double()
        cnt = w.sum()
        some = cnt > 0
        inv = torch.where(some, 1.0 / torch.where(some, cnt, torch.ones_like(cnt)), torch.zeros_like(cnt))
        losses.append((w * rho).sum() * inv)
        counts.append(cnt.detach())
    return torch.stack(losses).to(dt), torch.stack(counts).to(dt)


def _one_pair(op: str, depth, weights, view_src, view_dst, image_dst, pinhole_src, pinhole_dst, depth_dst, weights_dst, occlusion, min_weight,
              min_depth):
    Ds, As, Vs, Vd, _, imgs, _, Dt, At, pin_i, pin_j, _, occlusion, min_weight, min_depth = _arguments(
        op, depth, weights, view_src, view_dst, None, image_dst, pinhole_src, pinhole_dst, None, depth_dst, weights_dst, EPS, occlusion, min_weight,
        min_depth)
    if len(Ds) != 1:
        raise ValueError(f"{op}: one pair per call")
    return Ds, As, Vs[0], Vd[0], imgs, Dt, At, pin_i[0], pin_j[0], occlusion, min_weight, min_depth


def warp_image_torch(depth, weights, view_src, view_dst, image_dst, pinhole_src, pinhole_dst, depth_dst=None, weights_dst=None, *,
                     occlusion=OCCLUSION, min_weight=0.5, min_depth=0.01):
    """``(warped (C,H,W), valid (H,W) bool)`` of one pair in plain PyTorch: ``S_c`` of the module docstring in the dtype of ``depth``
    where the pixel is solid, ``x_j.z >= min_depth``, inside, visible and every ``S_c`` finite; zeros elsewhere.  On the valid pixels it
    is ``grid_sample(image_dst, bilinear, align_corners=True)`` at ``proj``: both put pixel centres at whole numbers."""
    op = "warp_image_torch"
    Ds, As, Vi, Vj, imgs, Dt, At, pin_i, pin_j, occlusion, min_weight, min_depth = _one_pair(
        op, depth, weights, view_src, view_dst, image_dst, pinhole_src, pinhole_dst, depth_dst, weights_dst, occlusion, min_weight, min_depth)
    H, W = Ds[0].shape[-2:]
    dt, dev = Ds[0].dtype, Ds[0].device
    with torch.no_grad():
        D, A = _pair_maps(Ds, As, 0, H, W)
        _, xj, geometric, _, _ = _geometry_torch(D, A, Vi, Vj, pin_i, min_weight, min_depth)
        S, ok = _sample_torch(xj, geometric, pin_j, *_target_of(imgs, Dt, At, 0, dt, dev), occlusion, min_weight)
    return torch.where(ok, S, torch.zeros_like(S)).to(dt).contiguous(), ok


# ------------------------------------------------------------------------------------------------------------------ HIP
_GROUPS = 9                                                    # tensor groups of a call: the first four take gradients


def _struct(H, W, cfg, n_ch, size_dst, pin_i, pin_j, groups):
    eps, occlusion, min_weight, min_depth = cfg
    depths, weights, vsrc, vdst, cols, imgs, confs, ddst, wdst = groups
    return L.BagsWarp(H, W, len(depths), min_weight, min_depth, n_ch, size_dst[0], size_dst[1], 0, eps, occlusion, _pinhole_field(pin_i),
                      _pinhole_field(pin_j), _ptr_field(depths), _ptr_field(weights), _ptr_field(confs), _ptr_field(vsrc), _ptr_field(vdst),
                      _ptr_field(cols), _ptr_field(imgs), _ptr_field(ddst), _ptr_field(wdst))


class _Warp(torch.autograd.Function):
    """``tensors``: K depth maps, K weights maps, K source and K target view matrices, K colours, K target images, K confidences, K
    target depth and K target weights maps (any of the last three groups' entries None), as separate tensors: nothing is stacked."""

    @staticmethod
    def forward(ctx, pin_i, pin_j, cfg, K, *tensors):
        groups = [list(tensors[k * K:(k + 1) * K]) for k in range(_GROUPS)]
        depths, cols, imgs = groups[0], groups[4], groups[5]
        dev, (H, W) = depths[0].device, depths[0].shape[-2:]
        loss = torch.empty(K, dtype=torch.float32, device=dev)
        count = torch.empty(K, dtype=torch.float32, device=dev)
        stats = torch.empty(K, L.CORRESPONDENCE_STATS, dtype=torch.float64, device=dev)
        ws = L.workspace(L.load().bags_warp_workspace_size(min(K, L.MAX_POSE_ROWS), H, W), dev)
        structs = []
        for b in range(0, K, L.MAX_POSE_ROWS):
            part = slice(b, b + L.MAX_POSE_ROWS)
            args = _struct(H, W, cfg, cols[0].shape[0], imgs[0].shape[-2:], pin_i[part], pin_j[part], [g[part] for g in groups])
            L.call("bags_warp_forward", dev, C.byref(args), L.ptr(ws), ws.numel(), loss[part].data_ptr(), count[part].data_ptr(),
                   stats[part].data_ptr())
            structs.append(args)
        ctx.mark_non_differentiable(count)
        if any(ctx.needs_input_grad):                          # nothing is kept under no_grad or for constant inputs
            ctx.save_for_backward(stats, *tensors)             # versions are checked at backward: the adjoint re-reads the maps and images
            ctx.structs, ctx.K = structs, K
        return loss, count

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss, _g_count):
        stats, *tensors = ctx.saved_tensors                    # raises if a tensor was written in place since the forward
        K, need = ctx.K, ctx.needs_input_grad
        dev = stats.device
        g = L.as_f32c(g_loss)
        grads = [[torch.empty_like(t) if need[4 + j * K + i] else None for i, t in enumerate(tensors[j * K:(j + 1) * K])] for j in range(4)]
        H, W = tensors[0].shape[-2:]
        views = any(t is not None for t in grads[2] + grads[3])
        ws = L.workspace(L.load().bags_warp_workspace_size(min(K, L.MAX_POSE_ROWS), H, W) if views else 0, dev)
        for k, args in enumerate(ctx.structs):
            part = slice(k * L.MAX_POSE_ROWS, (k + 1) * L.MAX_POSE_ROWS)
            L.call("bags_warp_backward", dev, C.byref(args), stats[part].data_ptr(), g[part].data_ptr(), L.ptr(ws), ws.numel(),
                   *(L.ptr_table(gs[part]) for gs in grads))
        return (None,) * 4 + tuple(grads[0] + grads[1] + grads[2] + grads[3]) + (None,) * ((_GROUPS - 4) * K)


_HOST = ": bags_raster.warp_loss_torch is the same function in PyTorch on any device and dtype"


def _require_sizes(op, imgs):
    Hd, Wd = imgs[0].shape[-2:]
    if Hd * Wd >= 2 ** 31:
        raise ValueError(f"{op}: a target image of {Wd}x{Hd} has 2^31 pixels or more")


def warp_loss(depth, weights, view_src, view_dst, color_src, image_dst, pinhole_src, pinhole_dst, conf=None, depth_dst=None, weights_dst=None,
              *, eps=EPS, occlusion=OCCLUSION, min_weight=0.5, min_depth=0.01):
    """The warping loss of the module docstring on an AMD GPU: ``(loss (K,), count (K,))``, ``count[k] = cnt`` of pair k.

    One ordered pair, or sequences of K of them; nothing is stacked or copied.  ``depth`` and ``weights`` are the SOURCE view's maps
    ``(1,H,W)`` as ``render_views`` returns them, ``view_src`` / ``view_dst`` the ``(4,4)`` view matrices of the source and the target
    camera (GPU tensors, usually with gradients: the host never reads them), ``color_src`` ``(C,H,W)`` the colour the source pixels are
    held to, ``image_dst`` ``(C,Hd,Wd)`` the target view's image, ``C`` 1 or 3, ``conf`` ``(H,W)`` or ``(1,H,W)`` (``conf=None``, or a None
    entry: every pixel weighs 1), ``depth_dst`` / ``weights_dst`` ``(1,Hd,Wd)`` the TARGET view's maps for the occlusion test (both None,
    or a None entry in both: no test for that pair).  A view used in several pairs is simply passed several times; autograd adds its
    gradients.  float32, contiguous tensors on one device; a bool ``conf`` raises (pass ``conf.float()``).  ``pinhole_src`` /
    ``pinhole_dst`` are one ``(fx, fy, cx, cy)`` for every pair or K of them, as host floats or a CPU tensor (``pinhole_of``); a GPU
    tensor raises, because reading it would synchronise.  ``eps`` is the Charbonnier width in units of colour, ``occlusion`` the
    relative depth tolerance of the occlusion test.  Two HIP launches forward and at most two backward per 16 pairs.  Differentiable
    in ``depth``, ``weights``, ``view_src`` and ``view_dst`` ONLY: there is no gradient to ``image_dst``, ``color_src``, the target maps,
    ``conf`` or the intrinsics (a gradient to the sampled image is a scatter; out of scope) -- pass constant images, e.g. the
    ground-truth images or detached renders; ``count`` is not differentiable.  ``depth`` is read as the pinhole view depth: with
    non-zero ``shift_factors`` the maps carry the D2 term, which this loss ignores.  The backward re-reads its inputs: writing one of
    them in place between forward and backward raises."""
    Ds, As, Vs, Vd, cols, imgs, cs, Dt, At, pin_i, pin_j, eps, occlusion, min_weight, min_depth = _arguments(
        _OP, depth, weights, view_src, view_dst, color_src, image_dst, pinhole_src, pinhole_dst, conf, depth_dst, weights_dst, eps, occlusion,
        min_weight, min_depth)
    cols, imgs, Dt, At = ([None if t is None else t.detach() for t in ts] for ts in (cols, imgs, Dt, At))
    _require_all(_OP, (("depth", Ds), ("weights", As), ("view_src", Vs), ("view_dst", Vd), ("color_src", cols), ("image_dst", imgs), ("conf", cs),
                       ("depth_dst", Dt), ("weights_dst", At)), _HOST)
    _require_sizes(_OP, imgs)
    return _Warp.apply(pin_i, pin_j, (eps, occlusion, min_weight, min_depth), len(Ds), *Ds, *As, *Vs, *Vd, *cols, *imgs, *cs, *Dt, *At)


def warp_image(depth, weights, view_src, view_dst, image_dst, pinhole_src, pinhole_dst, depth_dst=None, weights_dst=None, *, occlusion=OCCLUSION,
               min_weight=0.5, min_depth=0.01):
    """``(warped (C,H,W) float32, valid (H,W) bool)`` of one pair on an AMD GPU, in one HIP launch; the statement is
    ``warp_image_torch``.  Not differentiable: viewers, masks and the tests."""
    op = "warp_image"
    Ds, As, Vi, Vj, imgs, Dt, At, pin_i, pin_j, occlusion, min_weight, min_depth = _one_pair(
        op, depth, weights, view_src, view_dst, image_dst, pinhole_src, pinhole_dst, depth_dst, weights_dst, occlusion, min_weight, min_depth)
    host = ": bags_raster.warp_image_torch is the same function in PyTorch on any device and dtype"
    groups = [[t.detach()] for t in (Ds[0], As[0], Vi, Vj)] + [[None], [imgs[0].detach()], [None]] \
        + [[None if t[0] is None else t[0].detach()] for t in (Dt, At)]
    names = ("depth", "weights", "view_src", "view_dst", "color_src", "image_dst", "conf", "depth_dst", "weights_dst")
    _require_all(op, tuple(zip(names, groups)), host)
    _require_sizes(op, imgs)
    D, T = groups[0][0], groups[5][0]
    H, W = D.shape[-2:]
    out = torch.empty(T.shape[0], H, W, dtype=torch.float32, device=D.device)
    valid = torch.empty(H, W, dtype=torch.uint8, device=D.device)
    args = _struct(H, W, (EPS, occlusion, min_weight, min_depth), T.shape[0], T.shape[-2:], [pin_i], [pin_j], groups)
    L.call("bags_warp_image", D.device, C.byref(args), out.data_ptr(), valid.data_ptr())
    return out, valid.view(torch.bool)
