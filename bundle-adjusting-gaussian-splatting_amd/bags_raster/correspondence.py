"""correspondence_loss -- the multi-view correspondence loss on the rasterizer's ``depth`` and ``weights`` maps (csrc/correspondence.hip).

The operator returns ``depth = sum w_i z_i`` and ``weights = 1 - T_final``, differentiable with ``depth_weights_grad=True`` (DESIGN.md
decision D5).  ``depth_prior_loss`` and ``normal_prior_loss`` hold one view's geometry to a monocular prior; this module ties two
views together through the scene's geometry (SPARF, CoR-GS, the pose-free splatting family): a pixel of view i is un-projected with
the rendered depth, carried into view j with the two poses, and its distance to the pixel a matcher says it corresponds to is
penalised.  Conventions are the operator's: row vectors, ``x_cam = [X_w, 1] @ viewmatrix``; the view space of ``normal_prior.py``
(x right, y down, z forward); pinholes ``(fx, fy, cx, cy)`` in pixels (``pinhole_of``).  Per ordered pair k: source maps ``D``, ``A``
(1,H,W), the source and target view matrices ``Vi``, ``Vj`` (4,4), ``match`` (2,H,W) = the target pixel ``(x, y)`` source pixel
``(u, v)`` corresponds to, in pixels of the target image, an optional confidence ``conf >= 0`` (H,W) (``None``: 1), host pinholes.

    solid(u,v) = A >= min_weight and D > 0
    z          = D / A                      one division in the dtype of the maps; everything after it in float64
    Ai = Vi[:3,:3]  bi = Vi[3,:3]  Aj = Vj[:3,:3]  bj = Vj[3,:3]
    M  = inv(Ai) @ Aj ;  c = bj - bi @ M    the true 3x3 inverse adj(Ai) / det(Ai), not the transpose: a global alignment with a
                                            scale stays exact
    x_i = z * ((u - cx_i)/fx_i, (v - cy_i)/fy_i, 1) ;  x_j = x_i @ M + c
    valid(u,v) = solid and conf > 0 and match finite (both components) and x_j.z >= min_depth
    proj = (fx_j x_j.x / x_j.z + cx_j,  fy_j x_j.y / x_j.z + cy_j) ;  r = proj - match ;  e = |r|_2
    rho  = e^2 / 2                 where e <= delta
           delta (e - delta / 2)   elsewhere           (Huber on the Euclidean distance; delta = inf: half the squared distance;
                                                        d rho/dr = 0 at e = 0)
    w = conf on valid pixels ;  cnt = sum w ;  L_k = sum w rho / cnt

``cnt <= 0``, or ``det(Ai)`` zero or not finite: ``L_k = 0`` and every gradient an exact zero, never NaN.  Validity is a decision and
is not differentiated through; invalid pixels get exact-zero ``dL/dD`` and ``dL/dA``.  Gradients go to ``D``, ``A`` (and through them
to the Gaussians), ``Vi`` and ``Vj`` (both cameras); the fourth column of both matrix gradients is exactly zero.  ``match``, ``conf`` and
the pinholes are constant data: there is NO gradient to the intrinsics (out of scope).  ``depth`` is read as the pinhole view depth:
with non-zero ``shift_factors`` the operator's maps carry the D2 term, which this loss ignores.

``correspondence_loss_torch`` is the function in plain PyTorch on any device and dtype.  ``correspondence_loss`` is the HIP path: the
pairs of a step in two launches forward and two backward per 16 pairs, sums without atomics, so it repeats bit for bit and a pair's
result does not depend on its neighbours.  ``reproject_pixels`` / ``reproject_pixels_torch`` give ``proj`` and a covisibility mask of
one pair: the counterpart of ``depth_to_normal``, for masks, viewers and pseudo-matches.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib as L
from .depth_prior import _map_list, _ptr_field
from .normal_prior import _pinhole_field, _pinholes

_OP = "correspondence_loss"


def _view_list(op: str, name: str, views, K: int):
    seq = [views] if torch.is_tensor(views) else list(views)
    if len(seq) != K:
        raise ValueError(f"{op}: {K} depth maps but {len(seq)} {name}")
    for i, t in enumerate(seq):
        if not torch.is_tensor(t) or tuple(t.shape) != (4, 4):
            raise ValueError(f"{op}: {name}[{i}] must be a (4,4) view matrix"
                             + (f", got {tuple(t.shape)}" if torch.is_tensor(t) else f", got {type(t).__name__}"))
    return seq


def _match_list(op: str, match, like):
    seq = [match] if torch.is_tensor(match) else list(match)
    if len(seq) != len(like):
        raise ValueError(f"{op}: {len(like)} depth maps but {len(seq)} match")
    for i, t in enumerate(seq):
        if not torch.is_tensor(t) or t.dim() != 3 or t.shape[0] != 2 or tuple(t.shape[-2:]) != tuple(like[0].shape[-2:]):
            raise ValueError(f"{op}: match[{i}] must be (2,H,W) with the maps' H, W"
                             + (f", got {tuple(t.shape)}" if torch.is_tensor(t) else f", got {type(t).__name__}"))
    return seq


def _scalars(op: str, min_weight, min_depth, delta=1.0):
    min_weight, min_depth, delta = float(min_weight), float(min_depth), float(delta)
    if not (min_weight > 0 and math.isfinite(min_weight)):
        raise ValueError(f"{op}: min_weight must be a positive number, got {min_weight}")
    if not (min_depth > 0 and math.isfinite(min_depth)):
        raise ValueError(f"{op}: min_depth must be a positive number, got {min_depth}")
    if not delta > 0:
        raise ValueError(f"{op}: delta must be a positive number or inf, got {delta}")
    return min_weight, min_depth, delta


def _arguments(op: str, depth, weights, view_src, view_dst, match, pinhole_src, pinhole_dst, conf, delta, min_weight, min_depth):
    """The checks the HIP path and the PyTorch statement share."""
    Ds = _map_list(op, "depth", depth)
    Ds = _map_list(op, "depth", Ds, like=Ds)
    As = _map_list(op, "weights", weights, like=Ds)
    K = len(Ds)
    Vs, Vd = _view_list(op, "view_src", view_src, K), _view_list(op, "view_dst", view_dst, K)
    ms = _match_list(op, match, Ds)
    cs = [None] * K if conf is None else _map_list(op, "conf", conf, like=Ds, optional=True)
    for i, t in enumerate(cs):
        if t is not None and t.dtype == torch.bool:
            raise TypeError(f"{op}: conf[{i}] is a bool tensor; the confidence is a float pixel weight: pass conf.float()")
    return (Ds, As, Vs, Vd, ms, cs, _pinholes(op, pinhole_src, K), _pinholes(op, pinhole_dst, K)) + _scalars(op, min_weight, min_depth, delta)


# ------------------------------------------------------------------------------------------------------------------ PyTorch
def _transform_torch(Vi, Vj):
    """``Vi``, ``Vj`` (4,4) float64: (M (3,3), c (3,), ok) with ``ok`` a 0-dim bool, ``det(Ai)`` non-zero and finite; where it is not,
    M and c are those of an identity ``Vi`` and carry no gradient to ``Vi``.  The inverse is ``adj(Ai) / det(Ai)``, spelled."""
    with torch.no_grad():
        a = Vi[:3, :3]
        det0 = (a[0, 0] * (a[1, 1] * a[2, 2] - a[1, 2] * a[2, 1]) + a[0, 1] * (a[1, 2] * a[2, 0] - a[1, 0] * a[2, 2])) \
            + a[0, 2] * (a[1, 0] * a[2, 1] - a[1, 1] * a[2, 0])
        ok = (det0 != 0) & torch.isfinite(det0)
    Vi = torch.where(ok, Vi, torch.eye(4, dtype=Vi.dtype, device=Vi.device))
    A, bi, Aj, bj = Vi[:3, :3], Vi[3, :3], Vj[:3, :3], Vj[3, :3]
    cof = torch.stack([
        torch.stack([A[1, 1] * A[2, 2] - A[1, 2] * A[2, 1], A[1, 2] * A[2, 0] - A[1, 0] * A[2, 2], A[1, 0] * A[2, 1] - A[1, 1] * A[2, 0]]),
        torch.stack([A[0, 2] * A[2, 1] - A[0, 1] * A[2, 2], A[0, 0] * A[2, 2] - A[0, 2] * A[2, 0], A[0, 1] * A[2, 0] - A[0, 0] * A[2, 1]]),
        torch.stack([A[0, 1] * A[1, 2] - A[0, 2] * A[1, 1], A[0, 2] * A[1, 0] - A[0, 0] * A[1, 2], A[0, 0] * A[1, 1] - A[0, 1] * A[1, 0]])])
    det = (A[0] * cof[0]).sum()
    M = (cof.t() / det) @ Aj
    return M, bj - bi @ M, ok


def _geometry_torch(D, A, Vi, Vj, pin_i, min_weight, min_depth):
    """``D``, ``A`` (H,W) in one dtype: (x_i (H,W,3), x_j (H,W,3) float64, geometric (H,W) bool = solid, a usable ``det(Ai)`` and
    ``x_j.z >= min_depth``, M, c).  A pixel that is not solid has z = 1 and no gradient; where not geometric x_j is (0, 0, 1)."""
    dt, dev = D.dtype, D.device
    H, W = D.shape
    solid = (A >= torch.as_tensor(min_weight, dtype=dt, device=dev)) & (D > 0)
    one = torch.ones((), dtype=dt, device=dev)
    z = (torch.where(solid, D, one) / torch.where(solid, A, one)).double()
    M, c, ok = _transform_torch(Vi.to(dev).double(), Vj.to(dev).double())
    fx, fy, cx, cy = pin_i
    u = torch.arange(W, dtype=torch.float64, device=dev)[None, :].expand(H, W)
    v = torch.arange(H, dtype=torch.float64, device=dev)[:, None].expand(H, W)
    xi = torch.stack([z * ((u - cx) / fx), z * ((v - cy) / fy), z], -1)
    xj = xi @ M + c
    with torch.no_grad():                                      # decisions
        geometric = solid & ok & (xj[..., 2] >= min_depth)
    away = torch.tensor((0.0, 0.0, 1.0), dtype=torch.float64, device=dev)
    return xi, torch.where(geometric[..., None], xj, away), geometric, M, c


def _project(xj, pin_j):
    fx, fy, cx, cy = pin_j
    return torch.stack([fx * xj[..., 0] / xj[..., 2] + cx, fy * xj[..., 1] / xj[..., 2] + cy], -1)


def correspondence_loss_torch(depth, weights, view_src, view_dst, match, pinhole_src, pinhole_dst, conf=None, *, delta=1.0, min_weight=0.5,
                              min_depth=0.01):
    """The function of the module docstring in plain PyTorch, on the device and in the dtype of ``depth``; autograd gives its
    backward.  Arguments and result as ``correspondence_loss``: ``(loss (K,), count (K,))`` in the dtype of ``depth``.  ``z`` is formed
    in that dtype, everything after it in float64, as the kernel does: in float64 this is the reference, in float32 the comparison
    path."""
    op = "correspondence_loss_torch"
    Ds, As, Vs, Vd, ms, cs, pin_i, pin_j, min_weight, min_depth, delta = _arguments(op, depth, weights, view_src, view_dst, match, pinhole_src,
                                                                                    pinhole_dst, conf, delta, min_weight, min_depth)
    H, W = Ds[0].shape[-2:]
    dt, dev = Ds[0].dtype, Ds[0].device
    losses, counts = [], []
    for k in range(len(Ds)):
        _, xj, geometric, _, _ = _geometry_torch(Ds[k].reshape(H, W), As[k].reshape(H, W).to(device=dev, dtype=dt), Vs[k], Vd[k], pin_i[k],
                                                 min_weight, min_depth)
        m = ms[k].to(device=dev, dtype=dt).permute(1, 2, 0)                                  # (H,W,2)
        cf = torch.ones(H, W, dtype=dt, device=dev) if cs[k] is None else cs[k].reshape(H, W).to(device=dev, dtype=dt)
        valid = geometric & (cf > 0) & torch.isfinite(m).all(-1)
        r = _project(xj, pin_j[k]) - torch.where(valid[..., None], m, torch.zeros((), dtype=dt, device=dev)).double()
        r = torch.where(valid[..., None], r, torch.zeros_like(r))
        e2 = (r * r).sum(-1)
        rho = 0.5 * e2
        if math.isfinite(delta):
            with torch.no_grad():
                linear = ~(torch.sqrt(e2) <= delta)
            e = torch.sqrt(torch.where(linear, e2, torch.ones_like(e2)))                      # (no square root at e = 0)
            rho = torch.where(linear, delta * (e - 0.5 * delta), rho)
        w = torch.where(valid, cf, torch.zeros((), dtype=dt, device=dev)).double()
        cnt = w.sum()
        some = cnt > 0
        inv = torch.where(some, 1.0 / torch.where(some, cnt, torch.ones_like(cnt)), torch.zeros_like(cnt))
        losses.append((w * rho).sum() * inv)
        counts.append(cnt.detach())
    return torch.stack(losses).to(dt), torch.stack(counts).to(dt)


def _inside(proj, size_dst):
    H_dst, W_dst = size_dst
    return (proj[..., 0] >= -0.5) & (proj[..., 0] < W_dst - 0.5) & (proj[..., 1] >= -0.5) & (proj[..., 1] < H_dst - 0.5)


def _size(op: str, size_dst):
    H_dst, W_dst = (int(s) for s in size_dst)
    if H_dst < 1 or W_dst < 1:
        raise ValueError(f"{op}: size_dst must be (H, W) of a non-empty image, got {tuple(size_dst)}")
    return H_dst, W_dst


def _one_pair(op: str, depth, weights, view_src, view_dst, pinhole_src, pinhole_dst, size_dst, min_weight, min_depth):
    Ds = _map_list(op, "depth", depth)
    As = _map_list(op, "weights", weights, like=Ds)
    if len(Ds) != 1:
        raise ValueError(f"{op}: one pair per call")
    Vs, Vd = _view_list(op, "view_src", view_src, 1), _view_list(op, "view_dst", view_dst, 1)
    min_weight, min_depth, _ = _scalars(op, min_weight, min_depth)
    return Ds[0], As[0], Vs[0], Vd[0], _pinholes(op, pinhole_src, 1)[0], _pinholes(op, pinhole_dst, 1)[0], _size(op, size_dst), min_weight, min_depth


def reproject_pixels_torch(depth, weights, view_src, view_dst, pinhole_src, pinhole_dst, size_dst, *, min_weight=0.5, min_depth=0.01):
    """``(proj (2,H,W), valid (H,W) bool)`` of one pair in plain PyTorch: ``proj`` of the module docstring in the dtype of ``depth``
    where the pixel is solid and ``x_j.z >= min_depth`` (zeros elsewhere); ``valid`` where ``proj`` also lies inside the target image
    ``size_dst = (H, W)``: ``-0.5 <= x < W - 0.5`` and ``-0.5 <= y < H - 0.5`` (pixel centres at whole numbers, ``pinhole_of``)."""
    op = "reproject_pixels_torch"
    D, A, Vi, Vj, pin_i, pin_j, size_dst, min_weight, min_depth = _one_pair(op, depth, weights, view_src, view_dst, pinhole_src, pinhole_dst,
                                                                            size_dst, min_weight, min_depth)
    H, W = D.shape[-2:]
    with torch.no_grad():
        _, xj, geometric, _, _ = _geometry_torch(D.reshape(H, W), A.reshape(H, W).to(device=D.device, dtype=D.dtype), Vi, Vj, pin_i, min_weight,
                                                 min_depth)
        proj = _project(xj, pin_j)
        valid = geometric & _inside(proj, size_dst)
        proj = torch.where(geometric[..., None], proj, torch.zeros_like(proj))
    return proj.permute(2, 0, 1).to(D.dtype).contiguous(), valid


# ------------------------------------------------------------------------------------------------------------------ HIP
class _Correspondence(torch.autograd.Function):
    """``tensors``: K depth maps, K weights maps, K source and K target view matrices, K matches, K confidences (any of the
    confidences None), as separate tensors: nothing is stacked."""

    @staticmethod
    def forward(ctx, pin_i, pin_j, delta, min_weight, min_depth, K, *tensors):
        depths, weights, vsrc, vdst, matches, confs = (list(tensors[k * K:(k + 1) * K]) for k in range(6))
        dev, (H, W) = depths[0].device, depths[0].shape[-2:]
        loss = torch.empty(K, dtype=torch.float32, device=dev)
        count = torch.empty(K, dtype=torch.float32, device=dev)
        stats = torch.empty(K, L.CORRESPONDENCE_STATS, dtype=torch.float64, device=dev)
        ws = L.workspace(L.load().bags_correspondence_workspace_size(min(K, L.MAX_POSE_ROWS), H, W), dev)
        structs = []
        for b in range(0, K, L.MAX_POSE_ROWS):
            part = slice(b, b + L.MAX_POSE_ROWS)
            args = L.BagsCorrespondence(H, W, len(depths[part]), min_weight, min_depth, delta, _pinhole_field(pin_i[part]),
                                        _pinhole_field(pin_j[part]), _ptr_field(depths[part]), _ptr_field(weights[part]),
                                        _ptr_field(matches[part]), _ptr_field(confs[part]), _ptr_field(vsrc[part]), _ptr_field(vdst[part]))
            L.call("bags_correspondence_forward", dev, C.byref(args), L.ptr(ws), ws.numel(), loss[part].data_ptr(), count[part].data_ptr(),
                   stats[part].data_ptr())
            structs.append(args)
        ctx.mark_non_differentiable(count)
        if any(ctx.needs_input_grad):                          # nothing is kept under no_grad or for constant inputs
            ctx.save_for_backward(stats, *tensors)             # versions are checked at backward: the adjoint re-reads the maps
            ctx.structs, ctx.K = structs, K
        return loss, count

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss, _g_count):
        stats, *tensors = ctx.saved_tensors                    # raises if a tensor was written in place since the forward
        K, need = ctx.K, ctx.needs_input_grad
        dev = stats.device
        g = L.as_f32c(g_loss)
        grads = [[torch.empty_like(t) if need[6 + j * K + i] else None for i, t in enumerate(tensors[j * K:(j + 1) * K])] for j in range(4)]
        H, W = tensors[0].shape[-2:]
        views = any(t is not None for t in grads[2] + grads[3])
        ws = L.workspace(L.load().bags_correspondence_workspace_size(min(K, L.MAX_POSE_ROWS), H, W) if views else 0, dev)
        for k, args in enumerate(ctx.structs):
            part = slice(k * L.MAX_POSE_ROWS, (k + 1) * L.MAX_POSE_ROWS)
            L.call("bags_correspondence_backward", dev, C.byref(args), stats[part].data_ptr(), g[part].data_ptr(), L.ptr(ws), ws.numel(),
                   *(L.ptr_table(gs[part]) for gs in grads))
        return (None,) * 6 + tuple(grads[0] + grads[1] + grads[2] + grads[3]) + (None,) * (2 * K)


_HOST = ": bags_raster.correspondence_loss_torch is the same function in PyTorch on any device and dtype"


def _require_all(op, groups, host):
    first = groups[0][1][0]
    L.require(op, f"{groups[0][0]}[0]", first, gpu=True, f32=True, contiguous=True, host=host)
    for name, ts in groups:
        for i, t in enumerate(ts):
            if t is not None:
                L.require(op, f"{name}[{i}]", t, gpu=True, f32=True, contiguous=True, on=first, host=host)
    H, W = first.shape[-2:]
    if H * W >= 2 ** 31:
        raise ValueError(f"{op}: a map of {W}x{H} has 2^31 pixels or more")


def correspondence_loss(depth, weights, view_src, view_dst, match, pinhole_src, pinhole_dst, conf=None, *, delta=1.0, min_weight=0.5,
                        min_depth=0.01):
    """The correspondence loss of the module docstring on an AMD GPU: ``(loss (K,), count (K,))``, ``count[k] = cnt`` of pair k.

    One ordered pair, or sequences of K of them; nothing is stacked or copied.  ``depth`` and ``weights`` are the SOURCE view's maps
    ``(1,H,W)`` as ``render_views`` returns them, ``view_src`` / ``view_dst`` the ``(4,4)`` view matrices of the source and the target
    camera (GPU tensors, usually with gradients: the host never reads them), ``match`` ``(2,H,W)``, ``conf`` ``(H,W)`` or ``(1,H,W)``
    (``conf=None``, or a None entry: every pixel weighs 1).  A source view used in several pairs is simply passed several times;
    autograd adds its gradients.  float32, contiguous tensors on one device; a bool ``conf`` raises (pass ``conf.float()``).
    ``pinhole_src`` / ``pinhole_dst`` are one ``(fx, fy, cx, cy)`` for every pair or K of them, as host floats or a CPU tensor
    (``pinhole_of``); a GPU tensor raises, because reading it would synchronise.  ``delta`` (pixels) may be ``inf``.  Two HIP launches
    forward and at most two backward per 16 pairs.  Differentiable in ``depth``, ``weights``, ``view_src`` and ``view_dst``; there is no
    gradient to ``match``, ``conf`` or the intrinsics (out of scope), and ``count`` is not differentiable.  ``depth`` is read as the
    pinhole view depth: with non-zero ``shift_factors`` the maps carry the D2 term, which this loss ignores.  The backward re-reads
    its inputs: writing one of them in place between forward and backward raises."""
    Ds, As, Vs, Vd, ms, cs, pin_i, pin_j, min_weight, min_depth, delta = _arguments(_OP, depth, weights, view_src, view_dst, match, pinhole_src,
                                                                                    pinhole_dst, conf, delta, min_weight, min_depth)
    _require_all(_OP, (("depth", Ds), ("weights", As), ("view_src", Vs), ("view_dst", Vd), ("match", ms), ("conf", cs)), _HOST)
    return _Correspondence.apply(pin_i, pin_j, delta, min_weight, min_depth, len(Ds), *Ds, *As, *Vs, *Vd, *ms, *cs)


def reproject_pixels(depth, weights, view_src, view_dst, pinhole_src, pinhole_dst, size_dst, *, min_weight=0.5, min_depth=0.01):
    """``(proj (2,H,W) float32, valid (H,W) bool)`` of one pair on an AMD GPU, in one HIP launch; the statement is
    ``reproject_pixels_torch``.  Not differentiable: covisibility masks, viewers and pseudo-matches."""
    op = "reproject_pixels"
    D, A, Vi, Vj, pin_i, pin_j, (H_dst, W_dst), min_weight, min_depth = _one_pair(op, depth, weights, view_src, view_dst, pinhole_src,
                                                                                  pinhole_dst, size_dst, min_weight, min_depth)
    host = ": bags_raster.reproject_pixels_torch is the same function in PyTorch on any device and dtype"
    D, A, Vi, Vj = (t.detach() for t in (D, A, Vi, Vj))
    _require_all(op, (("depth", [D]), ("weights", [A]), ("view_src", [Vi]), ("view_dst", [Vj])), host)
    H, W = D.shape[-2:]
    proj = torch.empty(2, H, W, dtype=torch.float32, device=D.device)
    valid = torch.empty(H, W, dtype=torch.uint8, device=D.device)
    args = L.BagsCorrespondence(H, W, 1, min_weight, min_depth, 1.0, _pinhole_field([pin_i]), _pinhole_field([pin_j]), _ptr_field([D]),
                                _ptr_field([A]), _ptr_field([None]), _ptr_field([None]), _ptr_field([Vi]), _ptr_field([Vj]))
    L.call("bags_reproject_pixels", D.device, C.byref(args), H_dst, W_dst, proj.data_ptr(), valid.data_ptr())
    return proj, valid.view(torch.bool)
