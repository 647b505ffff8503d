"""Mip-Splatting's 3D smoothing filter, the other half of antialiased rendering (``antialias_opacity`` is the 2D mip filter).

Each Gaussian gets a low-pass kernel whose size comes from the highest rate at which any training camera samples it
(``GaussianModel.compute_3D_filter`` upstream), and scale and opacity are evaluated through that kernel
(``get_scaling_with_3D_filter`` / ``get_opacity_with_3D_filter``):

    f        = (dist / focal) * sqrt(variance)          dist: the smallest view-space depth over the cameras that see the Gaussian
    scales'  = sqrt(exp(_scaling)^2 + f^2)
    opacity' = sigmoid(_opacity) * sqrt(prod(s^2) / prod(s^2 + f^2))

``filter_3D`` is the HIP function (csrc/filter3d.hip: xyz read once, the camera table walked in the kernel, two launches for any
number of cameras); ``filter_3D_torch`` is the same function in plain PyTorch on any device and dtype, and
``filtered_activations_torch`` states the two activations.  ``GaussianBag.compute_3D_filter`` / ``activated()`` are the call sites
(bags_raster/gaussians.py); the fused filtered activations are an instance of the activation kernels (csrc/activations.hip).
"""
from __future__ import annotations

import torch

from . import _lib as L
from .antialias import _sqrt

FAR = 100000.0                      # upstream's initial distance: the dmax of a set that no camera sees
_OP = "filter_3D"
_CHUNK = 8                          # cameras per pass of the PyTorch statement


def _shapes(op, xyz, viewmatrices, intrinsics, sizes) -> tuple:
    for name, t in (("xyz", xyz), ("viewmatrices", viewmatrices), ("intrinsics", intrinsics), ("sizes", sizes)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{op}: {name} must be a tensor, got {type(t).__name__}")
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"{op}: xyz must be (P,3), got {tuple(xyz.shape)}")
    if viewmatrices.dim() != 3 or tuple(viewmatrices.shape[1:]) != (4, 4):
        raise ValueError(f"{op}: viewmatrices must be (N,4,4), got {tuple(viewmatrices.shape)}")
    N = viewmatrices.shape[0]
    if tuple(intrinsics.shape) != (N, 4, 4):
        raise ValueError(f"{op}: intrinsics must be ({N},4,4), got {tuple(intrinsics.shape)}")
    if tuple(sizes.shape) != (N, 2):
        raise ValueError(f"{op}: sizes must be ({N},2) = (W, H) per camera, got {tuple(sizes.shape)}")
    if sizes.dtype.is_floating_point or sizes.dtype.is_complex or sizes.dtype == torch.bool:
        raise ValueError(f"{op}: sizes must be an integer tensor, got {sizes.dtype}")
    if N == 0:
        raise ValueError(f"{op}: needs at least one camera (N = 0)")
    return xyz.shape[0], N


def _variance(op, variance) -> float:
    variance = float(variance)
    if not variance >= 0.0:
        raise ValueError(f"{op}: variance must be non-negative, got {variance}")
    return variance


# ------------------------------------------------------------------------------------------------------------------ PyTorch
def _decide_torch(xyz, viewmatrices, intrinsics, sizes):
    """The per-camera part of the statement: ``(valid (P,N) bool, tz (P,N), fx (N,))`` on the device and in the dtype of ``xyz``."""
    dt, dev = xyz.dtype, xyz.device
    v = viewmatrices.to(device=dev, dtype=dt).reshape(-1, 16)
    k = intrinsics.to(device=dev, dtype=dt).reshape(-1, 16)
    W, H = sizes.to(device=dev, dtype=dt).unbind(1)
    x, y, z = (xyz[:, i:i + 1] for i in range(3))                        # (P,1) against (N,) rows of the table
    # csrc/projection.h's pj_view: products and sums in this order
    tx = x * v[:, 0] + y * v[:, 4] + z * v[:, 8] + v[:, 12]
    ty = x * v[:, 1] + y * v[:, 5] + z * v[:, 9] + v[:, 13]
    tz = x * v[:, 2] + y * v[:, 6] + z * v[:, 10] + v[:, 14]
    hw, hh = 0.5 * W, 0.5 * H
    fx, fy = k[:, 0] * hw, k[:, 5] * hh                                  # as pj_cov2d forms them
    px = tx / tz * fx + hw
    py = ty / tz * fy + hh
    valid = (tz > 0.2) & (px >= -0.15 * W) & (px <= 1.15 * W) & (py >= -0.15 * H) & (py <= 1.15 * H)
    return valid, tz, fx


@torch.no_grad()
def filter_3D_torch(xyz, viewmatrices, intrinsics, sizes, variance: float = 0.2) -> torch.Tensor:
    """``filter_3D`` in plain PyTorch, on the device and in the dtype of ``xyz``: ``(P,1)``, no gradient.

    ``viewmatrices`` / ``intrinsics (N,4,4)`` are the operator's row-vector matrices (``get_matrices``' ``viewmatrix`` and
    ``intrinsic``, stacked), ``sizes (N,2)`` the integer ``(W, H)`` of each camera.  Per Gaussian and camera, with ``v`` / ``k`` the
    camera's 16 entries:

        tx = x v0 + y v4 + z v8 + v12 ;  ty = x v1 + y v5 + z v9 + v13 ;  tz = x v2 + y v6 + z v10 + v14
        fx = k0 * (0.5 W) ;  fy = k5 * (0.5 H) ;  px = tx / tz * fx + 0.5 W ;  py = ty / tz * fy + 0.5 H
        valid = tz > 0.2  and  -0.15 W <= px <= 1.15 W  and  -0.15 H <= py <= 1.15 H
        dist  = min of tz over the valid cameras (100000 where there is none) ;  focal = max of fx
        dmax  = max of dist over the rows with a valid camera (100000 if there is no such row; upstream raises there)
        f     = ((a camera is valid ? dist : dmax) / focal) * sqrt(variance)

    ``a*b + c*d`` is two rounded products and one rounded sum, left to right, so that float32 on the CPU takes the decisions the
    kernel takes.  ``shift_factors`` is not part of the statement (upstream's test is a pinhole one)."""
    op = "filter_3D_torch"
    P, N = _shapes(op, xyz, viewmatrices, intrinsics, sizes)
    variance = _variance(op, variance)
    dt, dev = xyz.dtype, xyz.device
    far = torch.as_tensor(FAR, dtype=dt, device=dev)
    dist = torch.full((P,), FAR, dtype=dt, device=dev)
    any_valid = torch.zeros(P, dtype=torch.bool, device=dev)
    focal = None
    for c in range(0, N, _CHUNK):                                        # (P, _CHUNK) temporaries, whatever N is
        valid, tz, fx = _decide_torch(xyz.detach(), viewmatrices[c:c + _CHUNK].detach(), intrinsics[c:c + _CHUNK].detach(), sizes[c:c + _CHUNK])
        dist = torch.minimum(dist, torch.where(valid, tz, far).amin(dim=1))
        any_valid |= valid.any(dim=1)
        focal = fx.amax() if focal is None else torch.maximum(focal, fx.amax())
    dmax = dist[any_valid].amax() if bool(any_valid.any()) else far
    sv = _sqrt(torch.as_tensor(variance, dtype=dt, device=dev))
    return ((torch.where(any_valid, dist, dmax) / focal) * sv).reshape(P, 1)


def filtered_activations_torch(opacity_raw, scaling_raw, filter_3D):
    """``(opacity', scales')``: upstream's ``get_opacity_with_3D_filter`` and ``get_scaling_with_3D_filter`` of the raw leaves
    ``opacity_raw (P,1)`` and ``scaling_raw (P,3)`` under ``filter_3D (P,1)``; differentiable in the two leaves, not in the filter.

        scales'  = sqrt(exp(scaling_raw)^2 + f^2)
        opacity' = sigmoid(opacity_raw) * sqrt(prod(s^2) / prod(s^2 + f^2))"""
    f2 = torch.square(filter_3D.detach().reshape(-1, 1).to(device=scaling_raw.device, dtype=scaling_raw.dtype))
    s2 = torch.square(torch.exp(scaling_raw))
    s2f = s2 + f2
    coef = torch.sqrt(s2.prod(dim=1) / s2f.prod(dim=1))
    return torch.sigmoid(opacity_raw) * coef[..., None], torch.sqrt(s2f)


# ------------------------------------------------------------------------------------------------------------------ HIP
@torch.no_grad()
def filter_3D(xyz, viewmatrices, intrinsics, sizes, variance: float = 0.2) -> torch.Tensor:
    """The 3D smoothing filter of every Gaussian under N cameras, ``(P,1)``: ``filter_3D_torch``'s function in two HIP launches
    (csrc/filter3d.hip), whatever N is.  ``xyz (P,3)``, ``viewmatrices`` / ``intrinsics (N,4,4)`` float32 on one AMD GPU, ``sizes
    (N,2)`` integer ``(W, H)`` per camera on any device.  No atomics: the result repeats bit for bit and does not depend on the
    order of the rows or of the cameras.  It carries no gradient."""
    ts = (("xyz", xyz), ("viewmatrices", viewmatrices), ("intrinsics", intrinsics))
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for _, t in ts):
        raise NotImplementedError(f"{_OP} runs only on an AMD GPU and takes GPU tensors; there is no CPU fallback behind this name: "
                                  "bags_raster.filter_3D_torch is the same function in PyTorch on any device and dtype")
    for name, t in ts:
        L.require(_OP, name, t, gpu=True, f32=True, on=xyz)
    P, N = _shapes(_OP, xyz, viewmatrices, intrinsics, sizes)
    variance = _variance(_OP, variance)
    dev = xyz.device
    keep = [L.as_f32c(t) for t in (xyz, viewmatrices, intrinsics)]
    wh = sizes.detach().to(device=dev, dtype=torch.int32).contiguous()
    out = torch.empty(P, 1, dtype=torch.float32, device=dev)
    if P > 0:
        ws = L.workspace(L.load().bags_filter3d_workspace_size(P), dev)
        L.call("bags_filter3d_compute", dev, keep[0].data_ptr(), P, keep[1].data_ptr(), keep[2].data_ptr(), wh.data_ptr(), N, variance,
               ws.data_ptr(), ws.numel(), out.data_ptr())
    return out
