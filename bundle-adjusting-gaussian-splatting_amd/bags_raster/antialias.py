"""Antialiased rendering: the opacity scale of the mip filter (upstream ``diff_gaussian_rasterization``'s ``antialiasing``
setting, Mip-Splatting's 2D filter, gsplat's ``rasterize_mode="antialiased"``).

The rasterizer adds 0.3 px^2 to the diagonal of every projected covariance.  Per Gaussian

    h   = sqrt(max(0.000025, det(cov2D) / det(cov2D + 0.3 I)))          (1 for a Gaussian the forward culls)
    out = opacity * h

makes the dilated Gaussian carry the energy of the original one.  Upstream applies ``h`` in exactly one place, the opacity it
stores beside the conic, so the factor is a function IN FRONT of the operator's ``opacities`` input: ``antialias_opacity`` -- one
HIP launch each way (csrc/antialias.hip) -- chained with the operator's own ``dL/dopacities`` is upstream's antialiased forward
and backward.  ``GaussianRasterizationSettings(antialiasing=True)`` does exactly that inside ``GaussianRasterizer.forward``.
``antialias_opacity_torch`` is the same function in plain PyTorch on any device and dtype.
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import torch

from . import _lib as L

FLOOR = 0.000025                    # upstream's floor of the determinant ratio: h >= 0.005
_OP = "antialias_opacity"


def _sources(op, scales, rotations, cov3D_precomp) -> None:
    if ((scales is None or rotations is None) and cov3D_precomp is None) or \
            ((scales is not None or rotations is not None) and cov3D_precomp is not None):
        raise ValueError(f"{op}: provide exactly one of either scale/rotation pair or precomputed 3D covariance")


def _shapes(op, means3D, opacities, viewmatrix, intrinsic, scales, rotations, cov3D_precomp, shift_factors) -> int:
    if means3D.dim() != 2 or means3D.shape[1] != 3:
        raise ValueError(f"{op}: means3D must be (P,3), got {tuple(means3D.shape)}")
    P = means3D.shape[0]
    if opacities.numel() != P or opacities.dim() > 2:
        raise ValueError(f"{op}: opacities must be (P,1) with P = {P}, got {tuple(opacities.shape)}")
    for name, t, shape in (("viewmatrix", viewmatrix, (4, 4)), ("intrinsic", intrinsic, (4, 4)), ("scales", scales, (P, 3)),
                           ("rotations", rotations, (P, 4)), ("cov3D_precomp", cov3D_precomp, (P, 6)), ("shift_factors", shift_factors, (3,))):
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"{op}: {name} must be {shape}, got {tuple(t.shape)}")
    return P


def _clamp_mode(op, clamp_grad) -> int:
    if clamp_grad not in ("stock", "exact"):
        raise ValueError(f"{op}: clamp_grad must be 'stock' or 'exact'")
    return L.CLAMP_GRAD_EXACT if clamp_grad == "exact" else L.CLAMP_GRAD_STOCK


# ------------------------------------------------------------------------------------------------------------------ PyTorch
def _sqrt(x):
    """Correctly rounded: torch's vectorised fp32 CPU sqrt is not; the kernels' sqrtf is."""
    return torch.sqrt(x.double()).float() if x.dtype == torch.float32 else torch.sqrt(x)


def _atan2_pos(rho, tz):
    """atan2(rho, tz) for rho >= 0, tz > 0.  float32: csrc/bags_common.h's det_atan2_pos, operation for operation; any other
    dtype: torch.atan2."""
    if rho.dtype != torch.float32:
        return torch.atan2(rho, tz)
    f = lambda c: torch.as_tensor(c, dtype=rho.dtype, device=rho.device)        # noqa: E731
    lo, hi = torch.minimum(rho, tz), torch.maximum(rho, tz)
    u = lo / hi
    red = u.detach() > f(0.414213568)
    w = torch.where(red, (u - 1.0) / (u + 1.0), u)
    s = w * w
    p = f(-0.0607120693) * s + f(0.105907366)
    p = p * s + f(-0.142430589)
    p = p * s + f(0.199984416)
    p = p * s + f(-0.333333135)
    a = w + w * (s * p)
    a = torch.where(red, f(0.785398185) + a, a)
    return torch.where(rho.detach() > tz.detach(), f(1.57079637) - a, a)


def _chain_torch(means3D, opacities, viewmatrix, intrinsic, image_hw, tanfov, scales, rotations, cov3D_precomp, shift_factors,
                 scale_modifier, clamp_grad):
    """The statement behind ``antialias_opacity_torch``; what it decided per Gaussian in front of the near plane (rows ``idx``) comes
    back too -- ``ok`` (det(cov2D + 0.3 I) != 0), ``above`` (the ratio is above the floor), ``clx`` / ``cly`` (an axis sits on the
    field-of-view clamp) -- for the tests that count those rows."""
    op = "antialias_opacity_torch"
    _sources(op, scales, rotations, cov3D_precomp)
    _clamp_mode(op, clamp_grad)
    P = _shapes(op, means3D, opacities, viewmatrix, intrinsic, scales, rotations, cov3D_precomp, shift_factors)
    dt, dev = means3D.dtype, means3D.device
    H, W = int(image_hw[0]), int(image_hw[1])
    c = lambda t: None if t is None else t.to(device=dev, dtype=dt)              # noqa: E731
    f = lambda x: torch.as_tensor(x, dtype=dt, device=dev)                      # noqa: E731
    v, k = c(viewmatrix).reshape(16), c(intrinsic).reshape(16)
    sf = c(shift_factors).reshape(3) if shift_factors is not None else torch.zeros(3, dtype=dt, device=dev)
    opac = c(opacities).reshape(P)

    with torch.no_grad():
        tz_all = means3D[:, 0] * v[2] + means3D[:, 1] * v[6] + means3D[:, 2] * v[10] + v[14]
        idx = (tz_all > 0.2).nonzero().squeeze(1)                                # K1's near-plane cull
    sub = lambda t: None if t is None else c(t).index_select(0, idx)             # noqa: E731
    m3, sc_s, rot_s, cov_s = sub(means3D), sub(scales), sub(rotations), sub(cov3D_precomp)
    x, y, z = m3[:, 0], m3[:, 1], m3[:, 2]
    # pj_view
    tx = x * v[0] + y * v[4] + z * v[8] + v[12]
    ty = x * v[1] + y * v[5] + z * v[9] + v[13]
    tz = x * v[2] + y * v[6] + z * v[10] + v[14]
    # pj_shift
    rho = _sqrt(tx * tx + ty * ty + 1e-20)
    theta = _atan2_pos(rho, tz)
    th2 = theta * theta
    th3 = th2 * theta
    shift = sf[0] * th3 + sf[1] * (th3 * th2) + sf[2] * (th3 * th2 * th2)
    tzs = tz + shift
    # pj_cov3d
    if cov_s is not None:
        c0, c1, c2, c3, c4, c5 = [cov_s[:, i] for i in range(6)]
    else:
        mod = float(scale_modifier)
        s0, s1, s2 = sc_s[:, 0] * mod, sc_s[:, 1] * mod, sc_s[:, 2] * mod
        qr, qx, qy, qz = rot_s[:, 0], rot_s[:, 1], rot_s[:, 2], rot_s[:, 3]
        r00 = 1.0 - 2.0 * (qy * qy + qz * qz)
        r01 = 2.0 * (qx * qy - qr * qz)
        r02 = 2.0 * (qx * qz + qr * qy)
        r10 = 2.0 * (qx * qy + qr * qz)
        r11 = 1.0 - 2.0 * (qx * qx + qz * qz)
        r12 = 2.0 * (qy * qz - qr * qx)
        r20 = 2.0 * (qx * qz - qr * qy)
        r21 = 2.0 * (qy * qz + qr * qx)
        r22 = 1.0 - 2.0 * (qx * qx + qy * qy)
        l00, l01, l02 = r00 * s0, r01 * s1, r02 * s2
        l10, l11, l12 = r10 * s0, r11 * s1, r12 * s2
        l20, l21, l22 = r20 * s0, r21 * s1, r22 * s2
        c0 = l00 * l00 + l01 * l01 + l02 * l02
        c1 = l00 * l10 + l01 * l11 + l02 * l12
        c2 = l00 * l20 + l01 * l21 + l02 * l22
        c3 = l10 * l10 + l11 * l11 + l12 * l12
        c4 = l10 * l20 + l11 * l21 + l12 * l22
        c5 = l20 * l20 + l21 * l21 + l22 * l22
    # pj_cov2d
    fx = k[0] * (0.5 * W)
    fy = k[5] * (0.5 * H)
    limx = f(1.3) * f(float(tanfov[0]))
    limy = f(1.3) * f(float(tanfov[1]))
    txtz = tx / tzs
    tytz = ty / tzs
    cx_ = torch.minimum(limx, torch.maximum(-limx, txtz)) * tzs
    cy_ = torch.minimum(limy, torch.maximum(-limy, tytz)) * tzs
    with torch.no_grad():
        clx = (txtz < -limx) | (txtz > limx)
        cly = (tytz < -limy) | (tytz > limy)
    if clamp_grad == "stock":
        cx_ = torch.where(clx, cx_.detach(), cx_)
        cy_ = torch.where(cly, cy_.detach(), cy_)
    itz = 1.0 / tzs
    itz2 = itz * itz
    j00 = fx * itz
    j02 = -(fx * cx_) * itz2
    j11 = fy * itz
    j12 = -(fy * cy_) * itz2
    a00 = j00 * v[0] + j02 * v[2]
    a01 = j00 * v[4] + j02 * v[6]
    a02 = j00 * v[8] + j02 * v[10]
    a10 = j11 * v[1] + j12 * v[2]
    a11 = j11 * v[5] + j12 * v[6]
    a12 = j11 * v[9] + j12 * v[10]
    b00 = a00 * c0 + a01 * c1 + a02 * c2
    b01 = a00 * c1 + a01 * c3 + a02 * c4
    b02 = a00 * c2 + a01 * c4 + a02 * c5
    b10 = a10 * c0 + a11 * c1 + a12 * c2
    b11 = a10 * c1 + a11 * c3 + a12 * c4
    b12 = a10 * c2 + a11 * c4 + a12 * c5
    uxx = b00 * a00 + b01 * a01 + b02 * a02                    # cov2D before the + 0.3
    uxy = b00 * a10 + b01 * a11 + b02 * a12
    uyy = b10 * a10 + b11 * a11 + b12 * a12
    cxx = uxx + 0.3
    cyy = uyy + 0.3
    d0 = uxx * uyy - uxy * uxy
    d1 = cxx * cyy - uxy * uxy                                 # pj_conic's det
    one = torch.ones_like(d1)
    floor = f(FLOOR)
    ok = d1.detach() != 0                                      # K1's second cull
    ratio = d0 / torch.where(ok, d1, one)
    above = ok & (ratio.detach() > floor)
    h_sub = torch.where(above, _sqrt(torch.where(above, ratio, one)), torch.where(ok, _sqrt(floor), f(1.0)))
    return SimpleNamespace(P=P, idx=idx, opacities=opac, h=h_sub, ratio=ratio, ok=ok, above=above, clx=clx, cly=cly)


def antialias_opacity_torch(means3D, opacities, viewmatrix, intrinsic, image_hw, tanfov, scales=None, rotations=None, cov3D_precomp=None,
                            shift_factors=None, scale_modifier=1.0, clamp_grad="stock"):
    """``antialias_opacity`` in plain PyTorch, on the device and in the dtype of ``means3D``; autograd gives its backward.

    The chain is csrc/projection.h's, expression by expression in its order -- ``a*b + c*d`` is two rounded products and one
    rounded sum, left to right -- so that float32 on the CPU rounds as the kernel does.  The differentiable graph is built on the
    Gaussians in front of the near plane only, and a row whose ``det(cov2D + 0.3 I)`` is zero or whose ratio sits on the floor is
    switched off with ``where`` in front of the division and the square root: such rows give ``dL/dopacity`` and exactly nothing
    else, never a ``0 * inf``.  ``clamp_grad="stock"`` holds a clamped ``t.x`` constant (``detach``), ``"exact"`` differentiates
    the clamped expression."""
    r = _chain_torch(means3D, opacities, viewmatrix, intrinsic, image_hw, tanfov, scales, rotations, cov3D_precomp, shift_factors,
                     scale_modifier, clamp_grad)
    h = torch.ones(r.P, dtype=r.h.dtype, device=r.h.device).index_copy(0, r.idx, r.h)
    return (r.opacities * h).reshape(r.P, 1)


# ------------------------------------------------------------------------------------------------------------------ HIP
class _AntialiasOpacity(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, opacities, viewmatrix, intrinsic, scales, rotations, cov3D_precomp, shift_factors, H, W, tanfovx, tanfovy,
                scale_modifier, clamp):
        dev, P = means3D.device, means3D.shape[0]
        keep = tuple(L.as_f32c(t) for t in (means3D, scales, rotations, cov3D_precomp, opacities, shift_factors, viewmatrix, intrinsic))
        args = L.BagsAntialias(P, W, H, clamp, tanfovx, tanfovy, scale_modifier, 0, *[L.ptr(t) for t in keep])
        out = torch.empty(P, 1, dtype=torch.float32, device=dev)
        if P > 0:
            L.call("bags_antialias_forward", dev, C.byref(args), out.data_ptr())
        ctx.keep, ctx.args = keep, args                           # (the struct's pointers live as long as `keep`)
        ctx.shapes = tuple(None if t is None else t.shape for t in (means3D, opacities, viewmatrix, intrinsic, scales, rotations,
                                                                   cov3D_precomp, shift_factors))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        dev, P = grad_out.device, ctx.args.P
        need = ctx.needs_input_grad
        # outputs in the order of forward's first eight arguments; an input that is absent or not differentiated gets a NULL pointer
        grads = [torch.empty(sh, dtype=torch.float32, device=dev) if (n and sh is not None) else None for n, sh in zip(need[:8], ctx.shapes)]
        g_means, g_opac, g_view, g_intr, g_scales, g_rot, g_cov, g_shift = grads
        if P == 0:
            for g in (g_view, g_intr, g_shift):
                if g is not None:
                    g.zero_()
        elif any(g is not None for g in grads):
            pose = g_view is not None or g_intr is not None or g_shift is not None
            ws = L.workspace(L.load().bags_antialias_workspace_size(P) if pose else 0, dev)
            L.call("bags_antialias_backward", dev, C.byref(ctx.args), L.as_f32c(grad_out).data_ptr(), L.ptr(ws) if pose else None, ws.numel(),
                   L.ptr(g_opac), L.ptr(g_means), L.ptr(g_scales), L.ptr(g_rot), L.ptr(g_cov), L.ptr(g_view), L.ptr(g_intr), L.ptr(g_shift))
        return (*grads, None, None, None, None, None, None)


def antialias_opacity(means3D, opacities, viewmatrix, intrinsic, image_hw, tanfov, scales=None, rotations=None, cov3D_precomp=None,
                      shift_factors=None, scale_modifier=1.0, clamp_grad="stock"):
    """``opacities * h`` as ``(P,1)``, with the inputs of one ``GaussianRasterizer`` call: ``means3D (P,3)``, ``opacities (P,1)``,
    ``viewmatrix`` / ``intrinsic (4,4)``, ``image_hw = (H, W)``, ``tanfov = (tanfovx, tanfovy)`` (the static tangents of the
    settings), ``scales (P,3)`` with ``rotations (P,4)`` or ``cov3D_precomp (P,6)``, ``shift_factors (3,)`` or None (zeros), and the
    settings' ``scale_modifier`` and ``clamp_grad``.  float32 tensors on one AMD GPU; one HIP launch forward, two backward
    (csrc/antialias.hip).  Differentiable in every tensor argument; the pose gradients are summed without atomics and repeat bit
    for bit."""
    ts = (("means3D", means3D), ("opacities", opacities), ("viewmatrix", viewmatrix), ("intrinsic", intrinsic), ("scales", scales),
          ("rotations", rotations), ("cov3D_precomp", cov3D_precomp), ("shift_factors", shift_factors))
    given = [(n, t) for n, t in ts if t is not None]
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for _, t in given):
        raise NotImplementedError(f"{_OP} runs only on an AMD GPU and takes GPU tensors; there is no CPU fallback behind this name: "
                                  "bags_raster.antialias_opacity_torch is the same function in PyTorch on any device and dtype")
    for name, t in given:
        L.require(_OP, name, t, gpu=True, f32=True, on=means3D)
    _sources(_OP, scales, rotations, cov3D_precomp)
    clamp = _clamp_mode(_OP, clamp_grad)
    _shapes(_OP, means3D, opacities, viewmatrix, intrinsic, scales, rotations, cov3D_precomp, shift_factors)
    H, W = int(image_hw[0]), int(image_hw[1])
    if H <= 0 or W <= 0:
        raise ValueError(f"{_OP}: empty image {W}x{H}")
    return _AntialiasOpacity.apply(means3D, opacities, viewmatrix, intrinsic, scales, rotations, cov3D_precomp, shift_factors, H, W,
                                   float(tanfov[0]), float(tanfov[1]), float(scale_modifier), clamp)
