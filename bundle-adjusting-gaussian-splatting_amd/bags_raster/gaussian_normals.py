"""gaussian_normals -- the normal of every Gaussian in the camera frame (csrc/gaussian_normals.hip).

``normal_prior_loss`` and ``depth_to_normal`` take their normals from finite differences of the rendered depth.  The recipes they
were written for (DN-Splatter, GaussianShader, GaussianPro, the PGSR / GOF / RaDe-GS family) have a second source: the normal of
every Gaussian, its shortest axis turned towards the camera, splatted into a normal map through the rasterizer's
``override_color`` path (``render_normals``) and held to a monocular prior and to the depth normals (``normal_map_loss``).  Per
Gaussian and view, with ``q = (w,x,y,z)`` as given (it need not be a unit quaternion), scales ``s``, mean ``x`` and the row-vector
view matrix ``V`` (``t = x @ V[:3,:3] + V[3,:3]``, csrc/projection.h):

    k      = first minimum of (s0, s1, s2):  k = 0;  if s1 < s_k: k = 1;  if s2 < s_k: k = 2      (a decision; NaN compares false)
    Q(q)   = |q|^2 R(q/|q|), written without a division:
             col0 = (ww+xx-yy-zz, 2(xy+wz), 2(xz-wy));  col1 = (2(xy-wz), ww-xx+yy-zz, 2(yz+wx));  col2 = (2(xz+wy), 2(yz-wx), ww-xx-yy+zz)
    c      = col_k(Q(q))                     world frame: the axis of build_rotation's R that belongs to scale k
    m_j    = sum_i c_i V[i,j]                camera frame; a scale on the 3x3 block (global alignment) cancels below
    t      = x @ V[:3,:3] + V[3,:3]
    sigma  = -1 if m . t > 0 else +1         (a decision: the normal faces the camera, n_z < 0 for a wall seen head-on, the
                                              convention of normal_prior.py; m . t == 0 does not flip)
    l2     = |m|^2 ;  live = l2 is finite and > 0
    out    = sigma * m / sqrt(l2)  where live,  (0,0,0) elsewhere

Only the order of the scales is read, so any monotone function of them serves, the raw log-scales too.  Gradients go to
``rotations`` (through ``Q`` and the normalisation, summed over the views of a call) and to the 3x3 block of every view matrix (row
3 and column 3 of the ``(4,4)`` gradient are exact zeros).  ``k`` and ``sigma`` are decisions: ``scales`` and ``means3D`` get NO
gradient (autograd sees ``None``).  A dead row -- a zero or non-finite quaternion, a singular view block -- has a zero output and
exact-zero gradients, never NaN.

``gaussian_normals_torch`` / ``gaussian_normals_views_torch`` state this in PyTorch on any device and dtype: in float32 the
comparison path (the kernel's operations in the kernel's order), in float64 the reference.  ``gaussian_normals`` /
``gaussian_normals_views`` are the HIP path.
"""
from __future__ import annotations

import torch

from . import _lib as L
from .antialias import _sqrt

_OP = "gaussian_normals"


def _view_list(op: str, viewmatrices):
    if torch.is_tensor(viewmatrices) or not isinstance(viewmatrices, (list, tuple)):
        raise TypeError(f"{op}: viewmatrices must be a list or tuple of (4,4) tensors, got {type(viewmatrices).__name__}")
    if len(viewmatrices) < 1:
        raise ValueError(f"{op}: no view matrices")
    return list(viewmatrices)


def _shapes(op: str, rotations, scales, means3D, views) -> int:
    for name, t in (("rotations", rotations), ("scales", scales), ("means3D", means3D)):
        if not torch.is_tensor(t):
            raise TypeError(f"{op}: {name} must be a tensor, got {type(t).__name__}")
    if rotations.dim() != 2 or rotations.shape[1] != 4:
        raise ValueError(f"{op}: rotations must be (P,4), got {tuple(rotations.shape)}")
    P = rotations.shape[0]
    for name, t in (("scales", scales), ("means3D", means3D)):
        if tuple(t.shape) != (P, 3):
            raise ValueError(f"{op}: {name} must be (P,3) with P = {P}, got {tuple(t.shape)}")
    for v, m in enumerate(views):
        if not torch.is_tensor(m):
            raise TypeError(f"{op}: viewmatrix[{v}] must be a tensor, got {type(m).__name__}")
        if tuple(m.shape) != (4, 4):
            raise ValueError(f"{op}: viewmatrix[{v}] must be (4,4), got {tuple(m.shape)}")
    return P


# ------------------------------------------------------------------------------------------------------------------ PyTorch
def _axis_torch(rotations, scales):
    """``c = col_k(Q(q))`` as (c0, c1, c2) and ``k``: the statement's comparisons and sums in its order."""
    # a non-finite quaternion is dead under every view: it is zeroed here, so that no NaN meets a zero cotangent on the way back
    finite = torch.isfinite(rotations.detach()).all(1, keepdim=True)
    w, x, y, z = torch.where(finite, rotations, torch.zeros_like(rotations)).unbind(1)
    with torch.no_grad():                                      # decisions
        s0, s1, s2 = scales.unbind(1)
        is1 = s1 < s0
        sk = torch.where(is1, s1, s0)
        is2 = s2 < sk
        k = torch.where(is2, torch.full_like(is1, 2, dtype=torch.long), is1.long())
    ww, xx, yy, zz = w * w, x * x, y * y, z * z
    cols = ((ww + xx - yy - zz, 2.0 * (x * y + w * z), 2.0 * (x * z - w * y)),
            (2.0 * (x * y - w * z), ww - xx + yy - zz, 2.0 * (y * z + w * x)),
            (2.0 * (x * z + w * y), 2.0 * (y * z - w * x), ww - xx - yy + zz))
    return tuple(torch.where(k == 0, cols[0][j], torch.where(k == 1, cols[1][j], cols[2][j])) for j in range(3)), k


def _view_torch(c, means3D, V):
    """One view of the statement: ``(out (P,3), sigma (P,), live (P,))``."""
    x, y, z = means3D.detach().unbind(1)
    zero = torch.zeros_like(c[0])
    with torch.no_grad():                                      # decisions
        Vd = V.detach()
        md = [c[0] * Vd[0, j] + c[1] * Vd[1, j] + c[2] * Vd[2, j] for j in range(3)]
        l2d = md[0] * md[0] + md[1] * md[1] + md[2] * md[2]
        live = torch.isfinite(l2d) & (l2d > 0)
        t = [x * Vd[0, j] + y * Vd[1, j] + z * Vd[2, j] + Vd[3, j] for j in range(3)]
        d = md[0] * t[0] + md[1] * t[1] + md[2] * t[2]
        sigma = torch.where(d > 0, -torch.ones_like(d), torch.ones_like(d))
    # a dead row is switched off in front of every product: zeros out, exactly nothing back, never a 0 * inf
    c0, c1, c2 = (torch.where(live, cj, zero) for cj in c)
    m = [c0 * V[0, j] + c1 * V[1, j] + c2 * V[2, j] for j in range(3)]
    l2 = m[0] * m[0] + m[1] * m[1] + m[2] * m[2]
    length = _sqrt(torch.where(live, l2, torch.ones_like(l2)))
    out = torch.stack([torch.where(live, (sigma * mj) / length, zero) for mj in m], dim=1)
    return out, sigma, live


def gaussian_normals_views_torch(rotations, scales, means3D, viewmatrices):
    """The function of the module docstring in plain PyTorch, on the device and in the dtype of ``rotations``: a tuple of V ``(P,3)``
    tensors for the V ``(4,4)`` view matrices (any V).  Autograd gives its backward: to ``rotations`` and the view matrices, nothing
    to ``scales`` and ``means3D``.  The comparisons and the sums are spelled in the statement's order -- no ``torch.argmin``, whose
    tie rule is not documented; ``a*b + c*d`` is two rounded products and one rounded sum, left to right -- and the square root is
    ``antialias.py``'s correctly rounded one, so that float32 on the CPU rounds as the kernel does."""
    op = "gaussian_normals_views_torch"
    views = _view_list(op, viewmatrices)
    _shapes(op, rotations, scales, means3D, views)
    dt, dev = rotations.dtype, rotations.device
    c, _ = _axis_torch(rotations, scales.detach().to(device=dev, dtype=dt))
    x = means3D.to(device=dev, dtype=dt)
    return tuple(_view_torch(c, x, V.to(device=dev, dtype=dt))[0] for V in views)


def gaussian_normals_torch(rotations, scales, means3D, viewmatrix):
    """``gaussian_normals_views_torch`` for one ``(4,4)`` view matrix: ``(P,3)``."""
    if not torch.is_tensor(viewmatrix):
        raise TypeError(f"gaussian_normals_torch: viewmatrix must be a (4,4) tensor, got {type(viewmatrix).__name__}")
    return gaussian_normals_views_torch(rotations, scales, means3D, [viewmatrix])[0]


# ------------------------------------------------------------------------------------------------------------------ HIP
def _struct(P, rot, sc, xyz, views):
    return L.BagsGaussianNormals(P, len(views), L.ptr(rot), L.ptr(sc), L.ptr(xyz), L.ptr_table(list(views) + [None] * (L.MAX_SH_VIEWS - len(views))))


class _GaussianNormals(torch.autograd.Function):
    """The V <= 16 views of one call: V separate ``(P,3)`` outputs, one launch forward, two backward.  A view no loss depends on
    arrives in ``backward`` as None (``set_materialize_grads(False)``) and goes down as a NULL pointer."""

    @staticmethod
    def forward(ctx, rotations, scales, means3D, *views):
        ts = [L.as_f32c(t) for t in (rotations, scales, means3D) + views]
        dev, P, V = ts[0].device, ts[0].shape[0], len(views)
        out = tuple(torch.empty(P, 3, dtype=torch.float32, device=dev) for _ in range(V))
        if P > 0:
            L.call("bags_gaussian_normals_forward", dev, _struct(P, ts[0], ts[1], ts[2], ts[3:]), L.ptr_table(out))
        ctx.save_for_backward(*ts)                             # the inputs and nothing else: the backward recomputes the forward
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *g_out):
        if all(g is None for g in g_out):
            return (None,) * (3 + len(g_out))
        rot, sc, xyz, *views = ctx.saved_tensors
        dev, P, V = rot.device, rot.shape[0], len(views)
        need = ctx.needs_input_grad
        g_rot = torch.empty_like(rot) if need[0] else None
        g_views = [torch.empty(4, 4, dtype=torch.float32, device=dev) if need[3 + v] else None for v in range(V)]
        wanted = any(g is not None for g in g_views)
        if P == 0:
            for g in g_views:
                if g is not None:
                    g.zero_()
        elif g_rot is not None or wanted:
            g_out = [L.as_f32c(g) for g in g_out]
            ws = L.workspace(L.load().bags_gaussian_normals_workspace_size(P, V) if wanted else 0, dev)
            L.call("bags_gaussian_normals_backward", dev, _struct(P, rot, sc, xyz, views), L.ptr_table(g_out), L.ptr(ws) if wanted else None,
                   ws.numel(), L.ptr(g_rot), L.ptr_table(g_views))
        return (g_rot, None, None, *g_views)


_HOST = ": bags_raster.gaussian_normals_views_torch is the same function in PyTorch on any device and dtype"


def gaussian_normals_views(rotations, scales, means3D, viewmatrices):
    """The normals of the module docstring on an AMD GPU for the V views of one step: ``rotations (P,4)``, ``scales (P,3)`` (or any
    monotone function of them), ``means3D (P,3)``, ``viewmatrices`` a list or tuple of V ``(4,4)`` GPU tensors, which the host never
    reads; float32 on one device.  The result is a tuple of V ``(P,3)`` tensors, view v's the bits of a call of its own.

    One HIP launch forward and two backward per 16 views: a Gaussian's row is read once for all of them, ``dL/drotations`` is summed
    over the views on the chip in view order and written once, every view matrix gets its own ``(4,4)`` gradient (fourth row and
    column exact zeros), summed without atomics, so it repeats bit for bit.  More than 16 views are chunked here, on the host: one
    call of the kernels per chunk, and ``dL/drotations`` of the chunks is then added by autograd, one in-place add per further
    chunk.  A view whose normals no loss uses costs no cotangent in the backward.  ``scales`` and ``means3D`` get no gradient."""
    views = _view_list(_OP, viewmatrices)
    _shapes(_OP, rotations, scales, means3D, views)
    L.require(_OP, "rotations", rotations, gpu=True, f32=True, host=_HOST)
    for name, t in [("scales", scales), ("means3D", means3D)] + [(f"viewmatrix[{v}]", m) for v, m in enumerate(views)]:
        L.require(_OP, name, t, gpu=True, f32=True, on=rotations, host=_HOST)
    out = []
    for b in range(0, len(views), L.MAX_SH_VIEWS):
        out.extend(_GaussianNormals.apply(rotations, scales, means3D, *views[b:b + L.MAX_SH_VIEWS]))
    return tuple(out)


def gaussian_normals(rotations, scales, means3D, viewmatrix):
    """``gaussian_normals_views`` for one ``(4,4)`` view matrix, the V = 1 call of the same kernels: ``(P,3)``."""
    if not torch.is_tensor(viewmatrix):
        raise TypeError(f"{_OP}: viewmatrix must be a (4,4) tensor, got {type(viewmatrix).__name__}")
    return gaussian_normals_views(rotations, scales, means3D, [viewmatrix])[0]
