"""gaussian_reg_loss -- the regularisers on the Gaussians themselves, over all P rows of the raw leaves (csrc/gaussian_reg.hip).

The loss terms that live on a rendered map are the other modules; these live on ``_opacity (P,1)`` and ``_scaling (P,3)``.  With
``o`` and ``s_a`` the activated opacity and scales -- ``sigmoid`` and ``exp``, or Mip-Splatting's filtered ones under a 3D filter ``f``
(``filtered_activations_torch``: ``s_a = sqrt(exp(r_a)^2 + f^2)``, ``o = sigmoid * prod_a exp(r_a) / s_a``) -- and ``n`` the number of
rows that ``select`` keeps (``None``: all P):

    0 opacity   sum o / n                                     3DGS-MCMC's opacity_reg term, torch.abs(get_opacity).mean()
    1 scale     sum sum_a s_a / (3 n)                         3DGS-MCMC's scale_reg term, torch.abs(get_scaling).mean()
    2 flat      sum s_kmin / n                                the minimum-scale loss of PGSR, NeuSG, the 2DGS family, DN-Splatter
    3 aniso     sum max(s_kmax / s_kmin - max_ratio, 0) / n   PhysGaussian's and Splatfacto's anisotropy hinge
    4 big       sum sum_a max(s_a - max_scale, 0) / (3 n)     a hinge on large scales
    5 entropy   sum -(o log o + (1 - o) log(1 - o)) / n       the opacity entropy of pruning recipes

``kmin`` / ``kmax`` are the first minimum / maximum of the row's raw log-scales (``gaussian_normals``' tie rule; ``s`` is monotone in
them with and without a filter), and their terms send their gradient to those components only.  Both hinges are strict: exactly at
the threshold the value and the gradient are zero.  A row whose ``o`` is ``<= 0`` or ``>= 1`` in the working precision has no
entropy and gets no gradient from it.  ``n == 0`` (no rows, nothing selected): six zeros and all-zero gradients, never NaN.  Rows
that are not selected get exact-zero gradients.  With a filter the two opacity terms reach ``_scaling`` through ``c``.

``gaussian_reg_loss_torch`` states the six terms in plain PyTorch on any device and dtype and differentiates by autograd; in
float64 it is the reference.  ``gaussian_reg_loss`` is the HIP path: two launches forward, one backward, sums in double without
atomics, so it repeats bit for bit.  ``GaussianBag.regularizers`` is the call site on a bag.
"""
from __future__ import annotations

import ctypes as C
import torch

from . import _lib as L
from .filter3d import filtered_activations_torch

_OP = "gaussian_reg_loss"
REG_TERMS = ("opacity", "scale", "flat", "aniso", "big", "entropy")
ROWS_PER_GROUP = L.GAUSSIAN_REG_ROWS                           # rows a workgroup of the sums kernel takes (one workspace record)


def _arguments(op: str, opacity_raw, scaling_raw, filter_3D, select, terms, max_ratio, max_scale):
    """The checks the HIP path and the PyTorch statement share: (P, bitmask of the wanted terms, max_ratio, max_scale)."""
    for name, t in (("opacity_raw", opacity_raw), ("scaling_raw", scaling_raw)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{op}: {name} must be a tensor, got {type(t).__name__}")
        if not t.dtype.is_floating_point:
            raise TypeError(f"{op}: {name} must be a floating-point tensor, got {t.dtype}")
    if scaling_raw.dim() != 2 or scaling_raw.shape[1] != 3:
        raise ValueError(f"{op}: scaling_raw must be (P,3), got {tuple(scaling_raw.shape)}")
    P = scaling_raw.shape[0]
    if tuple(opacity_raw.shape) != (P, 1):
        raise ValueError(f"{op}: opacity_raw must be (P,1) with P = {P}, got {tuple(opacity_raw.shape)}")
    if opacity_raw.dtype != scaling_raw.dtype:
        raise TypeError(f"{op}: opacity_raw is {opacity_raw.dtype}, scaling_raw is {scaling_raw.dtype}: one dtype per call")
    if opacity_raw.device != scaling_raw.device:
        raise ValueError(f"{op}: opacity_raw is on {opacity_raw.device}, scaling_raw on {scaling_raw.device}: one device per call")
    if filter_3D is not None:
        if not isinstance(filter_3D, torch.Tensor):
            raise TypeError(f"{op}: filter_3D must be a tensor or None, got {type(filter_3D).__name__}")
        if not filter_3D.dtype.is_floating_point:
            raise TypeError(f"{op}: filter_3D must be a floating-point tensor, got {filter_3D.dtype}")
        if tuple(filter_3D.shape) not in ((P, 1), (P,)):
            raise ValueError(f"{op}: filter_3D must be (P,1) with P = {P}, got {tuple(filter_3D.shape)}")
        if filter_3D.device != scaling_raw.device:
            raise ValueError(f"{op}: filter_3D is on {filter_3D.device}, scaling_raw on {scaling_raw.device}: one device per call")
    if select is not None:
        if not isinstance(select, torch.Tensor):
            raise TypeError(f"{op}: select must be a tensor or None, got {type(select).__name__}")
        if select.dtype != torch.bool:
            raise TypeError(f"{op}: select must be a torch.bool tensor, got {select.dtype}")
        if tuple(select.shape) != (P,):
            raise ValueError(f"{op}: select must be (P,) with P = {P}, got {tuple(select.shape)}")
        if select.device != scaling_raw.device:
            raise ValueError(f"{op}: select is on {select.device}, scaling_raw on {scaling_raw.device}: one device per call")
    names = (terms,) if isinstance(terms, str) else tuple(terms)
    mask = 0
    for name in names:
        if name not in REG_TERMS:
            raise ValueError(f"{op}: unknown term {name!r} in terms; the terms are {REG_TERMS}")
        mask |= 1 << REG_TERMS.index(name)
    max_ratio, max_scale = float(max_ratio), float(max_scale)
    if not max_ratio >= 1.0:
        raise ValueError(f"{op}: max_ratio must be >= 1 (a ratio of largest to smallest scale), got {max_ratio}")
    if not max_scale >= 0.0:
        raise ValueError(f"{op}: max_scale must be >= 0, got {max_scale}")
    return P, mask, max_ratio, max_scale


# ------------------------------------------------------------------------------------------------------------------ PyTorch
def gaussian_reg_loss_torch(opacity_raw, scaling_raw, filter_3D=None, select=None, terms=REG_TERMS, max_ratio=10.0, max_scale=0.05):
    """The six terms of the module docstring in plain PyTorch, on the device and in the dtype of the leaves; autograd gives the
    backward.  Arguments and result as ``gaussian_reg_loss``: ``(terms (6,), count ())`` in that dtype.  In float64 this is the
    reference, in float32 the comparison path."""
    P, mask, max_ratio, max_scale = _arguments("gaussian_reg_loss_torch", opacity_raw, scaling_raw, filter_3D, select, terms, max_ratio,
                                               max_scale)
    dt, dev = scaling_raw.dtype, scaling_raw.device
    if filter_3D is None:
        o, s = torch.sigmoid(opacity_raw), torch.exp(scaling_raw)
    else:
        o, s = filtered_activations_torch(opacity_raw, scaling_raw, filter_3D)
    o = o.reshape(P)
    sel = torch.ones(P, dtype=torch.bool, device=dev) if select is None else select
    n = sel.sum().to(dt)
    inv_n = torch.where(n > 0, 1.0 / n.clamp_min(1.0), torch.zeros_like(n))
    zero = torch.zeros((), dtype=dt, device=dev)
    mean = lambda v, k=1: torch.where(sel, v, zero).sum() * (inv_n / k)                  # noqa: E731
    r = scaling_raw.detach()
    r0, r1, r2 = r.unbind(1)
    kmin = (r1 < r0).long()                                                               # the first minimum / maximum: strict tests
    kmin = torch.where(r2 < torch.where(kmin == 1, r1, r0), torch.full_like(kmin, 2), kmin)
    kmax = (r1 > r0).long()
    kmax = torch.where(r2 > torch.where(kmax == 1, r1, r0), torch.full_like(kmax, 2), kmax)
    s_min, s_max = s.gather(1, kmin[:, None])[:, 0], s.gather(1, kmax[:, None])[:, 0]
    out = [zero] * len(REG_TERMS)
    if mask & 1:
        out[0] = mean(o)
    if mask & 2:
        out[1] = mean(s.sum(1), 3)
    if mask & 4:
        out[2] = mean(s_min)
    if mask & 8:
        h = s_max / s_min - max_ratio
        out[3] = mean(torch.where(h > 0, h, zero))                                       # strict: at the threshold no gradient either
    if mask & 16:
        h = s - max_scale
        out[4] = mean(torch.where(h > 0, h, zero).sum(1), 3)
    if mask & 32:
        inside = (o > 0) & (o < 1)
        os_ = torch.where(inside, o, torch.full_like(o, 0.5))                            # a saturated row: no log(0) in the graph
        out[5] = mean(torch.where(inside, -(torch.xlogy(os_, os_) + torch.xlogy(1 - os_, 1 - os_)), zero))
    return torch.stack(out), n.detach()


# ------------------------------------------------------------------------------------------------------------------ HIP
class _GaussianReg(torch.autograd.Function):
    @staticmethod
    def forward(ctx, opacity_raw, scaling_raw, filter_3D, select, mask, max_ratio, max_scale):
        P, dev = scaling_raw.shape[0], scaling_raw.device
        terms = torch.empty(L.GAUSSIAN_REG_TERMS, dtype=torch.float32, device=dev)
        count = torch.empty((), dtype=torch.float32, device=dev)
        stats = torch.empty(L.GAUSSIAN_REG_STATS, dtype=torch.float64, device=dev)
        ws = L.workspace(L.load().bags_gaussian_reg_workspace_size(P), dev)
        args = L.BagsGaussianReg(P, mask, max_ratio, max_scale, L.ptr(opacity_raw), L.ptr(scaling_raw), L.ptr(filter_3D), L.ptr(select))
        L.call("bags_gaussian_reg_forward", dev, C.byref(args), L.ptr(ws), ws.numel(), L.ptr(terms), L.ptr(count), L.ptr(stats))
        ctx.mark_non_differentiable(count)
        if any(ctx.needs_input_grad):                          # nothing is kept under no_grad or for constant inputs
            ctx.save_for_backward(stats, opacity_raw, scaling_raw, filter_3D, select)      # versions are checked at backward: it re-reads them
            ctx.args = args
        return terms, count

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_terms, _g_count):
        stats, opacity_raw, scaling_raw, _filter, _select = ctx.saved_tensors              # raises if a leaf was written in place since
        need = ctx.needs_input_grad
        g = L.as_f32c(g_terms)
        # every element is written by the kernel (rows that are not selected: zeros): no fill launch
        g_opacity = torch.empty_like(opacity_raw) if need[0] else None
        g_scaling = torch.empty_like(scaling_raw) if need[1] else None
        L.call("bags_gaussian_reg_backward", stats.device, C.byref(ctx.args), L.ptr(stats), L.ptr(g), L.ptr(g_opacity), L.ptr(g_scaling))
        return g_opacity, g_scaling, None, None, None, None, None


def gaussian_reg_loss(opacity_raw, scaling_raw, filter_3D=None, select=None, terms=REG_TERMS, max_ratio=10.0, max_scale=0.05):
    """The regularisers of the module docstring on an AMD GPU: ``(terms (6,), count ())``, float32, ``terms`` always in
    ``REG_TERMS``' order, ``count = n`` without a gradient.

    ``opacity_raw (P,1)`` and ``scaling_raw (P,3)`` are the raw leaves, float32 and contiguous on one GPU; ``filter_3D (P,1)`` or
    None (no gradient to it); ``select (P,)`` ``torch.bool`` or None: the rows that count, e.g. a visibility filter.  ``terms=``
    names the subset to evaluate: an entry that is not named is an exact 0, carries no gradient, and the kernels skip its work.
    Usage: ``loss = loss + args.opacity_reg * terms[0] + args.scale_reg * terms[1]``.  The backward re-reads the leaves: writing one
    of them in place between forward and backward raises."""
    P, mask, max_ratio, max_scale = _arguments(_OP, opacity_raw, scaling_raw, filter_3D, select, terms, max_ratio, max_scale)
    if not (opacity_raw.is_cuda and scaling_raw.is_cuda):
        raise NotImplementedError(f"{_OP} runs only on an AMD GPU and takes GPU tensors; there is no CPU fallback behind this name: "
                                  "bags_raster.gaussian_reg_loss_torch is the same function in PyTorch on any device and dtype")
    for name, t in (("opacity_raw", opacity_raw), ("scaling_raw", scaling_raw)):
        L.require(_OP, name, t, gpu=True, f32=True, contiguous=True, on=scaling_raw)
    filt = None
    if filter_3D is not None:
        L.require(_OP, "filter_3D", filter_3D, gpu=True, on=scaling_raw)
        filt = L.as_f32c(filter_3D)
    sel = None if select is None else select.contiguous()
    return _GaussianReg.apply(opacity_raw, scaling_raw, filt, sel, mask, max_ratio, max_scale)
