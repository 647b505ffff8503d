"""depth_prior_loss -- a depth prior on the rasterizer's ``depth`` and ``weights`` maps (csrc/depth_prior.hip).

The operator returns ``depth = sum w_i z_i`` and ``weights = 1 - T_final``, differentiable with ``depth_weights_grad=True`` (DESIGN.md
decision D5).  This module is the loss that consumes them: the Pearson depth loss of sparse-view and pose-free splatting -- a
monocular prior has unknown scale and shift, and the correlation does not see either -- and upstream 3DGS's ``depth_l1_weight``
term with its per-image ``depth_params`` ``(a, b)``.  For one view with maps ``D``, ``A``, a prior ``p`` and an optional pixel
weight ``m >= 0`` (``None``: 1), a pixel is valid iff ``m > 0``, ``A >= min_weight``, ``D > 0`` and ``p > 0``; a NaN or non-positive
prior therefore means "no prior here".  Invalid pixels contribute nothing and get exact-zero gradients.  On valid pixels

    x = D / A   (space="depth": the expected depth of what was hit)   or   x = A / D   (space="inverse": the prior is an inverse
                                                                            depth, upstream's invdepthmap)
    w = m ;  n = sum w
    mode="l1":       r = x - (a*p + b) ;  L = sum w|r| / n                                  (sign(0) = 0; n <= 0: L = 0)
    mode="pearson":  L = 1 - rho ;  rho = C / sqrt(Vx*Vp) ;  Vx = sum w x^2 / n - (sum w x / n)^2, Vp likewise,
                     C = sum w x p / n - (sum w x / n)(sum w p / n)

A Pearson view with ``n <= 0``, ``Vx <= 1e-12 * sum w x^2 / n`` or ``Vp <= 1e-12 * sum w p^2 / n`` (no valid pixel, one valid pixel, a
constant prior) is degenerate: ``L = 0`` and all-zero gradients, never NaN.  ``x`` is formed in the dtype of the maps; every
product after it and every sum is float64, in the kernel and in ``depth_prior_loss_torch`` alike (a product of two float32 values
is exact in float64, which is what lets the ``1e-12`` test recognise a constant float32 prior).

``depth_prior_loss_torch`` is the function in plain PyTorch on any device and dtype.  ``depth_prior_loss`` is the HIP path: the V
views of a step in two launches forward and one (two with a table gradient) backward per 16 views, sums without atomics, so it
repeats bit for bit and a view's result does not depend on its neighbours.  ``DepthPriorBank`` is the ``(N,2)`` table as an
``nn.Module``.
"""
from __future__ import annotations

import ctypes as C
import torch

from . import _lib as L
from .pose_bank import _row_table, _rows

_OP = "depth_prior_loss"
MODES = {"pearson": L.DEPTH_PRIOR_PEARSON, "l1": L.DEPTH_PRIOR_L1}
SPACES = {"depth": L.DEPTH_PRIOR_DEPTH, "inverse": L.DEPTH_PRIOR_INVERSE}
DEGENERATE = 1e-12                                             # a variance at or below this share of its mean square is none


def _ptr_field(ts):
    """A pointer field of ``BagsDepthPrior``: the addresses of up to 16 tensors (None entries NULL), the rest NULL."""
    return L.ptr_table(list(ts) + [None] * (L.MAX_POSE_ROWS - len(ts)))


def _map_list(op: str, name: str, maps, like=None, optional=False):
    """``maps`` as a list of per-view tensors: one ``(H,W)`` / ``(1,H,W)`` tensor is one view, a sequence is V views (nothing is
    stacked or copied).  ``like``: the list the count and the pixel count must agree with.  ``optional``: None entries stay."""
    seq = [maps] if torch.is_tensor(maps) else list(maps)
    if not seq:
        raise ValueError(f"{op}: no {name}")
    for i, t in enumerate(seq):
        if t is None and optional:
            continue
        if not torch.is_tensor(t) or not (t.dim() == 2 or (t.dim() == 3 and t.shape[0] == 1)) or t.numel() < 1:
            raise ValueError(f"{op}: {name}[{i}] must be a non-empty (H,W) or (1,H,W) tensor"
                             + (f", got {tuple(t.shape)}" if torch.is_tensor(t) else f", got {type(t).__name__}"))
        if like is not None and tuple(t.shape[-2:]) != tuple(like[0].shape[-2:]):
            raise ValueError(f"{op}: {name}[{i}] is {tuple(t.shape)}, depth[0] is {tuple(like[0].shape)}: one size per call")
    if like is not None and len(seq) != len(like):
        raise ValueError(f"{op}: {len(like)} depth maps but {len(seq)} {name}")
    return seq


def _arguments(op: str, depth, weights, prior, mask, mode, space, table, rows):
    """The checks the HIP path and the PyTorch statement share: (depths, weights, priors, masks, rows or None)."""
    if mode not in MODES:
        raise ValueError(f"{op}: mode must be 'pearson' or 'l1', got {mode!r}")
    if space not in SPACES:
        raise ValueError(f"{op}: space must be 'depth' or 'inverse', got {space!r}")
    Ds = _map_list(op, "depth", depth)
    Ds = _map_list(op, "depth", Ds, like=Ds)
    As = _map_list(op, "weights", weights, like=Ds)
    ps = _map_list(op, "prior", prior, like=Ds)
    ms = [None] * len(Ds) if mask is None else _map_list(op, "mask", mask, like=Ds, optional=True)
    for i, m in enumerate(ms):
        if m is not None and m.dtype == torch.bool:
            raise TypeError(f"{op}: mask[{i}] is a bool tensor; the mask is a float pixel weight: pass mask.float()")
    if table is None:
        if rows is not None:
            raise ValueError(f"{op}: rows without a table")
        return Ds, As, ps, ms, None
    if mode == "pearson":
        raise ValueError(f"{op}: a table with mode='pearson': the correlation has no scale or shift to fit (table is for mode='l1')")
    if not torch.is_tensor(table) or table.dim() != 2 or table.shape[1] != 2 or table.shape[0] < 1:
        raise ValueError(f"{op}: table must be (N,2) with N >= 1")
    if rows is None:
        raise ValueError(f"{op}: a table needs rows: one row per view")
    rows = _rows(op, [rows] if isinstance(rows, int) else rows, table.shape[0])
    if len(rows) != len(Ds):
        raise ValueError(f"{op}: {len(Ds)} views but {len(rows)} rows")
    return Ds, As, ps, ms, rows


# ------------------------------------------------------------------------------------------------------------------ PyTorch
def depth_prior_loss_torch(depth, weights, prior, mask=None, *, mode="pearson", space="inverse", min_weight=0.5, table=None, rows=None):
    """The function of the module docstring in plain PyTorch, on the device and in the dtype of ``depth``; autograd gives its
    backward.  Arguments and result as ``depth_prior_loss``: ``(loss (V,), count (V,))`` in the dtype of ``depth``.  ``x`` is formed
    in that dtype, everything after it in float64, as the kernel does: in float64 this is the reference, in float32 the comparison
    path."""
    op = "depth_prior_loss_torch"
    Ds, As, ps, ms, rows = _arguments(op, depth, weights, prior, mask, mode, space, table, rows)
    H, W = Ds[0].shape[-2:]
    dt, dev = Ds[0].dtype, Ds[0].device
    D = torch.stack([t.reshape(H, W) for t in Ds])
    A = torch.stack([t.reshape(H, W) for t in As]).to(device=dev, dtype=dt)
    p = torch.stack([t.reshape(H, W) for t in ps]).to(device=dev, dtype=dt)
    m = torch.stack([torch.ones(H, W, dtype=dt, device=dev) if t is None else t.reshape(H, W).to(device=dev, dtype=dt) for t in ms])
    valid = (m > 0) & (A >= torch.as_tensor(min_weight, dtype=dt, device=dev)) & (D > 0) & (p > 0)
    one = torch.ones((), dtype=dt, device=dev)
    Dv, Av = torch.where(valid, D, one), torch.where(valid, A, one)            # an invalid pixel: x = 1, w = 0, zero gradients
    x = (Av / Dv if space == "inverse" else Dv / Av).double()
    pd = torch.where(valid, p, one).double()
    w = torch.where(valid, m, torch.zeros((), dtype=dt, device=dev)).double()
    n = w.sum((1, 2))
    some = n > 0
    inv_n = torch.where(some, 1.0 / torch.where(some, n, torch.ones_like(n)), torch.zeros_like(n))
    if mode == "l1":
        if table is None:
            r = x - pd
        else:
            ab = table[rows].to(device=dev).double()
            r = x - (ab[:, 0, None, None] * pd + ab[:, 1, None, None])
        loss = (w * r.abs()).sum((1, 2)) * inv_n
    else:
        wx, wp = w * x, w * pd
        mx, mp = wx.sum((1, 2)) * inv_n, wp.sum((1, 2)) * inv_n
        ex2, ep2 = (wx * x).sum((1, 2)) * inv_n, (wp * pd).sum((1, 2)) * inv_n
        Vx, Vp, Cxp = ex2 - mx * mx, ep2 - mp * mp, (wx * pd).sum((1, 2)) * inv_n - mx * mp
        live = some & (Vx > DEGENERATE * ex2) & (Vp > DEGENERATE * ep2)
        k1 = 1.0 / torch.sqrt(torch.where(live, Vx * Vp, torch.ones_like(n)))
        loss = torch.where(live, 1.0 - Cxp * k1, torch.zeros_like(n))
    return loss.to(dt), n.detach().to(dt)


# ------------------------------------------------------------------------------------------------------------------ HIP
class _DepthPrior(torch.autograd.Function):
    """``maps``: V depth maps, V weights maps, V priors, V masks (any of the masks None), as separate tensors: nothing is stacked."""

    @staticmethod
    def forward(ctx, table, rows, mode, space, min_weight, V, *maps):
        depths, weights, priors, masks = (list(maps[k * V:(k + 1) * V]) for k in range(4))
        dev, (H, W) = depths[0].device, depths[0].shape[-2:]
        loss = torch.empty(V, dtype=torch.float32, device=dev)
        count = torch.empty(V, dtype=torch.float32, device=dev)
        stats = torch.empty(V, L.DEPTH_PRIOR_STATS, dtype=torch.float64, device=dev)
        ws = L.workspace(L.load().bags_depth_prior_workspace_size(min(V, L.MAX_POSE_ROWS), H, W), dev)
        N = 0 if table is None else table.shape[0]
        structs = []
        for b in range(0, V, L.MAX_POSE_ROWS):
            part = slice(b, b + L.MAX_POSE_ROWS)
            n = len(depths[part])
            args = L.BagsDepthPrior(mode, space, H, W, min_weight, n, N, 0, L.ptr(table),
                                    _row_table(rows[part]) if rows is not None else (C.c_int32 * L.MAX_POSE_ROWS)(),
                                    _ptr_field(depths[part]), _ptr_field(weights[part]), _ptr_field(priors[part]), _ptr_field(masks[part]))
            L.call("bags_depth_prior_forward", dev, C.byref(args), L.ptr(ws), ws.numel(), loss[part].data_ptr(), count[part].data_ptr(),
                   stats[part].data_ptr())
            structs.append(args)
        ctx.mark_non_differentiable(count)
        if any(ctx.needs_input_grad):                          # nothing is kept under no_grad or for constant inputs
            ctx.save_for_backward(stats, table, *maps)         # versions are checked at backward: the adjoint re-reads the maps
            ctx.structs, ctx.V = structs, V
        return loss, count

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss, _g_count):
        stats, table, *maps = ctx.saved_tensors                # raises if a map or the table was written in place since the forward
        V, need = ctx.V, ctx.needs_input_grad
        dev = stats.device
        g = L.as_f32c(g_loss)
        g_depth = [torch.empty_like(t) if need[6 + i] else None for i, t in enumerate(maps[:V])]
        g_weights = [torch.empty_like(t) if need[6 + V + i] else None for i, t in enumerate(maps[V:2 * V])]
        g_table = None
        for k, args in enumerate(ctx.structs):
            part = slice(k * L.MAX_POSE_ROWS, (k + 1) * L.MAX_POSE_ROWS)
            # every element of the (N,2) gradient is written by the kernel: no fill launch; a further batch is added to the first
            g_part = torch.empty_like(table) if need[0] else None
            L.call("bags_depth_prior_backward", dev, C.byref(args), stats[part].data_ptr(), g[part].data_ptr(),
                   L.ptr_table(g_depth[part]), L.ptr_table(g_weights[part]), L.ptr(g_part))
            if g_part is not None:
                g_table = g_part if g_table is None else g_table.add_(g_part)
        return (g_table, None, None, None, None, None, *g_depth, *g_weights, *([None] * (2 * V)))


def depth_prior_loss(depth, weights, prior, mask=None, *, mode="pearson", space="inverse", min_weight=0.5, table=None, rows=None):
    """The depth prior of the module docstring on an AMD GPU: ``(loss (V,), count (V,))``, ``count[v] = n`` of view v.

    ``depth`` and ``weights`` are the operator's maps ``(1,H,W)`` of one view, or sequences of V of them -- the ``"depth"`` and
    ``"weights"`` entries of what ``render_views`` returns go in as they are, nothing is stacked or copied; ``prior`` and ``mask``
    are ``(H,W)`` or ``(1,H,W)`` per view (``mask=None``, or a None entry: every pixel weighs 1).  float32, contiguous tensors on
    one device; a bool mask raises (pass ``mask.float()``).  ``mode="l1"`` takes the per-image ``(a, b)`` of ``table`` ``(N,2)`` at
    the distinct ``rows`` (one per view; no table: ``(1, 0)``); ``mode="pearson"`` takes no table.  Two HIP launches forward and
    one backward (two with a table gradient) per 16 views.  Differentiable in ``depth``, ``weights`` and, for ``l1``, ``table``
    (dense, rows not listed exact zeros); ``count`` is not differentiable.  The backward re-reads the maps and the table: writing
    one of them in place between forward and backward raises."""
    Ds, As, ps, ms, rows = _arguments(_OP, depth, weights, prior, mask, mode, space, table, rows)
    host = ": bags_raster.depth_prior_loss_torch is the same function in PyTorch on any device and dtype"
    L.require(_OP, "depth[0]", Ds[0], gpu=True, f32=True, contiguous=True, host=host)
    for name, ts in (("depth", Ds), ("weights", As), ("prior", ps), ("mask", ms)):
        for i, t in enumerate(ts):
            if t is not None:
                L.require(_OP, f"{name}[{i}]", t, gpu=True, f32=True, contiguous=True, on=Ds[0], host=host)
    if table is not None:
        L.require(_OP, "table", table, gpu=True, f32=True, contiguous=True, on=Ds[0], host=host)
    H, W = Ds[0].shape[-2:]
    if H * W >= 2 ** 31:
        raise ValueError(f"{_OP}: a map of {W}x{H} has 2^31 pixels or more")
    return _DepthPrior.apply(table, rows, MODES[mode], SPACES[space], float(min_weight), len(Ds), *Ds, *As, *ps, *ms)


class DepthPriorBank(torch.nn.Module):
    """Upstream 3DGS's per-image ``depth_params`` for N training images as one parameter ``table`` ``(N,2)``: row i is the scale
    and offset ``(a, b)`` that bring image i's prior to the scene's units, initialised to ``(1, 0)``.  Upstream fits them once from
    the SfM points and keeps them fixed; here they may also train, with ONE ``torch.optim.Adam([bank.table], lr=...)``: a step's
    backward leaves a dense gradient whose unlisted rows are exact zeros."""

    def __init__(self, N: int, device="cpu"):
        super().__init__()
        if int(N) < 1:
            raise ValueError("DepthPriorBank: no images")
        self.table = torch.nn.Parameter(torch.tensor((1.0, 0.0), dtype=torch.float32, device=torch.device(device)).repeat(int(N), 1))

    def __len__(self) -> int:
        return self.table.shape[0]

    def loss(self, depth, weights, prior, rows, mask=None, *, mode="l1", space="inverse", min_weight=0.5):
        """``depth_prior_loss`` of the views ``rows`` with their rows of the table (``mode="pearson"`` does not read it): the HIP
        path where the table is on a GPU, ``depth_prior_loss_torch`` on the host."""
        rows = _rows("DepthPriorBank.loss", [rows] if isinstance(rows, int) else rows, len(self))
        fn = depth_prior_loss if self.table.is_cuda else depth_prior_loss_torch
        if mode == "pearson":
            return fn(depth, weights, prior, mask, mode=mode, space=space, min_weight=min_weight)
        return fn(depth, weights, prior, mask, mode=mode, space=space, min_weight=min_weight, table=self.table, rows=rows)
