"""BilateralGridBank -- per-image bilateral-grid colour on the rendered image, behind ``AppearanceBank`` and in front of the loss
(csrc/bilagrid.hip).

``AppearanceBank`` covers what is global per image: one exposure matrix and a radial falloff.  Auto-exposure, auto white balance,
local tone mapping and shadows vary over the image and with brightness; current splatting trainers explain them with a bilateral
grid per training image and a total-variation regulariser on the grids (gsplat's ``lib_bilagrid``, ``--use_bilateral_grid``).
What the appearance model cannot absorb, a bundle-adjusting optimiser pays for with geometry and pose.

Per image there is a grid ``G`` ``(12, L, Gy, Gx)`` in gsplat's layout: coefficient ``k = 4*c + j`` of a vertex is entry ``[c][j]``
of a 3x4 affine matrix, and the neutral grid is ``[I | 0]`` at every vertex.  For pixel ``(x, y)`` of a ``(3,H,W)`` image with
channels ``p_0..p_2``:

    u = (x + 0.5) / W * (Gx - 1)      x0 = min(floor(u), Gx-1)   x1 = min(x0+1, Gx-1)   tx = u - x0      (v, y0, y1, ty likewise)
    luma = 0.299 p_0 + 0.587 p_1 + 0.114 p_2
    s = luma * (L - 1);  w = clamp(s, 0, L-1);  z0 = min(floor(w), L-1);  z1 = min(z0+1, L-1);  tz = w - z0
    lerp(a, b, t) = a + t * (b - a)
    plane(z) = lerp( lerp(G[k,z,y0,x0], G[k,z,y0,x1], tx), lerp(G[k,z,y1,x0], G[k,z,y1,x1], tx), ty )
    A[k] = lerp(plane(z0), plane(z1), tz)                                   k = 0..11
    out_c = A[4c] p_0 + A[4c+1] p_1 + A[4c+2] p_2 + A[4c+3]

This is the published ``F.grid_sample(mode="bilinear", align_corners=True, padding_mode="border")`` over coordinates
``((x+0.5)/W - 0.5)*2`` and ``luma*2 - 1`` followed by the affine ``matmul``, in its ``lerp`` form: in that form the neutral grid
returns a finite float32 image bit for bit, which ``grid_sample``'s weight form does not.  The gradients go to the image and to
``G``; the image gets the direct term ``sum_c g_c A[4c+j]`` and the term through the guidance, ``dL/dtz * (L-1) * (0.299, 0.587,
0.114)``, which is exactly zero where ``s <= 0`` or ``s >= L-1`` (the border rule); nothing flows to ``u`` or ``v``.

The total variation of grids ``X`` ``(N,12,L,Gy,Gx)`` is gsplat's ``total_variation_loss``: per grid axis ``d`` with ``n_d >= 2``
the sum of the squared forward differences along ``d`` over ``12 * (n_d - 1) *`` the product of the other two sizes, the three terms
added and divided by ``N``; an axis of one vertex counts 0 (upstream divides 0 by 0 there).

``bilagrid_torch`` / ``bilagrid_tv_loss_torch`` are these statements in PyTorch on any device and dtype.  ``apply_bilagrid`` /
``bilagrid_tv_loss`` are the HIP paths; ``BilateralGridBank`` is the grids as an ``nn.Module``.
"""
from __future__ import annotations

import ctypes as C
import torch

from . import _lib as L
from .appearance import _image_list, _ptr_field
from .pose_bank import _row_table, _rows

_OP = "apply_bilagrid"
_HOST = ": bags_raster.bilagrid_torch is the same function in PyTorch on any device and dtype"
LUMA = (0.299, 0.587, 0.114)


def _check_grid_shape(op: str, grids, lead: int):
    """``grids`` is (..., 12, L, Gy, Gx) with ``lead`` leading dimensions; returns (Gx, Gy, L)."""
    if grids.dim() != lead + 4 or grids.shape[lead] != 12 or min(grids.shape) < 1:
        raise ValueError(f"{op}: grids must be ({'N,' * lead}12,L,Gy,Gx) with every size >= 1, got {tuple(grids.shape)}")
    return int(grids.shape[-1]), int(grids.shape[-2]), int(grids.shape[-3])


def _supported(op: str, Gx: int, Gy: int, Lz: int, torch_name: str):
    if not (1 <= Gx <= L.BILAGRID_MAX_G and 1 <= Gy <= L.BILAGRID_MAX_G and 1 <= Lz <= L.BILAGRID_MAX_L):
        raise ValueError(f"{op}: grid (Gx, Gy, L) = ({Gx}, {Gy}, {Lz}) is outside 1..{L.BILAGRID_MAX_G}, 1..{L.BILAGRID_MAX_G}, "
                         f"1..{L.BILAGRID_MAX_L}: bags_raster.{torch_name} is the same function in PyTorch for any size")


# ------------------------------------------------------------------------------------------------------------------ PyTorch
def _axis(n: int, G: int, dt, dev):
    """(i0, i1, t) of the n pixel centres along an axis of G vertices."""
    u = (torch.arange(n, dtype=dt, device=dev) + 0.5) / n * (G - 1)
    i0 = u.floor().clamp(max=G - 1)
    return i0.long(), (i0.long() + 1).clamp(max=G - 1), u - i0


def _lerp(a, b, t):
    return a + t * (b - a)


def _planes(img, G):
    """``(plane(z0), plane(z1), tz, live)`` per pixel, ``(V,12,H,W)`` twice, ``(V,1,H,W)`` and ``(V,H,W)``, of images ``(V,3,H,W)`` and
    grids ``(V,12,L,Gy,Gx)`` of one dtype and device; ``live``: ``0 < s < L-1``, where ``tz`` follows the pixel."""
    V, _, H, W = img.shape
    Lz, Gy, Gx = G.shape[2:]
    dt, dev = img.dtype, img.device
    x0, x1, tx = _axis(W, Gx, dt, dev)
    y0, y1, ty = _axis(H, Gy, dt, dev)
    luma = LUMA[0] * img[:, 0] + LUMA[1] * img[:, 1] + LUMA[2] * img[:, 2]            # (V,H,W)
    s = luma * (Lz - 1)
    w = s.clamp(0, Lz - 1)
    live = (s > 0) & (s < Lz - 1)                                                      # torch.clamp passes a gradient AT its bounds:
    w = torch.where(live, w, w.detach())                                               # the border rule does not
    z0 = w.detach().floor().clamp(max=Lz - 1)
    tz = (w - z0)[:, None]                                                             # (V,1,H,W)
    z0 = z0.long()
    z1 = (z0 + 1).clamp(max=Lz - 1)
    vi = torch.arange(V, device=dev)[:, None, None]
    tx, ty = tx[None, None, None, :], ty[None, None, :, None]

    def at(z, yy, xx):                                                                 # G[v, :, z, y, x] per pixel -> (V,12,H,W)
        return G[vi, :, z, yy[None, :, None], xx[None, None, :]].permute(0, 3, 1, 2)

    def plane(z):
        return _lerp(_lerp(at(z, y0, x0), at(z, y0, x1), tx), _lerp(at(z, y1, x0), at(z, y1, x1), tx), ty)

    return plane(z0), plane(z1), tz, live


def _affine(img, G):
    """The per-pixel coefficients ``A`` ``(V,12,H,W)``."""
    P0, P1, tz, _ = _planes(img, G)
    return _lerp(P0, P1, tz)


def _torch_args(op: str, images, grids_rows):
    imgs, kind = _image_list(op, images)
    img = imgs[0].unsqueeze(0) if kind == "one" else (images if kind == "stack" else torch.stack(imgs))
    G = grids_rows.to(device=img.device, dtype=img.dtype)
    if G.dim() == 4:
        G = G.unsqueeze(0)
    _check_grid_shape(op, G, 1)
    if G.shape[0] != img.shape[0]:
        raise ValueError(f"{op}: {img.shape[0]} images but {G.shape[0]} grids")
    return img, G, kind


def bilagrid_torch(images, grids_rows):
    """The function of the module docstring in plain PyTorch, on the device and in the dtype of the images; autograd gives its
    backward.  ``images``: ``(3,H,W)`` with ``grids_rows`` ``(12,L,Gy,Gx)``, or ``(V,3,H,W)`` / a sequence of V ``(3,H,W)`` tensors
    with ``grids_rows`` ``(V,12,L,Gy,Gx)``; the result has the form of ``images`` (a list for a sequence).  Any grid size.  The
    operations are the kernel's in the kernel's order."""
    img, G, kind = _torch_args("bilagrid_torch", images, grids_rows)
    A = _affine(img, G)
    out = torch.stack([A[:, 4 * c] * img[:, 0] + A[:, 4 * c + 1] * img[:, 1] + A[:, 4 * c + 2] * img[:, 2] + A[:, 4 * c + 3] for c in range(3)], dim=1)
    if kind == "one":
        return out[0]
    return out if kind == "stack" else list(out.unbind(0))


def bilagrid_tv_loss_torch(grids):
    """The total variation of ``grids`` ``(N,12,L,Gy,Gx)`` (module docstring) in plain PyTorch: a scalar of the grids' dtype."""
    _check_grid_shape("bilagrid_tv_loss_torch", grids, 1)
    N, _, Lz, Gy, Gx = grids.shape
    total = grids.new_zeros(())
    for dim, n, others in ((4, Gx, Gy * Lz), (3, Gy, Gx * Lz), (2, Lz, Gx * Gy)):
        if n >= 2:
            d = grids.narrow(dim, 1, n - 1) - grids.narrow(dim, 0, n - 1)
            total = total + (d * d).sum() / (12 * (n - 1) * others)
    return total / N


# ------------------------------------------------------------------------------------------------------------------ HIP
class _Bilagrid(torch.autograd.Function):
    """``imgs``: the V images as separate tensors (stacked == False; V outputs), or one (V,3,H,W) tensor whose rows are the
    images (stacked == True; one output): no image, output or gradient is copied or stacked either way."""

    @staticmethod
    def _args(grids, rows, H, W, path, views, outs=None):
        N, _, Lz, Gy, Gx = grids.shape
        return L.BagsBilagrid(N, L.ptr(grids), len(rows), _row_table(rows), 3, H, W, Gx, Gy, Lz, path, _ptr_field(views),
                              _ptr_field(outs if outs is not None else []))

    @staticmethod
    def forward(ctx, grids, rows, path, stacked, *imgs):
        views = list(imgs[0].unbind(0)) if stacked else list(imgs)
        dev, (_, H, W) = grids.device, views[0].shape
        if stacked:
            out = torch.empty_like(imgs[0])
            outs = list(out.unbind(0))
        else:
            outs = [torch.empty_like(t) for t in views]
        for b in range(0, len(views), L.MAX_POSE_ROWS):
            part = slice(b, b + L.MAX_POSE_ROWS)
            args = _Bilagrid._args(grids, rows[part], H, W, path, views[part], outs[part])
            L.call("bags_bilagrid_forward", dev, C.byref(args))
        if any(ctx.needs_input_grad):                          # nothing is kept under no_grad or for constant inputs
            ctx.save_for_backward(grids, *imgs)                # versions are checked at backward: the adjoint re-reads both
            ctx.rows, ctx.path, ctx.stacked = rows, path, stacked
        return out if stacked else tuple(outs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *g_outs):
        grids, *imgs = ctx.saved_tensors                       # raises if the grids were stepped in place since the forward
        rows, path, stacked = ctx.rows, ctx.path, ctx.stacked
        need = ctx.needs_input_grad
        dev = grids.device
        if stacked:
            views, gs = list(imgs[0].unbind(0)), list(L.as_f32c(g_outs[0]).unbind(0))
            g_stack = torch.empty_like(imgs[0]) if need[4] else None
            g_imgs = list(g_stack.unbind(0)) if need[4] else [None] * len(views)
        else:
            views, gs = list(imgs), [L.as_f32c(g) for g in g_outs]
            g_imgs = [torch.empty_like(t) if n else None for t, n in zip(views, need[4:])]
        _, H, W = views[0].shape
        g_grids = None
        for b in range(0, len(views), L.MAX_POSE_ROWS):
            part = slice(b, b + L.MAX_POSE_ROWS)
            args = _Bilagrid._args(grids, rows[part], H, W, path, views[part])
            # every element of the dense gradient is written by the kernel: no fill launch; a further batch is added to the first
            g_part = torch.empty_like(grids) if need[0] else None
            ws = L.workspace(L.load().bags_bilagrid_workspace_size(len(rows[part]), H, W) if need[0] else 0, dev)
            want_images = any(g is not None for g in g_imgs[part])
            L.call("bags_bilagrid_backward", dev, C.byref(args), L.ptr_table(gs[part]), L.ptr(ws) if ws.numel() else None, ws.numel(),
                   L.ptr_table(g_imgs[part]) if want_images else None, L.ptr(g_part))
            if g_part is not None:
                g_grids = g_part if g_grids is None else g_grids.add_(g_part)
        return (g_grids, None, None, None, *((g_stack,) if stacked else g_imgs))


def apply_bilagrid(images, grids, rows, path=L.BILAGRID_PATH_AUTO):
    """``images`` through the grids ``rows`` of ``grids`` ``(N,12,L,Gy,Gx)`` on an AMD GPU: image i through grid ``rows[i]``.

    ``images`` is one ``(3,H,W)`` tensor, a ``(V,3,H,W)`` tensor, or a sequence of V ``(3,H,W)`` tensors of one size -- what
    ``render_views`` returns goes in as it is, nothing is stacked or copied; the result has the same form (a tuple for a sequence).
    float32, contiguous tensors on the grids' device; ``rows`` distinct ints in [0, N); ``1 <= Gx, Gy <= 64``, ``1 <= L <= 16``.
    One HIP launch forward and two backward per 16 images.  Differentiable in the images and the grids; ``grids.grad`` is dense,
    rows not listed and vertices no pixel reaches are exact zeros, and the sums behind it use no atomics: a repeated backward gives
    the same bits.  The backward re-reads the grids: an in-place optimizer step between forward and backward raises.  ``path``:
    ``_lib.BILAGRID_PATH_DIRECT`` makes every tile read the grid directly instead of staging it in LDS (same bits; for tests)."""
    imgs, kind = _image_list(_OP, images)
    L.require(_OP, "grids", grids, gpu=True, f32=True, contiguous=True, host=_HOST)
    Gx, Gy, Lz = _check_grid_shape(_OP, grids, 1)
    _supported(_OP, Gx, Gy, Lz, "bilagrid_torch")
    if kind == "stack":
        L.require(_OP, "images", images, gpu=True, f32=True, contiguous=True, on=grids, host=_HOST)
    else:
        for i, t in enumerate(imgs):
            L.require(_OP, f"images[{i}]", t, gpu=True, f32=True, contiguous=True, on=grids, host=_HOST)
    rows = _rows(_OP, [rows] if isinstance(rows, int) else rows, grids.shape[0])
    if len(rows) != len(imgs):
        raise ValueError(f"{_OP}: {len(imgs)} images but {len(rows)} rows")
    _, H, W = imgs[0].shape
    if H * W >= 2 ** 31:
        raise ValueError(f"{_OP}: an image of {W}x{H} has 2^31 pixels or more: bags_raster.bilagrid_torch is the same function in PyTorch")
    if kind == "stack":
        return _Bilagrid.apply(grids, rows, int(path), True, images)
    out = _Bilagrid.apply(grids, rows, int(path), False, *imgs)
    return out[0] if kind == "one" else out


class _BilagridTV(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grids):
        N, _, Lz, Gy, Gx = grids.shape
        dev = grids.device
        loss = torch.empty((), dtype=torch.float32, device=dev)
        ws = L.workspace(L.load().bags_bilagrid_tv_workspace_size(N, Gx, Gy, Lz), dev)
        L.call("bags_bilagrid_tv_forward", dev, L.ptr(grids), N, Gx, Gy, Lz, L.ptr(ws), ws.numel(), L.ptr(loss))
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(grids)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss):
        (grids,) = ctx.saved_tensors
        N, _, Lz, Gy, Gx = grids.shape
        g_grids = torch.empty_like(grids)
        L.call("bags_bilagrid_tv_backward", grids.device, L.ptr(grids), N, Gx, Gy, Lz, L.ptr(L.as_f32c(g_loss)), L.ptr(g_grids))
        return g_grids


def bilagrid_tv_loss(grids):
    """The total variation of ``grids`` ``(N,12,L,Gy,Gx)`` (module docstring) on an AMD GPU: a float32 scalar.  Two HIP launches
    forward (partial sums in double in a fixed order, then the scalar), one backward (a gather: every element of the gradient is
    written once); no atomics, so value and gradient repeat bit for bit."""
    op = "bilagrid_tv_loss"
    L.require(op, "grids", grids, gpu=True, f32=True, contiguous=True,
              host=": bags_raster.bilagrid_tv_loss_torch is the same function in PyTorch on any device and dtype")
    Gx, Gy, Lz = _check_grid_shape(op, grids, 1)
    _supported(op, Gx, Gy, Lz, "bilagrid_tv_loss_torch")
    return _BilagridTV.apply(grids)


class BilateralGridBank(torch.nn.Module):
    """The bilateral grids of N training images: one parameter ``grids`` ``(N,12,L,Gy,Gx)`` -- gsplat's name and layout, so a
    trained tensor loads as it is -- every vertex initialised to the neutral matrix ``[I | 0]``.  ``grid = (Gx, Gy, L)``.

    The optimizer is upstream's: one ``torch.optim.Adam([bank.grids], lr=...)`` over the whole tensor.  A step's backward leaves a
    dense gradient whose unlisted rows are zeros, so that optimizer is a single fused step with no fill launch; the total variation
    of a neutral row has zero gradient, so such a row stays neutral bit for bit until its image is seen.  (A per-camera Adam is
    not offered.)"""

    def __init__(self, N: int, grid=(16, 16, 8), device="cpu"):
        super().__init__()
        if int(N) < 1:
            raise ValueError("BilateralGridBank: no cameras")
        Gx, Gy, Lz = (int(g) for g in grid)
        if min(Gx, Gy, Lz) < 1:
            raise ValueError(f"BilateralGridBank: grid (Gx, Gy, L) = ({Gx}, {Gy}, {Lz}) must be >= 1 each")
        neutral = torch.eye(3, 4, dtype=torch.float32, device=torch.device(device)).reshape(1, 12, 1, 1, 1)
        self.grids = torch.nn.Parameter(neutral.repeat(int(N), 1, Lz, Gy, Gx))

    def __len__(self) -> int:
        return self.grids.shape[0]

    def _on_my_device(self, op: str, images):
        imgs, _ = _image_list(op, images)
        for i, t in enumerate(imgs):
            if t.device != self.grids.device:
                raise RuntimeError(f"{op}: the grids are on {self.grids.device} but images[{i}] is on {t.device}: nothing is copied between "
                                   f"devices (a bank on an AMD GPU runs apply_bilagrid, a bank on the host bilagrid_torch)")

    def apply(self, images, rows):                             # (shadows nn.Module.apply, which nothing here uses)
        """``images`` (as ``apply_bilagrid`` takes them) through the grids ``rows``: the HIP path where the grids are on a GPU,
        ``bilagrid_torch`` on the host.  Images on another device than the grids are refused, not copied."""
        self._on_my_device("BilateralGridBank.apply", images)
        if self.grids.is_cuda:
            return apply_bilagrid(images, self.grids, rows)
        rows = _rows("BilateralGridBank.apply", [rows] if isinstance(rows, int) else rows, len(self))
        return bilagrid_torch(images, self.grids[rows])

    def tv_loss(self):
        """The total variation of the grids: ``bilagrid_tv_loss`` on a GPU, ``bilagrid_tv_loss_torch`` on the host.  gsplat
        weighs it with 10."""
        return bilagrid_tv_loss(self.grids) if self.grids.is_cuda else bilagrid_tv_loss_torch(self.grids)

    def affine(self, images, rows):
        """The per-pixel 3x4 matrices the images ``(V,3,H,W)`` / ``(3,H,W)`` select from the grids ``rows``, for viewers:
        ``(V,3,4,H,W)`` / ``(3,4,H,W)``, through the PyTorch path on the grids' device."""
        self._on_my_device("BilateralGridBank.affine", images)
        rows = _rows("BilateralGridBank.affine", [rows] if isinstance(rows, int) else rows, len(self))
        img, G, kind = _torch_args("BilateralGridBank.affine", images, self.grids[rows])
        A = _affine(img, G)
        A = A.reshape(A.shape[0], 3, 4, *A.shape[2:])
        return A[0] if kind == "one" else A
