"""AppearanceBank -- per-camera exposure and lens vignetting on the rendered image, in front of the loss (csrc/appearance.hip).

Upstream 3DGS trains a 3x4 exposure matrix per training image and multiplies the render by it before the loss; the reference
trains a vignetting model on the rendered image.  Without either, a bundle-adjusting optimiser
explains brightness differences between frames with geometry and pose.  Here both are one function of a ``(3,H,W)`` image and one
row of an ``(N,16)`` table -- columns 0..11 the exposure matrix ``E`` ``(3,4)`` row-major, 12..14 the vignetting coefficients
``k1 k2 k3``, 15 unused.  For pixel ``(x, y)`` with channels ``p_0..p_2``, centre ``(cx, cy)`` in pixels and
``s2 = (W*W + H*H) / 4``:

    dx = x + 0.5 - cx ; dy = y + 0.5 - cy ; r2 = (dx*dx + dy*dy) / s2        (0 at the centre, 1 at a corner)
    f  = 1 + r2*(k1 + r2*(k2 + r2*k3))                                        (lens falloff, an even radial polynomial)
    q_k = f * p_k
    out_c = q_0*E[0][c] + q_1*E[1][c] + q_2*E[2][c] + E[c][3]                 (upstream: image^T @ E[:3,:3] + E[:3,3])

Vignetting comes first because lens falloff comes before sensor gain.  The neutral row ``E = [I | 0]``, ``k = 0`` returns its
input bit for bit.  The step belongs after ``resample_image`` / ``resample_faces``, in sensor coordinates, so ``render()`` and
``render_views()`` do not apply it.

``appearance_torch`` is the function in plain PyTorch on any device and dtype.  ``apply_appearance`` is the HIP path: the V
images of a step in ONE launch forward and two backward, 16 per launch; the backward writes the dense ``(N,16)`` gradient itself,
rows that were not listed as exact zeros, sums without atomics, so it repeats bit for bit.  ``AppearanceBank`` is the table as an
``nn.Module``.
"""
from __future__ import annotations

import ctypes as C
import torch

from . import _lib as L
from .pose_bank import _row_table, _rows

_OP = "apply_appearance"
ROW = 16                                                       # floats per table row
NEUTRAL = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0)


def _ptr_field(ts):
    """The ``image`` / ``out`` field of ``BagsAppearance``: the addresses of up to 16 tensors, the rest NULL."""
    return L.ptr_table(list(ts) + [None] * (L.MAX_POSE_ROWS - len(ts)))


def _center(center, H: int, W: int):
    """(cx, cy) in pixels; None is the image centre (W/2, H/2)."""
    if center is None:
        return 0.5 * W, 0.5 * H
    cx, cy = center
    return float(cx), float(cy)


def _image_list(op: str, images):
    """``images`` as (list of (3,H,W) tensors, kind): kind is "one" for a (3,H,W) tensor, "stack" for (V,3,H,W), "seq" for a
    sequence.  The rows of a stack are views, never copies."""
    if torch.is_tensor(images):
        if images.dim() == 3:
            imgs, kind = [images], "one"
        elif images.dim() == 4:
            imgs, kind = list(images.unbind(0)), "stack"
        else:
            raise ValueError(f"{op}: images must be (3,H,W) or (V,3,H,W), got {tuple(images.shape)}")
    else:
        imgs, kind = list(images), "seq"
        for i, t in enumerate(imgs):
            if not torch.is_tensor(t) or t.dim() != 3:
                raise ValueError(f"{op}: images[{i}] must be a (3,H,W) tensor")
    if not imgs:
        raise ValueError(f"{op}: no images")
    for i, t in enumerate(imgs):
        if t.shape[0] != 3 or t.shape[1] < 1 or t.shape[2] < 1:
            raise ValueError(f"{op}: images[{i}] must be (3,H,W) with H, W >= 1, got {tuple(t.shape)}")
        if t.shape != imgs[0].shape:
            raise ValueError(f"{op}: images[{i}] is {tuple(t.shape)}, images[0] is {tuple(imgs[0].shape)}: one size per call")
    return imgs, kind


# ------------------------------------------------------------------------------------------------------------------ PyTorch
def appearance_torch(images, table_rows, center=None):
    """The function of the module docstring in plain PyTorch, on the device and in the dtype of the images; autograd gives its
    backward.  ``images``: ``(3,H,W)`` with ``table_rows`` ``(16,)``, or ``(V,3,H,W)`` / a sequence of V ``(3,H,W)`` tensors with
    ``table_rows`` ``(V,16)``; the result has the form of ``images`` (a list for a sequence).  ``center = (cx, cy)`` in pixels,
    None for the image centre.  The operations are the kernel's in the kernel's order."""
    op = "appearance_torch"
    imgs, kind = _image_list(op, images)
    img = imgs[0].unsqueeze(0) if kind == "one" else (images if kind == "stack" else torch.stack(imgs))
    V, _, H, W = img.shape
    dt, dev = img.dtype, img.device
    rows = table_rows.to(device=dev, dtype=dt).reshape(-1, ROW)
    if rows.shape[0] != V:
        raise ValueError(f"{op}: {V} images but {rows.shape[0]} table rows")
    cx, cy = _center(center, H, W)
    s2 = torch.as_tensor((W * W + H * H) / 4.0, dtype=dt, device=dev)
    dx = (torch.arange(W, dtype=dt, device=dev) + 0.5) - cx
    dy = (torch.arange(H, dtype=dt, device=dev) + 0.5) - cy
    r2 = ((dx * dx)[None, :] + (dy * dy)[:, None]) / s2                               # (H,W)
    E = rows[:, :12].reshape(V, 3, 4)
    k = rows[:, 12:15].reshape(V, 3, 1, 1)
    f = 1.0 + r2 * (k[:, 0] + r2 * (k[:, 1] + r2 * k[:, 2]))                          # (V,H,W)
    q = f[:, None] * img                                                              # (V,3,H,W)
    e = lambda a, b: E[:, a, b].reshape(V, 1, 1)                                      # noqa: E731
    out = torch.stack([q[:, 0] * e(0, c) + q[:, 1] * e(1, c) + q[:, 2] * e(2, c) + e(c, 3) for c in range(3)], dim=1)
    if kind == "one":
        return out[0]
    return out if kind == "stack" else list(out.unbind(0))


# ------------------------------------------------------------------------------------------------------------------ HIP
class _Appearance(torch.autograd.Function):
    """``imgs``: the V images as separate tensors (stacked == False; V outputs), or one (V,3,H,W) tensor whose rows are the
    images (stacked == True; one output): no image, output or gradient is copied or stacked either way."""

    @staticmethod
    def forward(ctx, table, rows, cx, cy, stacked, *imgs):
        views = list(imgs[0].unbind(0)) if stacked else list(imgs)
        dev, (_, H, W) = table.device, views[0].shape
        if stacked:
            out = torch.empty_like(imgs[0])
            outs = list(out.unbind(0))
        else:
            outs = [torch.empty_like(t) for t in views]
        for b in range(0, len(views), L.MAX_POSE_ROWS):
            part = slice(b, b + L.MAX_POSE_ROWS)
            args = L.BagsAppearance(table.shape[0], table.data_ptr(), len(rows[part]), _row_table(rows[part]), 3, H, W, cx, cy,
                                    _ptr_field(views[part]), _ptr_field(outs[part]))
            L.call("bags_appearance_forward", dev, C.byref(args))
        if any(ctx.needs_input_grad):                          # nothing is kept under no_grad or for constant inputs
            ctx.save_for_backward(table, *imgs)                # versions are checked at backward: the adjoint re-reads both
            ctx.rows, ctx.center, ctx.stacked = rows, (cx, cy), stacked
        return out if stacked else tuple(outs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *g_outs):
        table, *imgs = ctx.saved_tensors                       # raises if the table was stepped in place since the forward
        rows, (cx, cy), stacked = ctx.rows, ctx.center, ctx.stacked
        need = ctx.needs_input_grad
        dev = table.device
        if stacked:
            views, gs = list(imgs[0].unbind(0)), list(L.as_f32c(g_outs[0]).unbind(0))
            g_stack = torch.empty_like(imgs[0]) if need[5] else None
            g_imgs = list(g_stack.unbind(0)) if need[5] else [None] * len(views)
        else:
            views, gs = list(imgs), [L.as_f32c(g) for g in g_outs]
            g_imgs = [torch.empty_like(t) if n else None for t, n in zip(views, need[5:])]
        _, H, W = views[0].shape
        g_table = None
        for b in range(0, len(views), L.MAX_POSE_ROWS):
            part = slice(b, b + L.MAX_POSE_ROWS)
            n = len(rows[part])
            args = L.BagsAppearance(table.shape[0], table.data_ptr(), n, _row_table(rows[part]), 3, H, W, cx, cy, _ptr_field(views[part]))
            # every element of the (N,16) gradient is written by the kernel: no fill launch; a further batch is added to the first
            g_part = torch.empty_like(table) if need[0] else None
            ws = L.workspace(L.load().bags_appearance_workspace_size(n, H, W) if need[0] else 0, dev)
            want_images = any(g is not None for g in g_imgs[part])
            L.call("bags_appearance_backward", dev, C.byref(args), L.ptr_table(gs[part]), L.ptr(ws) if need[0] else None, ws.numel(),
                   L.ptr_table(g_imgs[part]) if want_images else None, L.ptr(g_part))
            if g_part is not None:
                g_table = g_part if g_table is None else g_table.add_(g_part)
        return (g_table, None, None, None, None, *((g_stack,) if stacked else g_imgs))


def apply_appearance(images, table, rows, center=None):
    """``images`` through the rows ``rows`` of ``table`` ``(N,16)`` on an AMD GPU: image i through row ``rows[i]``.

    ``images`` is one ``(3,H,W)`` tensor, a ``(V,3,H,W)`` tensor, or a sequence of V ``(3,H,W)`` tensors of one size -- what
    ``render_views`` returns goes in as it is, nothing is stacked; the result has the same form (a tuple for a sequence).  float32,
    contiguous tensors on the table's device; ``rows`` distinct ints in [0, N); ``center = (cx, cy)`` in pixels or None for the image
    centre.  One HIP launch forward and two backward per 16 images.  Differentiable in the images and the table; ``table.grad`` is
    dense, rows not listed are exact zeros, and the sums behind it use no atomics: a repeated backward gives the same bits.  The
    backward re-reads the table: an in-place optimizer step between forward and backward raises."""
    imgs, kind = _image_list(_OP, images)
    L.require(_OP, "table", table, gpu=True, f32=True, contiguous=True,
              host=": bags_raster.appearance_torch is the same function in PyTorch on any device and dtype")
    if table.dim() != 2 or table.shape[1] != ROW or table.shape[0] < 1:
        raise ValueError(f"{_OP}: table must be (N,16) with N >= 1, got {tuple(table.shape)}")
    if kind == "stack":
        L.require(_OP, "images", images, gpu=True, f32=True, contiguous=True, on=table)
    else:
        for i, t in enumerate(imgs):
            L.require(_OP, f"images[{i}]", t, gpu=True, f32=True, contiguous=True, on=table)
    rows = _rows(_OP, [rows] if isinstance(rows, int) else rows, table.shape[0])
    if len(rows) != len(imgs):
        raise ValueError(f"{_OP}: {len(imgs)} images but {len(rows)} rows")
    _, H, W = imgs[0].shape
    if H * W >= 2 ** 31:
        raise ValueError(f"{_OP}: an image of {W}x{H} has 2^31 pixels or more")
    cx, cy = _center(center, H, W)
    if kind == "stack":
        return _Appearance.apply(table, rows, cx, cy, True, images)
    out = _Appearance.apply(table, rows, cx, cy, False, *imgs)
    return out[0] if kind == "one" else out


class AppearanceBank(torch.nn.Module):
    """The appearance parameters of N training images: one parameter ``table`` ``(N,16)``, every row initialised to the neutral
    row ``E = [I | 0]``, ``k = 0``.

    The optimizer is upstream's: ONE ``torch.optim.Adam([bank.table], lr=...)`` over the whole table, as upstream keeps one Adam
    over its ``(N,3,4)`` exposure parameter.  A step's backward leaves a dense gradient whose unlisted rows are zeros, so that
    optimizer is a single fused step with no fill launch.  (A per-camera Adam, as ``PoseAdam`` is for the poses, is not offered.)
    The vignetting coefficients have no field in upstream's ``exposure.json``: they travel in this module's ``state_dict``."""

    def __init__(self, N: int, device="cpu"):
        super().__init__()
        if int(N) < 1:
            raise ValueError("AppearanceBank: no cameras")
        self.table = torch.nn.Parameter(torch.tensor(NEUTRAL, dtype=torch.float32, device=torch.device(device)).repeat(int(N), 1))

    def __len__(self) -> int:
        return self.table.shape[0]

    def exposure(self, i: int) -> torch.Tensor:
        """Camera i's exposure matrix: a ``(3,4)`` view of its row."""
        return self.table[_rows("AppearanceBank.exposure", [i], len(self))[0], :12].view(3, 4)

    def vignetting(self, i: int) -> torch.Tensor:
        """Camera i's ``(k1, k2, k3)``: a ``(3,)`` view of its row."""
        return self.table[_rows("AppearanceBank.vignetting", [i], len(self))[0], 12:15]

    def apply(self, images, rows, center=None):                # (shadows nn.Module.apply, which nothing here uses)
        """``images`` (as ``apply_appearance`` takes them) through the cameras ``rows``: the HIP path where the table is on a GPU,
        ``appearance_torch`` on the host."""
        if self.table.is_cuda:
            return apply_appearance(images, self.table, rows, center)
        rows = _rows("AppearanceBank.apply", [rows] if isinstance(rows, int) else rows, len(self))
        return appearance_torch(images, self.table[rows], center)
