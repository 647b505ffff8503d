"""Photometric loss that produces dL/dimage for the op: 0.8*L1 + 0.2*(1-SSIM)  (train.py:311-313,325;
utils/loss_utils.py:18-76).

Two implementations with the reference's names and semantics:
  * ``l1_loss / ssim / photometric_loss``        plain PyTorch (any device); the 11x11 Gaussian window is applied as two
    1-D passes, which is the same linear filter as the reference's dense 11x11 conv.
  * ``fused_l1_ssim / fused_photometric_loss``   the HIP kernels of csrc/loss.hip behind ``bags_loss_forward`` /
    ``bags_loss_backward`` (include/bags_raster.h): one forward and one backward kernel instead of ~50 launches.
    GPU tensors only; there is no fallback.
Both are pinned by tests/golden/loss.npz (values and dL/dimage from the reference's own functions)."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from . import _lib as L


def l1_loss(x: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    return torch.abs(x - gt).mean()


def _window(size: int, sigma: float, like: torch.Tensor) -> torch.Tensor:
    g = torch.tensor([math.exp(-(i - size // 2) ** 2 / float(2 * sigma ** 2)) for i in range(size)])
    return (g / g.sum()).to(like)


def _blur(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    c, n = x.shape[-3], w.numel()
    x = x if x.dim() == 4 else x.unsqueeze(0)
    x = F.conv2d(x, w.view(1, 1, n, 1).expand(c, 1, n, 1), padding=(n // 2, 0), groups=c)
    return F.conv2d(x, w.view(1, 1, 1, n).expand(c, 1, 1, n), padding=(0, n // 2), groups=c)


def ssim(img1: torch.Tensor, img2: torch.Tensor, window_size: int = 11) -> torch.Tensor:
    w = _window(window_size, 1.5, img1)
    mu1, mu2 = _blur(img1, w), _blur(img2, w)
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1 = _blur(img1 * img1, w) - mu1_sq
    s2 = _blur(img2 * img2, w) - mu2_sq
    s12 = _blur(img1 * img2, w) - mu12
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    m = ((2 * mu12 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))
    return m.mean()


def photometric_loss(image: torch.Tensor, gt: torch.Tensor, lambda_dssim: float = 0.2) -> torch.Tensor:
    return (1.0 - lambda_dssim) * l1_loss(image, gt) + lambda_dssim * (1.0 - ssim(image, gt))


# ------------------------------------------------------------------------------------------------ fused HIP path
def _fused_forward(ctx, op: str, entry: str, n_out: int, image: torch.Tensor, gt: torch.Tensor, *scalars) -> torch.Tensor:
    """The forward both fused losses share: the checked pair, the workspace, ``n_out`` floats out of ``entry``."""
    for name, t in (("image", image), ("gt", gt)):
        L.require(op, name, t, gpu=True, f32=True, type_error=RuntimeError, host=" (use bags_raster.loss.l1_loss / ssim on the host)")
    if image.shape != gt.shape or image.dim() != 3:
        raise RuntimeError(f"{op}: expected two (C,H,W) tensors of one shape, got {tuple(image.shape)} and {tuple(gt.shape)}")
    image, gt = image.contiguous(), gt.contiguous()
    Cn, H, W = image.shape
    ws = L.workspace(L.load().bags_loss_workspace_size(Cn, H, W), image.device)
    out = torch.empty(n_out, dtype=torch.float32, device=image.device)
    L.call(entry, image.device, image.data_ptr(), gt.data_ptr(), Cn, H, W, ws.data_ptr(), ws.numel(), *scalars, out.data_ptr())
    ctx.save_for_backward(image, gt, ws)
    return out


def _fused_backward(ctx, entry: str, cotangent: torch.Tensor, *scalars) -> torch.Tensor:
    """dL/dimage out of ``entry`` for the float32 ``cotangent`` of the forward's outputs."""
    image, gt, ws = ctx.saved_tensors
    Cn, H, W = image.shape
    grad = torch.empty_like(image)
    L.call(entry, image.device, image.data_ptr(), gt.data_ptr(), Cn, H, W, ws.data_ptr(), ws.numel(), *scalars, cotangent.data_ptr(),
           grad.data_ptr())
    return grad


class _FusedL1SSIM(torch.autograd.Function):
    """(image, gt) -> (mean |image - gt|, mean SSIM), differentiable w.r.t. ``image``."""

    @staticmethod
    def forward(ctx, image: torch.Tensor, gt: torch.Tensor):
        terms = _fused_forward(ctx, "fused_l1_ssim", "bags_loss_forward", 2, image, gt)
        return terms[0], terms[1]

    @staticmethod
    def backward(ctx, g_l1, g_ssim):
        if not ctx.needs_input_grad[0] or (g_l1 is None and g_ssim is None):
            return None, None
        z = torch.zeros((), dtype=torch.float32, device=(g_l1 if g_l1 is not None else g_ssim).device)
        g = torch.stack([z if g_l1 is None else g_l1.to(torch.float32), z if g_ssim is None else g_ssim.to(torch.float32)])
        return _fused_backward(ctx, "bags_loss_backward", g), None


def fused_l1_ssim(image: torch.Tensor, gt: torch.Tensor):
    """(l1_loss(image, gt), ssim(image, gt)) of utils/loss_utils.py in one HIP kernel; both scalars carry gradient."""
    return _FusedL1SSIM.apply(image, gt)


class _FusedPhotometric(torch.autograd.Function):
    """(image, gt, lambda) -> (loss, L1 mean, SSIM mean) with train.py:325's combination formed inside the reduce kernel and its
    backward inside the backward kernel (``bags_photometric_loss_*``): two launches forward, one backward, no one-element
    PyTorch kernels around them.  Only ``loss`` carries gradient; the two terms are returned for logging."""

    @staticmethod
    def forward(ctx, image: torch.Tensor, gt: torch.Tensor, lambda_dssim: float):
        ctx.lambda_dssim = float(lambda_dssim)
        out = _fused_forward(ctx, "fused_photometric_loss", "bags_photometric_loss_forward", 3, image, gt, ctx.lambda_dssim)
        loss, l1, s = out[0], out[1], out[2]
        ctx.mark_non_differentiable(l1, s)
        ctx.set_materialize_grads(False)          # no zero-fill launches for the two logging terms' absent gradients
        return loss, l1, s

    @staticmethod
    def backward(ctx, g_loss, _g_l1, _g_ssim):
        if not ctx.needs_input_grad[0] or g_loss is None:
            return None, None, None
        return _fused_backward(ctx, "bags_photometric_loss_backward", L.as_f32c(g_loss), ctx.lambda_dssim), None, None


def fused_photometric_loss(image: torch.Tensor, gt: torch.Tensor, lambda_dssim: float = 0.2, return_terms: bool = False):
    """train.py:325: (1 - lambda) L1 + lambda (1 - SSIM) as one fused op.  ``return_terms``: also the two means (detached)."""
    loss, l1, s = _FusedPhotometric.apply(image, gt, lambda_dssim)
    return (loss, l1, s) if return_terms else loss
