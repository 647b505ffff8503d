"""Input classes and the measured bar of tests/test_loss_gpu.py -- CPU only, so that tests/test_golden_cpu.py can check the
generators and the bar's inputs without a GPU.

``make_pair(kind, shape)``   the (image, target) pair of one input class, float32 numpy, seeded by class and shape.
``reference(a, b)``          the float64 oracle (oracle/loss_oracle.py) and ``err32``: what the project's own float32 PyTorch
                             loss (bags_raster.loss.l1_loss / ssim + autograd, on the CPU) loses against it on that input.
                             The bar of the kernel is ``4 * err32 + floor``; nothing in it comes from the kernel.
"""
import zlib

import numpy as np
import torch

from bags_raster import loss as L
from oracle import loss_oracle as LO

KINDS = ("noise", "flat_bright", "dark", "out_of_range", "checkerboard")
RAGGED_SHAPES = ((3, 40, 44), (1, 33, 36), (2, 5, 4), (3, 70, 100), (1, 64, 28))    # W % 4 == 0, W % 32 != 0
G_L1, G_SSIM = 0.8, -0.2
FACTOR = 4.0                       # the kernel and PyTorch round the same 11+11-term sums in another order: one order, not one value
GRAD_FLOOR_REL, L1_FLOOR, SSIM_FLOOR = 1e-6, 2e-7, 5e-7


def make_pair(kind, shape):
    rng = np.random.default_rng(zlib.crc32(kind.encode()) + sum(shape))
    C, H, W = shape
    if kind == "noise":                                        # as test_fused_loss_matches_oracle, with its identical half
        a = rng.random(shape, dtype=np.float32)
        b = np.clip(a + 0.2 * rng.standard_normal(shape).astype(np.float32), 0, 1).astype(np.float32)
        b[..., : W // 2] = a[..., : W // 2]
    elif kind == "flat_bright":                                # E[a^2] - mu^2 cancels against C2 = 9e-4
        a = (0.9 + 1e-3 * rng.standard_normal(shape)).astype(np.float32)
        b = (0.9 + 1e-3 * rng.standard_normal(shape)).astype(np.float32)
    elif kind == "dark":
        a = (1e-3 * rng.random(shape)).astype(np.float32)
        b = (1e-3 * rng.random(shape)).astype(np.float32)
    elif kind == "out_of_range":
        a = (3.0 * rng.random(shape) - 1.0).astype(np.float32)
        b = rng.random(shape, dtype=np.float32)
    elif kind == "checkerboard":                               # cells 7 rows x 5 columns, the target shifted one pixel
        y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        board = lambda yy, xx: (((yy // 7) + (xx // 5)) % 2).astype(np.float32)
        a = np.broadcast_to(board(y, x), shape).copy()
        b = np.broadcast_to(board(y, x + 1), shape).copy()
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


def reference(a, b, g_l1=G_L1, g_ssim=G_SSIM):
    """dict: oracle l1 / ssim / grad (float64) and err32_l1 / err32_ssim / err32_grad of the float32 PyTorch loss on the CPU."""
    l1o, so, go = LO.loss_and_grad(a, b, g_l1, g_ssim)
    at = torch.from_numpy(a).clone().requires_grad_(True)
    bt = torch.from_numpy(b)
    l1, s = L.l1_loss(at, bt), L.ssim(at, bt)
    (g_l1 * l1 + g_ssim * s).backward()
    return dict(l1=l1o, ssim=so, grad=go, scale=float(np.abs(go).max()),
                err32_l1=abs(float(l1.item()) - l1o), err32_ssim=abs(float(s.item()) - so),
                err32_grad=float(np.abs(at.grad.numpy().astype(np.float64) - go).max()))


def bars(ref):
    """(grad, l1, ssim) bars for the kernel's error against the oracle."""
    return (FACTOR * ref["err32_grad"] + GRAD_FLOOR_REL * ref["scale"], FACTOR * ref["err32_l1"] + L1_FLOOR,
            FACTOR * ref["err32_ssim"] + SSIM_FLOOR)
