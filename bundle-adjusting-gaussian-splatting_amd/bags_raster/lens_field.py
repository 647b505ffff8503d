"""The lens network of the distortion route: the reference's invertible ResNet (scene/iresnet.py, FrEIA's ``IResNetLayer`` shape)
evaluated on the control-point grid.  Its output is the ``ctrl_flow`` of ``resample_image``, whose backward hands
``dL/dctrl_flow`` back to it.

A point ``x`` in R^2 goes through ``blocks`` residual blocks ``x <- x + g_b(x)``; ``g_b`` is Linear(2, H), ELU, then
``internal_layers`` times (Linear(H, H), ELU), then Linear(H, 2).  Every parameter lives in ONE flat float32 vector; per block,
in order: ``W_0 (H,2)``, ``b_0 (H)``, ``W_i (H,H)``, ``b_i (H)`` for i = 1..n, ``W_out (2,H)``, ``b_out (2)``, each weight in
``nn.Linear``'s (out, in) row-major layout.  One parameter means any optimizer steps the net in one launch.

``lens_field``        the HIP kernels of csrc/lens_field.hip (``bags_lens_field_forward`` / ``_backward``): one launch forward, two
                      backward, nothing saved in between but the caller's ``x``.  GPU only, H <= 64, n <= 4, B <= 32.
``lens_field_torch``  the same function in plain PyTorch on views of the flat vector (any device, dtype and size); the host path.
``LensField``         the ``nn.Module`` around the flat parameter.
"""
from __future__ import annotations

import math
from typing import List, Tuple

import torch
import torch.nn.functional as F

from . import _lib as L


def block_floats(hidden: int, internal_layers: int) -> int:
    """Floats of one block in the flat vector."""
    H, n = int(hidden), int(internal_layers)
    return 3 * H + n * (H * H + H) + 2 * H + 2


def param_count(blocks: int, hidden: int, internal_layers: int) -> int:
    return int(blocks) * block_floats(hidden, internal_layers)


def layer_views(params: torch.Tensor, blocks: int, hidden: int, internal_layers: int) -> List[List[Tuple[torch.Tensor, torch.Tensor]]]:
    """Per block, the n + 2 (weight, bias) views of the flat vector, first layer first."""
    B, H, n = int(blocks), int(hidden), int(internal_layers)
    if B < 1 or H < 1 or n < 0:
        raise ValueError(f"lens_field: need blocks >= 1, hidden >= 1, internal_layers >= 0 (got {B}, {H}, {n})")
    if params.dim() != 1 or params.numel() != param_count(B, H, n):
        raise ValueError(f"lens_field: params must be a flat vector of blocks * (3H + n(H^2 + H) + 2H + 2) = {param_count(B, H, n)} elements "
                         f"for blocks {B}, hidden {H}, internal_layers {n}; got shape {tuple(params.shape)}")
    out, o = [], 0
    for _ in range(B):
        layers = []
        for rows, cols in [(H, 2)] + [(H, H)] * n + [(2, H)]:
            W = params[o:o + rows * cols].view(rows, cols)
            o += rows * cols
            layers.append((W, params[o:o + rows]))
            o += rows
        out.append(layers)
    return out


def _check_points(x: torch.Tensor) -> None:
    if not isinstance(x, torch.Tensor) or x.dim() < 1 or x.shape[-1] != 2:
        raise ValueError(f"lens_field: the points must have shape (..., 2), got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__}")


def _block_g(layers, x):
    h = x
    for W, b in layers[:-1]:
        h = F.elu(F.linear(h, W, b))
    return F.linear(h, layers[-1][0], layers[-1][1])


def lens_field_torch(params: torch.Tensor, x: torch.Tensor, blocks: int, hidden: int, internal_layers: int) -> torch.Tensor:
    """``x (..., 2) -> y (..., 2)`` with the PyTorch calls of an ``nn.Linear`` / ``nn.ELU`` stack; ``params`` and ``x`` share device and dtype."""
    _check_points(x)
    for layers in layer_views(params, blocks, hidden, internal_layers):
        x = x + _block_g(layers, x)
    return x


def lens_field_inverse_torch(params: torch.Tensor, y: torch.Tensor, blocks: int, hidden: int, internal_layers: int, iterations: int = 50) -> torch.Tensor:
    """The blocks in reverse order, each by ``iterations`` steps of ``x <- y - g_b(x)`` from ``x = y``."""
    _check_points(y)
    for layers in reversed(layer_views(params, blocks, hidden, internal_layers)):
        x = y
        for _ in range(int(iterations)):
            x = y - _block_g(layers, x)
        y = x
    return y


def _check_fused(op: str, params, x, blocks: int, hidden: int, internal_layers: int) -> None:
    B, H, n = int(blocks), int(hidden), int(internal_layers)
    if not (1 <= B <= L.LENS_MAX_BLOCKS and 1 <= H <= L.LENS_MAX_HIDDEN and 0 <= n <= L.LENS_MAX_INTERNAL_LAYERS):
        raise ValueError(f"{op}: blocks {B}, hidden {H}, internal_layers {n} not in 1..{L.LENS_MAX_BLOCKS}, 1..{L.LENS_MAX_HIDDEN}, "
                         f"0..{L.LENS_MAX_INTERNAL_LAYERS}; a larger net is a GEMM problem, not a launch-count one: use the PyTorch path, lens_field_torch")
    L.require(op, "params", params)
    L.require(op, "x", x)
    layer_views(params, B, H, n)                 # the length of the flat vector
    _check_points(x)
    L.require(op, "params", params, gpu=True, host=" (use lens_field_torch on the host)")
    L.require(op, "x", x, gpu=True, on=params, host=" (use lens_field_torch on the host)")


def _net(p: torch.Tensor, dims) -> L.BagsLensField:
    return L.BagsLensField(dims[0], dims[1], dims[2], 0, p.data_ptr())


class _LensField(torch.autograd.Function):
    @staticmethod
    def forward(ctx, params, x, blocks, hidden, internal_layers):
        _check_fused("lens_field", params, x, blocks, hidden, internal_layers)
        p, pts = L.as_f32c(params), L.as_f32c(x).reshape(-1, 2)
        y = torch.empty_like(pts)
        ctx.dims = (int(blocks), int(hidden), int(internal_layers))
        L.call("bags_lens_field_forward", p.device, _net(p, ctx.dims), pts.data_ptr(), pts.shape[0], y.data_ptr())
        ctx.save_for_backward(p, pts)
        ctx.x_shape = x.shape
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, g_y):
        p, pts = ctx.saved_tensors
        M = pts.shape[0]
        g_y = L.as_f32c(g_y).reshape(-1, 2)
        g_p = torch.empty_like(p) if ctx.needs_input_grad[0] else None
        g_x = torch.empty_like(pts) if ctx.needs_input_grad[1] else None
        ws = L.workspace(L.load().bags_lens_field_workspace_size(*ctx.dims, M), p.device)
        L.call("bags_lens_field_backward", p.device, _net(p, ctx.dims), pts.data_ptr(), M, g_y.data_ptr(), ws.data_ptr(), ws.numel(),
               L.ptr(g_x), L.ptr(g_p))
        return g_p, (None if g_x is None else g_x.view(ctx.x_shape)), None, None, None


def lens_field(params: torch.Tensor, x: torch.Tensor, blocks: int, hidden: int, internal_layers: int) -> torch.Tensor:
    """``x (..., 2) -> y (..., 2)``, float32, through the fused kernels; gradients reach ``params`` and, when it asks for one, ``x``
    (the control points are constants in the reference's use: then the first layer's input gradient is not formed)."""
    return _LensField.apply(params, x, blocks, hidden, internal_layers)


def lens_field_inverse(params: torch.Tensor, y: torch.Tensor, blocks: int, hidden: int, internal_layers: int, iterations: int = 50) -> torch.Tensor:
    """The fused fixed-point inverse (``bags_lens_field_inverse``); no gradient.  GPU only."""
    _check_fused("lens_field_inverse", params, y, blocks, hidden, internal_layers)
    if int(iterations) < 0:
        raise ValueError(f"lens_field_inverse: iterations {iterations} < 0")
    p, pts = L.as_f32c(params), L.as_f32c(y).reshape(-1, 2)
    x = torch.empty_like(pts)
    L.call("bags_lens_field_inverse", p.device, _net(p, (int(blocks), int(hidden), int(internal_layers))), pts.data_ptr(), pts.shape[0],
           int(iterations), x.data_ptr())
    return x.view(y.shape)


class LensField(torch.nn.Module):
    """The lens network as a module with ONE parameter, ``params``.  ``forward(x)`` is fused on a GPU and ``lens_field_torch`` on the
    host; ``flow = lens(control_points)`` is the ``ctrl_flow`` of ``resample_image``."""

    def __init__(self, blocks: int = 5, hidden: int = 64, internal_layers: int = 1, device=None, seed=None, identity_init: bool = False):
        super().__init__()
        self.blocks, self.hidden, self.internal_layers = int(blocks), int(hidden), int(internal_layers)
        flat = torch.zeros(param_count(self.blocks, self.hidden, self.internal_layers), dtype=torch.float32)
        gen = None if seed is None else torch.Generator().manual_seed(int(seed))
        for layers in layer_views(flat, self.blocks, self.hidden, self.internal_layers):
            for W, b in layers:                  # nn.Linear.reset_parameters: both uniform in +-1 / sqrt(fan_in)
                bound = 1.0 / math.sqrt(W.shape[1])
                W.copy_((torch.rand(W.shape, generator=gen) * 2.0 - 1.0) * bound)
                b.copy_((torch.rand(b.shape, generator=gen) * 2.0 - 1.0) * bound)
            if identity_init:
                layers[-1][0].zero_()
                layers[-1][1].zero_()
        self.params = torch.nn.Parameter(flat.to(device) if device is not None else flat)

    def extra_repr(self) -> str:
        return f"blocks={self.blocks}, hidden={self.hidden}, internal_layers={self.internal_layers}"

    @property
    def dims(self) -> Tuple[int, int, int]:
        return self.blocks, self.hidden, self.internal_layers

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.params.is_cuda:
            return lens_field(self.params, x, *self.dims)
        return lens_field_torch(self.params, x, *self.dims)

    @torch.no_grad()
    def inverse(self, y: torch.Tensor, iterations: int = 50) -> torch.Tensor:
        if self.params.is_cuda:
            return lens_field_inverse(self.params, y, *self.dims, iterations)
        return lens_field_inverse_torch(self.params, y, *self.dims, iterations)

    def layers(self) -> List[List[Tuple[torch.Tensor, torch.Tensor]]]:
        """Per block, the list of (weight, bias) views of ``params`` (detached: writing to one writes the parameter)."""
        return layer_views(self.params.detach(), *self.dims)

    @torch.no_grad()
    def load_linear_stacks(self, blocks_of_linears) -> None:
        """Copy the weights of ``blocks`` lists of n + 2 ``nn.Linear`` each (a FrEIA-shaped state, without FrEIA) into ``params``."""
        mine = self.layers()
        if len(blocks_of_linears) != len(mine):
            raise ValueError(f"LensField: {len(blocks_of_linears)} blocks given, the net has {len(mine)}")
        for k, (linears, layers) in enumerate(zip(blocks_of_linears, mine)):
            linears = list(linears)
            if len(linears) != len(layers):
                raise ValueError(f"LensField: block {k} has {len(linears)} linear layers, expected {len(layers)}")
            for lin, (W, b) in zip(linears, layers):
                if tuple(lin.weight.shape) != tuple(W.shape) or lin.bias is None:
                    raise ValueError(f"LensField: block {k}: a Linear of weight {tuple(lin.weight.shape)} where {tuple(W.shape)} with a bias is expected")
                W.copy_(lin.weight)
                b.copy_(lin.bias)

    @torch.no_grad()
    def export_linear_stacks(self) -> List[List[torch.nn.Linear]]:
        out = []
        for layers in self.layers():
            stack = []
            for W, b in layers:
                lin = torch.nn.Linear(W.shape[1], W.shape[0], device=W.device, dtype=W.dtype)
                lin.weight.copy_(W)
                lin.bias.copy_(b)
                stack.append(lin)
            out.append(stack)
        return out

    @torch.no_grad()
    def lipschitz_correction(self, iterations: int = 10, spectral_norm_max: float = 0.8, generator=None) -> None:
        """Scale down every weight matrix whose spectral norm, estimated by power iteration, exceeds ``spectral_norm_max``.  ELU is
        1-Lipschitz, so every ``g_b`` is then a contraction of constant ``spectral_norm_max^(n+2)`` and the blocks stay invertible.

        The iteration runs on the smaller Gram matrix G of W from a random start vector, and squares the (normalised) matrix it
        applies after every step: step j multiplies by G^(2^j), so ``iterations`` steps are 2^iterations - 1 plain ones.  Plain steps
        shrink the error only as (sigma_2 / sigma_1)^(4k), which leaves 50 of them percents short on a (H, 2) matrix whose two singular
        values are close.  The estimate is a Rayleigh quotient of G: it does not exceed the norm, so a matrix below the maximum is left
        untouched.  Called every few hundred iterations: not a hot path, plain PyTorch."""
        for layers in self.layers():
            for W, _ in layers:
                G = (W.t() @ W) if W.shape[1] <= W.shape[0] else (W @ W.t())         # same spectral norm, squared
                v = torch.randn(G.shape[0], generator=generator).to(device=W.device, dtype=W.dtype)
                A = G
                for _ in range(int(iterations)):
                    A = A / A.norm().clamp_min(1e-30)
                    v = A @ (v / v.norm().clamp_min(1e-30))
                    A = A @ A
                v = v / v.norm().clamp_min(1e-30)
                sigma = float(torch.sqrt(torch.clamp(v @ (G @ v), min=0.0)))
                if sigma > spectral_norm_max:
                    W.mul_(spectral_norm_max / sigma)
