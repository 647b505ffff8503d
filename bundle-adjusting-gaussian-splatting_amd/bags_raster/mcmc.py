"""``compute_relocation`` of the 3DGS-MCMC strategy (utils/reloc_utils.py: the reference imports it from
``diff_gaussian_rasterization``) -- one HIP launch on a GPU (csrc/mcmc.hip), ``compute_relocation_torch`` anywhere -- and the
binomial table both take.  The strategy's three call sites are ``GaussianBag.relocate`` / ``add_new`` / ``mcmc_noise``
(bags_raster.gaussians).
"""
from __future__ import annotations

import math

import torch

from . import _lib as L

N_MAX = L.MCMC_MAX_BINOMS           # the reference's N_max = 51: a row is relocated with a count of at most 50
_BINOMS = {}


def relocation_binoms(n_max: int = N_MAX, device="cpu") -> torch.Tensor:
    """The ``(n_max, n_max)`` float32 table ``binoms[n][k] = C(n, k)`` (zero above the diagonal), as utils/reloc_utils.py builds
    its ``BINOMS``; one per (n_max, device), cached."""
    key = (int(n_max), str(torch.device(device)))
    if key not in _BINOMS:
        t = torch.zeros(n_max, n_max, dtype=torch.float32)
        for n in range(n_max):
            for k in range(n + 1):
                t[n, k] = math.comb(n, k)
        _BINOMS[key] = t.to(device)
    return _BINOMS[key]


def compute_relocation_torch(opacity_old, scale_old, N, binoms, n_max):
    """``compute_relocation`` in plain PyTorch, on any device and in the dtype of ``opacity_old``: the published kernel's double loop,
    term by term in its order.  With ``n = clamp(N, 1, n_max - 1)`` (``N`` is not modified)

        opacity_new = 1 - (1 - opacity_old)^(1/n)
        denom       = sum_{i=1..n} sum_{k=0..i-1} binoms[i-1][k] * (-1)^k / sqrt(k+1) * opacity_new^(k+1)
        scale_new   = (opacity_old / denom) * scale_old

    ``opacity_old`` holds P values (any shape, returned in that shape), ``scale_old`` is ``(P,3)``."""
    o = opacity_old.reshape(-1)
    dt = o.dtype
    n = N.reshape(-1).to(o.device, torch.int64).clamp(1, int(n_max) - 1)
    b = binoms.to(o.device, dt)
    o_new = 1 - torch.pow(1 - o, 1 / n.to(dt))
    denom = torch.zeros_like(o)
    zero = torch.zeros_like(o)
    for i in range(1, (int(n.max()) if n.numel() else 0) + 1):
        active = n >= i
        for k in range(i):
            term = (b[i - 1, k] * ((-1.0) ** k / math.sqrt(k + 1))) * torch.pow(o_new, k + 1)
            denom = denom + torch.where(active, term, zero)
    coeff = o / denom
    return o_new.reshape(opacity_old.shape), coeff.unsqueeze(-1) * scale_old


def compute_relocation(opacity_old, scale_old, N, binoms, n_max):
    """utils/reloc_utils.py:11-13 on GPU tensors, one HIP launch: ``(opacity_new, scale_new)`` of ``compute_relocation_torch``, the
    sums formed in double and rounded to float32 once.  ``opacity_old`` (P values) and ``scale_old (P,3)`` float32, ``N`` (P) int32
    or int64, ``binoms (n_max, n_max)`` float32, all contiguous on one device; ``n_max`` in 2..51."""
    what = "compute_relocation"
    ts = (("opacity_old", opacity_old), ("scale_old", scale_old), ("N", N), ("binoms", binoms))
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for _, t in ts):
        raise NotImplementedError(f"{what} runs only on an AMD GPU and takes GPU tensors; there is no CPU fallback behind this name: "
                                  "bags_raster.compute_relocation_torch is the same function in PyTorch on any device and dtype")
    n_max = int(n_max)
    if not 2 <= n_max <= N_MAX:
        raise ValueError(f"{what}: n_max must be in 2..{N_MAX}, got {n_max}")
    for name, t in ts:
        L.require(what, name, t, gpu=True, f32=name != "N", contiguous=True, on=opacity_old)
    if N.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"{what}: N must be int32 or int64, got {N.dtype}")
    P = opacity_old.numel()
    if tuple(scale_old.shape) != (P, 3) or N.numel() != P or tuple(binoms.shape) != (n_max, n_max):
        raise RuntimeError(f"{what}: expected opacity_old with P values, scale_old (P,3), N (P) and binoms ({n_max},{n_max}); got "
                           f"{tuple(opacity_old.shape)}, {tuple(scale_old.shape)}, {tuple(N.shape)}, {tuple(binoms.shape)}")
    n32 = N if N.dtype == torch.int32 else N.to(torch.int32)
    o_new, s_new = torch.empty_like(opacity_old), torch.empty_like(scale_old)
    L.call("bags_compute_relocation", opacity_old.device, L.ptr(L.as_f32c(opacity_old)), L.ptr(L.as_f32c(scale_old)), n32.data_ptr(), binoms.data_ptr(),
           n_max, P, o_new.data_ptr(), s_new.data_ptr())
    return o_new, s_new
