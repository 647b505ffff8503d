"""Named case images for bags_raster.normal_map_loss, built on the CPU from a fixed seed (tests/test_normal_map_cpu.py and
tests/test_normal_map_gpu.py run the same ones).  A case is V views of: a normal map N (3,H,W), a weights map A (1,H,W), a target p
(3,H,W) and a pixel weight m (H,W), float32.

    generic       |N| in [0.3, 1], A in [0.6, 1], |p| in [0.8, 1.2], m in [0.2, 1] with a tenth of the pixels at 0
    holes         generic with 2 x 2 blocks of: A < min_weight; |N| < min_norm; a zero target; a NaN target; an Inf in N
    empty         generic with A = 0.2 everywhere: no valid pixel
    depth_target  the target is depth_to_normal's output on a tilted plane (zeros on the border, where it has no normal)
"""
import torch

from bags_raster import depth_to_normal_torch

SIZES = ((1, 1), (3, 3), (5, 7), (33, 70), (64, 256))
VIEWS = (1, 5, 17)
CASES = ("generic", "holes", "empty", "depth_target")
MIN_WEIGHT, MIN_NORM = 0.5, 0.1
_cache = {}


def _unit(g, V, H, W):
    d = torch.randn(V, 3, H, W, generator=g, dtype=torch.float64)
    return d / d.norm(dim=1, keepdim=True)


def hole_kind(H, W):
    """(H,W) int: 0 A < min_weight, 1 short N, 2 zero target, 3 NaN target, 4 Inf in N, 5..9 left alone; in 2 x 2 blocks."""
    y, x = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    return (y // 2 * 3 + x // 2) % 10


def case(name, H, W, V):
    """dict(normal=[V x (3,H,W)], weights=[V x (1,H,W)], target=[V x (3,H,W)], mask=[V x (H,W)]); the same tensors every call."""
    key = (name, H, W, V)
    if key in _cache:
        return _cache[key]
    assert name in CASES, name
    g = torch.Generator().manual_seed(4100 + 7 * H + W)
    N = _unit(g, V, H, W) * (0.3 + 0.7 * torch.rand(V, 1, H, W, generator=g, dtype=torch.float64))
    A = 0.6 + 0.4 * torch.rand(V, 1, H, W, generator=g, dtype=torch.float64)
    p = _unit(g, V, H, W) * (0.8 + 0.4 * torch.rand(V, 1, H, W, generator=g, dtype=torch.float64))
    m = 0.2 + 0.8 * torch.rand(V, H, W, generator=g, dtype=torch.float64)
    m[torch.rand(V, H, W, generator=g) < 0.1] = 0.0
    N, A, p, m = N.float(), A.float(), p.float(), m.float()
    if name == "holes":
        kind = hole_kind(H, W)
        A[:, 0][:, kind == 0] = 0.3
        N[:, :, kind == 1] *= 0.05
        p[:, :, kind == 2] = 0.0
        p[:, 1, kind == 3] = float("nan")
        N[:, 2, kind == 4] = float("inf")
    elif name == "empty":
        A[:] = 0.2
    elif name == "depth_target":
        # a plane z = 2 + 0.3 u/W + 0.2 v/H + 0.05 view, seen through a pinhole; D = A z
        v_, u_ = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
        for k in range(V):
            z = 2.0 + 0.3 * u_ / W + 0.2 * v_ / H + 0.05 * k
            pin = (float(W), float(W), W / 2 - 0.5, H / 2 - 0.5)
            p[k] = depth_to_normal_torch(A[k] * z[None], A[k], pin)[0]
            # normals near the target's, so that both signs of nh - ph occur
            N[k] = (p[k] + 0.3 * N[k]) * 0.7
    out = dict(normal=[t.contiguous() for t in N], weights=[t.contiguous() for t in A], target=[t.contiguous() for t in p],
               mask=[t.contiguous() for t in m])
    _cache[key] = out
    return out


def cotangent(V):
    return torch.randn(17, generator=torch.Generator().manual_seed(5))[:V].double() + 2.0


def forward_backward(fn, name, H, W, V, mode, masked, dtype, device):
    """``fn`` is normal_map_loss or its PyTorch statement: (loss (V,), count (V,), [V x dL/dnormal])."""
    c = case(name, H, W, V)
    Ns = [t.to(device, dtype).requires_grad_() for t in c["normal"]]
    As = [t.to(device, dtype).requires_grad_() for t in c["weights"]]
    ps = [t.to(device, dtype) for t in c["target"]]
    ms = [t.to(device, dtype) for t in c["mask"]] if masked else None
    loss, count = fn(Ns, As, ps, ms, mode=mode, min_weight=MIN_WEIGHT, min_norm=MIN_NORM)
    assert not count.requires_grad
    gs = torch.autograd.grad(loss, Ns + As, cotangent(V).to(device, dtype), allow_unused=True)
    assert all(g is None for g in gs[V:]), "weights must get no gradient"
    return loss.detach(), count.detach(), [torch.zeros_like(n) if g is None else g for g, n in zip(gs[:V], Ns)]
