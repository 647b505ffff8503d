"""Named case images for bags_raster.depth_smooth_loss / normal_smooth_loss, built on the CPU from a fixed seed
(tests/test_smooth_cpu.py and tests/test_smooth_gpu.py run the same ones).  A case is V views of: a depth map D (1,H,W) and a normal
map N (3,H,W), a weights map A (1,H,W), a guide image of 3 channels and one of 1 channel, and a pixel weight m (H,W), float32.

    generic   z in [1, 5] (so the inverse depth x = A / D is in [0.2, 1]), D = A z, A in [0.6, 1], |N| in [0.3, 1], guide in [0, 1],
              m in [0.2, 1] with a tenth of the pixels at 0
    holes     generic with 2 x 2 blocks of: A < min_weight; D <= 0; an Inf in D and in N; a NaN guide pixel; a short N
    empty     generic with A = 0.2 everywhere: no usable pixel
    plane     an inverse depth linear in (u, v): the second differences vanish

A configuration is a dict of the keyword arguments plus ``guide`` ("none", "rgb", "gray") and ``masked``.
"""
import torch

SIZES = ((1, 1), (1, 5), (2, 2), (3, 3), (5, 7), (33, 70), (64, 256))
VIEWS = (1, 5, 17)
CASES = ("generic", "holes", "empty", "plane")
MIN_WEIGHT, MIN_NORM = 0.5, 0.1
MARGIN = 8.0 * 2.0 ** -24                                      # times max |x|: the smallest |d| an eps = 0 run may have (depth field)
_cache = {}


def hole_kind(H, W):
    """(H,W) int: 0 A < min_weight, 1 D <= 0, 2 Inf in D and N, 3 NaN guide pixel, 4 short N, 5..9 left alone; in 2 x 2 blocks."""
    y, x = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    return (y // 2 * 3 + x // 2) % 10


def unusable_kinds(normals):
    """The hole kinds whose pixels are not usable for the front-end (an Inf depth has the usable inverse depth 0, and its own
    gradients are exact zeros all the same: 1 / inf)."""
    return (0, 2, 4) if normals else (0, 1, 2)


def _small_stencils(D, A):
    """(V,H,W) bool: the first member of every stencil (both orders, both directions, both spaces) of the all-usable field whose |d|
    is below twice the margin."""
    bad = torch.zeros_like(D, dtype=torch.bool)
    for x in (A / D, D / A):
        lim = 2.0 * MARGIN * float(x.abs().max())
        for axis in (-1, -2):
            for order in (1, 2):
                n = x.shape[axis]
                if n <= order:
                    continue
                xs = [x.narrow(axis, k, n - order) for k in range(order + 1)]
                d = xs[1] - xs[0] if order == 1 else xs[0] - 2 * xs[1] + xs[2]
                bad.narrow(axis, 0, n - order).logical_or_(d.abs() < lim)
    return bad


def case(name, H, W, V):
    """dict(depth=[V x (1,H,W)], normal=[V x (3,H,W)], weights=[V x (1,H,W)], rgb=[V x (3,H,W)], gray=[V x (1,H,W)], mask=[V x (H,W)]);
    the same tensors every call."""
    key = (name, H, W, V)
    if key in _cache:
        return _cache[key]
    assert name in CASES, name
    g = torch.Generator().manual_seed(9300 + 7 * H + W)
    f64 = torch.float64
    z = 1.0 + 4.0 * torch.rand(V, 1, H, W, generator=g, dtype=f64)
    A = 0.6 + 0.4 * torch.rand(V, 1, H, W, generator=g, dtype=f64)
    d = torch.randn(V, 3, H, W, generator=g, dtype=f64)
    N = d / d.norm(dim=1, keepdim=True) * (0.3 + 0.7 * torch.rand(V, 1, H, W, generator=g, dtype=f64))
    rgb = torch.rand(V, 3, H, W, generator=g, dtype=f64)
    gray = torch.rand(V, 1, H, W, generator=g, dtype=f64)
    m = 0.2 + 0.8 * torch.rand(V, H, W, generator=g, dtype=f64)
    m[torch.rand(V, H, W, generator=g) < 0.1] = 0.0
    if name == "plane":
        v_, u_ = torch.meshgrid(torch.arange(H, dtype=f64), torch.arange(W, dtype=f64), indexing="ij")
        x = torch.stack([0.3 + 0.4 * u_ / W + 0.2 * v_ / H + 0.01 * k for k in range(V)])[:, None]
        z = 1.0 / x
    A = A.float()
    D = (A.double() * z).float()
    if name != "plane":
        # the margin condition: a random field has a few stencils whose |d| is below the float32 error of x, where the sign of d --
        # and with it a whole unit of an eps = 0 gradient -- may legitimately differ between float32 and float64.  Their pixels are
        # drawn again (from the same generator: the case stays a function of the seed) until none is left.
        for _ in range(100):
            bad = _small_stencils(D.double()[:, 0], A.double()[:, 0])
            if not bad.any():
                break
            z[:, 0][bad] = 1.0 + 4.0 * torch.rand(int(bad.sum()), generator=g, dtype=f64)
            D = (A.double() * z).float()
        assert not bad.any()
    N, rgb, gray, m = N.float(), rgb.float(), gray.float(), m.float()
    if name == "holes":
        kind = hole_kind(H, W)
        A[:, 0][:, kind == 0] = 0.3
        D[:, 0][:, kind == 1] = torch.where(torch.arange(int((kind == 1).sum())) % 2 == 0, 0.0, -1.0)
        D[:, 0][:, kind == 2] = float("inf")
        N[:, 2, kind == 2] = float("inf")
        rgb[:, 1, kind == 3] = float("nan")
        gray[:, 0, kind == 3] = float("nan")
        N[:, :, kind == 4] *= 0.05
    elif name == "empty":
        A[:] = 0.2
    out = dict(depth=[t.contiguous() for t in D], normal=[t.contiguous() for t in N], weights=[t.contiguous() for t in A],
               rgb=[t.contiguous() for t in rgb], gray=[t.contiguous() for t in gray], mask=[t.contiguous() for t in m])
    _cache[key] = out
    return out


def config(space="inverse", normalize=True, order=1, penalty="l1", eps=0.0, gamma=1.0, guide="rgb", masked=True):
    return dict(space=space, normalize=normalize, order=order, penalty=penalty, eps=eps, gamma=gamma, guide=guide, masked=masked)


def key_of(cfg):
    return tuple(sorted(cfg.items()))


def depth_configs(eps_l1):
    """The depth front-end's combinations: both orders, both penalties, normalize on / off, both spaces, with and without guide and
    mask, a guide of one channel; ``eps_l1`` is the eps of the l1 runs."""
    return [config(order=1, penalty="l1", eps=eps_l1),                                                          # Monodepth2's
            config(order=2, penalty="l1", eps=eps_l1, guide="gray"),
            config(order=1, penalty="l2", normalize=False, masked=False),
            config(order=2, penalty="l2", guide="none"),
            config(order=1, penalty="l1", eps=eps_l1, normalize=False, space="depth", guide="none", masked=False),
            config(order=2, penalty="l1", eps=eps_l1, normalize=False, space="depth", gamma=3.0),
            config(order=1, penalty="l2", space="depth", gamma=0.0),
            config(order=2, penalty="l2", space="depth", normalize=False, masked=False, guide="gray"),
            config(order=1, penalty="l1", eps=1e-2, masked=False),
            config(order=2, penalty="l1", eps=1e-2, normalize=False, guide="none")]


def normal_configs(eps_l1):
    return [config(order=1, penalty="l2", guide="none", masked=False),                                          # DN-Splatter's TVLoss
            config(order=1, penalty="l1", eps=eps_l1),
            config(order=2, penalty="l1", eps=eps_l1, guide="gray", masked=False),
            config(order=2, penalty="l2", gamma=2.5),
            config(order=1, penalty="l1", eps=1e-2, guide="none"),
            config(order=2, penalty="l1", eps=1e-2, guide="none", masked=False)]


def eps_l1_of(H, W, V):
    """The eps of the l1 runs of ``generic`` at a size: 0 (the margin condition is asserted in tests/test_smooth_cpu.py for every one
    of them), and 1e-3 at the largest field, which so covers the Charbonnier branch at a size with many tiles and two chunks."""
    return 1e-3 if (H, W, V) == (64, 256, 17) else 0.0


# holes: where they run and how.  An Inf depth has the usable inverse depth 0, so two of them side by side have d = 0 exactly (in
# float32 and in float64 alike): the eps = 0 runs of the depth front-end are in depth space, where an Inf depth is not usable.
HOLES_SIZES = ((33, 70, 5), (5, 7, 17))
HOLES_CONFIGS = [config(space="depth", order=1),
                 config(space="depth", order=2, normalize=False, guide="gray"),
                 config(space="inverse", order=1, eps=1e-3),
                 config(space="inverse", order=2, penalty="l2", guide="none", masked=False)]


def smallest_difference(name, H, W, V, order, space):
    """(the smallest |d| over the stencils of the depth field whose members are all solid with a finite x, max |x| over those
    pixels) in float64 -- the superset of the valid stencils of every mask and guide; (inf, 0) where there is none."""
    c = case(name, H, W, V)
    D, A = torch.stack(c["depth"]).double()[:, 0], torch.stack(c["weights"]).double()[:, 0]
    solid = (A >= MIN_WEIGHT) & (D > 0)
    x = torch.where(solid, A / D if space == "inverse" else D / A, torch.ones_like(D))
    solid = solid & torch.isfinite(x)
    x = torch.where(solid, x, torch.ones_like(x))
    small, big = float("inf"), float(x[solid].abs().max()) if solid.any() else 0.0
    for axis in (-1, -2):
        n = x.shape[axis]
        if n <= order:
            continue
        xs = [x.narrow(axis, k, n - order) for k in range(order + 1)]
        ok = solid.narrow(axis, 0, n - order)
        for k in range(1, order + 1):
            ok = ok & solid.narrow(axis, k, n - order)
        d = xs[1] - xs[0] if order == 1 else xs[0] - 2 * xs[1] + xs[2]
        if ok.any():
            small = min(small, float(d[ok].abs().min()))
    return small, big


def cotangent(V):
    return torch.randn(17, generator=torch.Generator().manual_seed(5))[:V].double() + 2.0


def arguments(name, H, W, V, cfg, normals, dtype, device, views=None):
    """(field list with requires_grad, weights list with requires_grad, guide, mask, keywords) of a case for a front-end."""
    c = case(name, H, W, V)
    views = range(V) if views is None else views
    Fs = [c["normal" if normals else "depth"][v].to(device, dtype, copy=True).requires_grad_() for v in views]
    As = [c["weights"][v].to(device, dtype, copy=True).requires_grad_() for v in views]
    Gs = None if cfg["guide"] == "none" else [c[cfg["guide"]][v].to(device, dtype) for v in views]
    ms = [c["mask"][v].to(device, dtype) for v in views] if cfg["masked"] else None
    kw = dict(order=cfg["order"], penalty=cfg["penalty"], eps=cfg["eps"], gamma=cfg["gamma"], min_weight=MIN_WEIGHT)
    if normals:
        kw["min_norm"] = MIN_NORM
    else:
        kw.update(space=cfg["space"], normalize=cfg["normalize"])
    return Fs, As, Gs, ms, kw


def forward_backward(fn, name, H, W, V, cfg, normals, dtype, device):
    """``fn`` is a front-end or its PyTorch statement: (loss (V,), count (V,), [V x dL/dfield], [V x dL/dweights]); the weights of the
    normals front-end must get no gradient (zeros are returned for them)."""
    Fs, As, Gs, ms, kw = arguments(name, H, W, V, cfg, normals, dtype, device)
    loss, count = fn(Fs, As, Gs, ms, **kw)
    assert not count.requires_grad
    if not loss.requires_grad:                                  # the statement on a view with nothing to differentiate
        return loss.detach(), count.detach(), [torch.zeros_like(t) for t in Fs], [torch.zeros_like(t) for t in As]
    gs = torch.autograd.grad(loss, Fs + As, cotangent(V).to(device, dtype), allow_unused=True)
    if normals:
        assert all(g is None for g in gs[V:]), "weights must get no gradient"
    zero = lambda g, t: torch.zeros_like(t) if g is None else g                 # noqa: E731
    return loss.detach(), count.detach(), [zero(g, t) for g, t in zip(gs[:V], Fs)], [zero(g, t) for g, t in zip(gs[V:], As)]
