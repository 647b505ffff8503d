"""Named case images for bags_raster.alpha_loss, built on the CPU from a fixed seed, generated in float32 and cast
(tests/test_alpha_cpu.py and tests/test_alpha_gpu.py run the same ones).  A case is V views of: a weights map A (1,H,W), a target t
(H,W), a pixel weight m (H,W), and the eps it is run with.

    generic   A in [0.002, 0.998] with a tenth of the pixels exactly 0 and a tenth exactly 1 (clamped in the clamped modes; and, on
              the binary half of the target, A == t: sign(0)); t binary on the left half of the image and soft on the right;
              m in [0.2, 1] with a tenth of the pixels at 0 (never the first pixel of a view)
    holes     A in [0.002, 0.998], no planted pixels, m in [0.2, 1] without zeros, then 2 x 2 blocks of one pixel kind each
              (hole_kind / HOLES): NaN in A, inf in A, a NaN target, a target above 1, a target below 0, m = 0, m < 0
    empty     generic with A = NaN everywhere in the even views (view 0 included): no usable pixel there, with or without a mask
    edges     eps = 2**-10, a power of two, so that lo and hi are the same numbers in float32 and float64; the first seven pixels of
              every view (EDGES) sit exactly at lo, one float32 step below and above it, exactly at hi, one step below and above
              it, and at A == t; the rest as holes' base

Apart from the exact 0 and 1 of generic (which no rounding moves) and the placed pixels of edges, every A is at least 1e-3 away
from lo and hi: float32 and float64 never decide differently.

Every eps here is a power of two (2**-13 where a case does not say otherwise), so that lo = eps and hi = 1 - eps are the same numbers
in float32 and in float64.  The statement rounds both once to the dtype of the maps, and a clamped pixel's a IS that number: with
eps = 1e-4, float32(1 - 1e-4) and 1 - 1e-4 differ by 2.7e-8, which is 2.7e-4 of 1 - a and so 2.7e-4 in log(1 - a) -- the float64
reference would then state another function than the float32 paths it is the reference of, by more than the bar on the loss.
"""
import torch

SIZES = ((1, 1), (3, 3), (5, 7), (17, 67), (33, 70), (64, 256))
VIEWS = (1, 5, 17)
CASES = ("generic", "holes", "empty", "edges")
MODES = ("bce", "l1", "l2", "entropy")
CLAMPED = ("bce", "entropy")
EPS, EDGE_EPS = 2.0 ** -13, 2.0 ** -10
MARGIN = 2e-3
HOLES = ("nan_A", "inf_A", "nan_t", "t_above_1", "t_below_0", "m_zero", "m_negative")
_cache = {}


def hole_kind(H, W):
    """(H,W) int: the index into HOLES of the pixel's kind, len(HOLES) .. 11 left alone; in 2 x 2 blocks."""
    y, x = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    return (y // 2 * 5 + x // 2) % 12


def unusable_kinds(mode, masked):
    """The labels of HOLES whose pixels are not usable in ``mode``: they get exact zeros, the others do not."""
    out = ["nan_A", "inf_A"]
    if mode != "entropy":
        out.append("nan_t")
    if mode == "bce":
        out += ["t_above_1", "t_below_0"]
    if masked:
        out += ["m_zero", "m_negative"]
    return [HOLES.index(k) for k in out]


def _edge_values(eps):
    f = lambda x: torch.tensor(x, dtype=torch.float32)                                      # noqa: E731
    lo, hi, zero, one = f(eps), f(1.0 - eps), f(0.0), f(1.0)
    return torch.stack([lo, torch.nextafter(lo, zero), torch.nextafter(lo, one), hi, torch.nextafter(hi, zero), torch.nextafter(hi, one),
                        f(0.25)])


EDGES = dict(inside=(False, False, True, False, True, False, True), equal_target=6)       # of the first seven pixels of an edges view


def case(name, H, W, V):
    """dict(weights=[V x (1,H,W)], target=[V x (H,W)], mask=[V x (H,W)], eps=float); the same tensors every call."""
    key = (name, H, W, V)
    if key in _cache:
        return _cache[key]
    assert name in CASES, name
    g = torch.Generator().manual_seed(5200 + 7 * H + W)
    A = (MARGIN + (1.0 - 2.0 * MARGIN) * torch.rand(V, H * W, generator=g, dtype=torch.float64)).float()
    t = torch.rand(V, H, W, generator=g, dtype=torch.float64).float()
    t[:, :, :W // 2] = (t[:, :, :W // 2] < 0.5).float()
    m = (0.2 + 0.8 * torch.rand(V, H * W, generator=g, dtype=torch.float64)).float()
    zeros = torch.rand(V, H * W, generator=g) < 0.1
    eps = EPS
    if name in ("generic", "empty"):
        i = torch.arange(H * W)[None, :] + torch.arange(V)[:, None]
        A[i % 10 == 3] = 0.0
        A[i % 10 == 7] = 1.0
        zeros[:, 0] = False
        m[zeros] = 0.0
        if name == "empty":
            A[0::2] = float("nan")
    elif name == "holes":
        kind = hole_kind(H, W).reshape(-1)
        A[:, kind == 0] = float("nan")
        A[:, kind == 1] = float("inf")
        t.view(V, -1)[:, kind == 2] = float("nan")
        t.view(V, -1)[:, kind == 3] = 1.5
        t.view(V, -1)[:, kind == 4] = -0.25
        m[:, kind == 5] = 0.0
        m[:, kind == 6] = -0.5
    elif name == "edges":
        eps = EDGE_EPS
        e = _edge_values(eps)
        assert H * W >= len(e)
        A[:, :len(e)] = e
        t.view(V, -1)[:, :len(e)] = 0.5
        t.view(V, -1)[:, EDGES["equal_target"]] = 0.25
        m[:, :len(e)] = 1.0
    out = dict(weights=[x.reshape(1, H, W).contiguous() for x in A], target=[x.contiguous() for x in t],
               mask=[x.reshape(H, W).contiguous() for x in m], eps=eps)
    _cache[key] = out
    return out


def cotangent(V):
    return torch.randn(17, generator=torch.Generator().manual_seed(5))[:V].double() + 2.0


def forward_backward(fn, name, H, W, V, mode, masked, dtype, device):
    """``fn`` is alpha_loss or its PyTorch statement: (loss (V,), count (V,), [V x dL/dweights])."""
    c = case(name, H, W, V)
    As = [x.to(device, dtype).requires_grad_() for x in c["weights"]]
    ts = None if mode == "entropy" else [x.to(device, dtype) for x in c["target"]]
    ms = [x.to(device, dtype) for x in c["mask"]] if masked else None
    loss, count = fn(As, ts, ms, mode=mode, eps=c["eps"])
    assert not count.requires_grad
    gs = torch.autograd.grad(loss, As, cotangent(V).to(device, dtype))
    return loss.detach(), count.detach(), list(gs)
