"""Cases, float64 reference and bars of tests/test_appearance_gpu.py -- CPU only, so that tests/test_appearance_cpu.py can check the
generators and what the bars are built from without a GPU.

``make_case(H, W, V)``   images ``(V,3,H,W)`` float32 in [0,1] plus a few out-of-range and negative pixels, a table ``(N,16)`` with
                         ``E`` within 0.3 of the identity, ``|k| <= 0.5`` and NaN in the unused column 15, an unordered list of V
                         distinct rows, a cotangent of mixed sign, a centre off the image centre; all from a seed (cached).
``run_torch(case, dt)``  ``appearance_torch`` in ``dt`` on the host with autograd: (out, dL/dimages, dL/dtable rows ``(V,16)``) as
                         float64 tensors.
``reference(H, W, V)``   ... in float64 (cached, never modified); ``float32_path`` the same in float32.
``term_sums(H, W, V)``   ``sum |terms|`` of each of the 15 sums per view, ``(V,16)``, from the float64 pieces of the formula.
``bars(H, W, V)``        the project's rule (lens_cases.py, loss_cases.py): 4 x what the float32 PyTorch path loses against float64
                         on the same input, plus 16 float32 epsilons times the scale -- ``1 + |ref|`` per element of the output and of
                         dL/dimage, ``sum |terms|`` per sum of the table gradient (a term is formed in at most eight float32 roundings
                         and the accumulation beyond the lane is in double).  Nothing in a bar comes from the kernel.
"""
import functools

import torch

from bags_raster import _lib as L
from bags_raster.appearance import appearance_torch

N = 23                                                       # rows of the table
FACTOR, FLOOR_EPS = 4.0, 16.0
EPS32 = float(torch.finfo(torch.float32).eps)
USED = [c for c in range(16) if c != 15]                     # the columns of a row that carry a sum

QUADS_PER_TILE = L.APPEARANCE_BLOCK                          # a thread takes a quad of 4 pixels, a workgroup a tile of 256 quads


def tiles(H, W):
    return -(-(H * ((W + 3) // 4)) // QUADS_PER_TILE)


def slots(H, W):
    """Workgroups per view of the backward's pixels kernel (include/bags_raster.h: BAGS_APPEARANCE_*)."""
    t = tiles(H, W)
    return min(t, max(L.APPEARANCE_MIN_SLOTS, -(-t // L.APPEARANCE_TILES_PER_SLOT)))


def _strided_shape():
    """From the kernel's constants: whole quads (the vector path is eligible), more tiles than a view has workgroups, so some
    workgroups walk two tiles, and a last tile that is not full."""
    W = 520
    H = (L.APPEARANCE_MIN_SLOTS * QUADS_PER_TILE) // (W // 4) + 1
    assert W % 4 == 0 and tiles(H, W) > slots(H, W) >= 2 and (H * (W // 4)) % QUADS_PER_TILE != 0 and H <= 160 and W <= 520
    return H, W


STRIDED = _strided_shape()                                   # (127, 520) with 256 / 64 / 4
SHAPES = ((1, 1), (3, 5), (16, 64), (17, 67), (37, 259), STRIDED)
VIEWS = (1, 2, 16, 17)
SEED = 7                                                     # of seeds 0..7 the one whose worst-conditioned sum is best conditioned
                                                             # (tests/test_appearance_cpu.py holds every sum of every case to its bound)


@functools.lru_cache(maxsize=None)
def make_case(H, W, V, seed=SEED):
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * H + 31 * W + V)
    images = torch.rand(V, 3, H, W, generator=g)
    n_odd = max(1, (V * 3 * H * W) // 50)                    # about 2 % of the values leave [0,1]: half above 1, half negative
    at = torch.randperm(V * 3 * H * W, generator=g)[:n_odd]                          # distinct places
    odd = torch.rand(n_odd, generator=g) * 0.5 + 1.0
    odd[::2] = -torch.rand((n_odd + 1) // 2, generator=g) * 0.5 - 0.01
    images.view(-1)[at] = odd
    table = torch.zeros(N, 16)
    table[:, :12] = torch.eye(3, 4).reshape(12) + (torch.rand(N, 12, generator=g) * 2 - 1) * 0.3
    table[:, 12:15] = (torch.rand(N, 3, generator=g) * 2 - 1) * 0.5
    table[:, 15] = float("nan")                              # never read
    rows = torch.randperm(N, generator=g)[:V].tolist()
    if rows == sorted(rows):                                 # unordered for every V > 1
        rows.reverse()
    cot = torch.randn(V, 3, H, W, generator=g) + 0.5         # mixed sign (about 3 in 10 negative), and no sum cancels to nothing
    center = (0.5 * W + 0.37, 0.5 * H - 0.21)
    return dict(H=H, W=W, V=V, images=images, table=table, rows=rows, cot=cot, center=center)


def run_torch(case, dtype):
    """(out (V,3,H,W), dL/dimages (V,3,H,W), dL/dtable rows (V,16)) of appearance_torch in ``dtype`` on the host, as float64."""
    img = case["images"].detach().clone().to(dtype).requires_grad_(True)             # the cached case stays as it is
    rows = case["table"][case["rows"]].detach().clone().to(dtype).requires_grad_(True)
    out = appearance_torch(img, rows, case["center"])
    out.backward(case["cot"].to(dtype))
    g_rows = rows.grad.detach().double()
    assert bool((g_rows[:, 15] == 0).all())                  # autograd: nothing depends on column 15
    return out.detach().double(), img.grad.detach().double(), g_rows


@functools.lru_cache(maxsize=None)
def reference(H, W, V, seed=SEED):
    return run_torch(make_case(H, W, V, seed), torch.float64)


@functools.lru_cache(maxsize=None)
def float32_path(H, W, V, seed=SEED):
    return run_torch(make_case(H, W, V, seed), torch.float32)


def sums_of_terms(p, g, rows, center):
    """(sum of terms (V,16), sum of |terms| (V,16)) of the 15 sums in float64, stated from the pieces of the formula, for images ``p``
    and cotangents ``g`` ``(V,3,H,W)`` and table rows ``(V,16)``."""
    p, g, rows = p.double(), g.double(), rows.double()
    V, _, H, W = p.shape
    cx, cy = center
    dx = torch.arange(W, dtype=torch.float64) + 0.5 - cx
    dy = torch.arange(H, dtype=torch.float64) + 0.5 - cy
    r2 = ((dx * dx)[None, :] + (dy * dy)[:, None]) / ((W * W + H * H) / 4.0)
    E, k = rows[:, :12].reshape(V, 3, 4), rows[:, 12:15]
    f = 1 + r2 * (k[:, 0, None, None] + r2 * (k[:, 1, None, None] + r2 * k[:, 2, None, None]))
    q = f[:, None] * p
    t = torch.einsum("vchw,vkc->vkhw", g, E[:, :, :3])
    df = (p * t).sum(1)
    total, absum = torch.zeros(V, 16, dtype=torch.float64), torch.zeros(V, 16, dtype=torch.float64)
    for kk in range(3):
        for cc in range(3):
            term = g[:, cc] * q[:, kk]
            total[:, 4 * kk + cc], absum[:, 4 * kk + cc] = term.sum((1, 2)), term.abs().sum((1, 2))
        total[:, 4 * kk + 3], absum[:, 4 * kk + 3] = g[:, kk].sum((1, 2)), g[:, kk].abs().sum((1, 2))
    for j in range(3):
        term = r2 ** (j + 1) * df
        total[:, 12 + j], absum[:, 12 + j] = term.sum((1, 2)), term.abs().sum((1, 2))
    return total, absum


@functools.lru_cache(maxsize=None)
def term_sums(H, W, V, seed=SEED):
    c = make_case(H, W, V, seed)
    return sums_of_terms(c["images"], c["cot"], c["table"][c["rows"]], c["center"])


@functools.lru_cache(maxsize=None)
def bars(H, W, V, seed=SEED):
    """(bar of out, bar of dL/dimages, bar of dL/dtable rows): tensors of the references' shapes."""
    o64, gi64, gt64 = reference(H, W, V, seed)
    o32, gi32, gt32 = float32_path(H, W, V, seed)
    _, absum = term_sums(H, W, V, seed)
    return (FACTOR * (o32 - o64).abs() + FLOOR_EPS * EPS32 * (1 + o64.abs()),
            FACTOR * (gi32 - gi64).abs() + FLOOR_EPS * EPS32 * (1 + gi64.abs()),
            FACTOR * (gt32 - gt64).abs() + FLOOR_EPS * EPS32 * absum)


def margins(H, W, V, out, g_images, g_rows, seed=SEED):
    """Largest error over bar of (out, dL/dimages, dL/dtable rows' used columns) against the float64 reference."""
    ref, bar = reference(H, W, V, seed), bars(H, W, V, seed)
    got = (out, g_images, g_rows)
    m = []
    for i in range(3):
        err = (got[i].detach().double().cpu() - ref[i]).abs()
        if i == 2:
            err, b = err[:, USED], bar[i][:, USED]
        else:
            b = bar[i]
        m.append(float((err / b).max()))
    return tuple(m)
