"""Cases, float64 reference and bars of tests/test_bilagrid_gpu.py -- CPU only, so that tests/test_bilagrid_cpu.py can check the
generators and what the bars are built from without a GPU.

``make_case(grid, H, W, V)``  images ``(V,3,H,W)`` float32 in [0,1] with about 1 % of the pixels above 1 and 1 % below 0 in every
                         channel (luma outside [0,1] on both sides) and about 1 % exactly black; grids ``(N,12,L,Gy,Gx)`` within 0.3
                         of neutral, every vertex different; an unordered list of V distinct rows; a cotangent of mixed sign; all
                         from a seed (cached).  ``grid = (Gx, Gy, L)``.  The guidance term of dL/dimage jumps where
                         ``s = luma * (L-1)`` crosses an integer, so every pixel that is not deliberately placed is redrawn until
                         its float64 ``s`` is at least ``S_MARGIN = 1e-3`` from every integer of [0, L-1] -- hundreds of times the
                         float32 error of ``s`` -- and no pixel is excluded from any comparison.  (With L = 1 ``s`` is 0 for every
                         pixel and the guidance term is zero by rule: nothing to redraw.)  The deliberate pixels: black ones have
                         ``s = 0`` in both precisions; the out-of-range ones are at least 0.01 outside.  No white pixels:
                         ``0.299 + 0.587 + 0.114`` need not round to 1 alike in float32 and float64.
``run_torch(case, dt)``  ``bilagrid_torch`` in ``dt`` on the host with autograd: (out, dL/dimages, dL/dgrid rows ``(V,12,L,Gy,Gx)``)
                         as float64 tensors.
``reference(...)``       ... in float64 (cached, never modified); ``float32_path`` the same in float32.
``term_sums(...)``       ``sum |terms|`` per element of dL/dimage and of dL/dgrid, in float64 from the pieces of the formula.
``bars(...)``            the project's rule (appearance_cases.bars): 4 x what the float32 PyTorch path loses against float64 on the
                         same input, plus 16 float32 epsilons times the scale -- ``1 + |ref|`` per element of the output,
                         ``sum |terms|`` per element of dL/dgrid and (see ``IMAGE_SCALE``) of dL/dimage.  Nothing in a bar comes from
                         the kernel.
``tv_case / tv_reference / tv_bars``  the same for the total variation.
"""
import functools

import torch

from bags_raster import _lib as L
from bags_raster.bilagrid import LUMA, _planes, bilagrid_torch, bilagrid_tv_loss_torch

N = 23                                                       # grids of the bank
FACTOR, FLOOR_EPS = 4.0, 16.0
EPS32 = float(torch.finfo(torch.float32).eps)
S_MARGIN = 1e-3
F32, F64 = torch.float32, torch.float64

GRIDS = ((16, 16, 8), (5, 4, 3), (2, 3, 2), (1, 1, 1))       # (Gx, Gy, L)
TILE_W, TILE_H, BLOCK = L.BILAGRID_TILE_W, L.BILAGRID_TILE_H, L.BILAGRID_TILE_W * L.BILAGRID_TILE_H

# The scale of dL/dimage's floor.  The rule takes 1 + |ref| if the float32 PyTorch path itself stays inside 16 eps32 * (1 + |ref|)
# on every case (read as "inside the whole bar", which contains four times that path's own error, the condition could not fail).
# It does not stay inside: the guidance term is (L-1) times a sum of 12 products with plane(z1) - plane(z0), a difference of two
# numbers near the neutral matrix, and it cancels; the float32 path reaches 6.8 times that floor and a pixel's sum |terms| 90 times
# 1 + |ref| (tests/test_bilagrid_cpu.py::test_image_gradient_scale_is_the_sum_of_terms measures both).  So the scale is the
# pixel's sum |terms|.
IMAGE_SCALE = "terms"


def _axis32(n, G):
    """x0, x1 of the n pixels of an axis with G vertices, in the kernel's float32 operations."""
    u = (torch.arange(n, dtype=F32) + 0.5) / n * (G - 1)
    i0 = u.floor().clamp(max=G - 1).long()
    return i0, (i0 + 1).clamp(max=G - 1)


def tile_paths(grid, H, W):
    """(staged tiles, direct tiles) of the slice kernels: a tile stages its vertices in LDS iff it reaches at most
    BAGS_BILAGRID_STAGE_VERTS of them."""
    Gx, Gy, _ = grid
    x0, x1 = _axis32(W, Gx)
    y0, y1 = _axis32(H, Gy)
    staged = direct = 0
    for ty in range(0, H, TILE_H):
        for tx in range(0, W, TILE_W):
            nvx = int(x1[min(tx + TILE_W, W) - 1] - x0[tx]) + 1
            nvy = int(y1[min(ty + TILE_H, H) - 1] - y0[ty]) + 1
            if nvx * nvy <= L.BILAGRID_STAGE_VERTS:
                staged += 1
            else:
                direct += 1
    return staged, direct


def rectangles(grid, H, W):
    """The pixel counts of the support rectangles the dL/dgrid workgroups walk, one per xy-vertex (the kernel's integer bound)."""
    Gx, Gy, _ = grid

    def span(v, n, G):
        if G == 1:
            return 0, n - 1
        lo = -((-(v - 1) * n) // (G - 1)) if v < 1 else ((v - 1) * n) // (G - 1)        # C division truncates towards zero
        return max(0, lo - 2), min(n - 1, ((v + 1) * n + (G - 2)) // (G - 1) + 2)
    out = []
    for vy in range(Gy):
        for vx in range(Gx):
            (xl, xh), (yl, yh) = span(vx, W, Gx), span(vy, H, Gy)
            out.append(max(0, xh - xl + 1) * max(0, yh - yl + 1))
    return out


def _derived_shape():
    """From the kernel's constants: more than one tile each way with ragged last ones; over GRIDS both tile paths are reached, and
    some dL/dgrid workgroup walks its rectangle in more than one round of 256 pixels, the last one ragged."""
    H, W = 5 * TILE_H + 1, 3 * TILE_W + 5
    paths = [tile_paths(g, H, W) for g in GRIDS]
    assert any(s > 0 for s, _ in paths) and any(d > 0 for _, d in paths)
    assert any(n > BLOCK and n % BLOCK != 0 for g in GRIDS for n in rectangles(g, H, W))
    return H, W


DERIVED = _derived_shape()                                   # (21, 197) with 64 x 4
SHAPES = ((1, 1), (3, 5), (16, 64), (17, 67), (37, 259), DERIVED)
VIEWS = (1, 2, 16, 17)
SEED = 11


def s_of(images, Lz, dtype):
    """``s = luma * (L-1)`` per pixel in ``dtype``, in the statement's operations."""
    p = images.to(dtype)
    return (LUMA[0] * p[:, 0] + LUMA[1] * p[:, 1] + LUMA[2] * p[:, 2]) * (Lz - 1)


def distance_to_integers(s, Lz):
    """Per pixel: how far ``s`` is from the nearest integer of [0, L-1]."""
    k = s.round().clamp(0, Lz - 1)
    return (s - k).abs()


@functools.lru_cache(maxsize=None)
def make_case(grid, H, W, V, seed=SEED):
    Gx, Gy, Lz = grid
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * H + 31 * W + V + 101 * (Gx + 64 * (Gy + 64 * Lz)))
    npix = V * H * W
    px = torch.rand(npix, 3, generator=g)                    # pixel i's three channels
    images = px.view(V, H, W, 3).permute(0, 3, 1, 2)         # a view of px until the case is returned
    # the deliberate pixels: distinct places, a third of them each above 1, below 0 and black
    n_each = npix // 100 if npix >= 300 else (1 if npix >= 15 else 0)
    at = torch.randperm(npix, generator=g)[:3 * n_each]
    kind = torch.zeros(npix, dtype=torch.long)               # 0 drawn, 1 above, 2 below, 3 black
    for i, which in enumerate((1, 2, 3)):
        kind[at[i * n_each:(i + 1) * n_each]] = which
    px[kind == 1] = torch.rand(n_each, 3, generator=g) * 0.49 + 1.01
    px[kind == 2] = -torch.rand(n_each, 3, generator=g) * 0.49 - 0.01
    px[kind == 3] = 0.0
    if Lz >= 2:
        for _ in range(64):                                  # redraw what sits too close to a jump of the guidance term
            close = (distance_to_integers(s_of(images, Lz, F64), Lz) < S_MARGIN).reshape(npix) & (kind == 0)
            if not close.any():
                break
            px[close] = torch.rand(int(close.sum()), 3, generator=g)
        else:
            raise AssertionError("redraw did not settle")
    grids = torch.eye(3, 4).reshape(1, 12, 1, 1, 1) + (torch.rand(N, 12, Lz, Gy, Gx, generator=g) * 2 - 1) * 0.3
    rows = torch.randperm(N, generator=g)[:V].tolist()
    if rows == sorted(rows):                                 # unordered for every V > 1
        rows.reverse()
    cot = torch.randn(V, 3, H, W, generator=g) + 0.5         # mixed sign (about 3 in 10 negative)
    return dict(grid=grid, H=H, W=W, V=V, images=images.contiguous(), kind=kind.reshape(V, H, W), grids=grids, rows=rows, cot=cot)


def run_torch(case, dtype):
    """(out (V,3,H,W), dL/dimages (V,3,H,W), dL/dgrid rows (V,12,L,Gy,Gx)) of bilagrid_torch in ``dtype`` on the host, as float64."""
    img = case["images"].detach().clone().to(dtype).requires_grad_(True)             # the cached case stays as it is
    G = case["grids"][case["rows"]].detach().clone().to(dtype).requires_grad_(True)
    out = bilagrid_torch(img, G)
    out.backward(case["cot"].to(dtype))
    return out.detach().double(), img.grad.detach().double(), G.grad.detach().double()


@functools.lru_cache(maxsize=None)
def reference(grid, H, W, V, seed=SEED):
    return run_torch(make_case(grid, H, W, V, seed), F64)


@functools.lru_cache(maxsize=None)
def float32_path(grid, H, W, V, seed=SEED):
    return run_torch(make_case(grid, H, W, V, seed), F32)


def sums_of_terms(p, g, G):
    """``sum |terms|`` in float64 of (dL/dimage (V,3,H,W), dL/dgrid (V,12,L,Gy,Gx)) for images ``p``, cotangents ``g`` and grids ``G``
    ``(V,12,L,Gy,Gx)``, from the pieces of the formula.  dL/dimage_j = sum_c g_c A[4c+j] + [0 < s < L-1] (L-1) luma_j sum_k dA[k]
    (plane(z1)[k] - plane(z0)[k]) with dA[4c+j] = g_c p_j, dA[4c+3] = g_c; a coefficient and a plane count with the terms they are made of, the
    trilinear weights on |G| (a difference of planes that cancels still carries the rounding of both).  dL/dgrid is linear in dA with the non-negative trilinear
    weights: its sum |terms| is the same scatter of |dA|."""
    p, g = p.double(), g.double()
    G = G.double().detach().clone().requires_grad_(True)
    V, _, H, W = p.shape
    Lz = G.shape[2]
    P0, P1, tz, live = _planes(p, G)
    A = P0 + tz * (P1 - P0)
    dA = torch.cat([torch.cat([g[:, c:c + 1] * p, g[:, c:c + 1]], 1) for c in range(3)], 1)       # (V,12,H,W)
    (grid_abs,) = torch.autograd.grad(A, G, dA.abs())
    with torch.no_grad():                                                                         # the same weights on |G|: a plane's own terms
        Q0, Q1, _, _ = _planes(p, G.abs())
    A_abs = (Q0 + tz * (Q1 - Q0)).detach().reshape(V, 3, 4, H, W)
    guide = (dA.abs() * (Q0 + Q1)).sum(1) * (Lz - 1) * live                                       # (V,H,W)
    image_abs = torch.stack([(g.abs() * A_abs[:, :, j]).sum(1) + guide * LUMA[j] for j in range(3)], 1)
    return image_abs, grid_abs.detach()


@functools.lru_cache(maxsize=None)
def term_sums(grid, H, W, V, seed=SEED):
    c = make_case(grid, H, W, V, seed)
    return sums_of_terms(c["images"], c["cot"], c["grids"][c["rows"]])


@functools.lru_cache(maxsize=None)
def bars(grid, H, W, V, seed=SEED):
    """(bar of out, bar of dL/dimages, bar of dL/dgrid rows): tensors of the references' shapes."""
    o64, gi64, gg64 = reference(grid, H, W, V, seed)
    o32, gi32, gg32 = float32_path(grid, H, W, V, seed)
    image_abs, grid_abs = term_sums(grid, H, W, V, seed)
    return (FACTOR * (o32 - o64).abs() + FLOOR_EPS * EPS32 * (1 + o64.abs()),
            FACTOR * (gi32 - gi64).abs() + FLOOR_EPS * EPS32 * image_abs,
            FACTOR * (gg32 - gg64).abs() + FLOOR_EPS * EPS32 * grid_abs)


def margins(grid, H, W, V, out, g_images, g_rows, seed=SEED):
    """Largest error over bar of (out, dL/dimages, dL/dgrid rows) against the float64 reference; an element whose bar is 0 (a
    vertex no pixel reaches: reference, float32 path and every term exactly 0) must be exactly 0 and counts 0 or inf."""
    ref, bar = reference(grid, H, W, V, seed), bars(grid, H, W, V, seed)
    m = []
    for got, r, b in zip((out, g_images, g_rows), ref, bar):
        err = (got.detach().double().cpu() - r).abs()
        ratio = torch.where(b > 0, err / b.clamp(min=1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
        m.append(float(ratio.max()) if not torch.isnan(ratio).any() else float("nan"))
    return tuple(m)


# ---------------------------------------------------------------------------------------------------------------- total variation
@functools.lru_cache(maxsize=None)
def tv_case(grid, n, seed=SEED):
    """Grids (n,12,L,Gy,Gx) within 0.3 of neutral and a cotangent."""
    Gx, Gy, Lz = grid
    g = torch.Generator().manual_seed(7 * seed + n + 101 * (Gx + 64 * (Gy + 64 * Lz)))
    grids = torch.eye(3, 4).reshape(1, 12, 1, 1, 1) + (torch.rand(n, 12, Lz, Gy, Gx, generator=g) * 2 - 1) * 0.3
    return grids, -0.75                                      # a cotangent that is no power of two


def _tv_torch(grids, cot, dtype):
    x = grids.detach().clone().to(dtype).requires_grad_(True)
    loss = bilagrid_tv_loss_torch(x)
    (gx,) = torch.autograd.grad(loss, x, torch.tensor(cot, dtype=dtype)) if loss.requires_grad else (torch.zeros_like(x),)
    return loss.detach().double(), gx.double()


@functools.lru_cache(maxsize=None)
def tv_reference(grid, n, seed=SEED):
    return _tv_torch(*tv_case(grid, n, seed), F64)


@functools.lru_cache(maxsize=None)
def tv_bars(grid, n, seed=SEED):
    """(bar of the scalar, bar per element of the gradient).  Every term of the scalar is a square, so its sum |terms| is the
    value; an element of the gradient is |cot| * 2 / (N count_d) * (|x_i - x_{i-1}| + |x_{i+1} - x_i|) over the axes."""
    grids, cot = tv_case(grid, n, seed)
    l64, g64 = tv_reference(grid, n, seed)
    l32, g32 = _tv_torch(grids, cot, F32)
    x = grids.double()
    n_, _, Lz, Gy, Gx = x.shape
    absum = torch.zeros_like(x)
    for dim, size, others in ((4, Gx, Gy * Lz), (3, Gy, Gx * Lz), (2, Lz, Gx * Gy)):
        if size >= 2:
            d = (x.narrow(dim, 1, size - 1) - x.narrow(dim, 0, size - 1)).abs() * (abs(cot) * 2 / (n_ * 12 * (size - 1) * others))
            absum.narrow(dim, 0, size - 1).add_(d)
            absum.narrow(dim, 1, size - 1).add_(d)
    return FACTOR * (l32 - l64).abs() + FLOOR_EPS * EPS32 * l64.abs(), FACTOR * (g32 - g64).abs() + FLOOR_EPS * EPS32 * absum
