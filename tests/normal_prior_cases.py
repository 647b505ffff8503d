"""Cases, float64 reference and bars of tests/test_normal_prior_gpu.py -- CPU only, so that tests/test_normal_prior_cpu.py can check
the generators and what the bars are built from without a GPU.

``make_case(H, W, V, mode)``  V views of ``H x W``: a smooth surface ``z`` in about [2, 4] with per-view random frequencies and noise
                         of 0.3 pixel footprints (``0.3 z / fx``); where ``H, W >= 8`` a rectangle one unit nearer, so that
                         ``max_jump = 0.25`` has edges to drop; ``A`` in [0.55, 1] with a twenty-fifth of the pixels far below
                         ``min_weight = 0.5``; ``D = A z``; priors: unit vectors around (0,0,-1) with 0.3 spread, scaled by
                         [0.8, 1.2], a twentieth zeros and a few NaN; a mask with a tenth zeros and three tenths fractional;
                         pinholes ``fx`` in [0.9 W, 1.2 W], ``fy`` within 5 % of it, the principal point a pixel or so off centre,
                         different per view; per-view cotangents of mixed sign; all from a seed (cached, never modified).  The
                         generator asserts what keeps float32 and float64 on the same branch (``check_case``).
``degenerate_case(mode)``  the 16-view case of 17 x 67 with four views replaced: no solid pixel, an all-zero mask, an all-NaN prior,
                         a single valid centre.
``run_torch(case, dt)``  ``normal_prior_loss_torch`` in ``dt`` on the host with autograd: (loss, dL/dD, dL/dA) as float64 tensors and
                         the count.  ``reference`` is that in float64 (cached), ``float32_path`` in float32.
``closed_form(case)``    the same three from the closed forms of the issue, in float64, spelled through the point map ``P`` (the
                         statement spells the differences term by term), with the three wrong variants of
                         tests/test_normal_prior_cpu.py as switches.
``bars(...)``            the project's rule: 4 x what the float32 statement loses against the float64 statement on the same input,
                         plus 16 float32 epsilons times a scale.  The scale is ``1 + |ref|`` for the loss; for a per-pixel gradient
                         the sum of the absolute values of the terms of its closed form, summed over the up-to-four centres that
                         read the pixel.  Nothing in a bar comes from the kernel.  Where the scale is 0 (a pixel no valid centre
                         reads, a degenerate view) the bar is 0: exact zeros.
"""
import functools
import math

import torch

from bags_raster import _lib as L
from bags_raster.normal_prior import PRIOR_MIN_SQ, normal_prior_loss_torch

MIN_WEIGHT = 0.5
MAX_JUMP = 0.25
FACTOR, FLOOR_EPS = 4.0, 16.0
EPS32 = float(torch.finfo(torch.float32).eps)
F64 = torch.float64
MODES = ("cos", "l1")
TILE_W, TILE_H = L.NORMAL_PRIOR_TILE_W, L.NORMAL_PRIOR_TILE_H


def tiles(H, W):
    return (-(-W // TILE_W)) * (-(-H // TILE_H))


def _seam_shape():
    """From the kernel's tile: more than two tiles in each direction with partial last tiles both ways -- the last column of tiles is
    two pixels wide and the last row one pixel high, so a centre's neighbours, and a pixel's centres, lie across a seam."""
    H, W = 3 * TILE_H + 1, 2 * TILE_W + 2
    assert -(-H // TILE_H) >= 2 and -(-W // TILE_W) >= 2 and H % TILE_H != 0 and W % TILE_W != 0 and H * W < 100000
    return H, W


SEAM = _seam_shape()                                         # (25, 66) with a 32 x 8 tile
SHAPES = ((1, 1), (2, 7), (7, 2), (3, 3), (3, 5), (16, 64), (17, 67), (37, 259), SEAM)
FLAT = tuple(s for s in SHAPES if s[0] < 3 or s[1] < 3)      # no interior: loss 0
VIEWS = (1, 2, 16, 17)
SEED = 4                                                     # (one at which the only centre of the one-view 3 x 3 case is valid)


def _cross(a, b):
    return torch.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                        a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _cross_abs(a, b):
    return torch.stack([a[..., 1] * b[..., 2] + a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] + a[..., 0] * b[..., 2],
                        a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0]], -1)


def _pad(t, value):
    """(V,H,W,...) with one more pixel on every side of H and W."""
    V, H, W = t.shape[:3]
    out = torch.full((V, H + 2, W + 2) + tuple(t.shape[3:]), value, dtype=t.dtype)
    out[:, 1:-1, 1:-1] = t
    return out


def _pieces(c, max_jump=MAX_JUMP):
    """The float64 pieces of the closed forms for the case's maps as they are (z formed in float64), every pixel as a centre: a
    dict of (V,H,W[,3]) tensors and (V,) sums."""
    D, A, m = c["D"][:, 0].double(), c["A"][:, 0].double(), c["mask"].double()
    p = c["prior"].double().permute(0, 2, 3, 1)
    V, H, W = D.shape
    solid = (A >= MIN_WEIGHT) & (D > 0)
    z = torch.where(solid, D, torch.ones_like(D)) / torch.where(solid, A, torch.ones_like(A))
    pin = c["pinhole"].double()
    u = torch.arange(W, dtype=F64)[None, None, :].expand(V, H, W)
    v = torch.arange(H, dtype=F64)[None, :, None].expand(V, H, W)
    ray = torch.stack([(u - pin[:, 2, None, None]) / pin[:, 0, None, None], (v - pin[:, 3, None, None]) / pin[:, 1, None, None],
                       torch.ones(V, H, W, dtype=F64)], -1)
    P, sp, zp = _pad(z[..., None] * ray, 0.0), _pad(solid, False), _pad(z, 1.0)
    dx = P[:, 1:-1, 2:] - P[:, 1:-1, :-2]
    dy = P[:, 2:, 1:-1] - P[:, :-2, 1:-1]
    N = _cross(dy, dx)
    q = (N * N).sum(-1)
    all5 = sp[:, 1:-1, 1:-1] & sp[:, 1:-1, 2:] & sp[:, 1:-1, :-2] & sp[:, 2:, 1:-1] & sp[:, :-2, 1:-1]
    jx = (zp[:, 1:-1, 2:] - zp[:, 1:-1, :-2]).abs() / z
    jy = (zp[:, 2:, 1:-1] - zp[:, :-2, 1:-1]).abs() / z
    geometric = all5 & (jx <= max_jump) & (jy <= max_jump) & (q > 0) & torch.isfinite(q)
    pp = (p * p).sum(-1)
    valid = geometric & (m > 0) & torch.isfinite(pp) & (pp > PRIOR_MIN_SQ)
    away = torch.tensor((0.0, 0.0, -1.0), dtype=F64)
    sq = torch.sqrt(torch.where(valid, q, torch.ones_like(q)))
    n = torch.where(valid[..., None], N / sq[..., None], away)
    ph = torch.where(valid[..., None], p / torch.sqrt(torch.where(valid, pp, torch.ones_like(pp)))[..., None], away)
    w = torch.where(valid, m, torch.zeros_like(m))
    return dict(valid=valid, geometric=geometric, all5=all5, solid=solid, z=z, A=A, ray=ray, dx=dx, dy=dy, q=q, sq=sq, n=n, ph=ph, w=w,
                cnt=w.sum((1, 2)), jx=jx, jy=jy, pp=pp)


def interior(c):
    """(V,H,W) bool: the pixels with four neighbours inside the image."""
    t = torch.zeros(c["V"], c["H"], c["W"], dtype=torch.bool)
    t[:, 1:-1, 1:-1] = True
    return t


def check_case(c, max_jumps=(MAX_JUMP, math.inf)):
    """What keeps float32 and float64 on the same branch, and the case non-trivial; returns the figures."""
    A = c["A"].double()
    gap = float((A - MIN_WEIGHT).abs().min())
    assert gap >= 1e-3, gap                                                               # no A within 1e-3 of min_weight
    live = [v for v in range(c["V"]) if v not in c["degenerate"]]
    inner = interior(c)
    figures = dict(gap=gap, valid=1.0, jump=1.0, prior=1.0, kink=1.0)
    for mj in max_jumps:
        q = _pieces(c, mj)
        if inner.any() and live:
            share = float(q["valid"][live][inner[live]].double().mean())
            assert share >= 0.5, (share, mj)                                              # at least half of the interior pixels valid
            figures["valid"] = min(figures["valid"], share)
        if math.isfinite(mj) and q["all5"].any():
            jump = float(torch.minimum((q["jx"] - mj).abs(), (q["jy"] - mj).abs())[q["all5"]].min())
            assert jump >= 1e-3, jump                                                     # no relative jump within 1e-3 of max_jump
            figures["jump"] = min(figures["jump"], jump)
        pp = q["pp"][torch.isfinite(q["pp"])]
        figures["prior"] = min(figures["prior"], float((pp - PRIOR_MIN_SQ).abs().min())) if pp.numel() else figures["prior"]
        assert figures["prior"] >= 0.1, figures["prior"]                                  # |p|^2 away from 0.25
        if c["mode"] == "l1" and q["valid"].any():
            kink = float((q["n"] - q["ph"]).abs()[q["valid"]].min())
            assert kink >= 1e-4, kink                                                     # no valid |n_k - ph_k| below 1e-4
            figures["kink"] = min(figures["kink"], kink)
    return figures


@functools.lru_cache(maxsize=None)
def make_case(H, W, V, mode, seed=SEED):
    assert mode in MODES
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * H + 31 * W + V)
    px = H * W
    rnd = lambda *s: torch.rand(*s, generator=g)                                         # noqa: E731
    fx = W * (0.9 + 0.3 * rnd(V))
    fy = fx * (1.0 + 0.05 * (2 * rnd(V) - 1))
    pin = torch.stack([fx, fy, (W - 1) / 2 + 1.5 * (2 * rnd(V) - 1), (H - 1) / 2 + 1.5 * (2 * rnd(V) - 1)], 1).double()
    u = torch.arange(W, dtype=torch.float32)[None, None, :] / max(W, 32)
    v = torch.arange(H, dtype=torch.float32)[None, :, None] / max(H, 32)
    f = 0.5 + 0.75 * rnd(V, 2)
    ph0 = 6.2831853 * rnd(V, 2)
    z = 3.0 + 0.5 * torch.sin(6.2831853 * f[:, 0, None, None] * u + ph0[:, 0, None, None]) * torch.cos(6.2831853 * f[:, 1, None, None] * v + ph0[:, 1, None, None])
    z = z + 0.3 * z / fx[:, None, None] * torch.randn(V, H, W, generator=g).clamp(-3, 3)
    if H >= 8 and W >= 8:
        z[:, H // 4:H // 2 + 1, W // 4:W // 2 + 1] -= 1.0
    z = z.reshape(V, px)
    A = 0.55 + 0.45 * rnd(V, px)
    prior = torch.cat([0.3 * torch.randn(V, 2, px, generator=g), -torch.ones(V, 1, px)], 1)
    prior = prior / prior.norm(dim=1, keepdim=True) * (0.8 + 0.4 * rnd(V, 1, px))
    mask = torch.ones(V, px)
    n_low, n_zero, n_nan, n_off, n_frac = px // 25, px // 20, (max(1, px // 200) if px >= 64 else 0), px // 10, (3 * px) // 10
    for k in range(V):                                       # distinct places per kind; the kinds may overlap
        A[k, torch.randperm(px, generator=g)[:n_low]] = 0.3 * rnd(n_low)
        prior[k][:, torch.randperm(px, generator=g)[:n_zero]] = 0.0
        prior[k][:, torch.randperm(px, generator=g)[:n_nan]] = float("nan")
        at = torch.randperm(px, generator=g)
        mask[k, at[:n_off]] = 0.0
        mask[k, at[n_off:n_off + n_frac]] = 0.1 + 0.9 * rnd(n_frac)
    if px <= 9:
        mask[:] = 0.75                                       # cnt != the number of centres also for a single centre
    D = A * z
    cot = (0.5 + rnd(V)) * torch.where(torch.arange(V) % 2 == 0, 1.0, -1.0)
    c = dict(H=H, W=W, V=V, mode=mode, D=D.view(V, 1, H, W), A=A.view(V, 1, H, W), prior=prior.view(V, 3, H, W).contiguous(),
             mask=mask.view(V, H, W), pinhole=pin, cot=cot, degenerate=tuple(range(V)) if (H < 3 or W < 3) else ())
    for it in range(12):                                     # move a depth whose relative jump is too close to MAX_JUMP: the guard
        q = _pieces(c)
        near = (torch.minimum((q["jx"] - MAX_JUMP).abs(), (q["jy"] - MAX_JUMP).abs()) < 2e-3) & q["all5"]
        if not near.any():
            break
        c["D"] = torch.where(near[:, None], c["D"] * (1.02 + 0.003 * it), c["D"])
    for it in range(12 if mode == "l1" else 0):              # move a prior whose component is too close to the normal's: the kink of |.|
        q = _pieces(c, math.inf)                             # (every centre that is valid with the guard is valid without)
        near = ((q["n"] - q["ph"]).abs() < 1e-3).any(-1) & q["valid"]
        if not near.any():
            break
        bump = torch.tensor((0.013, -0.011, 0.0)).view(1, 3, 1, 1) * (1 + 0.37 * it)
        c["prior"] = torch.where(near[:, None], c["prior"] + bump, c["prior"])
    c["figures"] = check_case(c)
    return c


DEGENERATE_VIEWS = {"none_solid": 2, "mask_zero": 5, "prior_nan": 9, "one_centre": 12}


@functools.lru_cache(maxsize=None)
def degenerate_case(mode):
    """The 16-view case of 17 x 67 with the four views of DEGENERATE_VIEWS replaced; the other twelve are that case's."""
    base = make_case(17, 67, 16, mode)
    c = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in base.items()}
    k = DEGENERATE_VIEWS
    c["A"][k["none_solid"]] = 0.125
    c["D"][k["none_solid"]] = 0.125 * 3.0
    c["mask"][k["mask_zero"]] = 0.0
    c["prior"][k["prior_nan"]] = float("nan")
    ok = _pieces(base)["valid"][k["one_centre"]].nonzero()[7]
    one = torch.zeros(17, 67)
    one[ok[0], ok[1]] = 0.625
    c["mask"][k["one_centre"]] = one
    c["degenerate"] = (k["none_solid"], k["mask_zero"], k["prior_nan"])
    c["figures"] = check_case(c)
    return c


def run_torch(c, dtype, views=None, max_jump=MAX_JUMP):
    """(loss (V,), dL/dD (V,1,H,W), dL/dA (V,1,H,W)) of normal_prior_loss_torch in ``dtype`` on the host for L = sum cot_v loss_v, as
    float64, and the count (V,)."""
    idx = list(range(c["V"])) if views is None else list(views)
    D = [c["D"][i].detach().clone().to(dtype).requires_grad_(True) for i in idx]        # the cached case stays as it is
    A = [c["A"][i].detach().clone().to(dtype).requires_grad_(True) for i in idx]
    loss, count = normal_prior_loss_torch(D, A, [c["prior"][i].to(dtype) for i in idx], c["pinhole"][idx], [c["mask"][i].to(dtype) for i in idx],
                                          mode=c["mode"], min_weight=MIN_WEIGHT, max_jump=max_jump)
    assert loss.dtype == dtype and count.dtype == dtype and not count.requires_grad
    (loss.double() * c["cot"][idx].double()).sum().backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad                   # noqa: E731
    return (loss.detach().double(), torch.stack([zero(t) for t in D]).double(), torch.stack([zero(t) for t in A]).double(),
            count.detach().double())


@functools.lru_cache(maxsize=None)
def reference(H, W, V, mode, max_jump=MAX_JUMP):
    return run_torch(make_case(H, W, V, mode), F64, max_jump=max_jump)


@functools.lru_cache(maxsize=None)
def float32_path(H, W, V, mode, max_jump=MAX_JUMP):
    return run_torch(make_case(H, W, V, mode), torch.float32, max_jump=max_jump)


def _gather(q, gdx, gdy):
    """dL/dP (V,H,W,3) from the centres' dL/ddx and dL/ddy: P(u+1,v) += dL/ddx, P(u-1,v) -= dL/ddx, P(u,v+1) += dL/ddy,
    P(u,v-1) -= dL/ddy (a centre that is valid has all four inside the image)."""
    gP = _pad(torch.zeros_like(gdx), 0.0)
    gP[:, 1:-1, 2:] += gdx
    gP[:, 1:-1, :-2] -= gdx
    gP[:, 2:, 1:-1] += gdy
    gP[:, :-2, 1:-1] -= gdy
    assert float(gP[:, 0].abs().max()) == 0 and float(gP[:, -1].abs().max()) == 0 and float(gP[:, :, 0].abs().max()) == 0 and float(gP[:, :, -1].abs().max()) == 0
    return gP[:, 1:-1, 1:-1]


def closed_form(c, max_jump=MAX_JUMP, drop_projection=False, flip_dA=False, n_is_pixels=False):
    """(loss, dL/dD, dL/dA) from the closed forms, in float64, the cotangent included.  The switches make the three wrong answers
    the bars must reject: the ``n (n . g)`` projection dropped, the sign of dL/dA flipped, 1/cnt of the gradient replaced by
    1 / (H W)."""
    q = _pieces(c, max_jump)
    cnt, w, n, ph = q["cnt"], q["w"], q["n"], q["ph"]
    inv = torch.where(cnt > 0, 1.0 / cnt.clamp_min(1e-300), torch.zeros_like(cnt))
    inv_g = torch.where(cnt > 0, torch.full_like(cnt, 1.0 / (c["H"] * c["W"])), inv) if n_is_pixels else inv
    e = lambda t: t[:, None, None]                                                       # noqa: E731
    if c["mode"] == "l1":
        lpix, g = (n - ph).abs().sum(-1), torch.sign(n - ph)
    else:
        lpix, g = 1.0 - (n * ph).sum(-1), -ph
    loss = (w * lpix).sum((1, 2)) * inv
    s = e(c["cot"].double()) * w * e(inv_g)
    t = g if drop_projection else g - n * (n * g).sum(-1, keepdim=True)
    G = (s / q["sq"])[..., None] * t
    gP = _gather(q, _cross(G, q["dy"]), _cross(q["dx"], G))
    gz = (q["ray"] * gP).sum(-1)
    gD = gz / q["A"]
    gA = -(q["z"] / q["A"]) * gz * (-1.0 if flip_dA else 1.0)
    zero = torch.zeros_like(gz)
    return loss, torch.where(q["solid"], gD, zero)[:, None], torch.where(q["solid"], gA, zero)[:, None]


def scales(c, max_jump=MAX_JUMP):
    """sum |terms| of the closed forms in float64: (None, dL/dD (V,1,H,W), dL/dA (V,1,H,W))."""
    q = _pieces(c, max_jump)
    cnt, w, n, ph = q["cnt"], q["w"], q["n"].abs(), q["ph"].abs()
    inv = torch.where(cnt > 0, 1.0 / cnt.clamp_min(1e-300), torch.zeros_like(cnt))
    e = lambda t: t[:, None, None]                                                       # noqa: E731
    g = torch.ones_like(n) if c["mode"] == "l1" else ph
    s = e(c["cot"].double().abs()) * w * e(inv)
    G = (s / q["sq"])[..., None] * (g + n * (n * g).sum(-1, keepdim=True))
    gdx, gdy = _cross_abs(G, q["dy"].abs()), _cross_abs(q["dx"].abs(), G)
    gP = _pad(torch.zeros_like(gdx), 0.0)
    gP[:, 1:-1, 2:] += gdx
    gP[:, 1:-1, :-2] += gdx
    gP[:, 2:, 1:-1] += gdy
    gP[:, :-2, 1:-1] += gdy
    gz = (q["ray"].abs() * gP[:, 1:-1, 1:-1]).sum(-1)
    zero = torch.zeros_like(gz)
    return None, torch.where(q["solid"], gz / q["A"], zero)[:, None], torch.where(q["solid"], (q["z"] / q["A"]) * gz, zero)[:, None]


def bars_of(c, r64, r32, max_jump=MAX_JUMP):
    """(bar of loss, of dL/dD, of dL/dA) from the two runs of the statement and the case's scales."""
    _, sD, sA = scales(c, max_jump)
    lost = [FACTOR * (b - a).abs() for a, b in zip(r64[:3], r32[:3])]
    return (lost[0] + FLOOR_EPS * EPS32 * (1 + r64[0].abs()), lost[1] + FLOOR_EPS * EPS32 * sD, lost[2] + FLOOR_EPS * EPS32 * sA)


@functools.lru_cache(maxsize=None)
def bars(H, W, V, mode, max_jump=MAX_JUMP):
    return bars_of(make_case(H, W, V, mode), reference(H, W, V, mode, max_jump), float32_path(H, W, V, mode, max_jump), max_jump)


def margins_of(bar, ref, got):
    """Largest error over bar of each of (loss, dL/dD, dL/dA) against ``ref``; where a bar is 0 the value must be the reference's
    exactly (a pixel no valid centre reads, a degenerate view: zeros), which counts as margin 0 -- anything else as infinity."""
    m = []
    for b, r, g in zip(bar, ref[:3], got):
        err = (g.detach().double().cpu() - r).abs()
        ratio = torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
        ratio = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), ratio)
        m.append(float(ratio.max()))
    return tuple(m)


def margins(H, W, V, mode, got, max_jump=MAX_JUMP):
    return margins_of(bars(H, W, V, mode, max_jump), reference(H, W, V, mode, max_jump), got)
